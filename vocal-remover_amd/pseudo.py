"""The reference's pseudo.py (pseudo.py:16-74) on the device: for every (mixture, instrumental) pair of two folders, what the model
still hears as instruments in mixture - instrumental is added back to the instrumental,

    pseudo = y + Separator.separate_tta(X - y)[0]

and saved as {basename}_PseudoInstruments.npy with the reference's one-sample placeholder .wav beside it.  The pairs go through
Separator.pseudo_instruments_wave_many in groups of --songs_per_call: both transforms, the difference, the network and the sum
run in one library call per group, and the label is stored once.  The reference's arguments, plus --songs_per_call, --output_dir
(the reference writes into ./pseudo) and --rows ([T, 2, bins], the training cache's layout, instead of pseudo.py's [2, bins, T])."""
import argparse
import os

import numpy as np


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--gpu', '-g', type=int, default=-1)
    p.add_argument('--pretrained_model', '-P', type=str, default='models/baseline.pth')
    p.add_argument('--mixtures', '-m', required=True)
    p.add_argument('--instruments', '-i', required=True)
    p.add_argument('--sr', '-r', type=int, default=44100)
    p.add_argument('--n_fft', '-f', type=int, default=2048)
    p.add_argument('--hop_length', '-H', type=int, default=1024)
    p.add_argument('--batchsize', '-B', type=int, default=4)
    p.add_argument('--cropsize', '-c', type=int, default=256)
    p.add_argument('--postprocess', '-p', action='store_true')
    p.add_argument('--songs_per_call', type=int, default=8)          # pairs per pseudo_instruments_wave_many call
    p.add_argument('--output_dir', '-o', type=str, default='pseudo')
    p.add_argument('--rows', action='store_true')                    # save [T, 2, bins] (the cache's rows) instead of [2, bins, T]
    return p


def main(argv=None):
    import torch

    from . import audio, dataset, nets
    from .inference import Separator
    args = build_parser().parse_args(argv)
    device = torch.device('cuda:{}'.format(max(args.gpu, 0)))       # (there is no CPU path: --gpu -1 runs on device 0)
    model = nets.CascadedNet(args.n_fft, args.hop_length, 32, 128)
    model.load_state_dict(torch.load(args.pretrained_model, map_location='cpu'))
    model.to(device)
    sp = Separator(model, device, args.batchsize, args.cropsize, args.postprocess)
    os.makedirs(args.output_dir, exist_ok=True)
    filelist = dataset.make_pair(args.mixtures, args.instruments)
    step = max(args.songs_per_call, 1)
    for g in range(0, len(filelist), step):
        group = filelist[g:g + step]
        pairs = [dataset.load_aligned_pair(m, i, args.sr) for m, i in group]
        labels = sp.pseudo_instruments_wave_many([X for X, _ in pairs], [y for _, y in pairs], tta=True,
                                                 layout='rows' if args.rows else 'spec')
        for (mix_path, _), P in zip(group, labels):
            basename = os.path.splitext(os.path.basename(mix_path))[0]
            print(basename)
            audio.write(os.path.join(args.output_dir, '{}_PseudoInstruments.wav'.format(basename)), np.zeros(1, np.float32), args.sr)
            np.save(os.path.join(args.output_dir, '{}_PseudoInstruments.npy'.format(basename)), P)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
