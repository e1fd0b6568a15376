"""The spectrogram caches of two folders of (mixture, instrumental) files, built on the device: what the first epoch of the reference's
train.py does through spec_utils.cache_or_load, as a command of its own.  Every pair is decoded on the host (audio.load); the pairs that
have no cache yet are trimmed, aligned by the cross-correlation of their heads, cut to the common window and transformed, and the pair's
peak is taken, --pairs_per_call pairs per library call (dataset.make_training_set(pairs_per_call=...)).  The files
are <folder>/sr{sr}_hl{hop}_nf{n_fft}/<song>.npy, rows [T, 2, bins] complex64: the bytes SpectrogramCache.pair writes.  A pair whose
two files exist is left alone.  --pairs_per_call 0 takes the host route for every pair."""
import argparse


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--sr', '-r', type=int, default=44100)
    p.add_argument('--hop_length', '-l', type=int, default=1024)
    p.add_argument('--n_fft', '-f', type=int, default=2048)
    p.add_argument('--mixtures', '-m', required=True)
    p.add_argument('--instruments', '-i', required=True)
    p.add_argument('--pairs_per_call', type=int, default=4)          # pairs per spec_utils.prepare_pair_many call; 0: the host route
    return p


def main(argv=None):
    from . import dataset
    args = build_parser().parse_args(argv)
    filelist = dataset.make_pair(args.mixtures, args.instruments)
    rows = dataset.make_training_set(filelist, args.sr, args.hop_length, args.n_fft,
                                     pairs_per_call=args.pairs_per_call if args.pairs_per_call > 0 else None)
    for X_path, y_path, peak in rows:
        print('{}\t{}\t{:.6g}'.format(X_path, y_path, float(peak)))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
