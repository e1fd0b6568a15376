"""The reference's augment.py (augment.py:14-78) on the device: for every (mixture, instrumental) pair of two folders the aligned waves are
split into y and v = X - y, both are shifted by --pitch semitones, X' = y' + v' is rebuilt, and the STFTs of X' and y' are saved as
<folder>/sr{sr}_hl{hop}_nf{n_fft}/<song>_pitch{n}.npy beside the plain caches.  The pairs go through audio.pitch_pair_many in groups of
--songs_per_call (dataset.make_pitch_training_set); a pair whose two files exist is skipped, as there.  The shift is
librosa.effects.pitch_shift's phase vocoder, not the reference's external `soundstretch` binary, and the files
hold the training cache's rows [T, 2, bins].  The reference's arguments, plus --songs_per_call."""
import argparse


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--sr', '-r', type=int, default=44100)
    p.add_argument('--hop_length', '-l', type=int, default=1024)
    p.add_argument('--n_fft', '-f', type=int, default=2048)
    p.add_argument('--pitch', '-p', type=int, default=-1)
    p.add_argument('--mixtures', '-m', required=True)
    p.add_argument('--instruments', '-i', required=True)
    p.add_argument('--songs_per_call', type=int, default=4)          # pairs per audio.pitch_pair_many call
    return p


def main(argv=None):
    from . import dataset
    args = build_parser().parse_args(argv)
    filelist = dataset.make_pair(args.mixtures, args.instruments)
    for X_path, y_path, peak in dataset.make_pitch_training_set(filelist, args.sr, args.hop_length, args.n_fft, args.pitch,
                                                                 songs_per_call=args.songs_per_call):
        print('{}\t{}\t{:.6g}'.format(X_path, y_path, float(peak)))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
