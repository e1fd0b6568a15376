"""Validation data from file lists: the patch route against the patch-free route (profiles/song_windows.md).

    python tools/bench_song_windows.py  [--songs 16] [--rows 7750] [--reps 3] [--batch 8] [--out FILE.json]

One process.  --songs synthetic spectrogram caches of --rows rows ([rows, 2, 1025] complex64; 7750 rows are three minutes at hop 1024)
are written where SpectrogramCache looks for them, under a temporary directory, and the default-size net with bench.py's seeded
weights supplies the handle, the crop size (256) and the offset (64).  Every figure is a host clock around work that ends in a device
synchronisation, repeated --reps times in alternation, reported as the median and, as *_spread, the lowest and highest repetition.

    route_patches_cold_s   file lists -> make_validation_set (patch folder absent: it normalises, pads and writes every window) ->
                           ResidentValidationSet -> DeviceLoader: the first batch, then the rest of one pass (batches only, no model)
    route_patches_warm_s   the same with the patch folder already written (make_validation_set still loads every song for its peak)
    route_songs_s          file lists -> make_training_set(peaks=False) -> ResidentSongValidationSet -> DeviceLoader, the same pass
    *_first_batch_s        the part of each up to the first batch on the device
    patch_folder_bytes, patches_device_bytes, songs_device_bytes
    peaks_host_s           make_training_set(peaks=True) on the cached songs: every file read whole, np.abs and max on the host
    peaks_device_s         make_training_set(peaks=False), then vr_dataset_peak of every song of the store already resident
    peak_call_ms           one vr_dataset_peak (two launches, a 24-byte copy back, a synchronise), songs taken in turn so that no
                           call finds its song in the 256 MiB Infinity Cache; peak_gbps = bytes of the song's two slabs over that time

The song caches were written moments before and stay in the host's page cache: every route reads them warm, which is the patch
route's best case as well.  The batches of the two routes are compared (torch.equal) on the first, the middle and the last batch,
and the device peaks with the host peaks; a difference is an error (exit status 1).  --dry stops before anything needs a GPU.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BINS, SR, HOP, N_FFT = 1025, 44100, 1024, 2048


def write_caches(folder, songs, rows):
    """-> file list of (mixture, instruments) audio paths whose caches exist (the audio itself is never opened on a cache hit)."""
    import numpy as np
    rng = np.random.default_rng(0)
    filelist = []
    for kind in ('mixtures', 'instruments'):
        os.makedirs(os.path.join(folder, kind, 'sr{}_hl{}_nf{}'.format(SR, HOP, N_FFT)))
    base = rng.standard_normal((rows, 2, BINS, 2), dtype=np.float32).view(np.complex64)[..., 0]
    for i in range(songs):
        X = np.roll(base, 97 * i, axis=0) * np.float32(0.5 + 0.1 * i)
        y = (X * rng.random((rows, 2, BINS), dtype=np.float32)).astype(np.complex64)
        pair = []
        for kind, a in (('mixtures', X), ('instruments', y)):
            np.save(os.path.join(folder, kind, 'sr{}_hl{}_nf{}'.format(SR, HOP, N_FFT), 'song%02d.npy' % i), a)
            pair.append(os.path.join(folder, kind, 'song%02d.wav' % i))
        filelist.append(tuple(pair))
    return filelist


def folder_bytes(path):
    return sum(os.path.getsize(os.path.join(path, n)) for n in os.listdir(path))


def med(values):
    return statistics.median(values), [min(values), max(values)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--songs', type=int, default=16)
    ap.add_argument('--rows', type=int, default=7750)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--out', default=None)
    ap.add_argument('--dry', action='store_true')
    args = ap.parse_args()
    args.out = os.path.abspath(args.out) if args.out else None      # (the measurement runs inside its temporary directory)
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import __graft_entry__ as entry
    import bench                                    # the seeded weights and the crop size of the flagship benchmark
    vr = entry.load_package()
    ds_mod = vr.dataset
    if not args.dry and not torch.cuda.is_available():
        raise SystemExit('bench_song_windows: needs a GPU (nothing here is measured without one)')
    res = {'songs': args.songs, 'rows': args.rows, 'bins': BINS, 'cropsize': bench.CROP, 'batch': args.batch, 'reps': args.reps}

    def note(msg):
        print('[bench_song_windows] %s' % msg, flush=True)

    with tempfile.TemporaryDirectory() as folder:
        os.chdir(folder)                            # make_validation_set writes its patch folder under the working directory
        try:
            return measure(args, res, folder, vr, bench, note)
        finally:
            os.chdir(ROOT)


def measure(args, res, folder, vr, bench, note):
    import numpy as np
    import torch
    ds_mod = vr.dataset
    t0 = time.perf_counter()
    filelist = write_caches(folder, args.songs, args.rows)
    note('caches written in %.1f s' % (time.perf_counter() - t0))
    if args.dry:
        rows = ds_mod.make_training_set(filelist, SR, HOP, N_FFT, peaks=False)
        full = ds_mod.make_training_set(filelist, SR, HOP, N_FFT)
        patches = ds_mod.make_validation_set(filelist, bench.CROP, SR, HOP, N_FFT, 64)
        ds = ds_mod.ResidentSongValidationSet(rows, bench.CROP, 64)
        assert len(ds) == len(patches) and [r[:2] for r in rows] == [r[:2] for r in full]
        note('dry run: %d songs, %d windows, patch folder %d bytes, song store %d bytes'
             % (len(rows), len(ds), folder_bytes(os.path.dirname(patches[0])), ds.nbytes))
        return 0
    dev = torch.device('cuda:0')
    net, _ = bench.seeded_state(vr)
    net.to(dev).eval()
    offset, crop = net.offset, bench.CROP
    res['offset'] = offset
    patch_dir = 'cs{}_sr{}_hl{}_nf{}_of{}'.format(crop, SR, HOP, N_FFT, offset)

    def one_pass(ds, keep):
        """first batch, then the rest of one DeviceLoader pass -> (seconds to the first batch from t0 of the caller, kept batches)"""
        kept = {}
        first = None
        for k, (X, y) in enumerate(ds_mod.DeviceLoader(ds, batch_size=args.batch, shuffle=False)):
            torch.cuda.synchronize()
            if first is None:
                first = time.perf_counter()
            if k in keep:
                kept[k] = (X, y)
        torch.cuda.synchronize()
        return first, kept

    def route_patches(cold, keep):
        if cold and os.path.isdir(patch_dir):
            shutil.rmtree(patch_dir)
        torch.cuda.synchronize()
        t = time.perf_counter()
        patches = ds_mod.make_validation_set(filelist, crop, SR, HOP, N_FFT, offset)
        with ds_mod.ResidentValidationSet(patches, model=net) as ds:
            first, kept = one_pass(ds, keep)
            end = time.perf_counter()
            dev_bytes = ds.nbytes
        return end - t, first - t, kept, dev_bytes, len(patches)

    def route_songs(keep):
        torch.cuda.synchronize()
        t = time.perf_counter()
        rows = ds_mod.make_training_set(filelist, SR, HOP, N_FFT, peaks=False)
        with ds_mod.ResidentSongValidationSet(rows, crop, offset, model=net) as ds:
            first, kept = one_pass(ds, keep)
            end = time.perf_counter()
            dev_bytes = ds.nbytes
        return end - t, first - t, kept, dev_bytes, None

    # warm-up of every code path at a small size (code objects, the handle's staging), then the repetitions in alternation
    small = filelist[:1]
    ds_mod.make_validation_set(small, crop, SR, HOP, N_FFT, offset)
    with ds_mod.ResidentValidationSet(ds_mod.make_validation_set(small, crop, SR, HOP, N_FFT, offset)[:2], model=net) as ds:
        ds.batch([0, 1])
    with ds_mod.ResidentSongValidationSet(ds_mod.make_training_set(small, SR, HOP, N_FFT, peaks=False), crop, offset, model=net) as ds:
        ds.batch([0, 1])
    torch.cuda.synchronize()
    note('warm-up done')

    n_batches = None
    times = {'cold': [], 'warm': [], 'songs': []}
    firsts = {'cold': [], 'warm': [], 'songs': []}
    same = True
    for rep in range(args.reps):
        keep = () if n_batches is None else (0, n_batches // 2, n_batches - 1)
        total, first, kept_c, res['patches_device_bytes'], n_patches = route_patches(True, keep)
        times['cold'].append(total)
        firsts['cold'].append(first)
        res['patch_folder_bytes'] = folder_bytes(patch_dir)
        n_batches = -(-n_patches // args.batch)
        keep = (0, n_batches // 2, n_batches - 1)
        total, first, kept_w, _, _ = route_patches(False, keep)
        times['warm'].append(total)
        firsts['warm'].append(first)
        total, first, kept_s, res['songs_device_bytes'], _ = route_songs(keep)
        times['songs'].append(total)
        firsts['songs'].append(first)
        for k in keep:
            same = same and torch.equal(kept_w[k][0], kept_s[k][0]) and torch.equal(kept_w[k][1], kept_s[k][1])
        del kept_c, kept_w, kept_s
        note('rep %d: patches cold %.2f s, patches warm %.2f s, songs %.2f s (first batch %.2f / %.2f / %.2f s), same batches: %s'
             % (rep, times['cold'][-1], times['warm'][-1], times['songs'][-1], firsts['cold'][-1], firsts['warm'][-1],
                firsts['songs'][-1], same))
    res['windows'] = n_patches
    for key, name in (('cold', 'route_patches_cold'), ('warm', 'route_patches_warm'), ('songs', 'route_songs')):
        res[name + '_s'], res[name + '_s_spread'] = med(times[key])
        res[name + '_first_batch_s'], res[name + '_first_batch_s_spread'] = med(firsts[key])
    res['batches_equal'] = bool(same)

    # peaks: the host's against the device's, on a store that is already resident (as in a training run)
    rows = ds_mod.make_training_set(filelist, SR, HOP, N_FFT, peaks=False)
    with ds_mod.ResidentTrainingSet(rows, crop, 0.0, None, 0.0, 0.4, model=net) as ts:
        ts._upload(0)                            # (fills the peaks once: warm-up of the two peak launches)
        store = ts._store
        host_t, dev_t = [], []
        for rep in range(args.reps):
            t = time.perf_counter()
            full = ds_mod.make_training_set(filelist, SR, HOP, N_FFT, peaks=True)
            host_t.append(time.perf_counter() - t)
            t = time.perf_counter()
            bare = ds_mod.make_training_set(filelist, SR, HOP, N_FFT, peaks=False)
            peaks = [store.peak(ts._song[(r[0], r[1])]) for r in bare]
            dev_t.append(time.perf_counter() - t)
        res['peaks_host_s'], res['peaks_host_s_spread'] = med(host_t)
        res['peaks_device_s'], res['peaks_device_s_spread'] = med(dev_t)
        res['peaks_equal'] = bool(all(np.float32(a[2]).tobytes() == np.float32(b).tobytes() for a, b in zip(full, peaks))
                                  and all(np.float32(a[2]).tobytes() == np.float32(b[2]).tobytes() for a, b in zip(full, ts.training_set)))
        call = []
        for rnd in range(4):
            for song in range(len(rows)):
                t = time.perf_counter()
                store.peak(song)
                call.append((time.perf_counter() - t) * 1e3)
        call = call[len(rows):]                  # the first round is warm-up
        res['peak_call_ms'], res['peak_call_ms_spread'] = med(call)
        res['peak_call_bytes'] = 2 * args.rows * 2 * BINS * 8
        res['peak_gbps'] = res['peak_call_bytes'] / (res['peak_call_ms'] * 1e-3) / 1e9
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if res['batches_equal'] and res['peaks_equal'] else 1


if __name__ == '__main__':
    sys.exit(main())
