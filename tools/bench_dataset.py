"""The training input pipeline: file-backed set against the set resident in HBM (profiles/resident_dataset.md).

    python tools/bench_dataset.py  [--rounds 5] [--calls 10] [--songs 8] [--rows 1000]

One process, the default training shape: batch 16, cropsize 256, 1025 bins, reduction_rate 0.03, mixup_rate 0.5, the default-size net
with bench.py's seeded weights.  --songs synthetic spectrogram pairs of --rows rows ([rows, 2, 1025] complex64, about 260 MB for the
defaults) are written to a temporary directory in the cache's .npy format and listed four times, so that a DeviceLoader pass has
batches of 16.  Two measurements, the two sides alternating --rounds times, each round the median of its timed calls, the JSON line
the median over the rounds and, as *_spread, the lowest and highest round:

    (a) batch_ms_*   dataset.batch(16 indices) alone, ending in a device synchronisation;
    (b) step_ms_*    one DeviceLoader iteration plus model.train_step on its batch, ending in a device synchronisation.

The file-backed side is VocalRemoverTrainingSet as it stands, reading files that were written moments before and read again by the
warm-up calls: a WARM page cache, its best case -- a set larger than host memory reads from disk instead.  Both sides draw from the
same numpy seed at the start of every round.  upload_ms is the one-time cost of the resident side (every song through a memory map
into its device slab), resident_bytes what it holds afterwards.  The line ends with resident_not_slower (batch_ms_resident <=
batch_ms_file); the exit status is 1 when that is false.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BATCH, BINS = 16, 1025


def reduction_weight(bins, level=0.2):
    """train.py:197-205."""
    import numpy as np
    u, s = bins // 10, bins - bins // 8
    return np.concatenate([np.linspace(0, 1, u, dtype=np.float32)[:, None], np.linspace(1, 0, s - u, dtype=np.float32)[:, None],
                           np.zeros((bins - s, 1), dtype=np.float32)], axis=0) * level


def write_songs(folder, songs, rows):
    import numpy as np
    rng = np.random.default_rng(0)
    out = []
    for i in range(songs):
        X = (rng.standard_normal((rows, 2, BINS), dtype=np.float32) + 1j * rng.standard_normal((rows, 2, BINS), dtype=np.float32)).astype(np.complex64)
        y = (X * rng.random((rows, 2, BINS), dtype=np.float32)).astype(np.complex64)
        paths = [os.path.join(folder, 'song%d_%s.npy' % (i, tag)) for tag in ('X', 'y')]
        np.save(paths[0], X)
        np.save(paths[1], y)
        out.append([paths[0], paths[1], float(max(np.abs(X).max(), np.abs(y).max()))])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=10, help='timed batch() calls per side and round')
    ap.add_argument('--epochs', type=int, default=3, help='DeviceLoader passes (two iterations each) per side and round')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--songs', type=int, default=8)
    ap.add_argument('--rows', type=int, default=1000)
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit('at least 5 rounds')
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import __graft_entry__ as entry
    import bench                                    # the seeded weights and the crop size of the flagship benchmark
    vr = entry.load_package()
    if not torch.cuda.is_available():
        raise SystemExit('bench_dataset: needs a GPU (nothing here is measured without one)')
    dev = torch.device('cuda:0')
    net, _ = bench.seeded_state(vr)
    net.to(dev).train()
    with tempfile.TemporaryDirectory() as folder:
        ts = write_songs(folder, args.songs, args.rows) * 4
        kw = dict(cropsize=bench.CROP, reduction_rate=0.03, reduction_weight=reduction_weight(BINS), mixup_rate=0.5, mixup_alpha=0.4, model=net)
        sets = {'file': vr.dataset.VocalRemoverTrainingSet(ts, **kw), 'resident': vr.dataset.ResidentTrainingSet(ts, **kw)}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sets['resident']._upload(net._need_handle().device)
        torch.cuda.synchronize()
        upload_ms = (time.perf_counter() - t0) * 1e3
        indices = [(5 * k + 1) % len(ts) for k in range(BATCH)]

        def batch_ms(ds, calls):
            times = []
            for _ in range(calls):
                torch.cuda.synchronize()
                t = time.perf_counter()
                ds.batch(indices)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t) * 1e3)
            return times

        def step_ms(ds, epochs):
            loader = vr.dataset.DeviceLoader(ds, batch_size=BATCH, shuffle=True, generator=torch.Generator().manual_seed(0))
            times = []
            for _ in range(epochs):
                it = iter(loader)
                while True:
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    try:
                        X, y = next(it)
                    except StopIteration:
                        break
                    net.zero_grad()
                    net.train_step(X, y, 1)
                    torch.cuda.synchronize()
                    times.append((time.perf_counter() - t) * 1e3)
            return times

        for ds in sets.values():                    # warm-up: code objects, the train step's workspace, the page cache
            np.random.seed(0)
            batch_ms(ds, args.warmup)
            step_ms(ds, 1)
        rounds = {k: [] for k in ('batch_file', 'batch_resident', 'step_file', 'step_resident')}
        for r in range(args.rounds):
            for what, fn, n in (('batch', batch_ms, args.calls), ('step', step_ms, args.epochs)):
                for side in ('file', 'resident'):
                    np.random.seed(100 + r)
                    rounds['%s_%s' % (what, side)].append(statistics.median(fn(sets[side], n)))
        out = {'batch': BATCH, 'cropsize': bench.CROP, 'bins': BINS, 'songs': args.songs, 'rows_per_song': args.rows, 'rounds': args.rounds,
               'upload_ms': round(upload_ms, 1), 'resident_bytes': sets['resident'].nbytes, 'page_cache': 'warm'}
        for k, v in rounds.items():
            out[k.replace('_', '_ms_', 1)] = round(statistics.median(v), 3)
            out[k.replace('_', '_ms_', 1) + '_spread'] = [round(min(v), 3), round(max(v), 3)]
        out['resident_not_slower'] = out['batch_ms_resident'] <= out['batch_ms_file']
        sets['resident'].close()
    print(json.dumps(out), flush=True)
    return 0 if out['resident_not_slower'] else 1


if __name__ == '__main__':
    raise SystemExit(main())
