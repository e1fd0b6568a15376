"""What the remix and mono augmentations cost a batch (profiles/remix.md).

    python tools/bench_remix.py  [--visits 3] [--rounds 5] [--calls 100] [--parent-tree DIR | --parent-rev HEAD^]

ResidentTrainingSet.batch(16 indices) alone at the default training shape -- B 16, T 256, 1025 bins, on the rows store, --songs synthetic
songs of --rows rows -- ending in a device synchronisation, a host clock around it.  Five cases, every rate 0 apart from the one named:

    zero     all rates 0: today's descriptors, today's entry point, the AugDesc instantiation
    mixup    mixup_rate 1: four crops a sample
    remix    remix_rate 1: the same four crops through the AugDescEx instantiation
    mono     mono_rate 1: two crops a sample, each read by both channel blocks
    parent   `zero` on the PARENT commit's package and library

The parent is a tree of its own: --parent-tree names a checkout of it that has been built, else `git archive --parent-rev` is unpacked
into a temporary directory and built there (python __graft_entry__.py).  Each tree runs in worker processes of its own (--worker), this
tree's and the parent's alternating --visits times in one call; a worker measures its cases alternating --rounds times, a round the median
of --calls timed calls after warm-up; the JSON line gives per case the median over all rounds of all visits and, as *_spread, the lowest and
highest round.  Nothing here is a threshold.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BATCH, CROP, BINS, N_FFT, HOP = 16, 256, 1025, 2048, 1024
CASES = {'zero': {}, 'mixup': {'mixup_rate': 1.0}, 'remix': {'remix_rate': 1.0}, 'mono': {'mono_rate': 1.0}}


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


def worker(args):
    """One tree, its cases alternating -> one JSON line {case: [round medians in ms]}"""
    sys.path.insert(0, args.tree)
    import numpy as np
    import torch
    import __graft_entry__ as entry
    vr = entry.load_package()
    if not torch.cuda.is_available():
        raise SystemExit('bench_remix: needs a GPU (nothing here is measured without one)')
    h = vr.spec_utils._signal_handle(N_FFT, HOP)                    # batch() asks a model for its handle alone
    model = types.SimpleNamespace(n_fft=N_FFT, hop_length=HOP, _need_handle=lambda: h)
    ts = [list(r) for r in json.loads(args.songs_json)] * 4
    sets = {}
    for case in args.cases.split(','):
        kw = dict(cropsize=CROP, reduction_rate=0.0, reduction_weight=None, mixup_rate=0.0, mixup_alpha=0.4, model=model)
        kw.update(CASES[case])
        sets[case] = vr.dataset.ResidentTrainingSet(ts, **kw)
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
    for ds in sets.values():                                        # the upload, the code objects, torch's allocator
        np.random.seed(0)
        batch_ms(ds, args.warmup)
    rounds = {case: [] for case in sets}
    for r in range(args.rounds):
        for case, ds in sets.items():
            np.random.seed(100 + r)
            rounds[case].append(statistics.median(batch_ms(ds, args.calls)))
    for ds in sets.values():
        ds.close()
    print('BENCH_REMIX ' + json.dumps(rounds), flush=True)


def parent_tree(rev, into):
    """the parent commit unpacked into `into` and built there -> its path"""
    tar = subprocess.run(['git', '-C', ROOT, 'archive', '--format=tar', rev], check=True, stdout=subprocess.PIPE).stdout
    subprocess.run(['tar', '-x', '-C', into], input=tar, check=True)
    subprocess.run([sys.executable, '__graft_entry__.py'], cwd=into, check=True, stdout=subprocess.DEVNULL)
    return into


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--visits', type=int, default=3, help='worker processes per tree, the two trees alternating')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=100, help='timed batch() calls per case and round')
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--songs', type=int, default=8)
    ap.add_argument('--rows', type=int, default=1000)
    ap.add_argument('--parent-tree', default=None, help='a built checkout of the parent commit')
    ap.add_argument('--parent-rev', default='HEAD^')
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--tree', default=ROOT)
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--songs-json', default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    with tempfile.TemporaryDirectory() as folder:
        parent = os.path.abspath(args.parent_tree) if args.parent_tree else parent_tree(args.parent_rev, os.path.join(folder, 'parent'))
        os.makedirs(os.path.join(folder, 'songs'))
        songs = json.dumps(write_songs(os.path.join(folder, 'songs'), args.songs, args.rows))
        merged = {}
        for _ in range(args.visits):
            for tree, cases, rename in ((ROOT, ','.join(CASES), None), (parent, 'zero', 'parent')):
                cmd = [sys.executable, os.path.abspath(__file__), '--worker', '--tree', tree, '--cases', cases, '--songs-json', songs,
                       '--rounds', str(args.rounds), '--calls', str(args.calls), '--warmup', str(args.warmup)]
                env = dict(os.environ)
                env.pop('VR_LIB_PATH', None)                        # each tree loads its own library
                out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, env=env).stdout
                line = [ln for ln in out.splitlines() if ln.startswith('BENCH_REMIX ')][-1]
                for case, v in json.loads(line[len('BENCH_REMIX '):]).items():
                    merged.setdefault(rename or case, []).extend(v)
    out = {'batch': BATCH, 'cropsize': CROP, 'bins': BINS, 'songs': args.songs, 'rows_per_song': args.rows, 'visits': args.visits,
           'rounds_per_visit': args.rounds, 'calls_per_round': args.calls}
    for case, v in merged.items():
        out['batch_ms_' + case] = round(statistics.median(v), 4)
        out['batch_ms_' + case + '_spread'] = [round(min(v), 4), round(max(v), 4)]
    print(json.dumps(out), flush=True)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
