"""Pitch-shifted training pairs: vr_pitch_pair_many against the numpy definition (profiles/pitch.md).

    python tools/bench_pitch.py [--runs 5] [--warmup 2] [--pitch -1] [--workers 16] [--no-ref]

One process for the device route, a pool of --workers processes for the definition (tests/pitch_ref.py, one task per shifted signal, then
the two STFTs per pair).  Seeded noise-plus-tones pairs at 44.1 kHz, the shift at n_fft 2048 / hop 512, the training transform at 2048 /
1024, host arrays in and out, rows layout.  Workloads: 16 pairs x 5 s, 8 x 30 s, 2 x 180 s.  Per workload: the device's median and range
over --runs timed calls after --warmup (the one call of all pairs, alternating with a Python loop of one call per pair), the
definition's wall time for one pass, the launch profiler's per-kernel split of one call, and each kernel's noted (algorithmic) bytes over
its time -- for the vocoder pass each spectrogram read once and the stretched one written once; no hardware counter is read.  Before
anything is timed the device's first pair is compared with the definition's (max-abs difference over the peak, reported, not gated)."""
import argparse
import ctypes
import json
import multiprocessing
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SR, N_FFT, HOP, SHIFT_N_FFT, SHIFT_HOP = 44100, 2048, 1024, 2048, 512


def make_pair(seconds, seed):
    import numpy as np
    L = int(seconds * SR)
    rng = np.random.default_rng(seed)
    t = np.arange(L) / SR
    y = np.asarray([0.1 * rng.standard_normal(L) + 0.3 * np.sin(2 * np.pi * 220.0 * (c + 1) * t) for c in range(2)], dtype=np.float32)
    v = np.asarray([0.05 * rng.standard_normal(L) + 0.2 * np.sin(2 * np.pi * 523.0 * (c + 1) * t) for c in range(2)], dtype=np.float32)
    return y + v, y


def _ref_shift(task):
    import pitch_ref
    row, rate, ratio = task
    return pitch_ref.pitch_shift(row, rate, ratio, SHIFT_N_FFT, SHIFT_HOP)


def _ref_stft(row):
    import pitch_ref
    return pitch_ref.stft(row, N_FFT, HOP)


def reference(pool, pairs, rate, ratio):
    """the definition over the pool: -> [(X' rows, y' rows, peak)]"""
    import numpy as np
    tasks = []
    for X, y in pairs:
        v = X - y
        tasks += [(y[0], rate, ratio), (y[1], rate, ratio), (v[0], rate, ratio), (v[1], rate, ratio)]
    shifted = pool.map(_ref_shift, tasks, chunksize=1)
    waves = []
    for k in range(len(pairs)):
        ys, vs = np.asarray(shifted[4 * k:4 * k + 2]), np.asarray(shifted[4 * k + 2:4 * k + 4])
        Xs = ys + vs
        waves += [Xs[0], Xs[1], ys[0], ys[1]]
    specs = pool.map(_ref_stft, waves, chunksize=1)
    out = []
    for k in range(len(pairs)):
        SX, Sy = np.asarray(specs[4 * k:4 * k + 2]), np.asarray(specs[4 * k + 2:4 * k + 4])
        out.append((SX.transpose(2, 0, 1), Sy.transpose(2, 0, 1), max(np.abs(SX).max(), np.abs(Sy).max())))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--runs', type=int, default=5)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--pitch', type=int, default=-1)
    p.add_argument('--workers', type=int, default=16)
    p.add_argument('--no-ref', action='store_true')
    args = p.parse_args()
    pool = None if args.no_ref else multiprocessing.get_context('spawn').Pool(args.workers)      # before the GPU is opened: the workers never touch it
    import numpy as np
    import torch
    import __graft_entry__ as entry
    vr = entry.load_package()
    rate, ratio = vr.audio.pitch_rate_and_ratio(SR, args.pitch)
    handle = vr.spec_utils._signal_handle(N_FFT, HOP)

    def device(mixes, insts):
        return vr.audio.pitch_pair_many(mixes, insts, SR, args.pitch, HOP, N_FFT, shift_n_fft=SHIFT_N_FFT, shift_hop_length=SHIFT_HOP, layout='rows')

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def profiled(fn):
        nat, h = vr.native, handle.h
        nat.check(nat.lib().vr_profile_begin(h))
        try:
            fn()
        finally:
            a, b, c, d = ctypes.c_double(), ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
            nat.check(nat.lib().vr_profile_end(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
        need = nat.lib().vr_profile_report(h, None, 0)
        buf = ctypes.create_string_buffer(int(need) + 1)
        nat.lib().vr_profile_report(h, buf, need)
        return buf.value.decode().splitlines()

    workloads = (('16 x 5 s', [make_pair(5.0, k) for k in range(16)]), ('8 x 30 s', [make_pair(30.0, 20 + k) for k in range(8)]),
                 ('2 x 180 s', [make_pair(180.0, 40 + k) for k in range(2)]))
    for name, pairs in workloads:
        mixes, insts = [X for X, _ in pairs], [y for _, y in pairs]
        run = lambda: device(mixes, insts)
        got = run()
        line = {'workload': name, 'pitch': args.pitch, 'samples': int(sum(X.shape[1] for X in mixes))}
        if pool is not None:
            t0 = time.perf_counter()
            ref = reference(pool, pairs, rate, ratio)
            line['definition_s'] = round(time.perf_counter() - t0, 2)
            line['definition_workers'] = args.workers
            errs = [max(float(np.abs(got[0][k] - ref[k][0]).max()), float(np.abs(got[1][k] - ref[k][1]).max())) / float(ref[k][2]) for k in range(len(pairs))]
            line['max_err_over_peak'] = float('%.3e' % max(errs))
        loop = lambda: [device([X], [y]) for X, y in pairs]              # the same pairs, one library call each
        t, tl = [], []
        for n in range(args.warmup + args.runs):
            ms, ml = timed(run), timed(loop)
            if n >= args.warmup:
                t.append(ms)
                tl.append(ml)
        line.update({'device_ms': round(statistics.median(t), 2), 'device_range': [round(min(t), 2), round(max(t), 2)],
                     'loop_ms': round(statistics.median(tl), 2), 'loop_range': [round(min(tl), 2), round(max(tl), 2)], 'runs': args.runs,
                     'warmup': args.warmup, 'gpu': torch.cuda.get_device_name(0)})
        if pool is not None:
            line['definition_over_device'] = round(line['definition_s'] * 1e3 / line['device_ms'], 1)
        print(json.dumps(line), flush=True)
        for ln in profiled(run):                    # name, calls, ms, flops, noted bytes, noted calls (+ the noted bytes over the time)
            f = ln.split('\t')
            gbs = float(f[4]) / float(f[2]) * 1e-6 if len(f) >= 5 and float(f[2]) > 0 and float(f[4]) > 0 else 0.0
            print('profile %s\t%s\t%.1f GB/s' % (name, ln, gbs), flush=True)
    if pool is not None:
        pool.close()
        pool.join()


if __name__ == '__main__':
    main()
