"""What scoring a separation costs, against the separation itself (profiles/evaluate.md).

    python tools/bench_evaluate.py [--runs 10] [--warmup 3] [--profile]

One process, default-size net, seeded weights, bench.py's audio as the mixture and 0.6 x mixture + noise as the true instruments,
batchsize 4, cropsize 256, host arrays in and out.  Per workload the routes alternate, --runs timed runs each after --warmup runs,
medians and ranges reported:
  A   what a user does without the library's help: separate_wave, then the float64 sums in numpy on the host
  B   evaluate_wave(stems=True)
  C   evaluate_wave, sums only
  D   separate_wave alone -- timed twice in the alternation (D1, D2), so that its own run-to-run spread is on the page
Workloads: a 30 s song, a 180 s song, 8 x 30 s through the many-calls.  The sums of A and C are compared to a relative 1e-9 before
anything is timed.  One JSON line per workload; --profile adds the launch profiler's lines of the iSTFT kernels for one C and one D."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--runs', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--profile', action='store_true')
    args = p.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as entry
    vr = entry.load_package()
    import bench
    dev = torch.device('cuda:0')
    net, _ = bench.seeded_state(vr)
    net.to(dev).eval()
    sp = vr.inference.Separator(net, dev, batchsize=4, cropsize=bench.CROP)
    hop, window = net.hop_length, 44100

    def song(seconds, seed):
        mix = bench.synth_wave(seconds, seed).astype(np.float32)
        rng = np.random.default_rng(1000 + seed)
        return mix, (0.6 * mix + 0.05 * rng.standard_normal(mix.shape)).astype(np.float32)

    def host_sums(mix, inst, y, v):
        n = y.shape[1]
        r_y = inst[:, :n].astype(np.float64)
        r_v = mix[:, :n].astype(np.float64) - r_y
        y, v = y.astype(np.float64), v.astype(np.float64)
        cols = [r_y ** 2, (r_y - y) ** 2, r_v ** 2, (r_v - v) ** 2]
        edges = np.arange(0, n, window)
        return np.stack([np.add.reduceat(c.sum(0), edges) for c in cols], axis=1)

    def routes(mixes, insts):
        one = len(mixes) == 1
        if one:
            m, i = mixes[0], insts[0]
            sep = lambda: [sp.separate_wave(m)]
            return {'A': lambda: [host_sums(m, i, *sp.separate_wave(m))], 'B': lambda: [sp.evaluate_wave(m, i, window=window, stems=True)['sums']],
                    'C': lambda: [sp.evaluate_wave(m, i, window=window)['sums']], 'D1': sep, 'D2': sep}
        sep = lambda: sp.separate_wave_many(mixes)
        return {'A': lambda: [host_sums(m, i, y, v) for m, i, (y, v) in zip(mixes, insts, sp.separate_wave_many(mixes))],
                'B': lambda: [r['sums'] for r in sp.evaluate_wave_many(mixes, insts, window=window, stems=True)],
                'C': lambda: [r['sums'] for r in sp.evaluate_wave_many(mixes, insts, window=window)], 'D1': sep, 'D2': sep}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def profiled(fn):
        nat, h = vr.native, net._handle.h
        nat.check(nat.lib().vr_profile_begin(h))
        try:
            fn()
        finally:
            a, b, c, d = ctypes.c_double(), ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
            nat.check(nat.lib().vr_profile_end(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
        need = nat.lib().vr_profile_report(h, None, 0)
        buf = ctypes.create_string_buffer(int(need) + 1)
        nat.lib().vr_profile_report(h, buf, need)
        return [ln for ln in buf.value.decode().splitlines() if 'istft_tile_kernel' in ln]

    workloads = (('30 s', [song(30.0, 0)]), ('180 s', [song(180.0, 1)]), ('8 x 30 s', [song(30.0, 10 + k) for k in range(8)]))
    for name, songs in workloads:
        mixes, insts = [m for m, _ in songs], [i for _, i in songs]
        r = routes(mixes, insts)
        worst = 0.0
        for a, c in zip(r['A'](), r['C']()):
            assert a.shape == c.shape, (a.shape, c.shape)
            worst = max(worst, float((np.abs(a - c) / a).max()))
        assert worst <= 1e-9, 'host sums and device sums differ by a relative %.3e' % worst
        t = {k: [] for k in r}
        for n in range(args.warmup + args.runs):
            for k, fn in r.items():
                ms = timed(fn)
                if n >= args.warmup:
                    t[k].append(ms)
        med = {k: statistics.median(v) for k, v in t.items()}
        line = {'workload': name, 'samples': int(sum(hop * (m.shape[1] // hop) for m in mixes)), 'sums_A_vs_C': worst}
        for k in t:
            line[k + '_ms'] = round(med[k], 2)
            line[k + '_range'] = [round(min(t[k]), 2), round(max(t[k]), 2)]
        line['D_spread_ms'] = round(abs(med['D1'] - med['D2']), 2)
        line.update({'C_minus_D_ms': round(med['C'] - min(med['D1'], med['D2']), 2), 'B_minus_D_ms': round(med['B'] - min(med['D1'], med['D2']), 2),
                     'A_minus_D_ms': round(med['A'] - min(med['D1'], med['D2']), 2), 'runs': args.runs, 'warmup': args.warmup,
                     'gpu': torch.cuda.get_device_name(0)})
        print(json.dumps(line), flush=True)
        if args.profile:
            for k in ('C', 'D1'):
                for ln in profiled(r[k]):
                    print('profile %s %s\t%s' % (name, k, ln), flush=True)


if __name__ == '__main__':
    main()
