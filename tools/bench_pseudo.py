"""Pseudo-instrument labels: the one call against the composition through the calls the package had before (DESIGN.md section 6q,
profiles/pseudo.md).

    python tools/bench_pseudo.py [--runs 10] [--warmup 3]

One process, default-size net, seeded weights, bench.py's audio as the mixture and 0.6 x mixture + noise as the instrumental (aligned,
stereo), batchsize 16, cropsize 256, tta, host arrays in and out.  Per workload the routes alternate, --runs timed runs each after
--warmup runs, medians and ranges reported:
  A   wave_to_spectrogram x 2, numpy X - y, separate_many(tta=True), numpy y + a, a .transpose(2, 0, 1) copy into the cache's rows
  B   pseudo_instruments_wave_many(layout='rows')
  C   pseudo_instruments_wave_many(layout='spec')
Workloads: 16 pairs x 5 s, 8 x 30 s, 2 x 180 s.  A and B are compared bit for bit before anything is timed.  One JSON line per
workload, then the launch profiler's lines of the two front-end and the two back-end forms for one B and one C."""
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
    args = p.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as entry
    vr = entry.load_package()
    import bench
    dev = torch.device('cuda:0')
    net, _ = bench.seeded_state(vr)
    net.to(dev).eval()
    sp = vr.inference.Separator(net, dev, batchsize=16, cropsize=bench.CROP)
    hop, n_fft = net.hop_length, net.n_fft
    stft = vr.spec_utils.wave_to_spectrogram

    def pair(seconds, seed):
        mix = bench.synth_wave(seconds, seed).astype(np.float32)
        rng = np.random.default_rng(1000 + seed)
        return mix, (0.6 * mix + 0.05 * rng.standard_normal(mix.shape)).astype(np.float32)

    def composed(mixes, insts):
        Xs, ys = [stft(m, hop, n_fft) for m in mixes], [stft(i, hop, n_fft) for i in insts]
        stems = sp.separate_many([X - y for X, y in zip(Xs, ys)], tta=True)
        return [np.ascontiguousarray((y + a).transpose(2, 0, 1)) for y, (a, _) in zip(ys, stems)]

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
        return [ln for ln in buf.value.decode().splitlines() if 'Pseudo' in ln]

    workloads = (('16 x 5 s', [pair(5.0, k) for k in range(16)]), ('8 x 30 s', [pair(30.0, 20 + k) for k in range(8)]),
                 ('2 x 180 s', [pair(180.0, 40 + k) for k in range(2)]))
    for name, songs in workloads:
        mixes, insts = [m for m, _ in songs], [i for _, i in songs]
        r = {'A': lambda: composed(mixes, insts), 'B': lambda: sp.pseudo_instruments_wave_many(mixes, insts, layout='rows'),
             'C': lambda: sp.pseudo_instruments_wave_many(mixes, insts, layout='spec')}
        equal = all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(r['A'](), r['B']()))
        t = {k: [] for k in r}
        for n in range(args.warmup + args.runs):
            for k, fn in r.items():
                ms = timed(fn)
                if n >= args.warmup:
                    t[k].append(ms)
        med = {k: statistics.median(v) for k, v in t.items()}
        line = {'workload': name, 'frames': int(sum(1 + m.shape[1] // hop for m in mixes)), 'A_equals_B_bitwise': bool(equal)}
        for k in t:
            line[k + '_ms'] = round(med[k], 2)
            line[k + '_range'] = [round(min(t[k]), 2), round(max(t[k]), 2)]
        line.update({'A_over_B': round(med['A'] / med['B'], 3), 'A_over_C': round(med['A'] / med['C'], 3), 'runs': args.runs,
                     'warmup': args.warmup, 'gpu': torch.cuda.get_device_name(0)})
        print(json.dumps(line), flush=True)
        for k in ('B', 'C'):
            for ln in profiled(r[k]):
                print('profile %s %s\t%s' % (name, k, ln), flush=True)


if __name__ == '__main__':
    main()
