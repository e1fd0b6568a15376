"""The stems' spectrogram pictures from the separation call, against forming them on the host (profiles/image.md).

    python tools/bench_image.py [--runs 10] [--warmup 2] [--workloads 30,180,8x30]

One process, default-size net, seeded weights, bench.py's synthetic audio, batchsize 4, cropsize 256, numpy in and numpy out.  Per
workload (a 30 s song, a 180 s song, 8 songs of 30 s in one call) the routes alternate, medians of --runs timed runs after --warmup:
  device   Separator.separate_wave_many(waves, images=True): stems and pictures from one call
  plain    Separator.separate_wave_many(waves): the same call without pictures -- device - plain is what asking for them costs
  host     Separator.separate_many(specs) and spectrogram_to_image in numpy on the two stems it returns: how the pictures are had
           without this feature (the spectrograms are formed before the clock starts; this route returns no wave)
and from the launch profiler the two launches' own time with the bytes they must move (the range pass reads spectrogram and mask,
the write pass reads them again and writes two pictures).  The device pictures are compared with the host's before anything is
timed (pixels that differ, largest difference).  One JSON line per workload."""
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


def numpy_image(spec):
    """lib/spec_utils.py:34-57 for a complex [2, bins, T] input, as numpy evaluates it"""
    import numpy as np
    y = np.abs(spec)
    y = np.log10(y * y + np.float32(1e-8))
    y -= y.min()
    y *= np.float32(255) / y.max()
    img = y.astype(np.uint8).transpose(1, 2, 0)
    return np.concatenate([img.max(axis=2, keepdims=True), img], axis=2)


def profiled(vr, model, fn):
    nat, h = vr.native, model._need_handle().h
    nat.check(nat.lib().vr_profile_begin(h))
    try:
        fn()
    finally:
        a, b, c, d = ctypes.c_double(), ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
        nat.check(nat.lib().vr_profile_end(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
    need = nat.lib().vr_profile_report(h, None, 0)
    buf = ctypes.create_string_buffer(int(need) + 1)
    nat.lib().vr_profile_report(h, buf, need)
    out = {}
    for ln in buf.value.decode().splitlines():
        f = ln.split('\t')
        out[f[0]] = {'calls': int(f[1]), 'ms': float(f[2]), 'bytes': float(f[4])}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--runs', type=int, default=10)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--workloads', type=str, default='30,180,8x30')
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

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for w in args.workloads.split(','):
        count, seconds = (int(w.split('x')[0]), float(w.split('x')[1])) if 'x' in w else (1, float(w))
        waves = []
        for k in range(count):
            x = bench.synth_wave(seconds, k)
            waves.append((x / max(1.0, float(np.abs(x).max())) * 0.9).astype(np.float32))
        specs = [vr.spec_utils.wave_to_spectrogram(x, net.hop_length, net.n_fft) for x in waves]
        got = sp.separate_wave_many(waves, images=True)
        stored = sp.separate_many(specs)
        differ = worst = values = 0
        for (_, _, y_img, v_img), (y, v) in zip(got, stored):
            for a, b in ((y_img, numpy_image(y)), (v_img, numpy_image(v))):
                d = np.abs(a[..., 1:].astype(np.int16) - b[..., 1:].astype(np.int16))
                differ += int(np.count_nonzero(d)); worst = max(worst, int(d.max())); values += d.size
        del got, stored

        def device():
            sp.separate_wave_many(waves, images=True)

        def plain():
            sp.separate_wave_many(waves)

        def host():
            for y, v in sp.separate_many(specs):
                numpy_image(y)
                numpy_image(v)

        t = {'device': [], 'plain': [], 'host': []}
        for i in range(args.warmup + args.runs):
            for key, fn in (('device', device), ('plain', plain), ('host', host)):
                ms = timed(fn)
                if i >= args.warmup:
                    t[key].append(ms)
        med = {k: statistics.median(v) for k, v in t.items()}
        rep = profiled(vr, net, device)
        launches = {}
        for name, r in rep.items():
            if 'StemImage' in name:
                key = 'range' if 'mag_pad_kernel' in name else 'write'
                launches[key] = {'us': round(r['ms'] * 1e3, 1), 'mbytes': round(r['bytes'] * 1e-6, 1),
                                 'gb_per_s': round(r['bytes'] / (r['ms'] * 1e-3) * 1e-9, 1) if r['ms'] > 0 else None}
        print(json.dumps({'workload': w, 'songs': count, 'seconds': seconds, 'frames': [int(s.shape[2]) for s in specs][:1],
                          'values': values, 'values_differ': differ, 'largest_difference': worst,
                          'device_ms': round(med['device'], 2), 'plain_ms': round(med['plain'], 2), 'host_ms': round(med['host'], 2),
                          'asking_ms': round(med['device'] - med['plain'], 2),
                          'device_range': [round(min(t['device']), 2), round(max(t['device']), 2)],
                          'plain_range': [round(min(t['plain']), 2), round(max(t['plain']), 2)],
                          'host_range': [round(min(t['host']), 2), round(max(t['host']), 2)],
                          'launches': launches, 'runs': args.runs, 'warmup': args.warmup, 'gpu': torch.cuda.get_device_name(0)}), flush=True)


if __name__ == '__main__':
    main()
