"""Plain training pairs: the host route against spec_utils.prepare_pair_many (profiles/prepare_pair.md).

    python tools/bench_prepare.py  [--reps 3] [--out FILE.json] [--dry]

One process, decoded host arrays in (float32 [2, L] at 44.1 kHz, n_fft 2048, hop 1024): synthetic stems -- white noise with a slow
envelope, the mixture the instrumental plus weaker noise -- with exact-zero silence in front of the mixture and behind the instrumental
and a few hundred samples of offset, so that trim, lag and window all do something.  Every figure is a host clock around work that ends
in a device synchronisation, repeated --reps times, reported as the median and, as *_spread, the lowest and highest repetition.

    stage_ms           one 30 s pair through vr_align_pair_many and vr_pair_rows_many under the library's launch profiler: milliseconds
                       per kernel (HIP events around every launch); align_call_ms / both_calls_ms: the wall time of the first call
                       and of the two together, from host arrays to host arrays and (*_device_in_out) from cuda tensors to cuda tensors
    per_lag_call_ms    vr_xcorr_argmax on the same two heads: xcorr_full_kernel's arithmetic, one workgroup per lag, with its
                       copies (2.1 MB) and its host scan -- what the lag search costs without the tiled form
    host_s / device_s  16 x 30 s and 4 x 180 s pairs: align_wave_head_and_tail (audio.trim twice, vr_xcorr_argmax), two
                       wave_to_spectrogram calls and dataset._song_peak per pair, against one prepare_pair_many call of all pairs
The two routes' windows, rows and peaks are compared bit for bit on every pair; a difference is an error (exit status 1)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SR, HOP, N_FFT = 44100, 1024, 2048


def make_pairs(np, count, seconds, seed):
    rng = np.random.default_rng(seed)
    n = seconds * SR
    base = rng.standard_normal((2, n + 4096), dtype=np.float32)
    voc = rng.standard_normal((2, n + 4096), dtype=np.float32)
    env = (0.08 + 0.04 * np.sin(np.arange(n + 4096, dtype=np.float32) * np.float32(2e-5))).astype(np.float32)
    pairs = []
    for i in range(count):
        q, p = 97 * i % 1500, 211 * i % 1300                        # the content offsets: lag p - q before trimming
        inst = np.roll(base, 1013 * i, axis=1) * env
        mix = inst + np.float32(0.3) * np.roll(voc, 577 * i, axis=1) * env
        lead, tail = 3000 + 700 * (i % 3), 2500 + 900 * (i % 2)
        m = np.concatenate([np.zeros((2, lead), np.float32), mix[:, q:q + n - lead]], axis=1)
        y = np.concatenate([inst[:, p:p + n - tail], np.zeros((2, tail), np.float32)], axis=1)
        pairs.append((np.ascontiguousarray(m), np.ascontiguousarray(y)))
    return pairs


def med(values):
    return statistics.median(values), [min(values), max(values)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--dry', action='store_true')
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import __graft_entry__ as entry
    vr = entry.load_package()
    nat, su, ds = vr.native, vr.spec_utils, vr.dataset
    if args.dry:
        m, y = make_pairs(np, 1, 2, 0)[0]
        print(json.dumps({'dry': True, 'pair_shape': [list(m.shape), list(y.shape)]}))
        return 0
    import torch
    res = {'sr': SR, 'hop': HOP, 'n_fft': N_FFT, 'reps': args.reps, 'device': torch.cuda.get_device_name(0)}

    def host_route(m, y):
        a, b = su.align_wave_head_and_tail(m, y, SR)
        X, Y = su.wave_to_spectrogram(a, HOP, N_FFT), su.wave_to_spectrogram(b, HOP, N_FFT)
        return X, Y, ds._song_peak(X, Y)

    # ---- the stage split of one 30 s pair --------------------------------------------------------------------------------------
    (m, y), = make_pairs(np, 1, 30, 1)
    su.prepare_pair_many([m], [y], SR, HOP, N_FFT)                    # warm: handle, FFT plan, code objects
    h = su._signal_handle(N_FFT, HOP)
    md, yd = torch.from_numpy(m).cuda(), torch.from_numpy(y).cuda()
    su.prepare_pair_many([md], [yd], SR, HOP, N_FFT)
    for tag, a, b in (('', m, y), ('_device_in_out', md, yd)):        # host arrays in and out; cuda tensors in and out (no PCIe copies)
        t_align, t_both = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            w = su.align_pair_many([a], [b], SR)
            t1 = time.perf_counter()
            su.prepare_pair_many([a], [b], SR, HOP, N_FFT)            # the align call again, then the rows call
            t2 = time.perf_counter()
            t_align.append((t1 - t0) * 1e3)
            t_both.append((t2 - t1) * 1e3)
        res['align_call_ms' + tag], res['align_call_ms' + tag + '_spread'] = med(t_align)
        res['both_calls_ms' + tag], res['both_calls_ms' + tag + '_spread'] = med(t_both)
    del md, yd
    nat.check(nat.lib().vr_profile_begin(h.h))
    try:
        su.prepare_pair_many([m], [y], SR, HOP, N_FFT)
    finally:
        a, b, c, d = ctypes.c_double(), ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
        nat.check(nat.lib().vr_profile_end(h.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
    need = nat.lib().vr_profile_report(h.h, None, 0)
    buf = ctypes.create_string_buffer(int(need) + 1)
    nat.lib().vr_profile_report(h.h, buf, need)
    stages = {}
    for ln in buf.value.decode().splitlines():
        f = ln.split('\t')
        if len(f) >= 3:
            stages[f[0].replace('vr::', '')] = {'calls': int(f[1]), 'ms': float(f[2])}
    res['stage_ms'] = stages
    lag_ms = sum(v['ms'] for k, v in stages.items() if 'XcorrTile' in k)
    res['lag_search_share_of_kernels'] = lag_ms / max(sum(v['ms'] for v in stages.values()), 1e-9)
    res['window_30s'] = w[0].as_dict()
    # xcorr_full_kernel's arithmetic on the same heads
    heads = []
    for wave, s, e in ((m, w[0].a_start, w[0].a_end), (y, w[0].b_start, w[0].b_end)):
        hd = wave[:, s:e][:, :4 * SR].sum(axis=0)
        heads.append(np.ascontiguousarray(hd - hd.mean(), dtype=np.float32))
    t = []
    k = ctypes.c_int64()
    for _ in range(args.reps):
        t0 = time.perf_counter()
        nat.check(nat.lib().vr_xcorr_argmax(0, nat.np_ptr(heads[0]), len(heads[0]), nat.np_ptr(heads[1]), len(heads[1]), ctypes.byref(k)))
        t.append((time.perf_counter() - t0) * 1e3)
    res['per_lag_call_ms'], res['per_lag_call_ms_spread'] = med(t)
    res['per_lag_lag'] = int(k.value) - (len(heads[0]) - 1)
    ok = res['per_lag_lag'] == w[0].lag

    # ---- the host route against one call ----------------------------------------------------------------------------------------
    for count, seconds in ((16, 30), (4, 180)):
        pairs = make_pairs(np, count, seconds, 10 + seconds)
        key = '%dx%ds' % (count, seconds)
        th, td = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            host = [host_route(m, y) for m, y in pairs]
            t1 = time.perf_counter()
            Xs, ys, peaks, wins = su.prepare_pair_many([m for m, _ in pairs], [y for _, y in pairs], SR, HOP, N_FFT)
            t2 = time.perf_counter()
            th.append(t1 - t0)
            td.append(t2 - t1)
        res[key + '_host_s'], res[key + '_host_s_spread'] = med(th)
        res[key + '_device_s'], res[key + '_device_s_spread'] = med(td)
        res[key + '_rows_bytes'] = int(sum(X.nbytes + y.nbytes for X, y in zip(Xs, ys)))
        for (X, Y, pk), Xr, yr, pr in zip(host, Xs, ys, peaks):
            same = (np.ascontiguousarray(X.transpose(2, 0, 1)).tobytes() == Xr.tobytes() and
                    np.ascontiguousarray(Y.transpose(2, 0, 1)).tobytes() == yr.tobytes() and np.float32(pk).tobytes() == pr.tobytes())
            ok = ok and same
        res[key + '_lags'] = [int(x.lag) for x in wins]
        del host, Xs, ys
    res['routes_agree'] = bool(ok)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    raise SystemExit(main())
