"""Wall time of the streaming route with the file's bytes in against the decoded route (profiles/pcm_stream.md).

    python tools/bench_pcm_stream.py [--runs 10] [--warmup 3] [--seconds 30]

One process, default-size net, seeded weights, bench.py's synthetic audio, batchsize 4, cropsize 256, pcm16 stems.  Per case the two routes
alternate, --runs timed runs each after --warmup runs, medians and ranges reported; the margin of a comparison is the spread of the
pcm_in=False runs themselves.  The two routes' outputs are compared byte for byte before anything is timed.
  stream_file    a 44.1 kHz stereo file with 1 s blocks as PCM16, PCM24 and float32; the same audio as a 48 kHz PCM24 file (resampler)
  stream_files   8 such 44.1 kHz PCM16 files in one group, and 8 48 kHz PCM24 files
  push           one 2.97 s block (131072 frames) per Stream.push / Stream.push_pcm, from host memory and from device memory
Last, the kernel times of the two new instantiations from the launch profiler (vr_profile_report) beside their float forms.
One JSON line per case."""
import argparse
import ctypes
import json
import os
import statistics
import struct
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def write_wav(path, tag, ch, sr, bits, body):
    align = ch * bits // 8
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', 36 + len(body)) + b'WAVE')
        f.write(b'fmt ' + struct.pack('<IHHIIHH', 16, tag, ch, sr, sr * align, align, bits))
        f.write(b'data' + struct.pack('<I', len(body)) + body)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--runs', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--seconds', type=float, default=30.0)
    args = p.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as entry
    vr = entry.load_package()
    import bench
    audio, inference, nat = vr.audio, vr.inference, vr.native
    dev = torch.device('cuda:0')
    net, _ = bench.seeded_state(vr)
    net.to(dev).eval()
    sp = inference.Separator(net, dev, batchsize=4, cropsize=bench.CROP)
    sr = 44100
    wave = bench.synth_wave(args.seconds, 0)
    wave = (wave / max(1.0, float(np.abs(wave).max())) * 0.9).astype(np.float32)
    tmp = tempfile.mkdtemp(prefix='bench_pcm_stream_')

    def s24(x):
        v = np.rint(x.T.astype(np.float64) * (1 << 23)).astype('<i4').reshape(-1)
        return np.ascontiguousarray(v.view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()

    files = {}
    for name, tag, bits, body in (('pcm16', 1, 16, np.rint(wave.T * 32767.0).astype('<i2').tobytes()), ('pcm24', 1, 24, s24(wave)),
                                  ('float32', 3, 32, np.ascontiguousarray(wave.T).astype('<f4').tobytes())):
        files[name] = os.path.join(tmp, name + '.wav')
        write_wav(files[name], tag, 2, sr, bits, body)
    n48 = int(wave.shape[1] * 48000 // sr)
    files['pcm24_48k'] = os.path.join(tmp, 'pcm24_48k.wav')
    write_wav(files['pcm24_48k'], 1, 2, 48000, 24, s24(wave[:, :n48] if n48 <= wave.shape[1] else np.pad(wave, ((0, 0), (0, n48 - wave.shape[1])), mode='wrap')))
    outs = {k: [os.path.join(tmp, '%s_%s_%d.wav' % (k, s, i)) for i in range(8) for s in 'yv'] for k in ('old', 'new')}

    def one(path, key, pcm_in):
        inference.stream_file(sp, path, outs[key][0], outs[key][1], sr, block_seconds=1.0, resample=True, pcm16=True, pcm_in=pcm_in)

    def group(path, key, pcm_in):
        o = outs[key]
        inference.stream_files(sp, [path] * 8, [(o[2 * i], o[2 * i + 1]) for i in range(8)], sr, block_seconds=1.0, resample=True, pcm16=True,
                               pcm_in=pcm_in)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def compare(case, old, new, same):
        old(); new()
        ok = bool(same())
        t = {'old': [], 'new': []}
        for i in range(args.warmup + args.runs):
            for key, fn in (('old', old), ('new', new)):
                ms = timed(fn)
                if i >= args.warmup:
                    t[key].append(ms)
        med = {k: statistics.median(v) for k, v in t.items()}
        spread = max(t['old']) - min(t['old'])
        verdict = 'equal' if abs(med['new'] - med['old']) <= spread else ('faster' if med['new'] < med['old'] else 'slower')
        print(json.dumps(dict(case, identical=ok, old_ms=round(med['old'], 3), new_ms=round(med['new'], 3),
                              old_range=[round(min(t['old']), 3), round(max(t['old']), 3)], new_range=[round(min(t['new']), 3), round(max(t['new']), 3)],
                              byte_route=verdict, runs=args.runs, warmup=args.warmup, gpu=torch.cuda.get_device_name(0))), flush=True)

    def files_same(n):
        return lambda: all(open(a, 'rb').read() == open(b, 'rb').read() for a, b in zip(outs['old'][:n], outs['new'][:n]))

    for name, path in files.items():
        compare({'mode': 'stream_file', 'file': name, 'seconds': args.seconds}, lambda: one(path, 'old', False), lambda: one(path, 'new', True),
                files_same(2))
    for name in ('pcm16', 'pcm24_48k'):
        path = files[name]
        compare({'mode': 'stream_files', 'file': name, 'files': 8, 'seconds': args.seconds}, lambda: group(path, 'old', False),
                lambda: group(path, 'new', True), files_same(16))

    # ---- one block per push: the steady state of a live source
    n_blk = 131072
    blk = np.ascontiguousarray(wave[:, :n_blk])
    coef = sp.measure_coef([wave])
    last = {}
    for name, fmt, body in (('pcm16', nat.VR_PCM_S16, np.rint(blk.T * 32767.0).astype('<i2').tobytes()), ('pcm24', nat.VR_PCM_S24, s24(blk))):
        data = np.frombuffer(body, np.uint8).copy()
        dec = np.empty((2, n_blk), np.float32)
        nat.check(nat.lib().vr_pcm_convert_host(fmt, data.ctypes.data, n_blk, 2, nat.np_ptr(dec)))
        for where in ('host', 'device'):
            xf = torch.from_numpy(dec).to(dev) if where == 'device' else dec
            raw = audio.RawPcm(torch.from_numpy(data).to(dev) if where == 'device' else data, fmt, 2, sr, n_blk)
            with sp.stream(coef=coef, pcm16=True) as sf, sp.stream(coef=coef, pcm16=True) as sq:
                def old():
                    last['old'] = sf.push(xf)

                def new():
                    last['new'] = sq.push_pcm(raw)
                compare({'mode': 'push', 'file': name, 'from': where, 'frames': n_blk}, old, new,
                        lambda: all(bytes(a.cpu().numpy().tobytes() if torch.is_tensor(a) else a.tobytes()) ==
                                    bytes(b.cpu().numpy().tobytes() if torch.is_tensor(b) else b.tobytes()) for a, b in zip(last['old'], last['new'])))

    # ---- kernel times of the new instantiations beside their float forms
    def profiled(fn):
        h = net._handle.h
        nat.check(nat.lib().vr_profile_begin(h))
        try:
            fn()
        finally:
            a, b, c, d = ctypes.c_double(), ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
            nat.check(nat.lib().vr_profile_end(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
        need = nat.lib().vr_profile_report(h, None, 0)
        buf = ctypes.create_string_buffer(int(need) + 1)
        nat.lib().vr_profile_report(h, buf, need)
        return [ln for ln in buf.value.decode().splitlines() if 'stft_tile_kernel' in ln or 'resample_kernel' in ln]

    data = np.frombuffer(s24(blk), np.uint8).copy()
    raw = audio.RawPcm(torch.from_numpy(data).to(dev), nat.VR_PCM_S24, 2, 48000, n_blk)
    xf = torch.from_numpy(blk).to(dev)
    with sp.stream(coef=coef) as sf, sp.stream(coef=coef) as sq, audio.StreamResampler(48000, sr, 2) as rf, audio.StreamResampler(48000, sr, 2) as rq:
        for s, r, arg, push in ((sf, rf, xf, 'push'), (sq, rq, raw, 'push_pcm')):
            for _ in range(3):
                getattr(s, push)(arg)
                getattr(r, push)(arg)
            print(json.dumps({'mode': 'kernels', 'call': push, 'frames': n_blk,
                              'report': profiled(lambda: (getattr(s, push)(arg), getattr(r, push)(arg)))}), flush=True)
    for root, _, names in os.walk(tmp):
        for n in names:
            os.remove(os.path.join(root, n))
    os.rmdir(tmp)


if __name__ == '__main__':
    main()
