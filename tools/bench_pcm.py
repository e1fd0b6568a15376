"""File-to-file wall time of the single-file command-line path, old route against new (profiles/pcm_device.md).

    python tools/bench_pcm.py [--runs 10] [--warmup 3] [--seconds 30]

One process, default-size net, seeded weights, a synthetic 44.1 kHz stereo WAV (bench.py's audio) written once as PCM16 and once as
PCM24, batchsize 4, cropsize 256.  Per file the two routes alternate, --runs timed runs each after --warmup runs, medians reported:
  offline  old: audio.load -> Separator.separate_wave -> audio.write x2      new: audio.read_wav_raw -> separate_pcm -> audio.write_pcm16 x2
  stream   inference.stream_file with 1 s blocks, pcm16=False against pcm16=True (the input side is the float path in both)
`io_ms` is the part of a route that is file I/O alone: reading the input's bytes and writing two stems' bytes, timed on their own.
The two routes' stems are compared byte for byte before anything is timed.  One JSON line per (file, mode)."""
import argparse
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
    audio, inference = vr.audio, vr.inference
    dev = torch.device('cuda:0')
    net, _ = bench.seeded_state(vr)
    net.to(dev).eval()
    sp = inference.Separator(net, dev, batchsize=4, cropsize=bench.CROP)
    sr = 44100
    wave = bench.synth_wave(args.seconds, 0)
    wave = (wave / max(1.0, float(np.abs(wave).max())) * 0.9).astype(np.float32)
    tmp = tempfile.mkdtemp(prefix='bench_pcm_')
    files = {'pcm16': os.path.join(tmp, 'in16.wav'), 'pcm24': os.path.join(tmp, 'in24.wav')}
    audio.write(files['pcm16'], wave.T, sr)
    v24 = np.rint(wave.T.astype(np.float64) * (1 << 23)).astype('<i4').reshape(-1)
    body = np.ascontiguousarray(v24.view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()
    with open(files['pcm24'], 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', 36 + len(body)) + b'WAVE')
        f.write(b'fmt ' + struct.pack('<IHHIIHH', 16, 1, 2, sr, sr * 6, 6, 24))
        f.write(b'data' + struct.pack('<I', len(body)) + body)
    out = [os.path.join(tmp, n) for n in ('old_y.wav', 'old_v.wav', 'new_y.wav', 'new_v.wav')]

    def old_offline(path):
        X, _ = audio.load(path, sr=sr, mono=False, dtype=np.float32, res_type='kaiser_fast')
        y, v = sp.separate_wave(X)
        audio.write(out[0], y.T, sr)
        audio.write(out[1], v.T, sr)

    def new_offline(path):
        y, v = sp.separate_pcm(audio.read_wav_raw(path))
        audio.write_pcm16(out[2], y, sr)
        audio.write_pcm16(out[3], v, sr)

    def old_stream(path):
        inference.stream_file(sp, path, out[0], out[1], sr, block_seconds=1.0)

    def new_stream(path):
        inference.stream_file(sp, path, out[2], out[3], sr, block_seconds=1.0, pcm16=True)

    def io_only(path):
        with open(path, 'rb') as f:
            f.read()
        stem = open(out[0], 'rb').read()
        for o in out[:2]:
            with open(o, 'wb') as f:
                f.write(stem)

    def timed(fn, path):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(path)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name, path in files.items():
        for mode, old, new in (('offline', old_offline, new_offline), ('stream', old_stream, new_stream)):
            old(path)
            new(path)
            same = all(open(a, 'rb').read() == open(b, 'rb').read() for a, b in ((out[0], out[2]), (out[1], out[3])))
            t = {'old': [], 'new': [], 'io': []}
            for i in range(args.warmup + args.runs):
                for key, fn in (('old', old), ('new', new), ('io', io_only)):
                    ms = timed(fn, path)
                    if i >= args.warmup:
                        t[key].append(ms)
            med = {k: statistics.median(v) for k, v in t.items()}
            print(json.dumps({'file': name, 'mode': mode, 'seconds': args.seconds, 'stems_identical': same,
                              'old_ms': round(med['old'], 2), 'new_ms': round(med['new'], 2), 'io_ms': round(med['io'], 2),
                              'old_range': [round(min(t['old']), 2), round(max(t['old']), 2)],
                              'new_range': [round(min(t['new']), 2), round(max(t['new']), 2)],
                              'io_share_old': round(med['io'] / med['old'], 3), 'io_share_new': round(med['io'] / med['new'], 3),
                              'runs': args.runs, 'warmup': args.warmup, 'gpu': torch.cuda.get_device_name(0)}), flush=True)
    for o in out + list(files.values()):
        if os.path.exists(o):
            os.remove(o)
    os.rmdir(tmp)


if __name__ == '__main__':
    main()
