"""The streamed resampler against the offline call (profiles/resample_stream.md).

    python tools/bench_resample_stream.py [--rounds 5] [--file-seconds 180] [--out profiles/resample_stream.md]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_resample_stream.py --kernel-only      (the kernel's own time)

One process, one MI355X; the sides of every comparison alternate --rounds times; a figure is the median round and (lowest - highest
round), each round the median of --calls timed calls after --warmup calls, every call bracketed by a device synchronisation.
    block   one 2.97 s stereo block at 48 kHz (the input of one roi * hop block at 44.1 kHz) through audio.resample (host arrays; it
            allocates and frees four device buffers per call), through StreamResampler.push with host arrays, and with cuda tensors
    many    16 sessions, one such block each: one resample_push_many call against a loop of 16 push calls (cuda tensors)
    file    stream_file(resample=True) on a --file-seconds 48 kHz WAV against audio.load + separate_wave + audio.write of the same file
            (default-size net, seeded weights, batchsize 4, 1 s blocks)
--kernel-only pushes 50 blocks and exits, for a profiler run of its own."""
import argparse
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BLOCK_48K = 142664            # ceil(131072 * 48000 / 44100)


def timed(fn, sync, warmup, calls):
    out = []
    for i in range(warmup + calls):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def fmt(v):
    return '%.3f (%.3f - %.3f)' % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--file-seconds', type=float, default=180.0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resample_stream.md'))
    ap.add_argument('--kernel-only', action='store_true')
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import __graft_entry__ as entry
    vr = entry.load_package()
    import bench
    audio, inf = vr.audio, vr.inference
    dev = torch.device('cuda:0')
    sync = torch.cuda.synchronize
    rng = np.random.default_rng(0)
    block = (0.1 * rng.standard_normal((2, BLOCK_48K))).astype(np.float32)
    block_d = torch.from_numpy(block).to(dev)
    if args.kernel_only:
        with audio.StreamResampler(48000, 44100, device=dev) as rs:
            for _ in range(50):
                rs.push(block_d)
        sync()
        return 0

    res = {k: [] for k in ('offline', 'push_host', 'push_dev', 'many', 'loop', 'file_stream', 'file_offline')}
    host_rs = audio.StreamResampler(48000, 44100, device=dev)
    dev_rs = audio.StreamResampler(48000, 44100, device=dev)
    sessions = [audio.StreamResampler(48000, 44100, device=dev) for _ in range(16)]
    blocks16 = [block_d] * 16
    for _ in range(args.rounds):
        res['offline'].append(timed(lambda: audio.resample(block, 48000, 44100), sync, args.warmup, args.calls))
        res['push_host'].append(timed(lambda: host_rs.push(block), sync, args.warmup, args.calls))
        res['push_dev'].append(timed(lambda: dev_rs.push(block_d), sync, args.warmup, args.calls))
        res['many'].append(timed(lambda: audio.resample_push_many(sessions, blocks16), sync, args.warmup, args.calls))
        res['loop'].append(timed(lambda: [s.push(b) for s, b in zip(sessions, blocks16)], sync, args.warmup, args.calls))
    state = dev_rs.state_bytes
    for s in [host_rs, dev_rs] + sessions:
        s.close()

    net, _ = bench.seeded_state(vr)
    net.to(dev).eval()
    sp = inf.Separator(net, dev, batchsize=4, cropsize=bench.CROP)
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, 'song48.wav')
        n = int(round(args.file_seconds * 48000))
        t = np.arange(n) / 48000.0
        wave = 0.1 * rng.standard_normal((2, n)) + 0.2 * np.sin(2 * np.pi * 440.0 * t)[None]
        audio.write(src, np.clip(wave, -1, 1).astype(np.float32).T, 48000)
        oy, ov = os.path.join(tmp, 'y.wav'), os.path.join(tmp, 'v.wav')

        def offline():
            X, sr = audio.load(src, sr=44100, mono=False)
            y, v = sp.separate_wave(X)
            audio.write(oy, y.T, sr)
            audio.write(ov, v.T, sr)
        for _ in range(args.rounds):
            res['file_stream'].append(timed(lambda: inf.stream_file(sp, src, oy, ov, 44100, resample=True), sync, 1, 1))
            res['file_offline'].append(timed(offline, sync, 1, 1))

    med = {k: statistics.median(v) for k, v in res.items()}
    lines = ['# The streamed resampler: `StreamResampler` against `audio.resample`', '',
             'Written by `tools/bench_resample_stream.py` (its docstring describes the sides).  One MI355X, one process, the sides alternated',
             '%d times; milliseconds, median round (lowest - highest round); a round is the median of %d calls after %d warm-up calls.'
             % (args.rounds, args.calls, args.warmup), '',
             '## One 2.97 s stereo block at 48 kHz (%d samples in, 131072 out)' % BLOCK_48K, '',
             '| | ms |', '|---|---|',
             '| `audio.resample`, host arrays (four device buffers allocated and freed per call) | %s |' % fmt(res['offline']),
             '| `StreamResampler.push`, host arrays | %s |' % fmt(res['push_host']),
             '| `StreamResampler.push`, cuda tensors | %s |' % fmt(res['push_dev']), '',
             '`Stream.push` of the block this feeds costs 2.61 ms (5.01 ms with tta) on record (`profiles/stream.md`): the device-resident push is',
             '%.1f %% (%.1f %%) of that, and %.2f %% of the 2.97 s block period.  State carried per session: %d bytes.'
             % (100 * med['push_dev'] / 2.613, 100 * med['push_dev'] / 5.011, 100 * med['push_dev'] / 2972.0, state), '',
             '## 16 sessions, one block each (cuda tensors)', '', '| | ms |', '|---|---|',
             '| one `resample_push_many` call | %s |' % fmt(res['many']),
             '| a loop of 16 `push` calls | %s |' % fmt(res['loop']), '',
             'loop / push_many = %.2f.' % (med['loop'] / med['many']), '',
             '## A whole %.0f s file at 48 kHz (default net, batchsize 4, 1 s blocks, WAV in, two WAVs out)' % args.file_seconds, '',
             '| | ms |', '|---|---|',
             '| `stream_file(resample=True)` | %s |' % fmt(res['file_stream']),
             '| `audio.load(sr=44100)` + `separate_wave` + `audio.write` | %s |' % fmt(res['file_offline']), '',
             'stream / offline = %.2f.  The streamed side reads and resamples the file twice (normaliser pass, separating pass) and runs the'
             % (med['file_stream'] / med['file_offline']),
             'network in one-block pushes; it never holds more than one block.']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
