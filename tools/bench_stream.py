"""Streaming separation against the offline entry point (profiles/stream.md).

    python tools/bench_stream.py [--rounds 5] [--calls 20] [--song-seconds 180] [--hour]

One process, default-size net, seeded weights, bench.py's synthetic audio, device-resident input and output, cropsize 256.  The two
sides of every comparison alternate --rounds times; a JSON line carries the median over the rounds and the lowest / highest round.
  latency     one steady-state push of roi * hop samples (batchsize 1; plain and tta) against the only block-wise use the offline entry
              point allows: separate_wave on the (cropsize - 1) * hop samples around that block.
  throughput  a --song-seconds song through pushes of 1, 4 and 16 blocks (batchsize 4) against one separate_wave call.
  memory      (--hour) device bytes the handle holds -- staging arena + workspace, and the stream's state -- after one hour of audio
              through a stream, and after separate_wave of the same hour.
"""
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


def timed(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(rounds):
    return {'median': round(statistics.median(rounds), 4), 'low': round(min(rounds), 4), 'high': round(max(rounds), 4)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--calls', type=int, default=20)
    p.add_argument('--song-seconds', type=float, default=180.0)
    p.add_argument('--hour', action='store_true')
    args = p.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as entry
    vr = entry.load_package()
    import bench
    dev = torch.device('cuda:0')
    net, _ = bench.seeded_state(vr)
    net.to(dev).eval()
    hop, crop, offset = net.hop_length, bench.CROP, net.offset
    roi = crop - 2 * offset
    block = roi * hop

    def arena():
        a, b = ctypes.c_int64(), ctypes.c_int64()
        vr.native.check(vr.native.lib().vr_arena_bytes(net._handle.h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    song = torch.from_numpy(bench.synth_wave(args.song_seconds, 0)).to(dev)
    # ---- latency of one block
    for tta in (False, True):
        sp = vr.inference.Separator(net, dev, batchsize=1, cropsize=crop)
        coef = sp.measure_coef([song], tta=tta)
        window = song[:, 20 * block:20 * block + (crop - 1) * hop].contiguous()
        blocks = [song[:, k * block:(k + 1) * block].contiguous() for k in range(song.shape[1] // block)]
        s = sp.stream(coef=coef, tta=tta)
        at = 0
        for _ in range(6):                                   # past the look-ahead: every further push readies one crop per pass
            s.push(blocks[at]); at += 1
        sp.separate_wave(window, tta=tta)
        r_stream, r_window = [], []
        for _ in range(args.rounds):
            ts = []
            for _ in range(args.calls):
                b = blocks[at % len(blocks)]; at += 1
                ts.append(timed(lambda: s.push(b), torch))
            r_stream.append(statistics.median(ts))
            r_window.append(statistics.median([timed(lambda: sp.separate_wave(window, tta=tta), torch) for _ in range(args.calls)]))
        s.close()
        print(json.dumps({'what': 'latency', 'tta': tta, 'block_samples': block, 'window_samples': int(window.shape[1]),
                          'ms_stream_push': spread(r_stream), 'ms_window_call': spread(r_window)}), flush=True)
    # ---- throughput over a whole song
    sp = vr.inference.Separator(net, dev, batchsize=4, cropsize=crop)
    for tta in (False, True):
        coef = sp.measure_coef([song], tta=tta)

        def run_stream(k):
            with sp.stream(coef=coef, tta=tta) as s:
                for i in range(0, song.shape[1], k * block):
                    s.push(song[:, i:i + k * block])
                s.flush()
        res = {'offline': [], 1: [], 4: [], 16: []}
        sp.separate_wave(song, tta=tta)
        run_stream(4)
        for _ in range(args.rounds):
            res['offline'].append(timed(lambda: sp.separate_wave(song, tta=tta), torch))
            for k in (1, 4, 16):
                res[k].append(timed(lambda: run_stream(k), torch))
        off = statistics.median(res['offline'])
        print(json.dumps({'what': 'throughput', 'tta': tta, 'seconds': args.song_seconds, 'batchsize': 4, 'ms_offline': spread(res['offline']),
                          'ms_stream': {str(k): spread(res[k]) for k in (1, 4, 16)},
                          'stream_over_offline': {str(k): round(statistics.median(res[k]) / off, 3) for k in (1, 4, 16)}}), flush=True)
    del song
    # ---- memory for one hour
    if args.hour:
        net2, _ = bench.seeded_state(vr)                     # a fresh handle: its arenas have seen nothing else
        net2.to(dev).eval()
        sp2 = vr.inference.Separator(net2, dev, batchsize=4, cropsize=crop)
        minute = torch.from_numpy(bench.synth_wave(60.0, 1)).to(dev)

        def arena2():
            a, b = ctypes.c_int64(), ctypes.c_int64()
            vr.native.check(vr.native.lib().vr_arena_bytes(net2._handle.h, ctypes.byref(a), ctypes.byref(b)))
            return int(a.value), int(b.value)
        with sp2.stream(coef=30.0) as s:
            t = timed(lambda: [s.push(minute[:, i:i + 4 * block]) for _ in range(60) for i in range(0, minute.shape[1], 4 * block)], torch)
            st, (io_b, ws_b) = s.state_bytes, arena2()
            s.flush()
        print(json.dumps({'what': 'memory', 'side': 'stream', 'seconds': 3600, 'state_bytes': st, 'staging_bytes': io_b, 'workspace_bytes': ws_b,
                          'total_mib': round((st + io_b + ws_b) / 2 ** 20, 1), 'ms': round(t, 1)}), flush=True)
        hour = minute.repeat(1, 60)
        t = timed(lambda: sp2.separate_wave(hour), torch)
        io_b, ws_b = arena2()
        print(json.dumps({'what': 'memory', 'side': 'separate_wave', 'seconds': 3600, 'staging_bytes': io_b, 'workspace_bytes': ws_b,
                          'total_mib': round((io_b + ws_b) / 2 ** 20, 1), 'input_mib': round(hour.numel() * 4 / 2 ** 20, 1),
                          'output_mib': round(2 * hour.numel() * 4 / 2 ** 20, 1), 'ms': round(t, 1)}), flush=True)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
