"""Many songs per call against a loop of one-song calls (profiles/separate_many.md).

    python tools/bench_many.py --yardstick-tree <checkout of the parent commit, built>  [--rounds 3] [--configs 16x5,8x30,4x180]

For every configuration (songs x seconds, without and with --tta) one JSON line
    {songs, seconds_per_song, tta, ms_loop, ms_many, songs_per_s_loop, songs_per_s_many, ...}
where ms_loop is a Python loop of Separator.separate_wave over the songs, run by the library of --yardstick-tree (default: this
tree), and ms_many is ONE Separator.separate_wave_many call of this tree over the same songs.  Default-size net, seeded weights,
bench.py's synthetic audio, device-resident input and output, the same --batchsize on both sides.  Every measurement is a child
process of its own under `timeout`: median of --calls timed calls after --warmup warm-up calls, each call bracketed by a device
synchronisation.  The two sides alternate --rounds times (boxes and runs differ by about +-2 %); the line carries the median over the
rounds and, as *_spread, the lowest and highest round.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def child(args):
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import torch
    import __graft_entry__ as entry
    vr = entry.load_package()
    sys.path.insert(0, ROOT)
    import bench                                    # the audio recipe and the seeded weights of the flagship benchmark
    dev = torch.device('cuda:0')
    net, _ = bench.seeded_state(vr)
    net.to(dev).eval()
    sp = vr.inference.Separator(net, dev, batchsize=args.batchsize, cropsize=bench.CROP)
    waves = [torch.from_numpy(bench.synth_wave(args.seconds, k)).to(dev) for k in range(args.songs)]
    if args.mode == 'many':
        call = lambda: sp.separate_wave_many(waves, tta=args.tta)
    else:
        call = lambda: [sp.separate_wave(w, tta=args.tta) for w in waves]
    times = []
    for i in range(args.warmup + args.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if i >= args.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({'mode': args.mode, 'ms': statistics.median(times), 'ms_min': min(times), 'calls': len(times)}))
    return 0


def measure(args, mode, songs, seconds, tta):
    tree = os.path.abspath(args.yardstick_tree) if mode == 'loop' else ROOT
    cmd = ['timeout', '-k', '10', str(args.step_timeout), sys.executable, os.path.abspath(__file__), '--child', '--mode', mode,
           '--tree', tree, '--songs', str(songs), '--seconds', str(seconds), '--batchsize', str(args.batchsize),
           '--warmup', str(args.warmup), '--calls', str(args.calls)] + (['--tta'] if tta else [])
    env = dict(os.environ)
    env.pop('VR_LIB_PATH', None)
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=tree)
    if r.returncode != 0:
        # nothing more is started on the GPU after a step that failed, hung or faulted
        raise SystemExit('bench_many: %s step failed (exit %d), stopping:\n%s' % (mode, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])['ms']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--yardstick-tree', default=ROOT, help='a built checkout of the commit to compare the loop of one-song calls from')
    ap.add_argument('--configs', default='16x5,8x30,4x180', help='songs x seconds per song')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batchsize', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--step-timeout', type=int, default=240)
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--mode', choices=('loop', 'many'))
    ap.add_argument('--tree', default=ROOT)
    ap.add_argument('--songs', type=int)
    ap.add_argument('--seconds', type=float)
    ap.add_argument('--tta', action='store_true')
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.warmup < 3 or args.calls < 10:
        raise SystemExit('at least 3 warm-up and 10 timed calls')
    for cfg in args.configs.split(','):
        songs, seconds = cfg.split('x')
        songs, seconds = int(songs), float(seconds)
        for tta in (False, True):
            loop, many = [], []
            for _ in range(args.rounds):
                loop.append(measure(args, 'loop', songs, seconds, tta))
                many.append(measure(args, 'many', songs, seconds, tta))
            ms_loop, ms_many = statistics.median(loop), statistics.median(many)
            print(json.dumps({'songs': songs, 'seconds_per_song': seconds, 'tta': tta, 'ms_loop': round(ms_loop, 3),
                              'ms_many': round(ms_many, 3), 'songs_per_s_loop': round(songs / ms_loop * 1e3, 2),
                              'songs_per_s_many': round(songs / ms_many * 1e3, 2), 'batchsize': args.batchsize,
                              'ms_loop_spread': [round(min(loop), 3), round(max(loop), 3)],
                              'ms_many_spread': [round(min(many), 3), round(max(many), 3)], 'rounds': args.rounds}), flush=True)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
