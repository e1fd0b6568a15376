"""N live streams per block period: one push_many call against a loop of N push calls (profiles/stream_many.md).

    python tools/bench_stream_many.py --yardstick-lib <libvr_mi355.so built from the parent commit> [--rounds 5] [--out profiles/stream_many.md]

Three sides, default-size net, seeded weights, bench.py's synthetic audio, device-resident input and output, streams opened with
--batchsize (16), one roi * hop block per stream and period, steady state (the look-ahead is filled before anything is timed):
    a  the library of --yardstick-lib (the parent commit's build) running a Python loop of N Stream.push calls
    b  this tree's library, ONE Separator.push_many call over the N streams
    c  this tree's library running the same loop of N Stream.push calls
for N in --streams (1, 4, 16), without and with --tta.  A measurement is a child process of its own under `timeout` that opens 16
streams once and times every (N, tta) on them: median of --calls periods after --warmup periods, each period bracketed by a device
synchronisation.  The sides alternate a, b, c for --rounds rounds in one visit (boxes and runs differ by a few per cent); the report
carries the median over the rounds and the lowest and highest round of every side, the ratios a / b and c / a, and the device memory
16 streams hold.  It states for every row whether b lies below a by more than the spread (highest b round below lowest a round) and
whether c lies within the spread of a (the two ranges of rounds overlap).
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
    sys.path.insert(0, ROOT)
    import ctypes

    import torch
    import __graft_entry__ as entry
    vr = entry.load_package()
    import bench                                    # the audio recipe and the seeded weights of the flagship benchmark
    if args.side == 'a' and not hasattr(ctypes.CDLL(vr.native.LIB_PATH), 'vr_stream_push_many'):
        vr.native._SIGNATURES.pop('vr_stream_push_many')         # the parent's library: the binding table follows what it exports
    dev = torch.device('cuda:0')
    net, _ = bench.seeded_state(vr)
    net.to(dev).eval()
    sp = vr.inference.Separator(net, dev, batchsize=args.batchsize, cropsize=bench.CROP)
    counts = [int(n) for n in args.streams.split(',')]
    res = {'side': args.side, 'rows': []}
    for tta in (False, True):
        probe = sp.stream(coef=1.0, tta=tta)
        block = probe.block_samples
        probe.close()
        waves = [torch.from_numpy(bench.synth_wave(block * (args.warmup + 1) / 44100.0 + 0.1, k)).to(dev) for k in range(max(counts))]
        coefs = [sp.measure_coef([w], tta=tta) for w in waves]
        for n in counts:
            streams = [sp.stream(coef=c, tta=tta) for c in coefs[:n]]
            blocks = lambda i: [w[:, (i % (args.warmup + 1)) * block:(i % (args.warmup + 1) + 1) * block].contiguous() for w in waves[:n]]
            if args.side == 'b':
                period = lambda b: sp.push_many(streams, b)
            else:
                period = lambda b: [s.push(x) for s, x in zip(streams, b)]
            times = []
            for i in range(args.warmup + args.calls):
                b = blocks(i)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = period(b)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    times.append((time.perf_counter() - t0) * 1e3)
                    assert all(int(y.shape[1]) == block for y, _ in out), 'not in steady state'
            row = {'streams': n, 'tta': tta, 'ms': statistics.median(times), 'ms_min': min(times), 'calls': len(times)}
            if n == max(counts):
                a, w = ctypes.c_int64(), ctypes.c_int64()
                vr.native.check(vr.native.lib().vr_arena_bytes(net._handle.h, ctypes.byref(a), ctypes.byref(w)))
                row.update(state_bytes=sum(s.state_bytes for s in streams), staging_bytes=int(a.value), workspace_bytes=int(w.value))
            for s in streams:
                s.close()
            res['rows'].append(row)
    print(json.dumps(res))
    return 0


def measure(args, side):
    cmd = ['timeout', '-k', '10', str(args.step_timeout), sys.executable, os.path.abspath(__file__), '--child', '--side', side,
           '--streams', args.streams, '--batchsize', str(args.batchsize), '--warmup', str(args.warmup), '--calls', str(args.calls)]
    env = dict(os.environ)
    env.pop('VR_LIB_PATH', None)
    if side == 'a':
        env['VR_LIB_PATH'] = os.path.abspath(args.yardstick_lib)
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT)
    if r.returncode != 0:
        # nothing more is started on the GPU after a step that failed, hung or faulted
        raise SystemExit('bench_stream_many: side %s failed (exit %d), stopping:\n%s' % (side, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])['rows']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--yardstick-lib', help="libvr_mi355.so of the parent commit's build (side a)")
    ap.add_argument('--streams', default='1,4,16')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batchsize', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--step-timeout', type=int, default=170)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stream_many.md'))
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--side', choices=('a', 'b', 'c'))
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.yardstick_lib or not os.path.exists(args.yardstick_lib):
        raise SystemExit("--yardstick-lib: the parent commit's libvr_mi355.so is needed for side a")
    if args.rounds < 5 or args.warmup < 3 or args.calls < 10:
        raise SystemExit('at least 5 rounds, 3 warm-up and 10 timed periods')
    runs = {'a': [], 'b': [], 'c': []}
    for r in range(args.rounds):
        for side in ('a', 'b', 'c'):
            runs[side].append(measure(args, side))
            print('round %d side %s: %s' % (r, side, ' '.join('%dx%s %.3f' % (x['streams'], 'tta' if x['tta'] else 'plain', x['ms'])
                                                                for x in runs[side][-1])), flush=True)
    lines = ['# N live streams per block period: push_many against a loop of push calls', '',
             'Written by `tools/bench_stream_many.py` (its docstring describes the three sides).  One MI355X, default net, cropsize 256,',
             'streams opened with batchsize %d, call batchsize %d, one roi * hop block (%d frames) per stream and period, device-resident'
             % (args.batchsize, args.batchsize, 128),
             'input and output, steady state.  Milliseconds per period: median over %d alternating rounds [lowest round, highest round];'
             % args.rounds,
             'a round is the median of %d periods after %d warm-up periods.' % (args.calls, args.warmup), '',
             '| streams | tta | a: parent build, loop of push | b: push_many | c: this build, loop of push | a / b | c / a | b below a by more than the spread | c within the spread of a |',
             '|---|---|---|---|---|---|---|---|---|']
    mem = None
    tail = ['', 'With one stream `push_many` is `push` with a table of one entry: the rows of N = 1 are expected to tie, the comparison that matters is '
            'N = 4 and N = 16.']
    for i, row in enumerate(runs['a'][0]):
        ms = {s: [run[i]['ms'] for run in runs[s]] for s in runs}
        med = {s: statistics.median(v) for s, v in ms.items()}
        fmt = lambda s: '%.3f [%.3f, %.3f]' % (med[s], min(ms[s]), max(ms[s]))
        below = max(ms['b']) < min(ms['a'])
        within = min(ms['c']) <= max(ms['a']) and min(ms['a']) <= max(ms['c'])
        lines.append('| %d | %s | %s | %s | %s | %.2f | %.3f | %s | %s |' % (row['streams'], 'yes' if row['tta'] else 'no', fmt('a'), fmt('b'), fmt('c'),
                                                                         med['a'] / med['b'], med['c'] / med['a'], 'yes' if below else 'NO',
                                                                         'yes' if within else 'NO'))
        print(json.dumps({'streams': row['streams'], 'tta': row['tta'], 'ms_a': ms['a'], 'ms_b': ms['b'], 'ms_c': ms['c']}), flush=True)
        if 'state_bytes' in runs['b'][0][i]:
            mem = runs['b'][0][i]
    lines += tail
    if mem:
        lines += ['', 'Device memory with %d tta streams open (side b): stream state %.1f MB in all, the handle\'s staging arena %.1f MB, its network '
                  'workspace %.1f MB.' % (mem['streams'], mem['state_bytes'] / 1e6, mem['staging_bytes'] / 1e6, mem['workspace_bytes'] / 1e6)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
