"""What streaming --postprocess costs (profiles/stream_post.md).

    python tools/bench_stream_post.py [--parent-tree DIR] [--rounds 5] [--calls 20] [--song-seconds 180] [--out profiles/stream_post.md]

One MI355X, default-size net, seeded weights, bench.py's synthetic audio, device-resident input and output, cropsize 256.
  parent      a steady push of roi * hop samples (2.97 s at 44.1 kHz) into a PLAIN stream, batchsize 1, on this tree and on a built
              checkout of the parent commit (--parent-tree): one fresh process per side and round, the sides alternating; median of the
              rounds' medians and the lowest / highest round.  The plain stream must stay inside the parent's own spread.
  post        the same push into a plain and into a postprocess stream of this tree, plain and tta, alternating in one process: the
              difference is the cost of the two new launches and of the blend in the masked iSTFT.
  song        a --song-seconds song in pushes of 16 blocks (batchsize 4) through a postprocess stream against one offline
              separate_wave with postprocess, and the same pair without postprocess.
  state       vr_stream_info's state_bytes with and without the flag.
--side NAME is the child mode of `parent`: it times the plain push on the tree given by --tree and prints one JSON line.
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


def timed(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(rounds):
    return {'median': round(statistics.median(rounds), 4), 'low': round(min(rounds), 4), 'high': round(max(rounds), 4)}


def fmt(s):
    return '%.3f (%.3f - %.3f)' % (s['median'], s['low'], s['high'])


def load(tree):
    sys.path.insert(0, tree)
    import torch
    import __graft_entry__ as entry
    vr = entry.load_package()
    import bench
    dev = torch.device('cuda:0')
    net, _ = bench.seeded_state(vr)
    net.to(dev).eval()
    return torch, vr, bench, dev, net


def steady_stream(sp, blocks, warm, **kw):
    s = sp.stream(**kw)
    for k in range(warm):
        s.push(blocks[k])
    return s


def side(args):
    """child: the steady plain push on --tree"""
    torch, vr, bench, dev, net = load(os.path.abspath(args.tree))
    hop, crop = net.hop_length, bench.CROP
    block = (crop - 2 * net.offset) * hop
    song = torch.from_numpy(bench.synth_wave(60.0, 0)).to(dev)
    blocks = [song[:, k * block:(k + 1) * block].contiguous() for k in range(song.shape[1] // block)]
    sp = vr.inference.Separator(net, dev, batchsize=1, cropsize=crop)
    s = steady_stream(sp, blocks, 8, coef=sp.measure_coef([song]))
    ts = [timed(lambda: s.push(blocks[(8 + i) % len(blocks)]), torch) for i in range(args.calls + 5)][5:]
    s.close()
    print(json.dumps({'side': args.side, 'ms': statistics.median(ts)}), flush=True)
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent-tree', default=None)
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--calls', type=int, default=20)
    p.add_argument('--song-seconds', type=float, default=180.0)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stream_post.md'))
    p.add_argument('--side', default=None)
    p.add_argument('--tree', default=ROOT)
    args = p.parse_args()
    if args.side:
        return side(args)
    lines = ['# Streaming --postprocess: what the look-ahead costs', '',
             'One MI355X, default net (2048 / 1024, nout 32, nout_lstm 128), seeded weights, `bench.py`\'s synthetic audio, cropsize 256,',
             'device-resident input and output; `python tools/bench_stream_post.py%s --rounds %d --calls %d`.  Milliseconds, median of the'
             % (' --parent-tree <built checkout of the parent commit>' if args.parent_tree else '', args.rounds, args.calls),
             'rounds (lowest - highest round).', '']
    # ---- this tree against the parent commit: fresh processes, alternating
    res = {'this': [], 'parent': []}
    trees = [('this', ROOT)] + ([('parent', os.path.abspath(args.parent_tree))] if args.parent_tree else [])
    for r in range(args.rounds):
        for name, tree in (trees if r % 2 == 0 else trees[::-1]):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--side', name, '--tree', tree, '--calls', str(args.calls)],
                                 capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit('side %s failed:\n%s' % (name, out.stderr[-3000:]))
            res[name].append(json.loads(out.stdout.strip().splitlines()[-1])['ms'])
            print(json.dumps({'what': 'parent', 'round': r, 'side': name, 'ms': res[name][-1]}), flush=True)
    lines += ['## A steady 2.97 s push of a plain stream, this commit against its parent', '',
              'One fresh process per side and round, the sides alternating; batchsize 1.', '',
              '| side | ms per push |', '|---|---|', '| this commit | %s |' % fmt(spread(res['this']))]
    if res['parent']:
        sp_, st_ = spread(res['parent']), spread(res['this'])
        lines += ['| parent commit | %s |' % fmt(sp_), '',
                  'The medians differ by %+.2f %%; the parent\'s own rounds span %.2f %% of its median.'
                  % (100.0 * (st_['median'] / sp_['median'] - 1.0), 100.0 * (sp_['high'] - sp_['low']) / sp_['median'])]
    else:
        lines += ['', 'No parent tree was given: the parent side was not measured.']
    lines.append('')
    # ---- plain against postprocess streams of this tree
    torch, vr, bench, dev, net = load(ROOT)
    hop, crop = net.hop_length, bench.CROP
    block = (crop - 2 * net.offset) * hop
    song = torch.from_numpy(bench.synth_wave(args.song_seconds, 0)).to(dev)
    blocks = [song[:, k * block:(k + 1) * block].contiguous() for k in range(song.shape[1] // block)]
    sp = vr.inference.Separator(net, dev, batchsize=1, cropsize=crop)
    lines += ['## The same push into a postprocess stream', '', 'One process, the two streams alternating; batchsize 1.', '',
              '| | plain stream | postprocess stream | difference of the medians |', '|---|---|---|---|']
    cost = {}
    for tta in (False, True):
        coef = sp.measure_coef([song], tta=tta)
        a = steady_stream(sp, blocks, 12, coef=coef, tta=tta)
        b = steady_stream(sp, blocks, 12, coef=coef, tta=tta, postprocess=True)
        ra, rb, at = [], [], 12
        for _ in range(args.rounds):
            for s, dst in ((a, ra), (b, rb)):
                dst.append(statistics.median([timed(lambda: s.push(blocks[(at + i) % len(blocks)]), torch) for i in range(args.calls)]))
            at += args.calls
        a.close()
        b.close()
        cost[tta] = statistics.median(rb) - statistics.median(ra)
        print(json.dumps({'what': 'post', 'tta': tta, 'ms_plain': spread(ra), 'ms_post': spread(rb)}), flush=True)
        lines.append('| %s | %s | %s | %+.3f ms |' % ('tta' if tta else 'plain', fmt(spread(ra)), fmt(spread(rb)), cost[tta]))
    lines.append('')
    # ---- a whole song
    sp4 = vr.inference.Separator(net, dev, batchsize=4, cropsize=crop)
    spp = vr.inference.Separator(net, dev, batchsize=4, cropsize=crop, postprocess=True)
    coef = sp4.measure_coef([song])

    def run_stream(post):
        with sp4.stream(coef=coef, postprocess=post) as s:
            for i in range(0, song.shape[1], 16 * block):
                s.push(song[:, i:i + 16 * block])
            s.flush()
    offline_post = True
    try:
        spp.separate_wave(song)
    except IndexError:                                   # no frame of this input above merge_artifacts' threshold: the reference's error
        offline_post = False
    res = {'off': [], 'off_post': [], 'st': [], 'st_post': []}
    run_stream(False)
    run_stream(True)
    for _ in range(args.rounds):
        res['off'].append(timed(lambda: sp4.separate_wave(song), torch))
        if offline_post:
            res['off_post'].append(timed(lambda: spp.separate_wave(song), torch))
        res['st'].append(timed(lambda: run_stream(False), torch))
        res['st_post'].append(timed(lambda: run_stream(True), torch))
    print(json.dumps({'what': 'song', 'seconds': args.song_seconds, **{k: spread(v) for k, v in res.items() if v}}), flush=True)
    lines += ['## A %g s song, pushes of 16 blocks, batchsize 4' % args.song_seconds, '', '| | ms |', '|---|---|',
              '| offline `separate_wave` | %s |' % fmt(spread(res['off'])),
              '| offline `separate_wave`, postprocess | %s |' % (fmt(spread(res['off_post'])) if offline_post else
                                                                 'raises the reference\'s IndexError: no frame of this input is above the threshold'),
              '| stream | %s |' % fmt(spread(res['st'])), '| stream, postprocess | %s |' % fmt(spread(res['st_post'])), '']
    # ---- state
    lines += ['## State of one stream (`vr_stream_info`)', '', '| batchsize | flags | state bytes |', '|---|---|---|']
    for bs in (1, 4):
        spb = vr.inference.Separator(net, dev, batchsize=bs, cropsize=crop)
        for tta in (False, True):
            for post in (False, True):
                with spb.stream(coef=1.0 + 0j if tta else 1.0, tta=tta, postprocess=post) as s:
                    lines.append('| %d | %s | %d (%.1f MiB) |' % (bs, ' + '.join(n for n, on in (('tta', tta), ('postprocess', post)) if on) or 'plain',
                                                                   s.state_bytes, s.state_bytes / 2.0 ** 20))
                    if post and not tta and bs == 1:
                        look = s.lookahead_samples
    lines += ['', 'Look-ahead of a postprocess stream: %d samples = %.2f s at 44.1 kHz (plain: %d samples).' % (look, look / 44100.0, look - 161 * hop), '']
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines))
    print('wrote', args.out)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
