"""The train step of a complex-mask model under its losses (DESIGN.md sections 6n and 6o, profiles/wave_loss.md, profiles/wsdr_loss.md),
and the same step of another build of the project for an A / B comparison.

    python tools/bench_wave_loss.py  [--rounds 3] [--steps 10] [--warmup 3] [--baseline-root DIR]

The default-size net (n_fft 2048, nout 32, nout_lstm 128) as CascadedNet(..., is_complex=True, complex_train=True) with the package's seeded
default initialisation, batch 16, 256 frames, inputs resident on the device, Dropout2d live, the default mfma_mode and train_winograd.
A step is what train_epoch runs per batch: model.train_step(X, y, 1) (it returns the loss, so it ends in a stream synchronisation), the
native Adam step and zero_grad, closed by a device synchronisation and timed with the host clock.

Every measurement runs in a fresh child process, one at a time (a process loads one build of the library).  A child of this tree times
loss kind 0 (VR_LOSS_L1), kind 1 (VR_LOSS_MAG_L1_WAVE_SDR) and kind 3 (VR_LOSS_MAG_L1_WAVE_WSDR), alternating --steps timed steps of each
per inner round after --warmup untimed ones, then profiles one step of kind 1 and one of kind 3 with the library's launch profiler and
reports the kernel forms of the loss per launch.  With --baseline-root (another checkout of the project with its library built, e.g.
the parent commit) a child of THAT tree times the kinds it has, and the children of the two trees alternate --rounds times.  The JSON
line gives per side the median over the rounds of the children's medians and, as *_spread, the lowest and highest round:
`kind0_over_baseline` (and `kind1_over_baseline` where the baseline has kind 1) beside the spreads says whether those steps moved."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BATCH, FRAMES, N_FFT = 16, 256, 2048
NEW_FORMS = ('MagL1', 'WavePair', 'WaveTriple', 'WaveGrad', 'head_bwd_kernel<true>', 'reduce_rows_kernel')
KIND_NAMES = {0: 'l1', 1: 'mag_l1_wave_sdr', 3: 'mag_l1_wave_wsdr'}


def worker(args):
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import ctypes
    import torch
    import __graft_entry__ as entry
    vr = entry.load_package()
    if not torch.cuda.is_available():
        raise SystemExit('bench_wave_loss: needs a GPU (nothing here is measured without one)')
    from vocal_remover_amd import train as vtrain
    dev = torch.device('cuda:0')
    bins = N_FFT // 2 + 1
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(1234)
    model = vr.nets.CascadedNet(N_FFT, N_FFT // 2, 32, 128, is_complex=True, complex_train=True)
    model.to(dev).train()
    X = (torch.complex(torch.randn((BATCH, 2, bins, FRAMES), generator=g), torch.randn((BATCH, 2, bins, FRAMES), generator=g)) * 0.5)
    y = (X * torch.rand((BATCH, 2, bins, FRAMES), generator=g)).to(dev)
    X = X.to(dev)
    opt = vtrain.Adam(model.parameters(), lr=1e-4)
    have = getattr(vr.native, 'LOSS_KINDS', {}) if hasattr(model, 'set_loss') else {}
    kinds = [k for k in (0, 1, 3) if k == 0 or KIND_NAMES[k] in have]

    def select(kind):
        if len(kinds) > 1:
            model.set_loss(KIND_NAMES[kind])

    def steps(n):
        times = []
        for _ in range(n):
            torch.cuda.synchronize()
            t = time.perf_counter()
            model.train_step(X, y, 1)
            opt.step()
            model.zero_grad()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t) * 1e3)
        return times

    for kind in kinds:
        select(kind)
        steps(args.warmup)
    meds = {k: [] for k in kinds}
    for _ in range(args.inner):
        for kind in kinds:
            select(kind)
            meds[kind].append(statistics.median(steps(args.steps)))
    out = {'root': root, 'step_ms': {str(k): round(statistics.median(v), 3) for k, v in meds.items()}}
    for pk in (1, 3):                                     # one profiled step of each wave kind: the forms of the loss per launch
        if pk not in kinds:
            continue
        nat, h = vr.native, model._handle.h
        select(pk)
        nat.check(nat.lib().vr_profile_begin(h))
        try:
            model.train_step(X, y, 1)
        finally:
            a, b, c, d = ctypes.c_double(), ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
            nat.check(nat.lib().vr_profile_end(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)))
        need = nat.lib().vr_profile_report(h, None, 0)
        buf = ctypes.create_string_buffer(int(need) + 1)
        nat.lib().vr_profile_report(h, buf, need)
        launches = []
        for ln in buf.value.decode().splitlines():
            f = ln.split('\t')
            if any(s in f[0] for s in NEW_FORMS):
                calls, ms, byts = int(f[1]), float(f[2]), float(f[4])
                launches.append({'kernel': f[0].replace('vr::', ''), 'calls': calls, 'us_per_call': round(ms * 1e3 / calls, 1),
                                 'noted_MB_per_call': round(byts * 1e-6 / calls, 2),
                                 'GB_per_s': round(byts / calls / (ms * 1e-3 / calls) * 1e-9, 1) if byts and ms else None})
        out['kind%d_launches' % pk] = launches
        out['kind%d_terms' % pk] = model.loss_terms()
    print('BENCH_WAVE_LOSS ' + json.dumps(out), flush=True)
    return 0


def child(root, args):
    cmd = [sys.executable, os.path.abspath(__file__), '--worker', '--root', root, '--steps', str(args.steps), '--warmup', str(args.warmup),
           '--inner', str(args.inner)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
    if r.returncode != 0:            # a failed child ends the run: nothing more is started on the GPU after it
        raise SystemExit('bench_wave_loss: child for %s failed (%d):\n%s' % (root, r.returncode, r.stderr[-4000:]))
    for ln in r.stdout.splitlines():
        if ln.startswith('BENCH_WAVE_LOSS '):
            return json.loads(ln[len('BENCH_WAVE_LOSS '):])
    raise SystemExit('bench_wave_loss: child for %s printed no result' % root)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--inner', type=int, default=3, help='alternations of the two kinds inside one child')
    ap.add_argument('--baseline-root', default=None)
    ap.add_argument('--child-timeout', type=int, default=240)
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--root', default=ROOT)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    mine, base, last = [], [], None
    for _ in range(args.rounds):
        last = child(ROOT, args)
        mine.append(last['step_ms'])
        if args.baseline_root:
            base.append(child(os.path.abspath(args.baseline_root), args)['step_ms'])
    out = {'batch': BATCH, 'frames': FRAMES, 'n_fft': N_FFT, 'rounds': args.rounds, 'inner_rounds': args.inner, 'steps_per_round': args.steps,
           'warmup': args.warmup}

    def put(name, vals):
        out['step_ms_' + name] = round(statistics.median(vals), 3)
        out['step_ms_%s_spread' % name] = [round(min(vals), 3), round(max(vals), 3)]

    for k in ('0', '1', '3'):
        put('kind' + k, [m[k] for m in mine])
    out['kind1_minus_kind0_ms'] = round(out['step_ms_kind1'] - out['step_ms_kind0'], 3)
    out['kind3_minus_kind0_ms'] = round(out['step_ms_kind3'] - out['step_ms_kind0'], 3)
    for k in ('0', '1'):
        if base and all(k in m for m in base):
            put('baseline_kind' + k, [m[k] for m in base])
            out['kind%s_over_baseline' % k] = round(out['step_ms_kind' + k] / out['step_ms_baseline_kind' + k], 4)
    for k in ('1', '3'):
        out['kind%s_launches' % k] = last['kind%s_launches' % k]
        out['kind%s_terms' % k] = last['kind%s_terms' % k]
    print(json.dumps(out), flush=True)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
