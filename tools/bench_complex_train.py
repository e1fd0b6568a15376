"""One train step of a complex-mask model against one of a magnitude model (profiles/complex_train.md).

    python tools/bench_complex_train.py  [--rounds 5] [--steps 10] [--warmup 3]

One process, two default-size nets (n_fft 2048, nout 32, nout_lstm 128) on one GPU: CascadedNet(...) with bench.py's seeded weights and
CascadedNet(..., is_complex=True, complex_train=True) with the package's seeded default initialisation.  Batch 16, 256 frames, inputs
resident on the device, Dropout2d live (the library's generator), the default mfma_mode and train_winograd.  A step is what
train_epoch runs per batch: model.train_step(X, y, 1) (forward, loss, backward; it returns the loss, so it ends in a stream
synchronisation), the native Adam step and zero_grad, closed by a device synchronisation and timed with the host clock.  The two
sides alternate --rounds times, --steps timed steps each after --warmup untimed ones in the first round; a round's figure is the median
of its steps, the JSON line gives the median over the rounds and, as *_spread, the lowest and highest round.  The complex side moves
twice the input bytes (complex64 X and y), packs them into four planes, and its head has four outputs; everything between is the
same executor with Cin = 4 / nout/4 + 4 / 3 nout/4 + 4 at the stage inputs."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BATCH, FRAMES, N_FFT = 16, 256, 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as entry
    import bench
    vr = entry.load_package()
    if not torch.cuda.is_available():
        raise SystemExit('bench_complex_train: needs a GPU (nothing here is measured without one)')
    from vocal_remover_amd import train as vtrain
    dev = torch.device('cuda:0')
    bins = N_FFT // 2 + 1
    g = torch.Generator().manual_seed(0)
    mag, _ = bench.seeded_state(vr)
    mag.to(dev).train()
    torch.manual_seed(1234)
    cplx = vr.nets.CascadedNet(N_FFT, N_FFT // 2, 32, 128, is_complex=True, complex_train=True)
    cplx.to(dev).train()
    Xm = torch.rand((BATCH, 2, bins, FRAMES), generator=g)
    ym = Xm * torch.rand((BATCH, 2, bins, FRAMES), generator=g)
    Xc = torch.complex(torch.randn((BATCH, 2, bins, FRAMES), generator=g), torch.randn((BATCH, 2, bins, FRAMES), generator=g)) * 0.5
    yc = Xc * torch.rand((BATCH, 2, bins, FRAMES), generator=g)
    sides = {'magnitude': (mag, vtrain.Adam(mag.parameters(), lr=1e-4), Xm.to(dev), ym.to(dev)),
             'complex': (cplx, vtrain.Adam(cplx.parameters(), lr=1e-4), Xc.to(dev), yc.to(dev))}
    losses = {k: [] for k in sides}

    def steps(side, n):
        model, opt, X, y = sides[side]
        times = []
        for _ in range(n):
            torch.cuda.synchronize()
            t = time.perf_counter()
            loss = model.train_step(X, y, 1)
            opt.step()
            model.zero_grad()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t) * 1e3)
            losses[side].append(loss)
        return times

    for side in sides:
        steps(side, args.warmup)
    rounds = {k: [] for k in sides}
    for _ in range(args.rounds):
        for side in sides:
            rounds[side].append(statistics.median(steps(side, args.steps)))
    out = {'batch': BATCH, 'frames': FRAMES, 'n_fft': N_FFT, 'rounds': args.rounds, 'steps_per_round': args.steps, 'warmup': args.warmup}
    for side, v in rounds.items():
        out['step_ms_' + side] = round(statistics.median(v), 3)
        out['step_ms_%s_spread' % side] = [round(min(v), 3), round(max(v), 3)]
        out['loss_%s_first_last' % side] = [round(losses[side][0], 6), round(losses[side][-1], 6)]
    out['complex_over_magnitude'] = round(out['step_ms_complex'] / out['step_ms_magnitude'], 4)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
