"""The wave sets against the rows sets at sizes a user runs (profiles/resident_waves.md): batch() of ResidentWaveTrainingSet (float waves
and the files' PCM16 frames) against ResidentTrainingSet.batch() in one process, alternating; one DeviceLoader iteration plus train step;
the device bytes of both stores; the time from a file list to the end of the first batch on each route (the cache cold and warm); one
validation pass.  --batches N: only N wave batches, for a kernel trace of its own.  Prints one JSON line; --out also writes it to a file.

    python tools/bench_dataset_waves.py --songs 16 --seconds 180 --out result.json
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402

SR, N_FFT, HOP = 44100, 2048, 1024


def synth_files(folder, songs, seconds):
    """PCM16 stereo pairs: noise under a slow envelope, the mixture = instrumental + vocals"""
    vr = __graft_entry__.load_package()
    n = int(SR * seconds)
    files = []
    for k in range(songs):
        rng = np.random.default_rng(k)
        env = (0.6 + 0.4 * np.sin(np.arange(n) / 30000.0 + k)).astype(np.float32)
        inst = (0.2 * rng.standard_normal((2, n), dtype=np.float32)) * env
        mix = inst + 0.1 * rng.standard_normal((2, n), dtype=np.float32)
        paths = (os.path.join(folder, 'song%02d_mix.wav' % k), os.path.join(folder, 'song%02d_inst.wav' % k))
        vr.audio.write(paths[0], mix.T, SR)
        vr.audio.write(paths[1], inst.T, SR)
        files.append(paths)
    return files


def spread(ms):
    ms = sorted(ms)
    return {'median_ms': round(ms[len(ms) // 2], 3), 'min_ms': round(ms[0], 3), 'max_ms': round(ms[-1], 3), 'n': len(ms)}


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--songs', type=int, default=16)
    ap.add_argument('--seconds', type=float, default=180.0)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--cropsize', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--batches', type=int, default=0, help='only this many wave batches (for a kernel trace)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    vr = __graft_entry__.load_package()
    ds_mod = vr.dataset
    dev = torch.device('cuda:0')
    model = vr.nets.CascadedNet(N_FFT, HOP, 32, 128)
    model.to(dev)
    bins = N_FFT // 2 + 1
    rw = np.linspace(1.0, 0.2, bins).astype(np.float32)
    kw = dict(cropsize=args.cropsize, reduction_rate=0.5, reduction_weight=rw, mixup_rate=0.5, mixup_alpha=0.4, model=model)
    idx = list(range(args.batch))
    res = {'songs': args.songs, 'seconds': args.seconds, 'B': args.batch, 'T': args.cropsize, 'n_fft': N_FFT, 'hop': HOP}
    folder = tempfile.mkdtemp(prefix='bench_waves_')
    try:
        files = synth_files(folder, args.songs, args.seconds)
        listed = (files * (args.batch // len(files) + 1))[:max(args.batch, len(files))]

        def first_batch(make_rows, cls):
            def run():
                ds = cls(make_rows(), **kw)
                np.random.seed(0)
                ds.batch(idx)
                return ds
            return timed(run)

        if args.batches:
            ds, _ = first_batch(lambda: ds_mod.load_wave_rows(listed, SR, pairs_per_call=4), ds_mod.ResidentWaveTrainingSet)
            for _ in range(args.batches):
                ds.batch(idx)
            print(json.dumps({'wave_batches': args.batches}))
            return
        # ---- from the file list to the end of the first batch
        waves, t = first_batch(lambda: ds_mod.load_wave_rows(listed, SR, pairs_per_call=4), ds_mod.ResidentWaveTrainingSet)
        res['first_batch_wave_float_s'] = round(t / 1e3, 2)
        pcm, t = first_batch(lambda: ds_mod.load_wave_rows(listed, SR, pairs_per_call=4, pcm=True), ds_mod.ResidentWaveTrainingSet)
        res['first_batch_wave_pcm16_s'] = round(t / 1e3, 2)
        cache_rows = lambda: ds_mod.make_training_set(listed, SR, HOP, N_FFT, peaks=False, pairs_per_call=4)
        rows, t = first_batch(cache_rows, ds_mod.ResidentTrainingSet)
        res['first_batch_cache_cold_s'] = round(t / 1e3, 2)
        rows.close()
        rows, t = first_batch(cache_rows, ds_mod.ResidentTrainingSet)
        res['first_batch_cache_warm_s'] = round(t / 1e3, 2)
        res['device_bytes'] = {'rows': rows.nbytes, 'wave_float': waves.nbytes, 'wave_pcm16': pcm.nbytes}
        print(json.dumps(res), flush=True)
        # ---- batch(), the three routes alternating
        sets = {'rows': rows, 'wave_float': waves, 'wave_pcm16': pcm}
        ms = {k: [] for k in sets}
        for r in range(args.rounds + 3):
            for name, ds in sets.items():
                np.random.seed(r)
                _, t = timed(lambda: ds.batch(idx))
                if r >= 3:
                    ms[name].append(t)
        res['batch'] = {k: spread(v) for k, v in ms.items()}
        print(json.dumps(res['batch']), flush=True)
        # ---- one loader iteration plus the train step
        model.train()
        ms = {k: [] for k in ('rows', 'wave_float')}
        for r in range(args.steps + 2):
            for name in ms:
                def step():
                    np.random.seed(r)
                    X, y = sets[name].batch(idx)
                    model.zero_grad()
                    model.train_step(X, y, 1)
                _, t = timed(step)
                if r >= 2:
                    ms[name].append(t)
        res['iteration_plus_train_step'] = {k: spread(v) for k, v in ms.items()}
        print(json.dumps(res['iteration_plus_train_step']), flush=True)
        # ---- one validation pass over two songs
        model.eval()
        val_files = files[:2]
        vw = ds_mod.ResidentWaveValidationSet(ds_mod.load_wave_rows(val_files, SR, pairs_per_call=2), args.cropsize, model.offset, model=model)
        vs = ds_mod.ResidentSongValidationSet(ds_mod.make_training_set(val_files, SR, HOP, N_FFT, peaks=False), args.cropsize, model.offset,
                                              model=model)
        out = {}
        for name, ds in (('rows', vs), ('wave_float', vw)):
            ds.batch([0])                                           # (the upload and the peaks)
            passes = []
            for _ in range(3):
                _, t = timed(lambda: [ds.batch(list(range(i, min(i + args.batch, len(ds))))) for i in range(0, len(ds), args.batch)])
                passes.append(t)
            out[name] = dict(spread(passes), windows=len(ds))
        res['validation_pass_batches_only'] = out
        for ds in (rows, waves, pcm, vw, vs):
            ds.close()
    finally:
        shutil.rmtree(folder, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
