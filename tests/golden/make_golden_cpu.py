"""Generate tests/golden/reference_cpu.npz: what the REFERENCE's own Python returns for the CPU tests that pin the oracle and the
host-side code against it (tests/test_oracle_vs_reference.py, test_cpu_host.py, test_cpu_frontend.py), so that those tests need no
reference checkout.

Usage (CPU only):  python tests/golden/make_golden_cpu.py PATH_TO_REFERENCE_CHECKOUT
Every input is rebuilt from the tests' own seeded helpers, so test and fixture see the same data."""
import contextlib
import json
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [ROOT, TESTS]


@contextlib.contextmanager
def _cwd(path):
    old = os.getcwd()
    os.chdir(path)
    try:
        yield
    finally:
        os.chdir(old)


def main(reference):
    for name in ('librosa', 'soundfile', 'cv2'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['cv2'].IMREAD_COLOR = 1
    sys.path.insert(0, reference)
    import lib.dataset as ref_ds        # noqa: E402  (reference package `lib`)
    import lib.nets as ref_nets
    import lib.spec_utils as ref_spec
    import inference as ref_inference
    from oracle import weights
    import test_cpu_frontend
    import test_cpu_host
    import test_oracle_vs_reference as tovr

    out = {}
    # state_dict keys and shapes of the default net
    sd = ref_nets.CascadedNet(2048, 1024, 32, 128).state_dict()
    out['spec_json'] = np.array(json.dumps([[k, list(v.shape)] for k, v in sd.items()]))

    # Separator.separate / separate_tta of the small net (tests/test_oracle_vs_reference.py::small_sd).  Its outputs are
    # y = mask * |X| * exp(i angle X) and v = (1 - mask) * |X| * exp(i angle X): the mask is stored, quantised to 1/SEP_Q, as two
    # byte planes, together with the largest distance (relative to max|X|) between the outputs rebuilt from it and the real ones
    ref = ref_nets.CascadedNet(512, 256, 8, 32)
    ref.load_state_dict(weights.make_state_dict(7, n_fft=512, nout=8, nout_lstm=32))
    ref.eval()
    rng = np.random.default_rng(0)
    T = 300
    X_spec = (rng.standard_normal((2, 257, T)) + 1j * rng.standard_normal((2, 257, T))).astype(np.complex64)
    M = float(np.abs(X_spec).max())
    sp = ref_inference.Separator(ref, torch.device('cpu'), batchsize=2, cropsize=160)
    sp.offset = 64
    bound = 0.0
    for tta in (False, True):
        y, v = (sp.separate_tta if tta else sp.separate)(X_spec.copy())
        k = np.round((y / X_spec).real * tovr.SEP_Q).astype(np.uint16)
        hi, lo = (k >> 8).astype(np.uint8), (k & 255).astype(np.uint8)
        out['separate_mask_hi_%d' % tta], out['separate_mask_lo_%d' % tta] = hi, lo
        ry, rv = tovr.separation_from_mask(hi, lo, X_spec)
        bound = max(bound, float(np.abs(ry - y).max()) / M, float(np.abs(rv - v).max()) / M)
    assert bound < 0.4e-4, bound          # leaves the oracle (1e-4 - 2 bound) * max|X| of room
    out['separate_bound'] = np.float64(bound * 1.01)

    # VocalRemoverTrainingSet samples and the random numbers they consume
    with tempfile.TemporaryDirectory() as tmp:
        ts = tovr._synthetic_training_set(_P(tmp))
        rw = tovr._reduction_weight(33)
        ds = ref_ds.VocalRemoverTrainingSet(ts * 2, cropsize=32, reduction_rate=0.5, reduction_weight=rw, mixup_rate=0.5, mixup_alpha=0.4)
        digests, nxt = [], []
        for seed in range(24):
            np.random.seed(seed)
            X, y = ds[seed % len(ds)]
            digests.append([test_cpu_frontend._patch_digest(X), test_cpu_frontend._patch_digest(y)]), nxt.append(np.random.uniform())
        out['trainset_json'], out['trainset_next'] = np.array(json.dumps(digests)), np.array(nxt)
        ds = ref_ds.VocalRemoverTrainingSet(ts, 32, 0.5, rw, 0.5, 0.4)
        nxt = []
        for seed in range(16):
            np.random.seed(seed)
            ds[seed % 3]
            nxt.append(np.random.uniform())
        out['plan_next'] = np.array(nxt)

    # lib/spec_utils.merge_artifacts
    for name, fmin in sorted(test_cpu_host.MERGE_CASES.items()):
        out['merge_' + name] = ref_spec.merge_artifacts(test_cpu_host._mask_from_frame_min(fmin(400).astype(np.float32)))
    try:
        ref_spec.merge_artifacts(test_cpu_host._mask_from_frame_min(np.zeros(300, np.float32)))
        out['merge_all_below_raises'] = np.array(False)
    except IndexError:
        out['merge_all_below_raises'] = np.array(True)

    # dataset preparation on a fake spectrogram cache; paths relative to the cache root
    with tempfile.TemporaryDirectory() as tmp:
        sr, hop, n_fft = 44100, 256, 512
        root = test_cpu_frontend._fake_cache(_P(tmp), sr, hop, n_fft)
        rel = lambda p: os.path.relpath(p, root)           # noqa: E731
        with _cwd(tmp):
            pairs = ref_ds.make_pair(root + '/mixtures', root + '/instruments')
            random.seed(3)
            train, val = ref_ds.train_val_split(root, 'random', 0.34, [])
            tset = ref_ds.make_training_set(train, sr, hop, n_fft)
            os.makedirs('ref')
            with _cwd('ref'):
                patches = ref_ds.make_validation_set(val + train[:1], 160, sr, hop, n_fft, 64)
                digests = [[test_cpu_frontend._patch_digest(z['X']), test_cpu_frontend._patch_digest(z['y'])] for z in map(np.load, patches)]
        out['prep_json'] = np.array(json.dumps({
            'pairs': [[rel(a), rel(b)] for a, b in pairs], 'train': [[rel(a), rel(b)] for a, b in train],
            'val': [[rel(a), rel(b)] for a, b in val], 'training_set': [[rel(a), rel(b), float(c)] for a, b, c in tset],
            'patches': list(patches), 'patch_digests': digests}))
    path = os.path.join(HERE, 'reference_cpu.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, '%.2f MB' % (os.path.getsize(path) / 1e6))


class _P(str):
    """A str path that also joins with `/` like pytest's tmp_path (the tests' helpers use both)."""
    def __truediv__(self, p):
        return _P(os.path.join(self, p))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))
