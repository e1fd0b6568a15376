"""Remix and mono augmentation on the device: the AugDescEx forms of augment_kernel through the four _ex entry
points and the three training classes.  The dense form against tests/remix_ref.py at the project's 3e-6 bar for this kernel; rows store,
wave store and dense form against one another bit for bit; the _ex entry points without a new bit against the old ones, bit for bit;
the identity remix; mono's equal channels; what is refused; and a short training run.

Shapes: T = 40 and 37 bins for the dense and rows forms (both cross a 32-tile edge, 37 is odd), n_fft 128 = 65 bins for the wave store, 3
songs of 50-70 rows.  The seeded batches of the classes have B = 6; the descriptor batch has one sample per case of the list below, which
is more than six."""
import collections
import ctypes
import types

import numpy as np
import pytest
import torch

import remix_ref as ref
import wave_set_ref as wref
from oracle import weights
from test_gpu_resident import _profiled, _same_state
from test_oracle_vs_reference import _reduction_weight, _synthetic_training_set

pytestmark = pytest.mark.gpu

T, N_FFT, HOP = 40, 128, 64
LENGTHS = (50, 61, 70)
BAR = 3e-6
REMIX, MONO, MIX_MONO = 128, 256, 512

S = collections.namedtuple('S', 'song start flags psong pstart lam gy gv', defaults=(-1, 0, 1.0, 1.0, 1.0))
# one batch's descriptors: every case the kernel tells apart, crops at the first row and ending on the last row among them
SAMPLES = [
    S(0, 3, 0),                                                     # plain
    S(1, 0, REMIX, 2, 30, gy=0.625, gv=0.9),                        # remix (the partner's crop ends on its song's last row)
    S(2, 30, REMIX | 2 | 32, 0, 10, gy=0.9, gv=0.55),               # remix with both swaps
    S(0, 10, REMIX | 1, 1, 21, gy=0.7, gv=1.0),                     # remix on a sample with reduce
    S(1, 5, REMIX | 4, 0, 0, gy=1.0, gv=0.5),                       # remix on a sample with inst-only: X is rebuilt from g_y y
    S(2, 7, MONO),                                                  # mono
    S(0, 0, MONO | 2),                                              # mono + swap
    S(1, 11, 8 | MIX_MONO | 32, 2, 4, lam=0.3),                     # mixup whose partner is mono (and swapped)
    S(2, 0, 8 | 16, 1, 2, lam=0.75),                                # plain mixup (its partner reduced)
    S(0, 9, REMIX | MONO | 1 | 32, 2, 13, gy=0.5, gv=0.8),          # everything a remixed sample can carry
]
OLD_ONLY = [S(0, 3, 1 | 2), S(1, 0, 8 | 16 | 64, 2, 30, lam=0.25), S(2, 30, 4 | 8 | 32, 0, 10, lam=0.6), S(1, 21, 0)]


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.fixture(scope='module')
def model(vr):
    return wref.signal_model(vr, N_FFT, HOP)


@pytest.fixture(scope='module')
def case37(vr, tmp_path_factory):
    """37 bins: synthetic cached rows (exact zeros among them), their rows store."""
    ts = _synthetic_training_set(tmp_path_factory.mktemp('remix37'), bins=37, lengths=LENGTHS)
    rows = [(np.load(r[0]), np.load(r[1]), r[2]) for r in ts]
    store = vr.native.Dataset(0, 37)
    for X, y, _ in rows:
        store.add(X, y)
    yield dict(ts=ts, rows=rows, bins=37, rw=_reduction_weight(37), stores=dict(rows=store))
    store.close()


@pytest.fixture(scope='module')
def case65(vr, tmp_path_factory):
    """65 bins: three songs as waves, the rows of the whole waves, caches of those rows, a rows store and a wave store of them."""
    pairs = [wref.make_pair(HOP * (n - 1) + 9 * k, 70 + k) for k, n in enumerate(LENGTHS)]
    rows = [wref.pair_rows(vr, mix, inst, N_FFT, HOP) for mix, inst in pairs]
    assert [r[0].shape for r in rows] == [(n, 2, 65) for n in LENGTHS]
    by_mix = {id(mix): r for (mix, _), r in zip(pairs, rows)}
    ts = wref.write_caches(tmp_path_factory.mktemp('remix65'), pairs, lambda mix, inst: by_mix[id(mix)])
    rs, ws = vr.native.Dataset(0, 65), vr.native.Dataset.waves(0, N_FFT, HOP)
    for (mix, inst), (X, y, _) in zip(pairs, rows):
        rs.add(X, y)
        ws.add_waves(mix, inst)
    yield dict(ts=ts, rows=rows, pairs=pairs, bins=65, rw=_reduction_weight(65), stores=dict(rows=rs, waves=ws))
    rs.close()
    ws.close()


def _call(vr, model, case, form, samples, complex_output, ex=True, rw=True, sentinel=-7.0):
    """One raw call of the dense entry point ('dense') or of the store's ('rows', 'waves') -> (rc, vr_last_error, X, y)"""
    nat, h = vr.native, model._need_handle()
    B, bins = len(samples), case['bins']
    Desc = vr.dataset._AugEx if ex else vr.dataset._Aug
    desc = (Desc * B)()
    for b, s in enumerate(samples):
        coef_mix = case['rows'][s.psong][2] if s.psong >= 0 and s.psong < len(case['rows']) else 1.0
        f = (case['rows'][s.song][2], coef_mix, s.lam, s.flags)
        desc[b] = Desc(*(f + (s.gy, s.gv))) if ex else Desc(*f)
    dtype = torch.complex64 if complex_output else torch.float32
    X = torch.full((B, 2, bins, T), sentinel, dtype=dtype, device='cuda:0')
    y = torch.full((B, 2, bins, T), sentinel, dtype=dtype, device='cuda:0')
    rwp = nat.np_ptr(case['rw']) if rw else None
    name = ('vr_augment_batch' if form == 'dense' else 'vr_dataset_batch') + ('_complex' if complex_output else '') + ('_ex' if ex else '')
    fn = getattr(nat.lib(), name)
    if form == 'dense':
        a = [np.zeros((B, T, 2, bins), np.complex64) for _ in range(4)]
        partners = False
        for b, s in enumerate(samples):
            a[0][b], a[1][b] = (r[s.start:s.start + T] for r in case['rows'][s.song][:2])
            if s.psong >= 0:
                partners = True
                a[2][b], a[3][b] = (r[s.pstart:s.pstart + T] for r in case['rows'][s.psong][:2])
        rc = fn(h.h, nat.np_ptr(a[0]), nat.np_ptr(a[1]), nat.np_ptr(a[2]) if partners else None, nat.np_ptr(a[3]) if partners else None,
                ctypes.cast(desc, ctypes.c_void_p), rwp, B, T, bins, 0, ctypes.c_void_p(X.data_ptr()), ctypes.c_void_p(y.data_ptr()), 1)
    else:
        crops = (nat.Crop * B)(*[nat.Crop(s.song, s.psong, s.start, s.pstart) for s in samples])
        rc = fn(h.h, case['stores'][form].d, ctypes.cast(crops, ctypes.c_void_p), ctypes.cast(desc, ctypes.c_void_p), rwp, B, T,
                ctypes.c_void_p(X.data_ptr()), ctypes.c_void_p(y.data_ptr()), 1)
    return rc, nat.lib().vr_last_error().decode(), X, y


def _ref_plan(s):
    """a sample of this file in remix_ref.draw's terms"""
    p = dict(idx=s.song, start=s.start, flags=s.flags & (7 | MONO), remix=None, mix=None)
    if s.flags & REMIX:
        p['remix'] = dict(idx=s.psong, start=s.pstart, swap=bool(s.flags & 32), gain_y=s.gy, gain_v=s.gv)
    elif s.flags & 8:
        p['mix'] = dict(idx=s.psong, start=s.pstart, flags=((s.flags >> 4) & 7) | (MONO if s.flags & MIX_MONO else 0), lam=s.lam)
    return p


def _ref_batch(case, samples, complex_output):
    crop = lambda k, start: (case['rows'][k][0][start:start + T], case['rows'][k][1][start:start + T])
    return [ref.render(crop, lambda k: case['rows'][k][2], _ref_plan(s), case['rw'], complex_output) for s in samples]


def _check_against(got, want, what):
    """every element within BAR * max|ref|, of X and of y each by its own maximum"""
    for name, g, w in (('X', got[0], want[0]), ('y', got[1], want[1])):
        scale = float(np.abs(w).max())
        err = float(np.abs(g - w).max())
        print('%s %s: max error %.3e of max|ref| %.3e (%.2e of it)' % (what, name, err, scale, err / scale))
        assert err <= BAR * scale, (what, name, err, scale)


@pytest.fixture(scope='module')
def want37(case37):
    """remix_ref's batch of SAMPLES, computed once: {complex_output: [(X, y)]}"""
    return {c: _ref_batch(case37, SAMPLES, c) for c in (False, True)}


# ---- 1. the kernel against the numpy statement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('complex_output', (False, True))
def test_dense_form_against_remix_ref(vr, model, case37, want37, complex_output):
    rc, err, X, y = _call(vr, model, case37, 'dense', SAMPLES, complex_output)
    assert rc == 0, err
    X, y = X.cpu().numpy(), y.cpu().numpy()
    assert X.dtype == (np.complex64 if complex_output else np.float32)
    for b, (s, want) in enumerate(zip(SAMPLES, want37[complex_output])):
        _check_against((X[b], y[b]), want, 'sample %d (flags %d)' % (b, s.flags))
    # mono: the two channels hold the same bits, in X and in y
    for b, s in enumerate(SAMPLES):
        if s.flags & MONO and not s.flags & REMIX:
            assert X[b, 0].tobytes() == X[b, 1].tobytes() and y[b, 0].tobytes() == y[b, 1].tobytes(), b
            assert np.abs(X[b]).max() > 0
        elif s.flags & MONO:                                        # the remix adds a stereo partner to X; y stays mono
            assert y[b, 0].tobytes() == y[b, 1].tobytes() and X[b, 0].tobytes() != X[b, 1].tobytes(), b
        else:
            assert X[b, 0].tobytes() != X[b, 1].tobytes(), b
    # the rows store gives the dense form's bytes
    rc, err, Xr, yr = _call(vr, model, case37, 'rows', SAMPLES, complex_output)
    assert rc == 0, err
    assert Xr.cpu().numpy().tobytes() == X.tobytes() and yr.cpu().numpy().tobytes() == y.tobytes()


@pytest.mark.parametrize('complex_output', (False, True))
def test_three_forms_agree_bit_for_bit(vr, model, case65, complex_output):
    outs = {}
    for form in ('dense', 'rows', 'waves'):
        rc, err, X, y = _call(vr, model, case65, form, SAMPLES, complex_output)
        assert rc == 0, (form, err)
        outs[form] = (X, y)
    for form in ('rows', 'waves'):
        assert _bits(outs[form][0], outs['dense'][0]) and _bits(outs[form][1], outs['dense'][1]), form
    want = _ref_batch(case65, SAMPLES, complex_output)
    X, y = (a.cpu().numpy() for a in outs['waves'])
    for b, w in enumerate(want):
        _check_against((X[b], y[b]), w, 'wave store sample %d' % b)
    # two identical calls agree
    rc, err, X2, y2 = _call(vr, model, case65, 'waves', SAMPLES, complex_output)
    assert rc == 0 and _bits(X2, outs['waves'][0]) and _bits(y2, outs['waves'][1])


# ---- 2. nothing that exists changes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('complex_output', (False, True))
def test_ex_entry_points_without_a_new_bit_return_the_old_bytes(vr, model, case65, complex_output):
    h = model._need_handle()
    for form in ('dense', 'rows', 'waves'):
        rc, err, wX, wy = _call(vr, model, case65, form, OLD_ONLY, complex_output, ex=False)
        assert rc == 0, (form, err)
        (rc, err, X, y), report = _profiled(vr, h, lambda: _call(vr, model, case65, form, OLD_ONLY, complex_output, ex=True))
        assert rc == 0, (form, err)
        assert _bits(X, wX) and _bits(y, wy), form
        assert 'AugDescEx' not in report and 'augment_kernel' in report, report      # the old instantiation itself
        assert float(wX.abs().max()) > 0
    (rc, err, X, y), report = _profiled(vr, h, lambda: _call(vr, model, case65, 'rows', SAMPLES, complex_output))
    assert rc == 0 and 'AugDescEx' in report, report                # ... and, with a new bit, the new one


def test_the_identity_remix_is_the_plain_sample(vr, model, case37):
    """g_y = g_v = 1 and the sample's own crop as its partner: y + (X - y) is X to rounding."""
    plain = [S(k, st, 0) for k, st in ((0, 0), (1, 21), (2, 17))]
    same = [S(s.song, s.start, REMIX, s.song, s.start) for s in plain]
    for complex_output in (False, True):
        rc, err, wX, wy = _call(vr, model, case37, 'rows', plain, complex_output, ex=False)
        assert rc == 0, err
        rc, err, X, y = _call(vr, model, case37, 'rows', same, complex_output)
        assert rc == 0, err
        assert _bits(y, wy)                                         # 1.0f * y
        for b in range(len(plain)):
            _check_against((X[b].cpu().numpy(), y[b].cpu().numpy()), (wX[b].cpu().numpy(), wy[b].cpu().numpy()), 'identity %d' % b)


# ---- 3. the classes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('complex_output', (False, True))
def test_the_three_classes_give_one_batch_and_it_is_remix_refs(vr, model, case65, complex_output):
    ts = case65['ts'] * 2
    wave_rows = [[mix, inst, r[2]] for (mix, inst), r in zip(case65['pairs'], case65['ts'])] * 2
    rates = dict(remix_rate=0.4, remix_gain=(0.5, 1.25), mono_rate=0.3)
    kw = dict(cropsize=T, reduction_rate=0.5, reduction_weight=case65['rw'], mixup_rate=0.6, mixup_alpha=0.4, model=model,
              complex_output=complex_output, **rates)
    seen = set()
    dense = vr.dataset.VocalRemoverTrainingSet(ts, **kw)
    with vr.dataset.ResidentTrainingSet(ts, **kw) as rows, vr.dataset.ResidentWaveTrainingSet(wave_rows, **kw) as waves:
        for seed in range(6):
            idx = [(seed + k) % 6 for k in range(6)]                # B = 6
            np.random.seed(seed)
            want = [ref.training_sample(ts, i, T, 0.5, case65['rw'], 0.6, 0.4, complex_output=complex_output, **rates) for i in idx]
            state = np.random.get_state()
            np.random.seed(seed)
            for p in (dense.plan(i) for i in idx):
                seen.update(k for k, on in (('remix', p.get('remix') is not None), ('mono', p['flags'] & MONO), ('mixup', p['mix'] is not None),
                                            ('partner mono', p['mix'] is not None and p['mix']['flags'] & MONO)) if on)
            np.random.seed(seed)
            dX, dy = dense.batch(idx)
            assert _same_state(np.random.get_state(), state)
            for ds in (rows, waves):
                np.random.seed(seed)
                X, y = ds.batch(idx)
                assert _same_state(np.random.get_state(), state)
                assert _bits(X, dX) and _bits(y, dy), (type(ds).__name__, seed)
            assert tuple(dX.shape) == (6, 2, 65, T) and dX.dtype == (torch.complex64 if complex_output else torch.float32)
            dX, dy = dX.cpu().numpy(), dy.cpu().numpy()
            for b, w in enumerate(want):
                _check_against((dX[b], dy[b]), w, 'seed %d sample %d' % (seed, b))
    assert seen == {'remix', 'mono', 'mixup', 'partner mono'}, sorted(seen)


def test_with_the_rates_at_zero_the_old_entry_points_are_called(vr, model, case65, monkeypatch):
    """today's calls go out unchanged: with both rates 0 a batch never reaches an _ex entry point, with one on it does"""
    ts = case65['ts'] * 2
    kw = dict(cropsize=T, reduction_rate=0.5, reduction_weight=case65['rw'], mixup_rate=0.5, mixup_alpha=0.4, model=model)
    called = []
    real = vr.dataset._outputs
    monkeypatch.setattr(vr.dataset, '_outputs', lambda c, shape, dev, entry, ex=False: (called.append((entry, ex)), real(c, shape, dev, entry, ex))[1])
    with vr.dataset.ResidentTrainingSet(ts, **kw) as a, vr.dataset.ResidentTrainingSet(ts, mono_rate=1e-9, **kw) as b:
        np.random.seed(0)
        wX, wy = a.batch([0, 1, 2])
        vr.dataset.VocalRemoverTrainingSet(ts, **kw).batch([0])
        assert called == [('vr_dataset_batch', False), ('vr_augment_batch', False)]
        np.random.seed(0)
        b.batch([0, 1, 2])
        assert called[-1] == ('vr_dataset_batch', True)


# ---- 4. what is refused -------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(vr, model, case65):
    h = model._need_handle()
    ok = S(0, 3, 0)
    nan, inf = float('nan'), float('inf')
    stores = [
        ([ok, S(1, 0, REMIX | 8, 2, 0)], 'sample 1: remix and mixup are both flagged'),
        ([ok, S(1, 0, REMIX, -1, 0)], 'sample 1: remix flagged but mix_song is -1'),
        ([ok, S(1, 0, REMIX, 3, 0)], 'sample 1: remix partner: song 3 out of range'),
        ([S(1, 0, REMIX, 2, 31), ok], 'sample 0: remix partner: rows [31, 71) end past the 70 rows of song 2'),
        ([ok, S(1, 0, REMIX, 2, -1)], 'sample 1: remix partner: start -1 is negative'),
        ([ok, ok, S(1, 0, REMIX | 16, 2, 0)], "sample 2: remix flagged with the partner's reduce bit"),
        ([ok, S(1, 0, REMIX | 64, 2, 0)], "sample 1: remix flagged with the partner's inst-only bit"),
        ([ok, S(1, 0, REMIX, 2, 0, gy=nan)], 'sample 1: gain_y is not finite'),
        ([S(1, 0, REMIX, 2, 0, gv=inf), ok], 'sample 0: gain_v is not finite'),
        ([ok, S(1, 0, REMIX, 2, 0, gv=-inf)], 'sample 1: gain_v is not finite'),
    ]
    dense_too = {0, 5, 6, 7, 8, 9}                                  # (the others are about rows of a store)
    outs = []

    def run_refused():
        for complex_output in (False, True):
            for k, (samples, msg) in enumerate(stores):
                for form in ('rows', 'waves') + (('dense',) if k in dense_too else ()):
                    rc, err, X, y = _call(vr, model, case65, form, samples, complex_output)
                    assert rc == -2 and msg in err, (form, rc, err, msg)
                    outs.append((X, y))
            # the dense form's own: a remix needs the partner crops as a mixup does
            rc, err, X, y = _call(vr, model, case65, 'dense', [ok, S(1, 0, REMIX)], complex_output)
            assert rc == -2 and 'no partner crops given' in err, err
            outs.append((X, y))
    _, report = _profiled(vr, h, run_refused)
    assert 'augment_kernel' not in report and 'stft_tile_kernel' not in report, report
    torch.cuda.synchronize()
    for X, y in outs:
        assert _bits(X, torch.full_like(X, -7.0)) and _bits(y, torch.full_like(y, -7.0))       # the sentinel stands
    # native.check raises what the old entry points' refusals raise
    with pytest.raises(ValueError, match='sample 1: remix and mixup are both flagged'):
        vr.native.check(_call(vr, model, case65, 'rows', stores[0][0], False)[0])
    # and the largest rows a remix partner can have are accepted
    (rc, err, X, y), report = _profiled(vr, h, lambda: _call(vr, model, case65, 'waves', [ok, S(1, 21, REMIX, 2, 30)], False))
    assert rc == 0, err
    assert 'augment_kernel' in report and 'stft_tile_kernel' in report and float(X.min()) >= 0.0


def test_the_wave_scratch_is_what_it_was(vr, case65):
    """a batch in which every sample has a remix partner finds the buffer a plain batch of the same B and T reserved"""
    h = vr.native.Handle(0, N_FFT, HOP, 4, 4)
    own = types.SimpleNamespace(n_fft=N_FFT, hop_length=HOP, _need_handle=lambda: h)
    try:
        plain = [S(k % 3, k, 0) for k in range(6)]
        rc, err, _, _ = _call(vr, own, case65, 'waves', plain, False, ex=False)
        assert rc == 0, err
        held = h.pipeline_buffer_bytes()
        rows_b = T * 2 * 65 * 8
        assert 4 * 6 * rows_b <= held < 5 * 6 * rows_b + 65536, held
        rc, err, _, _ = _call(vr, own, case65, 'waves', [S(k % 3, k, REMIX | MONO, (k + 1) % 3, 9 - k, gy=0.5, gv=0.7) for k in range(6)], True)
        assert rc == 0, err
        rc, err, _, _ = _call(vr, own, case65, 'waves', plain, False)
        assert rc == 0 and h.pipeline_buffer_bytes() == held
    finally:
        h.close()


# ---- 5. training ----------------------------------------------------------------------------------------------------------------------------
def test_three_steps_of_training_on_remixed_batches(vr, tmp_path):
    from vocal_remover_amd import train as vtrain
    n_fft, nout, nl = 512, 8, 32                                    # the smallest net of tests/test_gpu_resident.py
    bins = n_fft // 2 + 1
    ts = _synthetic_training_set(tmp_path, bins=bins, lengths=(100, 80)) * 3
    dev = torch.device('cuda:0')
    net = vr.nets.CascadedNet(n_fft, n_fft // 2, nout, nl)
    net.load_state_dict(weights.make_state_dict(11, n_fft=n_fft, nout=nout, nout_lstm=nl))
    net.to(dev)
    net.set_dropout_masks(1234)
    losses = []
    step = net.train_step
    net.train_step = lambda *a, **k: (losses.append(step(*a, **k)), losses[-1])[1]
    before = net.state_dict()['out.weight'].clone()
    with vr.dataset.ResidentTrainingSet(ts, cropsize=64, reduction_rate=0.5, reduction_weight=_reduction_weight(bins), mixup_rate=0.5,
                                        mixup_alpha=0.4, model=net, remix_rate=1.0, mono_rate=0.25) as ds:
        np.random.seed(5)
        assert all(ds.plan(i).get('remix') is not None for i in range(6))
        loader = vr.dataset.DeviceLoader(ds, batch_size=2, shuffle=True)
        opt = vtrain.Adam(filter(lambda p: p.requires_grad, net.parameters()), lr=1e-3)
        np.random.seed(7)
        torch.manual_seed(7)
        mean = vtrain.train_epoch(loader, net, dev, opt, 1)
    print('losses', losses, 'mean', mean)
    assert len(losses) == 3 and all(np.isfinite(v) and v > 0 for v in losses) and np.isfinite(mean)
    after = net.state_dict()['out.weight']
    assert bool(torch.isfinite(after).all()) and float((after - before).abs().max()) > 0
    net.to('cpu')
