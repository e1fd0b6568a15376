"""Pseudo-instrument labels (vr_pseudo*), the parts that need no GPU: the numpy definition over the CPU oracle against the reference's
fixture, the C ABI's declarations, exports and before-the-handle errors, the command line's arguments, and the file names and list of
dataset.make_pseudo_training_set with a stub separator."""
import ctypes
import importlib.util
import os

import numpy as np

import pseudo_ref
from oracle import separator, weights

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = np.load(os.path.join(HERE, 'golden', 'pseudo.npz'))
_spec = importlib.util.spec_from_file_location('make_golden_pseudo', os.path.join(HERE, 'golden', 'make_golden_pseudo.py'))
MGP = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MGP)


def bar(X, y, P):
    """1e-4 max|D| (the separation's own bar) + 2^-23 max|P| (the one added rounding)"""
    return 1e-4 * float(np.abs(X - y).max()) + 2.0 ** -23 * float(np.abs(P).max())


def test_definition_over_the_oracle_reproduces_the_fixture():
    sd = weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32)
    assert abs(MGP.MGM.weight_checksum(sd) - float(G['small_wsum'])) < 1e-6 * float(G['small_wsum']), 'seeded weights drifted'
    changed = 0
    for post in (False, True):
        for i in MGP.PAIRS:
            X, y = MGP.pair(i)
            assert X.dtype == y.dtype == np.complex64 and X.shape == y.shape == (2, 257, MGP.MGM.LENGTHS[i])
            P = pseudo_ref.pseudo_instruments(lambda D: separator.separate(D, sd, tta=True, post=post, n_fft=512, batchsize=2, cropsize=160), X, y)
            want = G[('post_p%d' if post else 'tta_p%d') % i]
            err = float(np.abs(P[:, ::MGP.BIN_STEP] - want).max())
            print('pair %d postprocess %s: |P - fixture| %.3e, bar %.3e' % (i, post, err, bar(X, y, P)))
            assert P.dtype == np.complex64 and err <= bar(X, y, P)
        changed += sum(not np.array_equal(G['tta_p%d' % i], G['post_p%d' % i]) for i in MGP.PAIRS)
    assert changed                                   # --postprocess is not vacuous in the fixture
    for key in G.files:
        assert np.isfinite(np.asarray(G[key]).view(np.float32 if G[key].dtype == np.complex64 else G[key].dtype)).all(), key


def test_symbols_are_declared_exported_and_check_their_arguments(vr):
    header = open(os.path.join(ROOT, 'include', 'vr_mi355.h')).read()
    nat = vr.native
    L = nat.lib()
    assert 'enum vr_pseudo_layout { VR_PSEUDO_SPEC = 0' in header and 'VR_PSEUDO_ROWS = 1' in header
    assert (nat.VR_PSEUDO_SPEC, nat.VR_PSEUDO_ROWS) == (0, 1) and nat.PSEUDO_LAYOUTS == {'spec': 0, 'rows': 1}
    for name in ('vr_pseudo_many', 'vr_pseudo_wave_many', 'vr_pseudo', 'vr_pseudo_wave'):
        assert ('int %s(vr_handle h, ' % name) in header
        assert name in nat.exported_symbols() and getattr(L, name) is not None
    table = nat.ptr_table([0])
    for name, lens in (('vr_pseudo_many', (ctypes.c_int * 1)(5)), ('vr_pseudo_wave_many', (ctypes.c_int64 * 1)(4096))):
        fn = getattr(L, name)
        assert fn(None, 1, table, table, 0, lens, 1, 2, 160, 0, table, 0) == -2
        assert L.vr_last_error() == b'null handle'
        for n in (0, -3):                            # the count, the tables and the layout are looked at before the handle
            assert fn(None, n, table, table, 0, lens, 1, 2, 160, 0, table, 0) == -2
            assert b'n_songs' in L.vr_last_error()
        for args in ((None, table, 0, lens, 1, 2, 160, 0, table, 0), (table, None, 0, lens, 1, 2, 160, 1, table, 0),
                     (table, table, 0, None, 1, 2, 160, 0, table, 0), (table, table, 0, lens, 1, 2, 160, 1, None, 0)):
            assert fn(None, 1, *args) == -2
            assert L.vr_last_error() == b'null table'
        for layout in (2, -1):
            assert fn(None, 1, table, table, 0, lens, 1, 2, 160, layout, table, 0) == -2
            assert b'layout' in L.vr_last_error()
    buf = np.zeros(8, np.float32)
    p = buf.ctypes.data
    for fn, n in ((L.vr_pseudo, 5), (L.vr_pseudo_wave, 4096)):
        assert fn(None, p, p, 0, n, 1, 2, 160, 0, p, 0) == -2 and L.vr_last_error() == b'null handle'
        for args in ((None, p, 0, n, 1, 2, 160, 0, p, 0), (p, None, 0, n, 1, 2, 160, 0, p, 0), (p, p, 0, n, 1, 2, 160, 0, None, 0)):
            assert fn(None, *args) == -2 and L.vr_last_error() == b'null argument'
        assert fn(None, p, p, 0, n, 1, 2, 160, 7, p, 0) == -2 and b'layout' in L.vr_last_error()
        assert b'song' not in L.vr_last_error()


def test_command_line_arguments_and_defaults(vr):
    p = vr.pseudo.build_parser()
    a = p.parse_args(['--mixtures', 'm', '--instruments', 'i'])
    assert (a.gpu, a.pretrained_model, a.sr, a.n_fft, a.hop_length, a.batchsize, a.cropsize, a.postprocess) == \
        (-1, 'models/baseline.pth', 44100, 2048, 1024, 4, 256, False)               # the reference's (pseudo.py:17-28)
    assert (a.mixtures, a.instruments, a.songs_per_call, a.output_dir, a.rows) == ('m', 'i', 8, 'pseudo', False)
    b = p.parse_args(['-m', 'm', '-i', 'i', '-g', '0', '-P', 'w.pth', '-r', '22050', '-f', '512', '-H', '256', '-B', '2', '-c', '160', '-p',
                      '--songs_per_call', '3', '--output_dir', 'out', '--rows'])
    assert (b.gpu, b.pretrained_model, b.sr, b.n_fft, b.hop_length, b.batchsize, b.cropsize, b.postprocess, b.songs_per_call, b.output_dir,
            b.rows) == (0, 'w.pth', 22050, 512, 256, 2, 160, True, 3, 'out', True)
    for missing in (['--mixtures', 'm'], ['--instruments', 'i']):
        try:
            p.parse_args(missing)
        except SystemExit:
            pass
        else:
            raise AssertionError('--mixtures and --instruments are required')


class _StubSeparator(object):
    """pseudo_instruments_wave_many of a separator that needs no device: rows of a recognisable value per pair."""

    def __init__(self, hop, bins):
        self.hop, self.bins, self.calls = hop, bins, []

    def pseudo_instruments_wave_many(self, mixes, insts, tta=True, layout='spec'):
        assert layout == 'rows' and len(mixes) == len(insts)
        self.calls.append((len(mixes), tta))
        out = []
        for X, y in zip(mixes, insts):
            assert X.shape == y.shape and X.dtype == np.float32
            T = 1 + X.shape[1] // self.hop
            out.append(np.full((T, 2, self.bins), complex(float(X[0, 0]), 2.0), np.complex64))
        return out


def test_make_pseudo_training_set_files_and_list(vr, tmp_path, monkeypatch):
    hop, n_fft, sr, bins = 256, 512, 8000, 257
    mix_dir, inst_dir = tmp_path / 'mixtures', tmp_path / 'instruments'
    mix_dir.mkdir()
    inst_dir.mkdir()
    names = ['a', 'b', 'c']
    for k, n in enumerate(names):
        (mix_dir / (n + '.wav')).write_bytes(b'')
        (inst_dir / (n + '_inst.wav')).write_bytes(b'')
    filelist = vr.dataset.make_pair(str(mix_dir), str(inst_dir))
    lengths = {n: hop * (3 + k) + 7 for k, n in enumerate(names)}

    def fake_pair(mix_path, inst_path, rate):
        assert rate == sr
        n = os.path.splitext(os.path.basename(mix_path))[0]
        assert os.path.basename(inst_path) == n + '_inst.wav'
        return (np.full((2, lengths[n]), 3.0 + names.index(n), np.float32), np.zeros((2, lengths[n]), np.float32))

    def fake_stft(wave, h, f):
        assert (h, f) == (hop, n_fft)
        return np.full((2, bins, 1 + wave.shape[1] // h), 0.5, np.complex64)

    monkeypatch.setattr(vr.dataset, 'load_aligned_pair', fake_pair)
    monkeypatch.setattr(vr.spec_utils, 'wave_to_spectrogram', fake_stft)
    # song b's mixture is cached already, louder than its label: the list's peak must come from the cache
    cache = vr.spec_utils.SpectrogramCache(sr, hop, n_fft)
    cached = np.full((1 + lengths['b'] // hop, 2, bins), 9.0, np.complex64)
    np.save(cache.npy_path(str(mix_dir / 'b.wav')), cached)
    sp = _StubSeparator(hop, bins)
    rows = vr.dataset.make_pseudo_training_set(sp, filelist, sr, hop, n_fft, songs_per_call=2, tta=True)
    assert sp.calls == [(2, True), (1, True)]
    folder = 'sr%d_hl%d_nf%d' % (sr, hop, n_fft)
    assert len(rows) == 3
    for k, (n, (X_path, P_path, coef)) in enumerate(zip(names, rows)):
        assert X_path == str(mix_dir / folder / (n + '.npy'))
        assert P_path == str(inst_dir / folder / (n + '_inst_PseudoInstruments.npy'))
        X, P = np.load(X_path), np.load(P_path)
        T = 1 + lengths[n] // hop
        assert X.shape == P.shape == (T, 2, bins) and X.dtype == P.dtype == np.complex64           # the cache's layout, as the set reads it
        assert np.all(P == complex(3.0 + k, 2.0))
        assert float(coef) == float(max(np.abs(X).max(), np.abs(P).max()))
    assert np.array_equal(np.load(rows[1][0]), cached) and float(rows[1][2]) == 9.0
    assert not os.path.exists(str(inst_dir / folder / 'a_inst.npy'))                                # the instrumental itself is not cached here
    # the list is what the training set takes: its shape reader finds [T, 2, bins]
    ts = vr.dataset.VocalRemoverTrainingSet.__new__(vr.dataset.VocalRemoverTrainingSet)
    assert tuple(ts.read_npy_shape(rows[0][1])) == (1 + lengths['a'] // hop, 2, bins)
