"""Many songs in one call (vr_separate_many / vr_separate_wave_many), the parts that need no GPU: the reference fixture of the four
extra songs against the CPU oracle, the C ABI's declarations, exports and argument errors, and the command line's directory input."""
import ctypes
import importlib.util
import os

import numpy as np

from oracle import separator, weights

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = np.load(os.path.join(HERE, 'golden', 'separate_many.npz'))
_spec = importlib.util.spec_from_file_location('make_golden_many', os.path.join(HERE, 'golden', 'make_golden_many.py'))
MGM = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MGM)


def test_oracle_reproduces_the_many_song_fixture():
    sd = weights.make_state_dict(11, n_fft=512, nout=8, nout_lstm=32)
    assert abs(MGM.weight_checksum(sd) - float(G['small_wsum'])) < 1e-6 * float(G['small_wsum']), 'seeded weights drifted'
    scales = []
    for i in sorted(MGM.LENGTHS):
        X = MGM.song(i)
        assert X.shape == (2, 257, MGM.LENGTHS[i]) and G['y%d' % i].shape == (2, 52, MGM.LENGTHS[i])
        scales.append(float(np.abs(X).max()))
        y, _ = separator.separate(X.copy(), sd, n_fft=512, batchsize=2, cropsize=160)
        err = np.abs(y[:, ::5] - G['y%d' % i]).max()
        yt, _ = separator.separate(X.copy(), sd, tta=True, n_fft=512, batchsize=2, cropsize=160)
        err_t = np.abs(yt[:, ::5] - G['tta_y%d' % i]).max()
        print('song %d (T = %d): oracle vs reference %.3e, tta %.3e' % (i, MGM.LENGTHS[i], err, err_t))
        assert err < 1e-5 and err_t < 1e-5
    assert max(scales) / min(scales) > 2.5          # a normaliser shared between the songs could not reproduce the fixture


def test_many_song_symbols_are_declared_exported_and_check_their_arguments(vr):
    header = open(os.path.join(ROOT, 'include', 'vr_mi355.h')).read()
    nat = vr.native
    L = nat.lib()
    table = nat.ptr_table([0])
    for name, lens in (('vr_separate_many', (ctypes.c_int * 1)(5)), ('vr_separate_wave_many', (ctypes.c_int64 * 1)(4096))):
        assert ('int %s(vr_handle h, int n_songs,' % name) in header
        assert name in nat.exported_symbols()
        fn = getattr(L, name)
        # no handle: refused without a device
        assert fn(None, 1, table, 0, lens, 0, 2, 160, table, table, 0) == -2
        assert L.vr_last_error() == b'null handle'
        # the tables are looked at before the handle
        for n in (0, -3):
            assert fn(None, n, table, 0, lens, 0, 2, 160, table, table, 0) == -2
            assert b'n_songs' in L.vr_last_error()
        for args in ((None, 0, lens, 0, 2, 160, table, table, 0), (table, 0, None, 0, 2, 160, table, table, 0),
                     (table, 0, lens, 0, 2, 160, None, table, 0), (table, 0, lens, 0, 2, 160, table, None, 0)):
            assert fn(None, 1, *args) == -2
            assert L.vr_last_error() == b'null table'


def test_directory_input_is_expanded_sorted_and_grouped(vr, tmp_path):
    inf = vr.inference
    for name in ('b.wav', 'a.wav', 'c.WAV', 'notes.txt', 'd.wav', 'e.wav'):
        (tmp_path / name).write_bytes(b'')
    (tmp_path / 'sub.wav').mkdir()
    (tmp_path / 'sub.wav' / 'x.wav').write_bytes(b'')
    d = str(tmp_path)
    names = lambda groups: [[os.path.basename(f) for f in g] for g in groups]
    assert names(inf.expand_inputs(d, 2)) == [['a.wav', 'b.wav'], ['c.WAV', 'd.wav'], ['e.wav']]      # (sorted by name; files only)
    assert names(inf.expand_inputs(d, 8)) == [['a.wav', 'b.wav', 'c.WAV', 'd.wav', 'e.wav']]
    assert names(inf.expand_inputs(d, 1)) == [['a.wav'], ['b.wav'], ['c.WAV'], ['d.wav'], ['e.wav']]
    one = os.path.join(d, 'a.wav')
    assert inf.expand_inputs(one, 8) == [[one]]                   # a file stays one call of one song, whatever --songs_per_call says
    assert inf.expand_inputs(str(tmp_path / 'empty-not-there.wav'), 3) == [[str(tmp_path / 'empty-not-there.wav')]]
    try:
        inf.expand_inputs(d, 0)
    except ValueError:
        pass
    else:
        raise AssertionError('--songs_per_call 0 must be refused')
