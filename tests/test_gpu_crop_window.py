"""Column window of the stage-3 dec1 conv (vr_set_option("crop_window"), default 1).

predict_mask keeps only the columns [offset, cropsize - offset) of each crop (lib/nets.py:124-128), and the stage-3 dec1 output feeds
only the mask head.  With the option on, in eval and mfma_mode 3, that conv computes only the 32-column tiles that meet the kept columns
(ConvArgs::w_lo / w_hi, conv_x3h.hip) and the head reads only those columns.  A tile computes exactly what it computes in a full-width
launch (the power-of-two scaling is per tile), so the two paths must agree BIT FOR BIT: here they run in one process and are compared
with array_equal, through separate_wave (plain and --tta: the benched executor), predict_mask / predict with frame counts that are not
multiples of 32 (window edges inside a tile), validate_step, and batch 1 and 11."""
import numpy as np
import pytest
import torch

from oracle import separator, stft_np, weights

pytestmark = pytest.mark.gpu

HOP, N_FFT, CROP = 1024, 2048, 256


@pytest.fixture(scope='module')
def full(vr):
    sd = weights.make_state_dict(1234)
    model = vr.nets.CascadedNet(N_FFT, HOP, 32, 128)
    model.load_state_dict(sd)
    model.to(torch.device('cuda:0'))
    model.eval()
    yield model
    model.set_option('crop_window', 1)


def _both(model, fn):
    """fn() with the window off, then twice with it on (the default): (off, on, on again)."""
    model.set_option('crop_window', 0)
    try:
        off = fn()
    finally:
        model.set_option('crop_window', 1)
    return off, fn(), fn()


@pytest.mark.parametrize('tta', [False, True], ids=['plain', 'tta'])
def test_s30_separate_wave_window_is_bit_equal(vr, full, tta):
    model = full
    wave = separator.synth_wave(30.0, seed=0)
    wd = torch.from_numpy(wave).to('cuda:0')
    sp = vr.inference.Separator(model, torch.device('cuda:0'), batchsize=0, cropsize=CROP)
    spec = stft_np.wave_to_spectrogram(wave, HOP, N_FFT)

    def run():
        yw, vw = sp.separate_wave(wd, tta=tta)
        y, v = (sp.separate_tta if tta else sp.separate)(spec)
        return yw.cpu().numpy(), vw.cpu().numpy(), y, v

    off, on, again = _both(model, run)
    for a, b, c in zip(off, on, again):
        assert np.array_equal(a, b)
        assert np.array_equal(b, c)                       # deterministic
    assert np.isfinite(on[0]).all() and np.isfinite(on[2]).all()


@pytest.mark.parametrize('B,T', [(1, 256), (11, 256), (1, 272), (11, 240), (2, 208)])
def test_predict_and_validate_window_is_bit_equal(vr, full, B, T):
    model = full
    g = torch.Generator().manual_seed(B * 1000 + T)
    X = torch.rand(B, 2, N_FFT // 2 + 1, T, generator=g) * 3.0
    Y = torch.rand(B, 2, N_FFT // 2 + 1, T, generator=g) * 3.0
    Xd, Yd = X.to('cuda:0'), Y.to('cuda:0')
    with torch.no_grad():
        for fn in (model.predict_mask, model.predict):
            off, on, again = _both(model, lambda: fn(Xd).cpu().numpy())
            assert on.shape == (B, 2, N_FFT // 2 + 1, T - 2 * model.offset)
            assert np.array_equal(off, on) and np.array_equal(on, again)
            if fn == model.predict_mask:
                assert np.array_equal(on[:, :, -1], on[:, :, -2])      # the replicated last row (pad_rows)
        # mode 0 (full width) is untouched by the option
        off, on, _ = _both(model, lambda: model(Xd).cpu().numpy())
        assert on.shape == (B, 2, N_FFT // 2 + 1, T) and np.array_equal(off, on)
        off, on, again = _both(model, lambda: model.validate_step(Xd, Yd))
        assert off == on == again
