"""The float64 evaluation of the Mimi oracle (OracleMimi dtype=np.float64) and what makes the bar of
tests/test_mimi_f64_gpu.py mean something.  numpy only.

Unit (helpers.mimi_errors): per utterance and per 1920-sample frame (per latent step for the rows tap),
max |value - float64| / the utterance's largest |float64 value|.  e32 = the float32 oracle's figure in that
unit, its maximum over frames and utterances; bar = helpers.MIMI_BAR_MARGIN x e32 on every frame.

Each defect below is applied to the float32 oracle's output or evaluation.  Each must miss that bar by 2 x at
least on some frame -- and the three whose size is set here (the first, second and fifth; see RMS_SEES for the
other two) pass the whole-waveform ``rms <= 1e-4`` check the codec was held to before, which is what shows
the gap was real:
  * one PCM sample off by 1e-3 of full scale;
  * one 64-sample run off by 1e-4;
  * the last sample of each utterance's final frame replaced by its neighbour;
  * one history sample (one channel of the first decoder conv's carried input) zeroed in a streaming step;
  * the convs' activations cut to 16 significant bits (helpers.cut16).
The margin may not exceed half the smallest defect in units of e32: asserted here, so it cannot drift.
Nothing is a constant: e32 and every defect's figure are computed each run (and printed)."""
import contextlib

import numpy as np
import pytest

from helpers import MIMI_BAR_MARGIN, cut16, mimi_errors, mimi_pair, rms as _rms

CONFIGS = ["tiny", "mimi_202407"]
# The two defects whose size the waveform sets, not the test: on these synthetic weights the old
# whole-waveform check does see them.  The waveform is rough (neighbouring samples differ by about 0.03 of 1.9
# full scale), so two end samples replaced by their neighbours move the RMS over 46,080 samples to 1.9e-4
# (mimi_202407) / 6.3e-4 (tiny); a zeroed history sample of the first decoder conv (values of order 1, read by
# 7 taps of 1024 output channels) moves the 4-frame RMS to 1.2e-3 (mimi_202407) / 6.6e-5 (tiny).  Their bar side
# is asserted like the others'; their RMS is printed, not asserted.
RMS_SEES = ("last sample = its neighbour", "history sample zeroed")


def _codes(m, frames=12):
    return np.random.default_rng(5).integers(0, m.bins, (2, m.n_q, frames)).astype(np.int32)   # test_decode_parity's


_DEC = {}


def _decode_case(name):
    """(m, codes, float32 waveform, float64 waveform, e32) of the one-shot decode case, computed once."""
    if name not in _DEC:
        m, _, o32, o64 = mimi_pair(name, "mlx")
        codes = _codes(m)
        y32, y64 = o32.decode(codes), o64.decode(codes)
        _DEC[name] = (m, codes, y32, y64, float(mimi_errors(y32, y64, m.frame_size).max()))
    return _DEC[name]


def _stream(o, codes, spoil=None):
    o.reset_state()
    out = []
    for f in range(codes.shape[2]):
        if spoil is not None and f == spoil:
            o._hist = o._hist.copy()
            o._hist[0, 3, -1] = 0          # one carried input sample of the first decoder conv, one channel
        out.append(o.decode_step(codes[:, :, f: f + 1]))
    o.reset_state()
    return np.concatenate(out, axis=2)


@contextlib.contextmanager
def _cut_conv_activations():
    import oracle.mimi_oracle as mo
    c1, ct = mo.conv1d, mo.conv_transpose1d
    mo.conv1d = lambda x, *a, **k: c1(cut16(x), *a, **k)
    mo.conv_transpose1d = lambda x, *a, **k: ct(cut16(x), *a, **k)
    try:
        yield
    finally:
        mo.conv1d, mo.conv_transpose1d = c1, ct


@pytest.mark.parametrize("name", CONFIGS)
def test_default_dtype_is_the_float32_restatement(name):
    """dtype float32 leaves float32 arrays, float64 leaves float64 ones, and the two agree to float32
    rounding: the float64 evaluation is the same function, not another model."""
    m, codes, y32, y64, e32 = _decode_case(name)
    assert y32.dtype == np.float32 and y64.dtype == np.float64
    assert 0 < e32 < 1e-5, e32
    _, _, o32, o64 = mimi_pair(name, "mlx")
    assert o32.taps["rows"].dtype == np.float32 and o64.taps["rows"].dtype == np.float64
    assert o32.taps["rows"].shape == (2, 12 * m.downsample_stride, m.dimension)
    assert all(v.dtype == np.float32 for v in dict.values(o64.w)), "the stored weights stay float32"
    assert float(mimi_errors(o32.taps["rows"], o64.taps["rows"]).max()) < 1e-5


@pytest.mark.parametrize("name", CONFIGS)
def test_defects_miss_the_bar_and_pass_the_rms_check(name, capsys):
    m, codes, y32, y64, e32 = _decode_case(name)
    fs = m.frame_size
    full = np.abs(y64).reshape(2, -1).max(-1)
    defects = {}
    d = y32.copy()
    d[0, 0, 5 * fs + 777] += np.float32(1e-3 * full[0])
    defects["one sample off by 1e-3"] = (d, y32, y64, e32)
    d = y32.copy()
    d[1, 0, 3 * fs + 1000: 3 * fs + 1064] += np.float32(1e-4 * full[1])
    defects["64-sample run off by 1e-4"] = (d, y32, y64, e32)
    d = y32.copy()
    d[:, 0, -1] = d[:, 0, -2]
    defects["last sample = its neighbour"] = (d, y32, y64, e32)
    with _cut_conv_activations():
        d = mimi_pair(name, "mlx")[2].decode(codes)
    defects["conv activations cut to 16 bits"] = (d, y32, y64, e32)
    _, _, o32, o64 = mimi_pair(name, "mlx")
    s32, s64 = _stream(o32, codes[:, :, :4]), _stream(o64, codes[:, :, :4])
    e32s = float(mimi_errors(s32, s64, fs).max())
    defects["history sample zeroed"] = (_stream(o32, codes[:, :, :4], spoil=2), s32, s64, e32s)
    lines, cap = [], np.inf
    for what, (bad, ref32, ref64, e) in defects.items():
        fig = float(mimi_errors(bad, ref64, fs).max())
        rms = _rms(bad, ref32)
        lines.append(f"{name}: {what}: {fig / e:.1f} x e32 (e32 {e:.2e}), rms vs float32 {rms:.2e}")
        cap = min(cap, fig / e / 2)
        if what not in RMS_SEES:
            assert rms <= 1e-4, f"{what}: the old check would have caught it ({rms:.2e})"
        assert fig >= 2 * MIMI_BAR_MARGIN * e, f"{what}: {fig / e:.2f} x e32 does not miss the bar by 2 x"
    assert MIMI_BAR_MARGIN <= cap, (MIMI_BAR_MARGIN, cap)
    with capsys.disabled():
        print("\n" + "\n".join(lines) + f"\n{name}: margin {MIMI_BAR_MARGIN} <= cap {cap:.1f}")


def test_encode_latent_tap_and_dtype():
    """encode leaves the pre-RVQ latent as rows; the float64 latent is within float32 rounding of the float32
    one, and the codes of the two evaluations agree wherever the float32 margin allows."""
    from helpers import mimi_pcm_clip
    m, _, o32, o64 = mimi_pair("tiny", "mlx")
    pcm = np.stack([mimi_pcm_clip(24000 * 2 + 480, 1), mimi_pcm_clip(24000 * 2 + 480, 2)])[:, None, :]
    c32, c64 = o32.encode(pcm), o64.encode(pcm)
    r32, r64 = o32.taps["rows"], o64.taps["rows"]
    assert r32.dtype == np.float32 and r64.dtype == np.float64 and r32.shape == r64.shape == (2, c32.shape[2], m.dimension)
    assert np.array_equal(o32.debug_latent.transpose(0, 2, 1), r32)
    assert float(mimi_errors(r32, r64).max()) < 1e-5
    assert c32.shape == c64.shape and np.array_equal(c32[:, 0, 0], c64[:, 0, 0])
