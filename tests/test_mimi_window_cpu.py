"""What makes the cases of tests/test_mimi_window_gpu.py mean something: the faults of a windowed key range that
the suite could not see while no codec stream ran a range that both starts past key 0 and spans more than one
64-key chunk.  numpy only.

Tiny config with context = 70 (causal rows hold 70 live keys, mlx rows 72: one chunk and a tail), both attention
modes, plain and helpers.mimi_affine_rig weights; a decode stream of 72 frames (latent positions 0 .. 143, past
70 + 64 + 8) in calls of 1, 3 and 8 frames, the rows tap.  Unit and bar are tests/test_mimi_f64_cpu.py's:
helpers.mimi_errors (per utterance and latent step, max |value - float64| / the utterance's largest |float64
value|), e32 = the float32 oracle's largest figure on the stream, bar = helpers.MIMI_BAR_MARGIN x e32, all computed
in the run.

Each defect (mimi_window_ref.DEFECTS) is put into the float32 oracle's attention through TransformerRef's ``keep``
/ ``softmax_av`` hooks and must miss the bar by 2 x at least on some step at or after the first one whose range
starts past key 0 (mimi_window_ref.first_windowed):
  late / early   the range starts one key late / early;
  aligned        it starts at k0 rounded down to a multiple of 64;
  chunk          the 64-key chunk (counted from k0) holding its middle key is dropped, on the k0 > 0 path;
  no_rescale     online softmax over 64-key chunks from k0 without the exp(m_old - m_new) rescale -- its figure is
                 taken over every step whose range has a second chunk (more than 64 live keys; a row on which
                 the later chunk does not raise the maximum shows nothing, as tests/test_f64_long_cpu.py found:
                 here it clears the 2 x on the stream as a whole, in all four cases);
  tail           the last, partial chunk read as a full one: the keys past k1 that the call has already written
                 (a later frame's in the mlx mode, a later row's in the causal mode).
Measured (err / bar on the worst step, mlx / mlx rigged / causal / causal rigged): late 1.8e3 / 5.7e3 / 2.1e3 /
7.0e3, early 1.8e3 / 6.2e3 / 1.6e3 / 6.7e3, aligned 9.5e3 / 2.7e4 / 8.9e3 / 2.9e4, chunk 4.4e4 / 1.1e5 / 4.0e4 /
1.3e5, no_rescale 1.2e3 / 7.6e3 / 9.8e2 / 8.5e3, tail 5.1e3 / 1.5e4 / 4.4e3 / 1.6e4.

Control: on the same stream cut before position context - 1 (34 frames: every range starts at key 0, and one key
later would still be key 0's clamp) late, early, aligned and chunk are exact no-ops -- bit-identical rows -- which
is why the short streams of the other suites cannot see them."""
import numpy as np
import pytest

import mimi_stream_ref as sr
import mimi_window_ref as wr
from helpers import MIMI_BAR_MARGIN, mimi_affine_rig, mimi_errors, mimi_pair

CONTEXT, FRAMES, CALLS = 70, 72, (1, 3, 8)
CASES = [pytest.param(mode, rig, id=f"{mode}{'-affine_rig' if rig else ''}")
         for mode in wr.MODES for rig in (None, mimi_affine_rig)]
_REFS = {}


def _case(mode, rig, frames=FRAMES):
    """(m, float32 oracle, codes, calls, mimi_window_ref.decode_pair reference) of the stream's first ``frames``."""
    m, _, o32, o64 = mimi_pair("tiny", mode, rig, CONTEXT)
    codes = np.random.default_rng(21).integers(0, m.bins, (2, m.n_q, FRAMES)).astype(np.int32)[:, :, :frames]
    calls = wr.schedule(frames, CALLS)
    key = (mode, rig, frames)
    if key not in _REFS:
        _REFS[key] = wr.decode_pair(o32, o64, codes, calls, pcm=False)
    return m, o32, codes, calls, _REFS[key]


def _spoiled_rows(o32, kind, codes, calls):
    with wr.spoiled(o32.dec_tr, kind):
        return wr.decode_stream(o32, codes, calls, pcm=False)["rows"]


@pytest.mark.parametrize("mode,rig", CASES)
def test_stream_reaches_two_chunks_and_a_tail(mode, rig):
    """The stream's geometry: ranges start past key 0 from ``first_windowed`` on, hold context (+ 2) keys -- one
    chunk and a partial one -- and the last position is past context + 64 + 8; the hooks restated without a defect
    are the oracle's own mask, bit for bit."""
    m, o32, codes, calls, ref = _case(mode, rig)
    s = m.downsample_stride
    assert FRAMES * s - 1 >= CONTEXT + wr.CHUNK + 8
    p0 = wr.first_windowed(m)
    live = CONTEXT + (s if mode == "mlx" else 0)
    assert wr.CHUNK < live < 2 * wr.CHUNK
    off = 0
    for n in calls:
        T = n * s
        keep = o32.dec_tr.keep(off, T, off + T, s)
        u, k1 = wr.window(m, off, T, s)
        first = keep.argmax(-1)
        assert np.array_equal(first > 0, off + np.arange(T) >= p0)
        assert np.array_equal(keep.sum(-1)[first > 0], np.full(int((first > 0).sum()), live))
        assert np.array_equal(first, np.maximum(0, u)) and np.array_equal(T + off - 1 - keep[:, ::-1].argmax(-1), k1)
        off += T
    assert np.array_equal(_spoiled_rows(o32, "none", codes, calls), ref["f32"]["rows"])
    assert 0 < ref["e32"]["rows"] < 1e-5


@pytest.mark.parametrize("mode,rig", CASES)
def test_a_call_of_several_frames_is_the_frames_one_by_one(mode, rig):
    """OracleMimi.decode_steps: in a call of n frames each frame sees the keys a call of its own would (float64:
    the two agree to its rounding), with and without the SEANet; decode_step is its n = 1."""
    m, _, o32, o64 = mimi_pair("tiny", mode, rig, CONTEXT)
    codes = np.random.default_rng(21).integers(0, m.bins, (2, m.n_q, FRAMES)).astype(np.int32)[:, :, :44]
    calls = wr.schedule(44, CALLS)
    many = wr.decode_stream(o64, codes, calls, pcm=True)
    one = wr.decode_stream(o64, codes, [1] * 44, pcm=True)
    assert float(mimi_errors(many["rows"], one["rows"]).max()) < 1e-12
    assert float(mimi_errors(many["pcm"], one["pcm"], m.frame_size).max()) < 1e-12
    rows_only = wr.decode_stream(o64, codes, calls, pcm=False)
    assert np.array_equal(rows_only["rows"], many["rows"])
    o32.reset_state()
    a = [o32.decode_step(codes[:, :, f: f + 1]) for f in range(3)]
    o32.reset_state()
    b = [o32.decode_steps(codes[:, :, f: f + 1]) for f in range(3)]
    o32.reset_state()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("mode,rig", CASES)
def test_defects_miss_the_bar_past_the_window(mode, rig, capsys):
    m, o32, codes, calls, ref = _case(mode, rig)
    e32 = ref["e32"]["rows"]
    bar = MIMI_BAR_MARGIN * e32
    p0 = wr.first_windowed(m)
    two_chunks = wr.CHUNK                        # the first position with more than 64 live keys, in either mode
    lines = []
    for kind in wr.DEFECTS:
        err = mimi_errors(_spoiled_rows(o32, kind, codes, calls), ref["f64"]["rows"])
        fig = float(err[:, two_chunks if kind == "no_rescale" else p0:].max())
        lines.append(f"mimi-window tiny-{mode}{'-affine_rig' if rig else ''} {kind}: {fig / bar:.1f} x bar (e32 {e32:.2e})")
        assert fig >= 2 * bar, f"{kind}: {fig / bar:.2f} x bar does not miss it by 2 x"
    with capsys.disabled():
        print("\n" + "\n".join(lines))


@pytest.mark.parametrize("mode,rig", CASES)
def test_range_defects_are_noops_before_the_window(mode, rig):
    """The control: cut before position context - 1 the four range defects change nothing, bit for bit."""
    m, _, _, _, _ = _case(mode, rig)
    frames = (CONTEXT - 1) // m.downsample_stride
    assert frames * m.downsample_stride - 1 < CONTEXT - 1
    m, o32, codes, calls, ref = _case(mode, rig, frames)
    for kind in wr.RANGE_NOOPS:
        assert np.array_equal(_spoiled_rows(o32, kind, codes, calls), ref["f32"]["rows"]), kind


@pytest.mark.parametrize("context,mode,rig", wr.cases(wr.ENCODE_CONTEXTS) + [(wr.ONE_SHOT_CONTEXT, "causal", None),
                                                                              (wr.ONE_SHOT_CONTEXT, "mlx", None)])
def test_window_clips_have_no_code_near_a_tie(context, mode, rig):
    """The encode clips of tests/test_mimi_window_gpu.py, for the oracle alone: no code's RVQ margin is under
    RVQ_TIE (so the share the GPU test may leave out, 1 % at the most, is not used up by the references), and the
    float32 and float64 oracles choose the same codes."""
    m, _, o32, o64 = mimi_pair("tiny", mode, rig, context)
    if context == wr.ONE_SHOT_CONTEXT:
        from helpers import mimi_pcm_clip
        pcm = mimi_pcm_clip(wr.ONE_SHOT_FRAMES * m.frame_size, wr.ONE_SHOT_SEED)[None, None]
        c32, mg = o32.encode(pcm, with_margins=True)
        assert np.array_equal(c32, o64.encode(pcm))
        assert int((mg < sr.RVQ_TIE).sum()) * 100 <= mg.size, float(mg.min())
        return
    for seed in wr.ENCODE_SEEDS:
        _, ref = wr.encode_case(context, mode, rig, seed)
        mg = ref["f32"]["margins"]
        assert int((mg < sr.RVQ_TIE).sum()) == 0, (seed, float(mg.min()))
        assert np.array_equal(ref["f32"]["codes"], ref["f64"]["codes"])


def test_kv_read_refuses_a_null_codec():
    """mimi_kv_read checks its arguments before any device call (the ranges: tests/test_mimi_window_gpu.py)."""
    from csm_mlx import _lib
    with pytest.raises(ValueError):
        _lib.check(_lib.lib().mimi_kv_read(None, 0, 0, 0, 0, 1, None, None))
