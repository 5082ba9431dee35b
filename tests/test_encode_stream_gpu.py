"""The streaming Mimi encode (MimiCodec.encode_slots / encode_step, StreamEncoder) against the oracle alone, frame
by frame (tests/mimi_stream_ref.py), in float64 for the latent and float32 for the codes.

Bars, the ones of tests/test_mimi_f64_gpu.py's encode: every frame's pre-RVQ latent row (MimiCodec.debug_rows)
within helpers.MIMI_BAR_MARGIN x e32 of the float64 reference, e32 the float32 reference's own figure on that
stream; codes equal to the float32 reference's, except a frame's first differing code where the oracle's RVQ
margin is below RVQ_TIE.  tests/test_encode_stream_cpu.py asserts that the rigged-weight streams served here have
no such code, and that a wrong attention mode or a wrong stream start misses the latent bar by >= 1e3 x.
"""
import numpy as np
import pytest

import mimi_stream_ref as sr
from helpers import MIMI_BAR_MARGIN, mimi_affine_rig, mimi_pcm_clip
from rigs import mimi_codec

pytestmark = pytest.mark.gpu

FS = 1920
TINY = [pytest.param(mode, rig, id=f"{mode}{'-affine_rig' if rig else ''}")
        for mode in ("mlx", "causal") for rig in (None, mimi_affine_rig)]


def hold(tag, codec, codes, n, served):
    """After a call of n frames: served = [(row b, reference, first frame f0)]; rows and codes of each."""
    rows = codec.debug_rows().reshape(codes.shape[0], n, -1)
    for b, ref, f0 in served:
        err = sr.row_errors(rows[b], ref, f0)
        bar = MIMI_BAR_MARGIN * ref["e32"]
        print(f"encode-stream {tag} row {b} frames {f0}..{f0 + n - 1}: latent {err.max():.2e} = {err.max() / ref['e32']:.2f} x e32")
        assert float(err.max()) <= bar, (tag, b, f0, err.tolist(), bar)
        bad = sr.code_mismatches(codes[b], ref, f0)
        assert not bad, (tag, b, f0, bad)


@pytest.mark.parametrize("mode,rig", TINY)
def test_timeline(mode, rig):
    """15 frames in calls of 1, 3, 2, 5, 1, 3 on three slots: one long stream (past the 5-frame attention window), a
    slot reset between two streams, and a slot that sits out two calls on noise and goes on without a reset;
    a one-shot encode and a decoder slot pass in between move no encode stream."""
    m, codec, _ = mimi_codec("tiny", mode, max_batch=3, max_frames=40, rig=rig)
    case = {k: sr.stream_case("tiny", mode, rig, k) for k in ("long", "first", "second", "gap")}
    noise = np.random.default_rng(5).normal(0, 3.0, 7 * FS).astype(np.float32)
    for b in range(3):
        codec.encode_slot_reset(b)
    at = {"long": 0, "first": 0, "second": 0, "gap": 0}
    f = 0
    for call, n in enumerate([1, 3, 2, 5, 1, 3]):
        if call == 2:
            codec.encode_slot_reset(1)
        if call == 3:    # neither the one-shot encode (its own KV) nor the decoder's slot mode touches the streams
            codec.encode(mimi_pcm_clip(3 * FS + 480, 9)[None, None])
            codec.slot_reset(0)
            codec.decode_slots(np.zeros((4, 3, m.n_q), np.int32), 2, 0, [True, False, True])
        names = ["long", "first" if call < 2 else "second", "gap"]
        active = [True, True, call not in (2, 3)]
        pcm = np.zeros((3, n * FS), np.float32)
        served = []
        for b, k in enumerate(names):
            if active[b]:
                pcm[b] = case[k][0][at[k] * FS: (at[k] + n) * FS]
                served.append((b, case[k][1], at[k]))
                at[k] += n
            else:
                pcm[b] = noise[(f - 4) * FS: (f - 4 + n) * FS]
        codes = codec.encode_slots(pcm, active)
        assert codes.shape == (3, m.n_q, n) and codes.dtype == np.int32
        hold(f"tiny-{mode} call {call}", codec, codes, n, served)
        f += n
    assert at == {"long": 15, "first": 4, "second": 11, "gap": 8}


@pytest.mark.parametrize("mode", ["mlx", "causal"])
def test_mimi_202407_shapes(mode):
    """The real tile plans, bins = 2048 and n_q = 32: two streams, 4 frames in calls of 1, 2, 1."""
    m, codec, _ = mimi_codec("mimi_202407", mode, max_batch=2, max_frames=16, rig=mimi_affine_rig)
    case = [sr.stream_case("mimi_202407", mode, mimi_affine_rig, k) for k in ("a", "b")]
    for b in range(2):
        codec.encode_slot_reset(b)
    f = 0
    for n in (1, 2, 1):
        codes = codec.encode_slots(np.stack([c[0][f * FS: (f + n) * FS] for c in case]))
        assert codes.shape == (2, 32, n)
        hold(f"mimi_202407-{mode} frames {f}..", codec, codes, n, [(b, case[b][1], f) for b in range(2)])
        f += n


@pytest.mark.parametrize("mode", ["mlx", "causal"])
def test_encode_step(mode):
    """moshi's call: B = 2, five frames as 2 + 3, then reset_state() and the first two again, from position 0."""
    m, codec, _ = mimi_codec("tiny", mode, max_batch=3, max_frames=40, rig=mimi_affine_rig)
    case = [sr.stream_case("tiny", mode, mimi_affine_rig, k) for k in ("step_a", "step_b")]
    pcm = np.stack([c[0] for c in case])
    for f0, n, shape3 in ((0, 2, True), (2, 3, False)):
        x = pcm[:, f0 * FS: (f0 + n) * FS]
        codes = codec.encode_step(x[:, None, :] if shape3 else x)
        assert codes.shape == (2, m.n_q, n)
        hold(f"tiny-{mode} encode_step", codec, codes, n, [(b, case[b][1], f0) for b in range(2)])
    codec.reset_state()
    codes = codec.encode_step(pcm[:, None, : 2 * FS])
    hold(f"tiny-{mode} encode_step after reset_state", codec, codes, 2, [(b, case[b][1], 0) for b in range(2)])


def test_refusals():
    m, codec, _ = mimi_codec("tiny", "causal", max_batch=3, max_frames=40, rig=mimi_affine_rig)
    with pytest.raises(RuntimeError):
        codec.encode_slots(np.zeros((1, FS), np.float32))
    codec.encode_slot_reset(0)
    with pytest.raises(ValueError):
        codec.encode_slots(np.zeros((4, FS), np.float32))
    with pytest.raises(ValueError):
        codec.encode_slots(np.zeros((1, 0), np.float32))
    with pytest.raises(ValueError):
        codec.encode_slots(np.zeros((1, FS + 1), np.float32))
    with pytest.raises(ValueError):
        codec.encode_slot_reset(3)


@pytest.mark.parametrize("mode", ["mlx", "causal"])
def test_capacity(mode):
    """max_frames = 8: 32 latent positions, a slot may stand at 28 at the most.  A call that would take an active
    slot further is refused with nothing launched or advanced: the next call matches the reference.  A slot
    idling at the end of its cache (no room for the pass's keys) leaves its neighbour's stream right."""
    m, codec, _ = mimi_codec("tiny", mode, max_batch=2, max_frames=8, rig=mimi_affine_rig)
    (pa, ra), (pb, rb) = (sr.stream_case("tiny", mode, mimi_affine_rig, k) for k in ("cap_a", "cap_b"))
    pcm = np.stack([pa, pb])
    for b in range(2):
        codec.encode_slot_reset(b)

    def call(fa, fb, n, active):
        x = np.stack([pcm[0, fa * FS: (fa + n) * FS], pcm[1, fb * FS: (fb + n) * FS]])
        codes = codec.encode_slots(x, active)
        hold(f"tiny-{mode} capacity", codec, codes, n, [(b, r, f0) for b, r, f0 in ((0, ra, fa), (1, rb, fb)) if active[b]])

    call(0, 0, 11, [True, True])         # both at 22
    call(11, 11, 2, [False, True])       # slot 1 at 26
    with pytest.raises(ValueError):      # slot 1: 26 + 4 + 4 > 32
        call(11, 13, 2, [True, True])
    call(11, 13, 1, [True, True])        # 24 and 28
    with pytest.raises(ValueError):
        call(12, 13, 1, [False, True])
    call(12, 13, 2, [True, False])       # slot 1 idles at 28: its rows run in the spare cache row


def test_stream_encoder():
    """Two callers fed ragged chunks, one push per tick."""
    from csm_mlx import StreamEncoder
    from csm_mlx.tokenizers import audio_codes_to_frames
    m, codec, _ = mimi_codec("tiny", "mlx", max_batch=3, max_frames=40, rig=mimi_affine_rig)
    (pa, ra), (pb, rb) = (sr.stream_case("tiny", "mlx", mimi_affine_rig, k) for k in ("push_a", "push_b"))
    enc = StreamEncoder(codec)
    ha, hb = enc.open(), enc.open()
    ia = ib = 0
    for na, nb in [(1000, 2500), (2500, 340), (4000, 3000), (1920, 1), (0, 5000), (10 ** 6, 10 ** 6)]:
        out = enc.push({h: x[i: i + n] for h, x, i, n in ((ha, pa, ia, na), (hb, pb, ib, nb)) if n})
        ia, ib = ia + na, ib + nb
        assert all(v.shape[0] == m.n_q for v in out.values())
    for h, ref, frames in ((ha, ra, 6), (hb, rb, 5)):
        codes = enc.codes(h)
        assert codes.shape == (m.n_q, frames) and enc.pending(h) == 0
        assert not sr.code_mismatches(codes, ref), sr.code_mismatches(codes, ref)
        tok, mask = enc.rows(h, [998, 5, 999], 1)
        a_tok, a_mask = audio_codes_to_frames(codes)
        assert np.array_equal(tok[3:], a_tok) and np.array_equal(mask[3:], a_mask)
        assert np.array_equal(tok[:3, -1], [998, 5, 999]) and mask[:3, -1].all() and not mask[:3, :-1].any()
    enc.close(ha)
    hc = enc.open()    # slot 0 again, from position 0
    assert not sr.code_mismatches(enc.push({hc: pa[: 2 * FS]})[hc], ra)
