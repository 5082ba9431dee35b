"""What makes the streaming-encode bars of tests/test_encode_stream_gpu.py mean something, and StreamEncoder's
host logic (no GPU).

The reference is tests/mimi_stream_ref.py: the oracle's pieces composed frame by frame.  On
helpers.mimi_affine_rig weights:
  * causal mode: it equals OracleMimi.encode of the same audio (streaming is the one-shot encode split over calls);
  * moshi_mlx mode: the one-shot encode differs by design (every key of the call shown to every row) and its
    latent misses MIMI_BAR_MARGIN x e32 by >= 1e3 x, so a wrong attention mode cannot pass the bar;
  * a zero downsample history at stream start instead of the edge sample misses the bar on frame 0, and only there;
  * no code of the streams the GPU tests serve is near an RVQ tie (so there every code must match).
"""
import numpy as np
import pytest

import mimi_stream_ref as sr
from helpers import MIMI_BAR_MARGIN, mimi_affine_rig, mimi_errors, mimi_pair

FACT_CASES = [("tiny", "long"), ("tiny", "second"), ("mimi_202407", "a")]


def _one_shot(name, mode, pcm):
    _, _, o32, o64 = mimi_pair(name, mode, mimi_affine_rig)
    out = {}
    for tag, o in (("f32", o32), ("f64", o64)):
        codes = o.encode(pcm[None, None])
        out[tag] = {"codes": codes[0], "rows": o.taps["rows"][0]}
    return out


@pytest.mark.parametrize("name,stream", FACT_CASES)
def test_causal_stream_is_the_one_shot_encode(name, stream):
    pcm, ref = sr.stream_case(name, "causal", mimi_affine_rig, stream)
    one = _one_shot(name, "causal", pcm)
    for tag in ("f32", "f64"):
        assert np.array_equal(ref[tag]["codes"], one[tag]["codes"]), tag
    r, o = ref["f64"]["rows"], one["f64"]["rows"]
    rel = np.abs(r - o).max() / np.abs(o).max()
    print(f"{name} causal: frame-wise vs one-shot float64 latent {rel:.2e}")
    assert rel <= 1e-12
    # float32: another summation order at most (BLAS shapes), far inside the bar's unit
    assert float(mimi_errors(ref["f32"]["rows"][None], one["f32"]["rows"][None]).max()) <= MIMI_BAR_MARGIN * ref["e32"]


@pytest.mark.parametrize("name,stream", FACT_CASES)
def test_mlx_one_shot_misses_the_bar(name, stream):
    pcm, ref = sr.stream_case(name, "mlx", mimi_affine_rig, stream)
    one = _one_shot(name, "mlx", pcm)
    err = float(sr.row_errors(one["f32"]["rows"], ref).max())
    print(f"{name} mlx: one-shot latent against the frame-wise float64 {err:.2e} = {err / (MIMI_BAR_MARGIN * ref['e32']):.1e} x bar")
    assert err >= 1e3 * MIMI_BAR_MARGIN * ref["e32"]


@pytest.mark.parametrize("mode", ["mlx", "causal"])
@pytest.mark.parametrize("name,stream", FACT_CASES)
def test_zero_stream_start_misses_the_bar_on_frame_0(name, stream, mode):
    _, _, o32, _ = mimi_pair(name, mode, mimi_affine_rig)
    pcm, ref = sr.stream_case(name, mode, mimi_affine_rig, stream)
    err = sr.row_errors(sr.stream_reference(o32, pcm, zero_start=True)["rows"], ref)
    bar = MIMI_BAR_MARGIN * ref["e32"]
    print(f"{name} {mode}: zero-start frame 0 {err[0] / bar:.1e} x bar, later frames {err[1:].max() / bar:.2f} x bar")
    assert err[0] >= 1e3 * bar
    assert err[1:].max() <= bar


@pytest.mark.parametrize("mode", ["mlx", "causal"])
@pytest.mark.parametrize("name", sorted(sr.STREAMS))
def test_served_streams_have_no_near_tie(name, mode):
    for stream in sr.STREAMS[name]:
        _, ref = sr.stream_case(name, mode, mimi_affine_rig, stream)
        assert ref["e32"] < 1e-5, (stream, ref["e32"])
        assert np.array_equal(ref["f32"]["codes"], ref["f64"]["codes"]), stream
        mg = float(ref["f32"]["margins"].min())
        print(f"{name} {mode} {stream}: e32 {ref['e32']:.2e}, smallest RVQ margin {mg:.2e}")
        assert mg >= sr.MIN_MARGIN[name], (stream, mg)


# ----------------------------------------------------------------------------- StreamEncoder host logic
class _Args:
    frame_size, n_q = 1920, 3


class _StandIn:
    """encode_slots / encode_slot_reset / encode of a codec whose code for a frame is a function of the frame's
    samples and its index in the stream: a dropped, repeated or misplaced frame changes the codes."""
    m, max_batch = _Args, 3

    def __init__(self):
        self.pos = [None] * self.max_batch
        self.passes = []

    @staticmethod
    def _code(frame, pos):
        base = int(np.abs(frame.astype(np.float64)).sum() * 1e3) + 31 * pos
        return [(base + 7 * k) % 2048 for k in range(_Args.n_q)]

    def encode_slot_reset(self, b):
        self.pos[b] = 0

    def encode_slots(self, pcm, active=None):
        B, N = pcm.shape
        assert N % _Args.frame_size == 0 and N > 0 and B <= self.max_batch
        n = N // _Args.frame_size
        act = np.ones(B, bool) if active is None else np.asarray(active, bool)
        self.passes.append((n, act.copy()))
        out = np.full((B, _Args.n_q, n), -1, np.int32)
        for b in np.flatnonzero(act):
            assert self.pos[b] is not None, "slot used before a reset"
            for j in range(n):
                out[b, :, j] = self._code(pcm[b, j * 1920: (j + 1) * 1920], self.pos[b])
                self.pos[b] += 1
        return out

    def encode(self, pcm):    # one-shot on whole frames, for tokenize_segment
        x = np.asarray(pcm, np.float32).reshape(-1)
        return np.array([self._code(x[j * 1920: (j + 1) * 1920], j) for j in range(x.size // 1920)], np.int32).T[None]


def _audio(n, seed):
    return np.random.default_rng(seed).normal(0, 0.1, n).astype(np.float32)


def test_stream_encoder_ragged_pushes_equal_the_whole_clip():
    from csm_mlx import StreamEncoder
    a, b = _audio(5 * 1920 + 700, 1), _audio(3 * 1920 + 100, 2)
    enc = StreamEncoder(_StandIn())
    ha, hb = enc.open(), enc.open()
    ia = ib = 0
    got_a, got_b = [], []
    for na, nb in [(1000, 0), (2500, 4000), (340, 10), (3000, 1000), (1, 900), (10 ** 6, 10 ** 6)]:
        out = enc.push({h: x[i: i + n] for h, x, i, n in ((ha, a, ia, na), (hb, b, ib, nb)) if n})
        ia, ib = ia + na, ib + nb
        got_a.append(out.get(ha, np.zeros((3, 0), np.int32)))
        got_b.append(out[hb] if hb in out else np.zeros((3, 0), np.int32))
        assert enc.pending(ha) == min(ia, a.size) % 1920 and enc.pending(hb) == min(ib, b.size) % 1920
    whole = StreamEncoder(_StandIn())
    wa, wb = whole.open(), whole.open()
    ref = whole.push({wa: a, wb: b})
    assert ref[wa].shape == (3, 5) and ref[wb].shape == (3, 3)
    assert np.array_equal(np.concatenate(got_a, 1), ref[wa]) and np.array_equal(enc.codes(ha), ref[wa])
    assert np.array_equal(np.concatenate(got_b, 1), ref[wb]) and np.array_equal(enc.codes(hb), ref[wb])
    assert (enc.codes(ha) >= 0).all() and (enc.codes(hb) >= 0).all()      # never an inactive row's
    assert np.array_equal(ref[wa], _StandIn().encode(a)[0])


def test_stream_encoder_passes_take_the_smallest_pending_count():
    from csm_mlx import StreamEncoder
    codec = _StandIn()
    enc = StreamEncoder(codec)
    h0, h1, h2 = enc.open(), enc.open(), enc.open()
    enc.push({h0: _audio(3 * 1920, 3), h1: _audio(1920 + 5, 4), h2: _audio(100, 5)})
    assert [(n, a.tolist()) for n, a in codec.passes] == [(1, [True, True]), (2, [True])]
    assert enc.pending(h1) == 5 and enc.pending(h2) == 100 and enc.codes(h2).shape == (3, 0)


def test_stream_encoder_rows_are_tokenize_segment_rows():
    from csm_mlx import Segment, StreamEncoder
    from csm_mlx import tokenizers
    codec = _StandIn()
    audio, text = _audio(4 * 1920, 6), [998, 11, 12, 13, 999]
    enc = StreamEncoder(codec)
    h = enc.open()
    for i in range(0, audio.size, 1111):
        enc.push({h: audio[i: i + 1111]})
    tokenizers.set_audio_tokenizer(codec, 3)
    try:
        want_t, want_m = tokenizers.tokenize_segment(Segment(2, text, audio), n_audio_codebooks=3)
        assert StreamEncoder(n_audio_codebooks=3).codec is codec           # the registered tokenizer by default
    finally:
        tokenizers._audio_tokenizers.pop(3, None)
    got_t, got_m = enc.rows(h, text, 2)
    assert got_t.dtype == want_t.dtype and got_m.dtype == want_m.dtype
    assert np.array_equal(got_t, want_t) and np.array_equal(got_m, want_m)
    assert got_t.shape == (len(text) + 4 + 1, 4) and not got_t[-1].any()


def test_stream_encoder_recycles_slots():
    from csm_mlx import StreamEncoder
    codec = _StandIn()
    enc = StreamEncoder(codec, slots=2)
    h0, h1 = enc.open(), enc.open()
    with pytest.raises(RuntimeError):
        enc.open()
    enc.push({h0: _audio(1920, 7), h1: _audio(2 * 1920, 8)})
    enc.close(h0)
    h2 = enc.open()
    assert h2 not in (h0, h1) and codec.pos[0] == 0                      # slot 0 again, reset
    x = _audio(1920, 9)
    assert np.array_equal(enc.push({h2: x})[h2], _StandIn().encode(x)[0])
    with pytest.raises(KeyError):
        enc.codes(h0)
