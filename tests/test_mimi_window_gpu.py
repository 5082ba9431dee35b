"""The codec transformer past its attention window, at more than one 64-key chunk: every codec entry point on the
GPU against the float64 oracle, element-wise, on streams and calls whose key ranges start past key 0 (unaligned)
and span a chunk boundary -- the state every product stream is in after 10 s of audio.

attn_block's range per row (csrc/csm_kernels.hip): ATTN_WINDOW (causal mode) k0 = pos - context + 1; ATTN_FRAMES
(mlx mode, slot streams) and ATTN_BLOCK (mlx mode, decode_step) k0 = max(0, call / frame start - context).  Live
keys past the window: causal = context, mlx = context + 2, so the tiny contexts 62 .. 65 give exactly one chunk,
one chunk + 1 .. + 3 keys, and 130 two chunks and a tail, in each mode.

Taps: ``rows`` (MimiCodec.debug_rows) and the PCM, per frame, in helpers.mimi_errors' unit; bar =
helpers.MIMI_BAR_MARGIN x e32, e32 the float32 oracle's largest figure on the frames the case serves, computed each
run.  Codes: equal to the float32 oracle's, except a frame's first differing code where the oracle's RVQ margin is
under RVQ_TIE (mimi_stream_ref.code_mismatches), on 1 % of a case's codes at the most;
tests/test_mimi_window_cpu.py holds that the oracle alone has no such code on these clips, and which faults of a
range the bar sees (one key late or early, an aligned start, a dropped chunk, a missing rescale, a full last chunk:
1e3 .. 1e5 x the bar) and that the shorter streams of the other suites could not.  err / bar per case is printed.

Not reachable, so not covered: the matrix-core tile path with a range that starts past key 0
(attn_prefill_kernel's ATTN_BLOCK branch with kbeg > 0).  launch_attn sends a codec call there only in the mlx mode
without slot positions (ATTN_BLOCK), with rm.T >= 16 rows per utterance: the one-shot encode / decode, which start
at position 0 (kbeg = 0), and never decode_step (rm.T = 2 rows a call); the slot streams run ATTN_FRAMES and the
causal mode ATTN_WINDOW, both on the per-row kernel.

mimi_202407 widths: decode_slots only.  An encode_slots run of 140 frames at these widths in the causal mode was
left out for its reference's time: one stream's oracle pair takes 11 s on an idle CPU (the float64 SEANet encoder and
transformer 7.9 s, the float32 ones 3.1 s), against the few seconds a case may take."""
import numpy as np
import pytest

import mimi_stream_ref as sr
import mimi_window_ref as wr
from helpers import MIMI_BAR_MARGIN, mimi_affine_rig, mimi_errors, mimi_pair, mimi_pcm_clip
from rigs import mimi_codec

pytestmark = pytest.mark.gpu

CALLS = (1, 3, 8)
DECODE = [pytest.param(c, mode, rig, id=f"ctx{c}-{mode}{'-affine_rig' if rig else ''}")
          for c, mode, rig in wr.cases((62, 63, 64, 65, 130))]
ENCODE = [pytest.param(c, mode, rig, id=f"ctx{c}-{mode}{'-affine_rig' if rig else ''}")
          for c, mode, rig in wr.cases(wr.ENCODE_CONTEXTS)]


def _report(label, figs, capsys):
    """figs {tap: (largest error, e32, where)}: every tap within the bar, err / bar printed."""
    parts = [f"{tap}={e:.2e}={e / (MIMI_BAR_MARGIN * e32):.2f}x bar(e32 {e32:.2e})" for tap, (e, e32, _) in figs.items()]
    line = f"mimi-window {label}: " + " ".join(parts)
    with capsys.disabled():
        print("\n" + line)
    bad = [f"{tap}: {e:.3e} > {MIMI_BAR_MARGIN} x e32 = {MIMI_BAR_MARGIN * e32:.3e} at {at}"
           for tap, (e, e32, at) in figs.items() if not e <= MIMI_BAR_MARGIN * e32]
    assert not bad, line + "\n" + "\n".join(bad)


def _stream_figs(m, served, ref, taps, steps=None):
    """served [(name, oracle batch row, frames, {tap: what the engine gave for the stream's first ``frames``
    frames})]: per tap (largest error, e32, where) over the served frames -- each stream an utterance of
    helpers.mimi_errors, cut to what was served for the engine and the float32 oracle alike.
    steps: rows of the rows tap per frame (the decoder's downsample_stride; an encode's latent has 1)."""
    s, fs = m.downsample_stride if steps is None else steps, m.frame_size
    out = {}
    for tap in taps:
        per, fr = (fs, fs) if tap == "pcm" else (s, None)
        worst, e32 = (-1.0, None), 0.0
        for name, b, frames, got in served:
            cut = (lambda a: a[b: b + 1, :, : frames * per]) if tap == "pcm" else (lambda a: a[b: b + 1, : frames * per])
            r64 = cut(ref["f64"][tap])
            e32 = max(e32, float(mimi_errors(cut(ref["f32"][tap]), r64, fr).max()))
            err = mimi_errors(got[tap], r64, fr)[0]
            if float(err.max()) > worst[0]:
                worst = (float(err.max()), (name, int(err.argmax())))
        out[tap] = (worst[0], e32, worst[1])
    return out


def _kv(codec, side, b):
    """Cache row b of every layer, all positions: (layers, 2, heads, S_cap, hd)."""
    from csm_mlx import _lib
    m = codec.m
    S = codec.max_frames * m.downsample_stride + 16
    out = np.zeros((m.num_layers, 2, m.num_heads, S, m.dimension // m.num_heads), np.float32)
    for l in range(m.num_layers):
        _lib.check(_lib.lib().mimi_kv_read(codec._h, side, b, l, 0, S, _lib.ptr(out[l, 0]), _lib.ptr(out[l, 1])))
    return out


@pytest.mark.parametrize("context,mode,rig", DECODE)
def test_decode_slots(context, mode, rig, capsys):
    """Two slots through decode_slots in calls of 1, 3 and 8 frames until slot 0 is context + 70 steps in; slot 1 is
    reset once, shortly after it has passed its window, so that from there on the two slots sit on different sides
    of their windows in the same launch.  Rows and PCM of the three streams (slot 0's, slot 1's two) against the
    oracle's, which ran them as one batch in calls of 8 frames: a stream does not depend on how it is cut into calls.

    Untouched memory (mimi_kv_read): when slot 1 is reset its cache row holds the first stream's keys; at the end
    that row at and past slot 1's position is still what it was then, bit for bit, slot 0's row at and past its
    position is still the zeros it was allocated with, and both hold keys right below their positions."""
    m, _, o32, o64 = mimi_pair("tiny", mode, rig, context)
    s, D = m.downsample_stride, m.dimension
    F = wr.depth_frames(context, s)
    calls = wr.schedule(F, CALLS)
    starts = np.cumsum([0] + calls[:-1])
    r = int(np.flatnonzero(starts >= context // s + 4)[0])           # the call before which slot 1 starts again
    R = int(starts[r])
    assert wr.first_windowed(m) < R * s and 0 < F - R < R
    codes = np.random.default_rng(1000 + context).integers(0, m.bins, (3, m.n_q, F)).astype(np.int32)
    ref = wr.decode_pair(o32, o64, codes, wr.schedule(F, (8,)))
    _, codec, _ = mimi_codec("tiny", mode, max_batch=2, max_frames=F + 8, rig=rig, context=context)
    got = {b: {"rows": [], "pcm": []} for b in range(3)}
    codec.slot_reset(0)
    codec.slot_reset(1)
    one, at1, before = 1, 0, None
    for i, n in enumerate(calls):
        if i == r:
            before = _kv(codec, 0, 1)
            codec.slot_reset(1)
            one, at1 = 2, 0
        f = int(starts[i])
        ring = np.stack([codes[0, :, f: f + n].T, codes[one, :, at1: at1 + n].T], axis=1)      # (n, 2, n_q)
        pcm = codec.decode_slots(ring, n, 0, [True, True])
        rows = codec.debug_rows().reshape(2, n * s, D)
        for slot, b in ((0, 0), (1, one)):
            got[b]["rows"].append(rows[slot].copy())
            got[b]["pcm"].append(pcm[slot].copy())
        at1 += n
    served = [(name, b, frames, {"rows": np.concatenate(got[b]["rows"])[None], "pcm": np.concatenate(got[b]["pcm"])[None, None]})
              for name, b, frames in (("slot 0", 0, F), ("slot 1 before its reset", 1, R), ("slot 1 after it", 2, F - R))]
    tag = f"tiny-{mode}{'-affine_rig' if rig else ''} context {context}"
    _report(f"{tag} decode_slots {F} frames, slot 1 reset at {R}", _stream_figs(m, served, ref, ("rows", "pcm")), capsys)
    kv0, kv1 = _kv(codec, 0, 0), _kv(codec, 0, 1)
    p0, p1 = F * s, (F - R) * s
    assert not kv0[:, :, :, p0:].any(), "slot 0's cache row was written at or past its position"
    assert np.array_equal(kv1[:, :, :, p1:], before[:, :, :, p1:]), "slot 1's cache row changed at or past its position"
    assert before[:, :, :, p1: R * s].any(axis=(0, 1, 2, 4)).all() and not before[:, :, :, R * s:].any()
    assert kv0[:, :, :, :p0].any(axis=(0, 1, 2, 4)).all() and kv1[:, :, :, :p1].any(axis=(0, 1, 2, 4)).all()
    assert not np.array_equal(kv1[:, :, :, :p1], before[:, :, :, :p1])


def test_decode_step(capsys):
    """The non-slot stream: ATTN_BLOCK through the per-row kernel at T = 2.  Context 70, mlx mode, B = 3, 70 frames
    (140 steps: 70 past the window)."""
    context, B, F = 70, 3, 70
    m, _, o32, o64 = mimi_pair("tiny", "mlx", mimi_affine_rig, context)
    codes = np.random.default_rng(1070).integers(0, m.bins, (B, m.n_q, F)).astype(np.int32)
    ref = wr.decode_pair(o32, o64, codes, wr.schedule(F, (8,)))     # (calls of 8 frames: the same stream, sooner)
    _, codec, _ = mimi_codec("tiny", "mlx", max_batch=B, max_frames=F + 8, rig=mimi_affine_rig, context=context)
    codec.reset_state(B)
    pcm, rows = [], []
    for f in range(F):
        pcm.append(codec.decode_step(codes[:, :, f: f + 1]))
        rows.append(codec.debug_rows().reshape(B, m.downsample_stride, m.dimension))
    pcm, rows = np.concatenate(pcm, axis=2), np.concatenate(rows, axis=1)
    served = [(f"utterance {b}", b, F, {"rows": rows[b: b + 1], "pcm": pcm[b: b + 1]}) for b in range(B)]
    _report(f"tiny-mlx-affine_rig context {context} decode_step B={B} {F} frames", _stream_figs(m, served, ref, ("rows", "pcm")), capsys)


def _hold_codes(got, ref, f0, excused):
    """A call's codes (n_q, n) of a stream's frames f0 ..: none differs where the oracle's margin allows no tie;
    ``excused`` counts the frames left out from their first differing code on."""
    bad = sr.code_mismatches(got, ref, f0)
    assert not bad, (f0, bad)
    excused[0] += int((got != ref["f32"]["codes"][:, f0: f0 + got.shape[1]]).any(0).sum())


@pytest.mark.parametrize("context,mode,rig", ENCODE)
def test_encode_slots(context, mode, rig, capsys):
    """Two encode streams to context + 70 steps each on ragged schedules: calls of 1, 3, 2 and 5 frames, slot 1
    sitting out every fourth call (on noise, its stream staying where it was) and finishing after slot 0, which then
    idles.  Every frame's latent row and codes."""
    m, codec, _ = mimi_codec("tiny", mode, max_batch=2, max_frames=wr.depth_frames(context) + 16, rig=rig, context=context)
    fs = m.frame_size
    F = wr.depth_frames(context, m.downsample_stride)
    case = [wr.encode_case(context, mode, rig, seed) for seed in wr.ENCODE_SEEDS]
    noise = np.random.default_rng(5).normal(0, 3.0, 5 * fs).astype(np.float32)
    for b in range(2):
        codec.encode_slot_reset(b)
    at, i, worst, excused, n_codes = [0, 0], 0, [(-1.0, None), (-1.0, None)], [0], 0
    while min(at) < F:
        active = [at[0] < F, at[1] < F and not (i % 4 == 2 and at[0] < F)]
        n = min([(1, 3, 2, 5)[i % 4]] + [F - at[b] for b in range(2) if active[b]])
        pcm = np.stack([case[b][0][at[b] * fs: (at[b] + n) * fs] if active[b] else noise[: n * fs] for b in range(2)])
        codes = codec.encode_slots(pcm, active)
        rows = codec.debug_rows().reshape(2, n, -1)
        for b in range(2):
            if active[b]:
                err = sr.row_errors(rows[b], case[b][1], at[b])
                if float(err.max()) > worst[b][0]:
                    worst[b] = (float(err.max()), at[b] + int(err.argmax()))
                _hold_codes(codes[b], case[b][1], at[b], excused)
                n_codes += codes[b].size
                at[b] += n
        i += 1
    assert at == [F, F] and n_codes == 2 * F * m.n_q and excused[0] * m.n_q * 100 <= n_codes, (at, excused, n_codes)
    tag = f"tiny-{mode}{'-affine_rig' if rig else ''} context {context}"
    for b in range(2):       # each stream against its own e32, as tests/test_encode_stream_gpu.py
        _report(f"{tag} encode_slots slot {b} {F} frames", {"latent": (worst[b][0], case[b][1]["e32"], f"frame {worst[b][1]}")}, capsys)


def _one_shot(mode):
    """(m, codec, oracles) of the one-shot cases: context 70, a codec with room for 100 frames."""
    F = wr.ONE_SHOT_FRAMES
    m, codec, _ = mimi_codec("tiny", mode, max_batch=2, max_frames=F + 4, context=wr.ONE_SHOT_CONTEXT)
    return (m, codec) + mimi_pair("tiny", mode, None, wr.ONE_SHOT_CONTEXT)[2:]


@pytest.mark.parametrize("mode", ["causal", "mlx"])
def test_decode_one_shot(mode, capsys):
    """decode of 100 frames, B = 2.  causal: 200 ATTN_WINDOW rows in one launch, each with its own k0, 130 of them
    past the window.  mlx (the control): every row sees all 200 keys -- four matrix-core tiles, the last key chunk
    partial."""
    m, codec, o32, o64 = _one_shot(mode)
    F = wr.ONE_SHOT_FRAMES
    codes = np.random.default_rng(1100).integers(0, m.bins, (2, m.n_q, F)).astype(np.int32)
    ref = {}
    for tag, o in (("f64", o64), ("f32", o32)):
        ref[tag] = {"pcm": o.decode(codes), "rows": o.taps["rows"]}
    pcm = codec.decode(codes)
    rows = codec.debug_rows().reshape(2, F * m.downsample_stride, m.dimension)
    served = [(f"utterance {b}", b, F, {"rows": rows[b: b + 1], "pcm": pcm[b: b + 1]}) for b in range(2)]
    _report(f"tiny-{mode} context {wr.ONE_SHOT_CONTEXT} decode B=2 F={F}", _stream_figs(m, served, ref, ("rows", "pcm")), capsys)


@pytest.mark.parametrize("mode", ["causal", "mlx"])
def test_encode_one_shot(mode, capsys):
    """encode of an 8 s clip (100 frames, 200 encoder-transformer rows): the latent, and the codes against the
    float32 oracle as tests/test_mimi_f64_gpu.py holds them (a code may part only at an oracle margin under
    RVQ_TIE, the oracle then taking the runner-up there; 1 % of the codes at the most)."""
    m, codec, o32, o64 = _one_shot(mode)
    F = wr.ONE_SHOT_FRAMES
    pcm = mimi_pcm_clip(F * m.frame_size, wr.ONE_SHOT_SEED)[None, None]
    want, margins = o32.encode(pcm, with_margins=True)
    r32 = o32.taps["rows"]
    o64.encode(pcm)
    ref = {"f64": {"rows": o64.taps["rows"]}, "f32": {"rows": r32}}
    codes = codec.encode(pcm)
    assert codes.shape == want.shape == (1, m.n_q, F)
    rows = codec.debug_rows().reshape(1, F, m.dimension)
    figs = _stream_figs(m, [("clip", 0, F, {"rows": rows})], ref, ("rows",), steps=1)
    _report(f"tiny-{mode} context {wr.ONE_SHOT_CONTEXT} encode {F} frames", {"latent": figs["rows"]}, capsys)
    forced = []
    while not np.array_equal(codes, want):
        b, t, k = min((int(b), int(t), int(k)) for b, k, t in np.argwhere(codes != want))
        assert margins[b, k, t] < sr.RVQ_TIE, (f"code (codebook {k}, frame {t}) differs at oracle margin {margins[b, k, t]:.2e}; "
                                               f"{int((codes != want).sum())} of {codes.size} differ")
        forced.append((b, k, t))
        assert len(forced) <= codes.size // 100, forced
        want, margins = o32.encode(pcm, with_margins=True, force=forced)


@pytest.mark.parametrize("mode,rig", [("mlx", None), ("causal", mimi_affine_rig)])
def test_mimi_202407_decode_slots(mode, rig, capsys):
    """The product's widths and true context = 250: two slots through decode_slots in calls of 5 frames to 170 frames
    (340 steps, 90 past the window); slot 1 joins 35 frames late, so for 35 frames the slots sit on different sides
    of their windows, and ends 270 steps in.  The rows tap against the oracle's rows-only stream."""
    F, LATE, N = 170, 35, 5
    m, _, o32, o64 = mimi_pair("mimi_202407", mode, rig)
    assert m.context == 250
    s = m.downsample_stride
    codes = np.random.default_rng(1250).integers(0, m.bins, (2, m.n_q, F)).astype(np.int32)
    ref = wr.decode_pair(o32, o64, codes, [N] * (F // N), pcm=False)
    _, codec, _ = mimi_codec("mimi_202407", mode, max_batch=2, max_frames=F + 2, rig=rig)
    codec.slot_reset(0)
    rows = [[], []]
    for f in range(0, F, N):
        if f == LATE:
            codec.slot_reset(1)
        live = f >= LATE
        ring = np.stack([codes[0, :, f: f + N].T, codes[1, :, max(f - LATE, 0): max(f - LATE, 0) + N].T], axis=1)
        codec.decode_slots(ring, N, 0, [True, live])
        got = codec.debug_rows().reshape(2, N * s, m.dimension)
        rows[0].append(got[0].copy())
        if live:
            rows[1].append(got[1].copy())
    served = [(f"slot {b}", b, frames, {"rows": np.concatenate(rows[b])[None]}) for b, frames in ((0, F), (1, F - LATE))]
    tag = f"mimi_202407-{mode}{'-affine_rig' if rig else ''}"
    _report(f"{tag} decode_slots {F} frames in calls of {N}", _stream_figs(m, served, ref, ("rows",)), capsys)


def test_kv_read_refusals():
    """mimi_kv_read: a side, row, layer or position range outside the codec's is refused; the streaming encoder's
    cache (with its spare row) exists from the first encode_slot_reset on."""
    from csm_mlx import _lib
    m, codec, _ = mimi_codec("tiny", "mlx", max_batch=2, max_frames=8)
    S = 8 * m.downsample_stride + 16
    k = np.zeros((m.num_heads, S, m.dimension // m.num_heads), np.float32)
    read = lambda side, b, layer, first, rows: _lib.check(
        _lib.lib().mimi_kv_read(codec._h, side, b, layer, first, rows, _lib.ptr(k), None))
    read(0, 1, m.num_layers - 1, 0, S)
    for bad in ((2, 0, 0, 0, 1), (0, 2, 0, 0, 1), (0, -1, 0, 0, 1), (0, 0, m.num_layers, 0, 1), (0, 0, 0, 0, S + 1),
                (0, 0, 0, S, 1), (0, 0, 0, -1, 1), (0, 0, 0, 0, 0), (1, 0, 0, 0, 1)):
        with pytest.raises(ValueError):
            read(*bad)
    codec.encode_slot_reset(0)
    read(1, 2, 0, 0, S)
    with pytest.raises(ValueError):
        read(1, 3, 0, 0, 1)
