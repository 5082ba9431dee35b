"""The whole Mimi codec on the GPU against the float64 oracle, element-wise.

Both configs (tiny, mimi_202407) and both attention modes; one-shot decode (B = 2, F = 12), streaming
decode_step (B = 1, 3 and 9, 4 frames -- at B = 9 the codec transformer sees 18 rows a frame: the tiled
split-K linears instead of the decode GEMV) and encode (the 2 s + 480-sample clip, B = 2: an odd number of
25 Hz steps, the downsample's replicate edge).

Taps: ``rows`` (MimiCodec.debug_rows: the pre-RVQ latent after encode, the decoder transformer's output after
decode / decode_step) and the PCM.
Unit (helpers.mimi_errors): per utterance and per 1920-sample frame (per latent step for rows),
max |got - float64| / the utterance's largest |float64 value| of that tap.
e32 = the float32 oracle's figure in that unit (its maximum over the case), computed each run.
Bar: engine figure <= helpers.MIMI_BAR_MARGIN (2) x e32 on every frame of every utterance;
tests/test_mimi_f64_cpu.py holds what makes that mean something and caps the margin.
The measured engine / e32 ratios are printed per tap and case (DESIGN.md section 2.1 records them).

Every case runs twice: on the synthetic weights, and ("-affine_rig") on helpers.mimi_affine_rig's -- LayerNorm
weights and biases, per-channel layer scales and cluster usages that are not degenerate, the decode codes holding
the two bins under the usage clamp in every codebook (tests/test_norm_rig_cpu.py: one such operand wrong misses the
bar by 4e3 x at least).  On the rigged weights the encode codes are also held bit-exact against the float32
oracle."""
import numpy as np
import pytest

from helpers import MIMI_BAR_MARGIN, mimi_affine_rig, mimi_errors, mimi_pair, mimi_pcm_clip, mimi_place_clamped

pytestmark = pytest.mark.gpu

_NAMES = [(n, mode) for n in ("tiny", "mimi_202407") for mode in ("mlx", "causal")]
RIGGED = [pytest.param(n, mode, mimi_affine_rig, id=f"{n}-{mode}-affine_rig") for n, mode in _NAMES]
CONFIGS = [pytest.param(n, mode, None, id=f"{n}-{mode}") for n, mode in _NAMES] + RIGGED
RVQ_TIE = 1e-5       # oracle RVQ margin below which a code is a tie at float32 resolution (tests/test_batched_long_gpu.py)
STREAM_B, STREAM_FRAMES = 9, 4

_CODECS, _REFS = {}, {}


def _codec(name, mode, rig=None):
    """One codec per config, mode and rig (max_batch 9 serves every case), kept for the module."""
    if (name, mode, rig) not in _CODECS:
        from csm_mlx.mimi import MimiCodec
        m, w, _, _ = mimi_pair(name, mode, rig)
        _CODECS[name, mode, rig] = MimiCodec(m, max_batch=STREAM_B, max_frames=200).load_weights(w)
    return _CODECS[name, mode, rig]


def _tag(name, mode, rig):
    return f"{name}-{mode}" + ("" if rig is None else "-affine_rig")


def _reference(name, mode, case, rig=None):
    """{tap: (float64 values, float32 oracle's values)} of a case, computed once and left unchanged.
    With a rig the codes hold each codebook's two clamped bins (helpers.mimi_place_clamped)."""
    key = (name, mode, case, rig)
    if key in _REFS:
        return _REFS[key]
    m, _, o32, o64 = mimi_pair(name, mode, rig)
    place = (lambda c: c) if rig is None else (lambda c: mimi_place_clamped(m, c))
    out = {}
    if case == "decode":
        codes = place(np.random.default_rng(5).integers(0, m.bins, (2, m.n_q, 12)).astype(np.int32))   # test_decode_parity's
        for tag, o in (("f64", o64), ("f32", o32)):
            out[tag] = {"pcm": o.decode(codes), "rows": o.taps["rows"]}
    elif case == "stream":
        codes = place(np.random.default_rng(9).integers(0, m.bins, (STREAM_B, m.n_q, STREAM_FRAMES)).astype(np.int32))
        for tag, o in (("f64", o64), ("f32", o32)):
            o.reset_state()
            pcm, rows = [], []
            for f in range(STREAM_FRAMES):
                pcm.append(o.decode_step(codes[:, :, f: f + 1]))
                rows.append(o.taps["rows"])
            o.reset_state()
            out[tag] = {"pcm": np.concatenate(pcm, axis=2), "rows": np.concatenate(rows, axis=1)}
    else:
        codes = np.stack([mimi_pcm_clip(24000 * 2 + 480, 1), mimi_pcm_clip(24000 * 2 + 480, 2)])[:, None, :]
        for tag, o in (("f64", o64), ("f32", o32)):
            o.encode(codes)
            out[tag] = {"rows": o.taps["rows"]}
    out["input"] = codes
    _REFS[key] = out
    return out


def _hold(label, got, ref, frame, capsys, rows_b=slice(None)):
    """got {tap: array}; every frame of every utterance within the bar, the ratios printed."""
    parts, bad = [], []
    for tap, g in got.items():
        r64, r32 = ref["f64"][tap][rows_b], ref["f32"][tap][rows_b]
        fr = frame if tap == "pcm" else None
        e32 = float(mimi_errors(r32, r64, fr).max())
        err = mimi_errors(g, r64, fr)
        parts.append(f"{tap}={err.max():.2e}({err.max() / e32:.2f}x e32 {e32:.2e})")
        if not float(err.max()) <= MIMI_BAR_MARGIN * e32:
            bad.append(f"{tap}: {err.max():.3e} > {MIMI_BAR_MARGIN} x e32 = {MIMI_BAR_MARGIN * e32:.3e} at (utterance, frame) "
                       f"{np.unravel_index(int(err.argmax()), err.shape)}")
    line = f"mimi-f64 {label}: " + " ".join(parts)
    with capsys.disabled():
        print("\n" + line)
    assert not bad, line + "\n" + "\n".join(bad)


@pytest.mark.parametrize("name,mode,rig", CONFIGS)
def test_decode(name, mode, rig, capsys):
    codec, ref = _codec(name, mode, rig), _reference(name, mode, "decode", rig)
    m = codec.m
    pcm = codec.decode(ref["input"])
    rows = codec.debug_rows().reshape(2, 12 * m.downsample_stride, m.dimension)
    _hold(f"{_tag(name, mode, rig)} decode B=2 F=12", {"rows": rows, "pcm": pcm}, ref, m.frame_size, capsys)


@pytest.mark.parametrize("B", [1, 3, STREAM_B])
@pytest.mark.parametrize("name,mode,rig", CONFIGS)
def test_decode_step(name, mode, rig, B, capsys):
    """The first B utterances of the case's codes (the oracle ran all 9 once; utterances are independent)."""
    codec, ref = _codec(name, mode, rig), _reference(name, mode, "stream", rig)
    m = codec.m
    codes = ref["input"][:B]
    codec.reset_state(B)
    pcm, rows = [], []
    for f in range(STREAM_FRAMES):
        pcm.append(codec.decode_step(codes[:, :, f: f + 1]))
        rows.append(codec.debug_rows().reshape(B, m.downsample_stride, m.dimension))
    got = {"rows": np.concatenate(rows, axis=1), "pcm": np.concatenate(pcm, axis=2)}
    _hold(f"{_tag(name, mode, rig)} decode_step B={B} F={STREAM_FRAMES}", got, ref, m.frame_size, capsys, rows_b=slice(0, B))


@pytest.mark.parametrize("name,mode,rig", CONFIGS)
def test_encode_latent(name, mode, rig, capsys):
    codec, ref = _codec(name, mode, rig), _reference(name, mode, "encode", rig)
    m = codec.m
    codes = codec.encode(ref["input"])
    Tf = codes.shape[2]
    assert ref["f64"]["rows"].shape == (2, Tf, m.dimension)
    _hold(f"{_tag(name, mode, rig)} encode B=2 Tf={Tf}", {"rows": codec.debug_rows().reshape(2, Tf, m.dimension)}, ref, None, capsys)


@pytest.mark.parametrize("name,mode,rig", RIGGED)
def test_encode_codes_bit_exact_rigged(name, mode, rig):
    """The encode clip's codes on the rigged weights (usage-scaled codebooks, two rows per codebook under the clamp)
    against the float32 oracle, bit-exact.  A code may part from the oracle only where the oracle's own RVQ margin
    for it is below RVQ_TIE; the oracle is then run again with the runner-up forced there
    (OracleMimi.encode(force=...)) and everything after must agree.  At most 1 % of the codes may take that;
    tests/test_norm_rig_cpu.py asserts that the float32 and float64 oracles alone need none."""
    codec = _codec(name, mode, rig)
    _, _, o32, _ = mimi_pair(name, mode, rig)
    pcm = _reference(name, mode, "encode", rig)["input"]
    codes = codec.encode(pcm)
    ref, margins = o32.encode(pcm, with_margins=True)
    assert codes.shape == ref.shape
    forced = []
    while not np.array_equal(codes, ref):
        b, t, k = min((int(b), int(t), int(k)) for b, k, t in np.argwhere(codes != ref))      # a frame's first codebook
        assert margins[b, k, t] < RVQ_TIE, (f"code (utterance {b}, codebook {k}, frame {t}) differs at oracle margin "
                                            f"{margins[b, k, t]:.2e}; {int((codes != ref).sum())} of {codes.size} differ")
        forced.append((b, k, t))
        assert len(forced) <= codes.size // 100, forced
        ref, margins = o32.encode(pcm, with_margins=True, force=forced)
    print(f"{_tag(name, mode, rig)}: {codes.size} encode codes, near-ties taken {forced}")
