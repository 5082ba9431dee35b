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
The measured engine / e32 ratios are printed per tap and case (DESIGN.md section 2.1 records them)."""
import numpy as np
import pytest

from helpers import MIMI_BAR_MARGIN, mimi_errors, mimi_pair, mimi_pcm_clip

pytestmark = pytest.mark.gpu

CONFIGS = [pytest.param(n, mode, id=f"{n}-{mode}") for n in ("tiny", "mimi_202407") for mode in ("mlx", "causal")]
STREAM_B, STREAM_FRAMES = 9, 4

_CODECS, _REFS = {}, {}


def _codec(name, mode):
    """One codec per config and mode (max_batch 9 serves every case), kept for the module."""
    if (name, mode) not in _CODECS:
        from csm_mlx.mimi import MimiCodec
        m, w, _, _ = mimi_pair(name, mode)
        _CODECS[name, mode] = MimiCodec(m, max_batch=STREAM_B, max_frames=200).load_weights(w)
    return _CODECS[name, mode]


def _reference(name, mode, case):
    """{tap: (float64 values, float32 oracle's values)} of a case, computed once and left unchanged."""
    key = (name, mode, case)
    if key in _REFS:
        return _REFS[key]
    m, _, o32, o64 = mimi_pair(name, mode)
    out = {}
    if case == "decode":
        codes = np.random.default_rng(5).integers(0, m.bins, (2, m.n_q, 12)).astype(np.int32)   # test_decode_parity's
        for tag, o in (("f64", o64), ("f32", o32)):
            out[tag] = {"pcm": o.decode(codes), "rows": o.taps["rows"]}
    elif case == "stream":
        codes = np.random.default_rng(9).integers(0, m.bins, (STREAM_B, m.n_q, STREAM_FRAMES)).astype(np.int32)
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


@pytest.mark.parametrize("name,mode", CONFIGS)
def test_decode(name, mode, capsys):
    codec, ref = _codec(name, mode), _reference(name, mode, "decode")
    m = codec.m
    pcm = codec.decode(ref["input"])
    rows = codec.debug_rows().reshape(2, 12 * m.downsample_stride, m.dimension)
    _hold(f"{name}-{mode} decode B=2 F=12", {"rows": rows, "pcm": pcm}, ref, m.frame_size, capsys)


@pytest.mark.parametrize("B", [1, 3, STREAM_B])
@pytest.mark.parametrize("name,mode", CONFIGS)
def test_decode_step(name, mode, B, capsys):
    """The first B utterances of the case's codes (the oracle ran all 9 once; utterances are independent)."""
    codec, ref = _codec(name, mode), _reference(name, mode, "stream")
    m = codec.m
    codes = ref["input"][:B]
    codec.reset_state(B)
    pcm, rows = [], []
    for f in range(STREAM_FRAMES):
        pcm.append(codec.decode_step(codes[:, :, f: f + 1]))
        rows.append(codec.debug_rows().reshape(B, m.downsample_stride, m.dimension))
    got = {"rows": np.concatenate(rows, axis=1), "pcm": np.concatenate(pcm, axis=2)}
    _hold(f"{name}-{mode} decode_step B={B} F={STREAM_FRAMES}", got, ref, m.frame_size, capsys, rows_b=slice(0, B))


@pytest.mark.parametrize("name,mode", CONFIGS)
def test_encode_latent(name, mode, capsys):
    codec, ref = _codec(name, mode), _reference(name, mode, "encode")
    m = codec.m
    codes = codec.encode(ref["input"])
    Tf = codes.shape[2]
    assert ref["f64"]["rows"].shape == (2, Tf, m.dimension)
    _hold(f"{name}-{mode} encode B=2 Tf={Tf}", {"rows": codec.debug_rows().reshape(2, Tf, m.dimension)}, ref, None, capsys)
