"""The streaming Mimi encode's yardstick: the oracle alone, frame by frame (tests/test_encode_stream_*.py).

``stream_reference`` composes OracleMimi's pieces per frame as its ``decode_step`` does for the decoder: the
causal SEANet evaluated on the whole history (which equals its streaming state machine), the encoder
transformer on the frame's latent steps with one persistent KV cache (so the moshi_mlx attention mode sees the
keys an ``encode_step`` call per frame sees), the downsample conv on the whole latent history with its replicate
left pad, and both quantizers with their margins.  ``stream_pair`` runs it in float32 and float64 and memoises.
"""
import numpy as np

from helpers import mimi_errors, mimi_pcm_clip
from oracle.mimi_oracle import conv1d

RVQ_TIE = 1e-5       # oracle RVQ margin below which a code is a tie at float32 resolution (tests/test_mimi_f64_gpu.py)
_REFS = {}


def stream_reference(o, pcm, zero_start=False, whole=False):
    """pcm (N,), N a multiple of the frame size, through oracle ``o`` one frame at a time.
    Returns {"rows": (F, D) pre-RVQ latent, "codes": (n_q, F) int32, "margins": (n_q, F)}.
    zero_start: the downsample conv starts from a zero history instead of the edge sample (the defect a
    streaming encoder without the stream-start case has; for the CPU facts only).
    whole: the causal SEANet runs once over the whole clip and each frame takes its steps from that (whole
    frames have no right padding, so these are the values of the per-frame evaluation up to BLAS summation
    order): linear instead of quadratic in the frames, for the streams of a hundred frames
    (tests/test_mimi_window_*.py)."""
    m, dt = o.m, o.dt
    fs, s = m.frame_size, m.downsample_stride
    x = np.asarray(pcm, np.float32).reshape(1, 1, -1).astype(dt)
    assert x.shape[2] % fs == 0 and x.shape[2] > 0
    F = x.shape[2] // fs
    cache = o.enc_tr.new_cache()
    dw = o.w["downsample.conv.conv.conv.weight"]
    lat, out = None, []
    e_all = o._seanet(o.enc_layout, x) if whole else None
    for f in range(F):
        e = o._seanet(o.enc_layout, x[..., :(f + 1) * fs])[..., -s:] if e_all is None else e_all[..., f * s: (f + 1) * s]
        y = o.enc_tr(e, cache)
        lat = y if lat is None else np.concatenate([lat, y], axis=2)
        src = np.concatenate([np.zeros_like(lat[..., :s]), lat], axis=2) if zero_start else lat
        out.append(conv1d(src, dw, None, s, 1, "replicate", dtype=dt)[..., -1:])
    z = np.concatenate(out, axis=2)                                           # (1, D, F)
    ms = []
    sem = o.rvq_encode("rvq_first", z, o.cb_first, ms)
    ac = o.rvq_encode("rvq_rest", z, o.cb_rest, ms)
    return {"rows": z[0].T.copy(), "codes": np.concatenate([sem, ac], axis=1)[0].astype(np.int32),
            "margins": np.stack([mg for mg, _ in ms], axis=1)[0]}


def stream_pair(o32, o64, pcm, key=None, whole=False):
    """{"f32": ..., "f64": ..., "e32": ...} of one stream: both references and the float32 one's error in
    helpers.mimi_errors' unit on the rows (its maximum over the stream's frames).  key: memoise under it.
    whole: ``stream_reference``'s."""
    if key is not None and key in _REFS:
        return _REFS[key]
    r = {"f32": stream_reference(o32, pcm, whole=whole), "f64": stream_reference(o64, pcm, whole=whole)}
    r["e32"] = float(mimi_errors(r["f32"]["rows"][None], r["f64"]["rows"][None]).max())
    if key is not None:
        _REFS[key] = r
    return r


def row_errors(got, ref, f0=0):
    """got (n, D): the engine's latent rows of frames f0..f0+n-1 of a stream with reference ``ref``
    (stream_pair).  Per frame, max |got - float64| / the stream's largest |float64 value|."""
    r64 = ref["f64"]["rows"]
    g = np.asarray(got, np.float64)
    return np.abs(g - r64[f0: f0 + g.shape[0]]).max(-1) / np.abs(r64).max()


def code_mismatches(got, ref, f0=0):
    """got (n_q, n) codes of frames f0.. of the stream: [(frame, codebook, margin)] of every frame's first
    differing codebook whose float32-oracle margin is not below RVQ_TIE (codebooks after a tie follow another
    residual and are not compared)."""
    want, mg = ref["f32"]["codes"], ref["f32"]["margins"]
    bad = []
    for j in range(got.shape[1]):
        ks = np.flatnonzero(got[:, j] != want[:, f0 + j])
        if ks.size and not mg[ks[0], f0 + j] < RVQ_TIE:
            bad.append((f0 + j, int(ks[0]), float(mg[ks[0], f0 + j])))
    return bad


def clip(frames, m, seed):
    return mimi_pcm_clip(frames * m.frame_size, seed)


# The streams the GPU tests serve, {config: {name: (mimi_pcm_clip seed, frames)}}; tests/test_encode_stream_cpu.py
# asserts that none of their codes is near a tie (so on the GPU every code must match).
STREAMS = {
    "tiny": {"long": (0, 15), "first": (2, 4), "second": (3, 11), "gap": (4, 8), "cap_a": (0, 15), "cap_b": (3, 15),
             "step_a": (0, 5), "step_b": (2, 5), "push_a": (3, 6), "push_b": (4, 5)},
    "mimi_202407": {"a": (0, 4), "b": (1, 4)},
}
MIN_MARGIN = {"tiny": 1e-4, "mimi_202407": RVQ_TIE}


def stream_case(name, mode, rig, stream):
    """(pcm (N,), stream_pair reference) of STREAMS[name][stream] on helpers.mimi_pair(name, mode, rig)'s oracles."""
    from helpers import mimi_pair
    m, _, o32, o64 = mimi_pair(name, mode, rig)
    seed, frames = STREAMS[name][stream]
    pcm = clip(frames, m, seed)
    return pcm, stream_pair(o32, o64, pcm, key=(name, mode, rig, seed, frames))
