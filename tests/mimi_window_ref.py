"""The codec transformer past its attention window: the oracle's side of tests/test_mimi_window_*.py.

A key range [k0, k1] of a row, as csrc/csm_kernels.hip attn_block computes it (``window``):
  causal (ATTN_WINDOW)             k0 = max(0, pos - context + 1),          k1 = pos
  mlx    (ATTN_FRAMES, ATTN_BLOCK) k0 = max(0, frame start - context),      k1 = frame start + rows of the frame - 1
so a causal row holds at most ``context`` live keys and an mlx row ``context + 2``.  The window "starts past key 0"
from position ``first_windowed`` on.

``decode_stream`` runs OracleMimi's streaming decoder over calls of several frames; ``DEFECTS`` are the faults of
such a range that the suite could not see before, each as hooks for TransformerRef (``spoiled``)."""
import contextlib

import numpy as np

from helpers import mimi_errors

CHUNK = 64          # attn_block's key chunk


def schedule(frames, calls):
    """Call sizes cycling through ``calls`` that add up to exactly ``frames`` (the last one cut)."""
    out, i = [], 0
    while sum(out) < frames:
        out.append(min(calls[i % len(calls)], frames - sum(out)))
        i += 1
    return out


def first_windowed(m):
    """The first latent position whose row's key range starts past key 0."""
    s = m.downsample_stride
    return m.context if m.attn_mode != "mlx" else (m.context // s + 1) * s


def decode_stream(o, codes, calls, pcm=True, window=8):
    """codes (B, n_q, F) through ``o``'s streaming decoder in calls of ``calls`` frames (they add up to F).
    Returns {"rows": (B, F * s, D)[, "pcm": (B, 1, F * frame_size)]}; pcm: OracleMimi.decode_steps'."""
    assert sum(calls) == codes.shape[2], (calls, codes.shape)
    o.reset_state()
    rows, out, f = [], [], 0
    for n in calls:
        y = o.decode_steps(codes[:, :, f: f + n], window=window, pcm=pcm)
        rows.append(o.taps["rows"])
        out.append(y)
        f += n
    o.reset_state()
    r = {"rows": np.concatenate(rows, axis=1)}
    if pcm:
        r["pcm"] = np.concatenate(out, axis=2)
    return r


def decode_pair(o32, o64, codes, calls, pcm=True):
    """{"f32", "f64": decode_stream's, "e32": {tap: the float32 oracle's largest error on the stream}}."""
    r = {"f32": decode_stream(o32, codes, calls, pcm), "f64": decode_stream(o64, codes, calls, pcm)}
    fs = o32.m.frame_size
    r["e32"] = {tap: float(mimi_errors(r["f32"][tap], r["f64"][tap], fs if tap == "pcm" else None).max()) for tap in r["f64"]}
    return r


# ----------------------------------------------------------------------------- key ranges and their defects
def window(m, off, T, blk):
    """Per row of a call (positions off .. off + T - 1, frames of blk rows): (u, k1), the first key before its
    clamp to 0 and the last key."""
    t = np.arange(T)
    if m.attn_mode == "mlx":
        f0 = off + t // blk * blk
        return f0 - m.context, f0 + blk - 1
    return off + t - m.context + 1, off + t


def _range_keep(k0, k1, S):
    kpos = np.arange(S)[None, :]
    return (kpos >= k0[:, None]) & (kpos <= k1[:, None])


def _keep_of(kind):
    def keep(tr, off, T, S, blk=None):
        u, k1 = window(tr.m, off, T, blk or T)
        k0 = np.maximum(0, u)
        if kind == "late":                                  # the window starts one key late
            k0 = np.maximum(0, u + 1)
        elif kind == "early":                               # ... one key early
            k0 = np.maximum(0, u - 1)
        elif kind == "aligned":                             # the chunk loop starts at k0 rounded down to a chunk
            k0 = k0 // CHUNK * CHUNK
        elif kind == "tail":                                # the last, partial chunk read as a full one: keys past
            n = k1 - k0 + 1                                 # k1 from the cache, as far as the call has written it
            k1 = np.minimum(S - 1, k0 + (n + CHUNK - 1) // CHUNK * CHUNK - 1)
        k = _range_keep(k0, k1, S)
        if kind == "chunk":                                 # the chunk (counted from k0) holding the middle key
            c0 = k0 + ((k0 + k1) // 2 - k0) // CHUNK * CHUNK   # dropped -- on the k0 > 0 path
            k &= ~(_range_keep(c0, c0 + CHUNK - 1, S) & (k0 > 0)[:, None])
        return k
    return keep


def _no_rescale(tr, s, keep, Vv):
    """The row's range as an online softmax over 64-key chunks counted from k0, the exp(m_old - m_new) rescale of
    what is already accumulated left out."""
    dt = tr.dt
    B, H, T, S = s.shape
    out = np.zeros((B, H, T, Vv.shape[-1]), dt)
    for t in range(T):
        ks = np.flatnonzero(keep[t])
        k0, k1 = int(ks[0]), int(ks[-1])
        m_run = np.full((B, H), -np.inf, dt)
        l_run = np.zeros((B, H), dt)
        o = np.zeros((B, H, Vv.shape[-1]), dt)
        for c in range(k0, k1 + 1, CHUNK):
            e = min(c + CHUNK, k1 + 1)
            m_run = np.maximum(m_run, s[:, :, t, c:e].max(-1))
            p = np.exp(s[:, :, t, c:e] - m_run[..., None]).astype(dt)
            l_run = (l_run + p.sum(-1)).astype(dt)
            o = (o + np.matmul(p[:, :, None, :], Vv[:, :, c:e])[:, :, 0]).astype(dt)
        out[:, :, t] = o / l_run[..., None]
    return out


DEFECTS = ("late", "early", "aligned", "chunk", "no_rescale", "tail")
RANGE_NOOPS = ("late", "early", "aligned", "chunk")     # exact no-ops while every range starts at key 0


@contextlib.contextmanager
def spoiled(tr, kind):
    """TransformerRef ``tr`` with defect ``kind`` (of DEFECTS; "none": the hooks restated, no defect) in place."""
    import types
    if kind == "no_rescale":
        tr.softmax_av = types.MethodType(_no_rescale, tr)
    else:
        tr.keep = types.MethodType(_keep_of(kind), tr)
    try:
        yield tr
    finally:
        tr.__dict__.pop("keep", None)
        tr.__dict__.pop("softmax_av", None)


# ----------------------------------------------------------------------------- the cases the GPU tests serve
def depth_frames(context, s=2):
    """Frames after which a stream is at least ``context + 70`` latent steps in."""
    return (context + 70 + s - 1) // s


MODES = ("mlx", "causal")


def cases(contexts):
    """[(context, mode, rig)]: every context in both modes, helpers.mimi_affine_rig on half of them -- on
    alternate contexts, the other way round in the other mode."""
    from helpers import mimi_affine_rig
    return [(c, mode, mimi_affine_rig if (i + j) % 2 else None)
            for i, c in enumerate(contexts) for j, mode in enumerate(MODES)]


# streaming encode: the two slots' mimi_pcm_clip seeds of every case (cases(ENCODE_CONTEXTS));
# tests/test_mimi_window_cpu.py holds that no code of these clips is near a tie for the oracle alone
ENCODE_CONTEXTS = (63, 65, 130)
ENCODE_SEEDS = (31, 32)
ONE_SHOT_CONTEXT, ONE_SHOT_FRAMES, ONE_SHOT_SEED = 70, 100, 33      # 100 frames = an 8 s clip


def encode_case(context, mode, rig, seed, frames=None):
    """(pcm (N,), mimi_stream_ref.stream_pair reference) of a streaming-encode clip of ``depth_frames`` frames."""
    import mimi_stream_ref as sr
    from helpers import mimi_pair, mimi_pcm_clip
    m, _, o32, o64 = mimi_pair("tiny", mode, rig, context)
    frames = depth_frames(context, m.downsample_stride) if frames is None else frames
    pcm = mimi_pcm_clip(frames * m.frame_size, seed)
    return pcm, sr.stream_pair(o32, o64, pcm, key=("window", context, mode, rig, seed, frames), whole=True)
