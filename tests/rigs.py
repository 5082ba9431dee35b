"""Engine-side rigs of the GPU tests (test infrastructure): build an engine, drive it frame by frame and read
its taps, split a batch's codes per utterance, switch an option, and the off / on comparison of a persistent
kernel.  The oracle and reference builders are in helpers.py.

Bars, tolerances, frame counts, batch sizes and seeds are never defaulted here: every caller writes its own.
tests/test_rigs_cpu.py holds these rigs against stub objects, without a GPU."""
import dataclasses
import os

import numpy as np

from helpers import csm_weights, tiny_prompt_ids

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture(name):
    """A committed oracle fixture (tests/golden/make_golden.py)."""
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


# ----------------------------------------------------------------------------- an engine with synthetic weights
def build_model(which, dtype, max_batch=1):
    """which: a ``csm_weights`` key ("tiny", "1b") or an (args, weights) pair.  Returns (args, weights, model)."""
    from csm_mlx.models import CSM
    args, w = csm_weights(which) if isinstance(which, str) else which
    model = CSM(args, dtype=dtype, max_batch=max_batch)
    model.load_weights(w)
    return args, w, model


def set_option(model, key, value):
    from csm_mlx import _lib
    _lib.check(_lib.lib().csm_set_option(model.engine, key.encode(), int(value)))


def epoch(model, name):
    """The hand-off counter ``<name>_epoch`` of the persistent kernel behind option ``name``."""
    from csm_mlx import _lib
    ep = np.zeros(1, np.uint32)
    _lib.check(_lib.lib().csm_debug_read(model.engine, f"{name}_epoch".encode(), _lib.ptr(ep), 4, None))
    return int(ep[0])


def synchronize(model):
    """Raises if a persistent kernel left a hand-off timeout behind."""
    from csm_mlx import _lib
    _lib.check(_lib.lib().csm_synchronize(model.engine))


# ----------------------------------------------------------------------------- the persistent kernels' hand-offs
def handoffs(name, K):
    """Epoch increments per unit of work of the kernel behind option ``name`` (K codebooks): dec_frame per
    frame, bb_step per backbone step of one decode row (every frame but an utterance's first, whose h_last
    comes from the prefill), dec_xsd per frame (one per codebook step >= 2)."""
    return {"dec_frame": 498, "bb_step": 80, "dec_xsd": K - 2}[name]


def ab(model, name, run, moved):
    """``run()`` with option ``name`` off, then on; the kernel's epoch must move by exactly ``moved`` over the
    on leg.  Leaves the option on.  Returns (off result, on result)."""
    set_option(model, name, 0)
    ref = run()
    set_option(model, name, 1)
    e0 = epoch(model, name)
    got = run()
    d = epoch(model, name) - e0
    assert d == moved, f"option {name}: the persistent kernel's epoch moved by {d}, not by {moved}: it did not run every time"
    return ref, got


# ----------------------------------------------------------------------------- frame by frame, with taps
TAP_NAMES = ("h_last", "c0_logits", "ci_logits")


def read_taps(model, cache, B, taps):
    """The engine's ``taps`` (of TAP_NAMES) of ``cache``'s B utterances as they stand, in TAP_NAMES' order: h_last (B, D),
    c0_logits (B, V), ci_logits (B, K-1, V), cut from the padded vocabulary and copied."""
    K, V = model.n_audio_codebooks, model.n_audio_vocab
    Vp = (V + 7) // 8 * 8                                     # the engine's logits rows are padded to 8 columns
    shapes = {"h_last": (B, model.n_backbone_embedding), "c0_logits": (B, Vp), "ci_logits": (K - 1, B, Vp)}
    assert set(taps) <= set(TAP_NAMES), taps
    out = {}
    for t in TAP_NAMES:
        if t in taps:
            a = cache.debug(t, shapes[t])
            if t != "h_last":
                a = a[..., :V]
            out[t] = (a.transpose(1, 0, 2) if t == "ci_logits" else a).copy()
    return out


def frame_taps(model, prompts, frames, sampler, seeds, taps, keep=None, step=None, processors=None, prefill_batch=False,
               prefill=None):
    """A FrameCache over ``prompts`` (tokens, mask), ``frames`` frames one at a time, the engine's ``taps`` (of
    TAP_NAMES) read back after every frame, or only after the frames in ``keep``.  step(cache, f) runs frame f
    in place of ``cache.run(1)``; processors: FrameCache's device pair; prefill_batch: one csm_prefill_batch
    pass for all prompts; prefill(cache) feeds the prompts itself, in place of either.  Returns (hist (F, B, K),
    n (B,), {tap: array}) with h_last (F', B, D), c0_logits (F', B, V), ci_logits (F', B, K-1, V) over the F'
    frames read (``read_taps``)."""
    from csm_mlx.generation import FrameCache
    B = len(prompts)
    assert set(taps) <= set(TAP_NAMES), taps
    cache = FrameCache(model, B, sampler, seeds, processors)
    if prefill is not None:
        prefill(cache)
    elif prefill_batch:
        cache.prefill_batch([(b, t, m) for b, (t, m) in enumerate(prompts)])
    else:
        for b, (t, m) in enumerate(prompts):
            cache.prefill(b, t, m)
    out = {t: [] for t in TAP_NAMES if t in taps}
    for f in range(frames):
        if step is None:
            cache.run(1)
        else:
            step(cache, f)
        if keep is not None and f not in keep:
            continue
        for t, a in read_taps(model, cache, B, taps).items():
            out[t].append(a)
    hist, n, _ = cache.codes()
    return hist, n, {t: np.stack(v) for t, v in out.items()}


def codes_per_utterance(model, prompts, frames, sampler, seeds=None, logits_processors=None):
    """generate_codes_batch, cut to each utterance's own frames: [codes (n_b, K)]."""
    from csm_mlx.generation import generate_codes_batch
    hist, n, _ = generate_codes_batch(model, prompts, frames, sampler=sampler, seeds=seeds,
                                      logits_processors=logits_processors)
    return [hist[: n[b], b].copy() for b in range(len(prompts))]


# ----------------------------------------------------------------------------- the codec beside its oracle
def mimi_codec(name, mode, max_batch, max_frames, rig=None, context=None):
    """(MimiArgs, MimiCodec with synthetic weights, float32 OracleMimi on the same weights).
    rig: a function (m, w) -> new weights applied to the synthetic ones (helpers.mimi_affine_rig);
    context: the attention window in place of the config's (tests/test_mimi_window_gpu.py)."""
    from csm_mlx.config import MIMI_CONFIGURATION
    from csm_mlx.mimi import MimiCodec
    from csm_mlx.weights import synthetic_mimi_weights
    from oracle.mimi_oracle import OracleMimi
    m = dataclasses.replace(MIMI_CONFIGURATION[name], attn_mode=mode)
    if context is not None:
        m = dataclasses.replace(m, context=context)
    w = synthetic_mimi_weights(m)
    if rig is not None:
        w = rig(m, w)
    codec = MimiCodec(m, max_batch=max_batch, max_frames=max_frames)
    codec.load_weights(w)
    return m, codec, OracleMimi(m, w)


# ----------------------------------------------------------------------------- the slot tests' tiny queue
N_TINY, CAP = 14, 40
SEEDS = [1234 + i for i in range(N_TINY)]


def slot_prompts(K):
    """14 prompts of 4..10 rows (tests/test_slots_gpu.py, tests/test_slot_stream_gpu.py)."""
    from csm_mlx.tokenizers import tokenize_text_segment
    return [tokenize_text_segment(tiny_prompt_ids(300 + i, 2 + i % 7), 0, K) for i in range(N_TINY)]
