"""Every execution path of the engine against the float64 oracle, tap by tap.

Procedure: prefill the prompts, run 2 frames one at a time (FrameCache.run(1), or csm_frame_forced); after
each frame read h_last, c0_logits, ci_logits and the frame's codes.  (Two frames: the decode-row backbone
kernels first run at frame 1.)  Then run the float64 and the float32 oracle teacher-forced on the codes the
engine produced (OracleCSM.frame(forced=...)), so a near-tie never cuts a comparison short: every row,
every codebook step and every frame is compared.

Unit: max over the vocabulary (over D for h_last) of |value - float64| / that row's largest |float64 value|.
e32 = the float32 oracle's error in that unit on the same codes, maximum over rows, steps and frames of the
case, per tap (h_last, c0, ci) -- measured from the two references alone, each run.
Bar: engine error <= helpers.BAR_MARGIN (2) x e32 per tap; tests/test_f64_oracle_cpu.py holds what makes
that mean something (an evaluation that loses the low activation bits misses the bar by 2x at least).

Also per case: greedy codes are the first-index arg-max of the engine's own logits row (the packed
partials, the in-launch heads); the kernel meant to run did run (dec_frame_epoch +498 per frame,
dec_xsd_epoch +(K-2) per frame, bb_step_epoch +80 per decode row -- and +0 on the paths that switch them
off); csm_synchronize returns clean."""
import dataclasses

import numpy as np
import pytest

from helpers import BAR_MARGIN, TAPS, csm_weights, f64_reference, norm_rig, prompt_ids, tap_errors, tiny_prompt_ids
from rigs import TAP_NAMES, build_model, epoch, frame_taps, handoffs, set_option, synchronize

pytestmark = pytest.mark.gpu

FRAMES = 2
EPOCHS = ("dec_frame_epoch", "dec_xsd_epoch", "bb_step_epoch")


def _engine(key, dtype, max_batch):
    return build_model(_weights(key), dtype, max_batch)


_W = {}


def _weights(key):
    """key: "tiny", "1b", "tiny_f1280", or one of them + "+norm": the same weights through helpers.norm_rig
    (tests/test_norm_rig_gpu.py runs this module's procedure on those)."""
    if key.endswith("+norm"):
        args, w = _weights(key[:-len("+norm")])
        return args, norm_rig(args, w)
    if key in ("tiny", "1b"):
        return csm_weights(key)
    if key not in _W:                                                       # tiny_f1280: the K = 1280 stage case
        assert key == "tiny_f1280", key                                     # (any other key is registered in _W)
        from csm_mlx.models import csm_tiny
        from csm_mlx.weights import synthetic_csm_weights
        args = dataclasses.replace(csm_tiny(), decoder_name=key)
        _W[key] = (args, synthetic_csm_weights(args, 0))
    return _W[key]


@pytest.fixture(scope="module")
def engine_1b_bf16():
    args, w, model = _engine("1b", "bf16", 32)
    yield args, w, model
    del model


@pytest.fixture(scope="module")
def engine_1b_q4():
    args, w, model = _engine("1b", "q4", 64)
    yield args, w, model
    del model


def _epochs(model):
    return {name: epoch(model, name[:-len("_epoch")]) for name in EPOCHS}


def _run(model, prompts, forced=None):
    """2 frames, one at a time; returns codes (F, B, K) and the taps (h_last (F, B, D), c0 (F, B, V),
    ci (F, B, K-1, V)).  forced (F, B, K): the frames are csm_frame_forced on these codes."""
    from csm_mlx import _lib
    from csm_mlx.sampling import Sampler

    def force(cache, f):
        codes = np.ascontiguousarray(forced[f], np.int32)
        _lib.check(_lib.lib().csm_frame_forced(model.engine, _lib.ptr(codes), None, None, None))
    hist, n, taps = frame_taps(model, prompts, FRAMES, Sampler(0.0, 0), [0] * len(prompts), TAP_NAMES,
                               step=None if forced is None else force)
    assert hist.shape[0] == FRAMES and (n == FRAMES).all(), "an utterance ended inside the window"
    return hist, tuple(taps[t] for t in TAP_NAMES)


_REFS = {}


def _reference(key, dtype, prompts, codes, block=None):
    """Memoised by (model, dtype, prompts, codes): the paths of one engine at one B produce the same codes.
    block: helpers.oracle_taps' (a prompt-sized prefill reaches the oracles in pieces)."""
    variant = {"float32": "fp32"}.get(dtype, dtype)
    k = (key, variant, tuple(t.tobytes() for t, _ in prompts), codes.tobytes())
    if k not in _REFS:
        args, w = _weights(key)
        _REFS[k] = f64_reference(args, w, variant, prompts, codes, block)
    return _REFS[k]


def _check(key, dtype, model, prompts, options=(), forced=None, expect=None, capsys=None, block=None):
    """Run the case with ``options`` (name -> 0) switched off, compare every tap with the float64 oracle
    forced on the engine's codes, hold the epoch deltas to ``expect``."""
    for name in options:
        set_option(model, name, 0)
    try:
        e0 = _epochs(model) if expect is not None else None
        codes, got = _run(model, prompts, forced)
        synchronize(model)                                                   # no hand-off timeout left behind
        if expect is not None:
            e1 = _epochs(model)
            delta = {n: e1[n] - e0[n] for n in EPOCHS}
            assert delta == expect, f"kernels that ran (epoch deltas) {delta}, expected {expect}"
    finally:
        for name in options:
            set_option(model, name, 1)
    if forced is not None:
        assert np.array_equal(codes, forced), "the forced codes are not the frame's codes"
    else:                                                                    # first-index arg-max of its own logits
        assert np.array_equal(codes[:, :, 0], got[1].argmax(-1)), "c0 is not the arg-max of the engine's c0 logits"
        assert np.array_equal(codes[:, :, 1:], got[2].argmax(-1)), "a code is not the arg-max of its ci logits row"
    t64, e32 = _reference(key, dtype, prompts, codes, block)
    err = tap_errors(got, t64)
    ci = err["ci"]
    split = {"h_last": err["h_last"].max(), "c0": err["c0"].max(), "ci1": ci[:, :, 0].max(), "ci2+": ci[:, :, 1:].max()}
    e = {"h_last": e32["h_last"], "c0": e32["c0"], "ci1": e32["ci"], "ci2+": e32["ci"]}
    line = (f"f64-taps {key} {dtype} B={len(prompts)} off={','.join(options) or '-'}"
            f"{' forced' if forced is not None else ''}: "
            + " ".join(f"{t}={split[t]:.2e}({split[t] / e[t]:.2f}x)" for t in split)
            + " | e32 " + " ".join(f"{t}={e32[t]:.2e}" for t in TAPS))
    if capsys is not None:
        with capsys.disabled():
            print("\n" + line)
    bad = [f"{t}: {float(err[t].max()):.3e} > {BAR_MARGIN} x e32 = {BAR_MARGIN * e32[t]:.3e} at (frame, row[, step]) "
           f"{np.unravel_index(int(err[t].argmax()), err[t].shape)}" for t in TAPS
           if not float(err[t].max()) <= BAR_MARGIN * e32[t]]
    assert not bad, line + "\n" + "\n".join(bad)


def _prompts_1b(B):
    from csm_mlx.tokenizers import tokenize_text_segment
    return [tokenize_text_segment(prompt_ids(3000 + 97 * B + b, 10 + b % 3), 0, 32) for b in range(B)]     # 12-14 rows


def _expect(K, B, dec_frame=False, dec_xsd=False, bb_step=False):
    return {"dec_frame_epoch": handoffs("dec_frame", K) * FRAMES if dec_frame else 0,
            "dec_xsd_epoch": handoffs("dec_xsd", K) * FRAMES if dec_xsd else 0,
            "bb_step_epoch": handoffs("bb_step", K) * (FRAMES - 1) * B if bb_step else 0}


# ----------------------------------------------------------------------------- csm_1b, batch 1
@pytest.mark.parametrize("persistent", [True, False], ids=["bb_step+dec_frame", "gemv_launches"])
@pytest.mark.parametrize("dtype", ["bf16", "q4"])
def test_1b_batch1(dtype, persistent, engine_1b_bf16, engine_1b_q4, capsys):
    args, w, model = engine_1b_bf16 if dtype == "bf16" else engine_1b_q4
    K = args.n_audio_codebooks
    _check("1b", dtype, model, _prompts_1b(1), options=() if persistent else ("bb_step", "dec_frame"),
           expect=_expect(K, 1, dec_frame=persistent, bb_step=persistent), capsys=capsys)


# ----------------------------------------------------------------------------- csm_1b, batched
BATCHED = [("bf16", 8, ()), ("bf16", 19, ()), ("bf16", 32, ()), ("bf16", 32, ("dec_xsd",)), ("bf16", 32, ("gemm_xs",)),
           ("bf16", 32, ("bb_xs",)), ("q4", 8, ()), ("q4", 40, ()), ("q4", 64, ()), ("q4", 64, ("dec_xsd",)),
           ("q4", 64, ("gemm_xs",))]


@pytest.mark.parametrize("dtype,B,off", BATCHED, ids=[f"{d}-B{b}-{'no_' + o[0] if o else 'default'}" for d, b, o in BATCHED])
def test_1b_batched(dtype, B, off, engine_1b_bf16, engine_1b_q4, capsys):
    """dec_xsd on: the persistent step (dec_step_xs) over gemm_xs step 1 / backbone; dec_xsd off: run_dec_xs;
    gemm_xs off: gemm_wide for the decoder (and no persistent step: it is the streaming path's); bb_xs off:
    the backbone rows on gemm_wide."""
    args, w, model = engine_1b_bf16 if dtype == "bf16" else engine_1b_q4
    K = args.n_audio_codebooks
    xsd = "dec_xsd" not in off and "gemm_xs" not in off
    _check("1b", dtype, model, _prompts_1b(B), options=off, expect=_expect(K, B, dec_xsd=xsd), capsys=capsys)


def _forced_codes(B, K, bins=2048):
    """Seeded random codes (FRAMES, B, K) in [0, bins) (the codec's bins), with 0 and bins - 1 placed in every
    codebook column of some row."""
    rng = np.random.default_rng(50 + B)
    forced = rng.integers(0, bins, (FRAMES, B, K)).astype(np.int32)
    forced[0, 0, :K - 1] = 0                                  # (an all-zero frame would be EOS: the last column's
    forced[0, B - 1, K - 1] = 0                               #  0 sits in another row)
    forced[1, B - 1, :] = bins - 1
    assert all((forced[:, :, k] == 0).any() and (forced[:, :, k] == bins - 1).any() for k in range(K))
    assert forced.any(-1).all()
    return forced


@pytest.mark.parametrize("B", [2, 32])
def test_1b_bf16_forced(B, engine_1b_bf16, capsys):
    """csm_frame_forced: seeded random codes in [0, 2048) (the codec's bins), with 0 and 2047 placed in every
    codebook column of some row; the reference is forced on the same codes.  B = 2: GEMV launches; 32: the
    persistent step."""
    args, w, model = engine_1b_bf16
    K = args.n_audio_codebooks
    _check("1b", "bf16", model, _prompts_1b(B), forced=_forced_codes(B, K), expect=_expect(K, B, dec_xsd=B >= 8),
           capsys=capsys)


# ----------------------------------------------------------------------------- tiny shapes
def _tiny_prompts(args, B, seed):
    from csm_mlx.tokenizers import tokenize_text_segment
    return [tokenize_text_segment(tiny_prompt_ids(seed + b, 10 + b % 3), 0, args.n_audio_codebooks) for b in range(B)]


def _tiny_case(key, dtype, B, seed, capsys):
    """A fresh engine on ``key``'s weights, B prompts seeded from ``seed``, the module's check."""
    args, w, model = _engine(key, dtype, B)
    _check(key, dtype, model, _tiny_prompts(args, B, seed), capsys=capsys)
    del model


@pytest.mark.parametrize("B", [1, 9, 33])
@pytest.mark.parametrize("dtype", ["float32", "bf16", "q4"])
def test_tiny(dtype, B, capsys):
    _tiny_case("tiny", dtype, B, 4000 + 97 * B, capsys)


@pytest.mark.parametrize("dtype", ["bf16", "q4"])
def test_tiny_f1280(dtype, capsys):
    """A decoder MLP of width 1280: 20 K-stages of 64, which an 8-wave block does not divide."""
    _tiny_case("tiny_f1280", dtype, 8, 4800, capsys)
