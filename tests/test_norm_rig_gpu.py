"""Every consumer of an RMSNorm weight in the engine against the float64 oracle, on weights whose norms are not
all ones (helpers.norm_rig: every norm tensor its own draw, 2^U(-2, 2) per element, about 10 % negated).

With the synthetic all-ones norms n1[l], n1[l + 1], n2[l] and the final norm are interchangeable and
sum(x * nw) = sum(x), so a norm weight that is skipped, applied twice, taken from another layer, read at a wrong
offset, summed before it is multiplied in, or left stale after a reload goes unseen.  On the rigged weights any
one of these moves a tap by more than 1e5 x the bar (tests/test_norm_rig_cpu.py).

Procedure, unit, e32 and bar are tests/test_f64_taps_gpu.py's own functions, run on the weight keys "<model>+norm":
two frames one at a time, both oracles teacher-forced on the engine's codes, error <= helpers.BAR_MARGIN x e32 per
tap with e32 measured each run, epoch deltas, arg-max of the engine's own logits, csm_synchronize clean.

Cases: tiny fp32 / bf16 / q4 at B = 1, 9, 33 and tiny_f1280 at B = 8; csm_1b bf16 / q4 at B = 1 on the persistent
kernels and on the GEMV launches (the folded layer-0 QKV table); csm_1b batched with each matrix-core option off;
csm_frame_forced; prompts of 100 and 300 rows (gemm_wide's norm prologue in its 4-wave and 8-wave block shapes);
a reload of the norm tensors alone into an engine that has already run (the folded table, the persistent kernels'
argument copies and the captured graphs must not keep the old values); every tensor handed over as bf16 bits (both
sides then hold bf16-exact norms -- with the fp32-in cases this pins the storage rule from both sides); scoring;
and a running batch of slots."""
import numpy as np
import pytest

import test_f64_taps_gpu as taps
from helpers import first_divergence, is_norm, long_prompt, norm_rig, oracle_for
from rigs import CAP, N_TINY, build_model, slot_prompts
from test_f64_taps_gpu import _check, _engine, _expect, _forced_codes, _prompts_1b, _tiny_case, _tiny_prompts, _weights

pytestmark = pytest.mark.gpu

BLOCK = 128          # rows per piece of a long prompt in the oracles (helpers.oracle_taps)


@pytest.fixture(scope="module")
def engine_1b_bf16():
    args, w, model = _engine("1b+norm", "bf16", 32)
    yield args, w, model
    del model


@pytest.fixture(scope="module")
def engine_1b_q4():
    args, w, model = _engine("1b+norm", "q4", 64)
    yield args, w, model
    del model


# ----------------------------------------------------------------------------- tiny shapes
@pytest.mark.parametrize("B", [1, 9, 33])
@pytest.mark.parametrize("dtype", ["float32", "bf16", "q4"])
def test_tiny(dtype, B, capsys):
    _tiny_case("tiny+norm", dtype, B, 4000 + 97 * B, capsys)


@pytest.mark.parametrize("dtype", ["bf16", "q4"])
def test_tiny_f1280(dtype, capsys):
    _tiny_case("tiny_f1280+norm", dtype, 8, 4800, capsys)


# ----------------------------------------------------------------------------- csm_1b
@pytest.mark.parametrize("persistent", [True, False], ids=["bb_step+dec_frame", "gemv_launches"])
@pytest.mark.parametrize("dtype", ["bf16", "q4"])
def test_1b_batch1(dtype, persistent, engine_1b_bf16, engine_1b_q4, capsys):
    """persistent: bb_step / bb_step_q4 and dec_frame (nw_fetch of n1[0], n2[l], n1[l + 1] | norm).  Off: the GEMV
    launches' nw prologue, the split-row producers and the folded layer-0 QKV table (built from layer 0's n1)."""
    args, w, model = engine_1b_bf16 if dtype == "bf16" else engine_1b_q4
    K = args.n_audio_codebooks
    _check("1b+norm", dtype, model, _prompts_1b(1), options=() if persistent else ("bb_step", "dec_frame"),
           expect=_expect(K, 1, dec_frame=persistent, bb_step=persistent), capsys=capsys)


BATCHED = [("bf16", 8, ()), ("bf16", 32, ()), ("bf16", 32, ("dec_xsd",)), ("bf16", 32, ("gemm_xs",)), ("bf16", 32, ("bb_xs",)),
           ("q4", 8, ()), ("q4", 64, ()), ("q4", 64, ("dec_xsd",))]


@pytest.mark.parametrize("dtype,B,off", BATCHED, ids=[f"{d}-B{b}-{'no_' + o[0] if o else 'default'}" for d, b, o in BATCHED])
def test_1b_batched(dtype, B, off, engine_1b_bf16, engine_1b_q4, capsys):
    """Default: dec_step_xs' O and D roles (n2[l], n1[l + 1] | norm) over gemm_xs' epilogues; dec_xsd off:
    run_dec_xs; gemm_xs off: gemm_wide's prologue for the decoder; bb_xs off: the backbone rows on gemm_wide."""
    args, w, model = engine_1b_bf16 if dtype == "bf16" else engine_1b_q4
    K = args.n_audio_codebooks
    xsd = "dec_xsd" not in off and "gemm_xs" not in off
    _check("1b+norm", dtype, model, _prompts_1b(B), options=off, expect=_expect(K, B, dec_xsd=xsd), capsys=capsys)


@pytest.mark.parametrize("B", [2, 32])
def test_1b_bf16_forced(B, engine_1b_bf16, capsys):
    args, w, model = engine_1b_bf16
    K = args.n_audio_codebooks
    _check("1b+norm", "bf16", model, _prompts_1b(B), forced=_forced_codes(B, K), expect=_expect(K, B, dec_xsd=B >= 8),
           capsys=capsys)


@pytest.mark.parametrize("rows", [100, 300])
@pytest.mark.parametrize("dtype", ["bf16", "q4"])
def test_1b_prompt_sized_prefill(dtype, rows, engine_1b_bf16, engine_1b_q4, capsys):
    """gemm_wide's norm prologue on prompt rows: 100 rows run its 4-wave blocks, 300 (>= GEMM_W8_MIN_M = 256) its
    8-wave blocks.  B = 2, each prompt prefilled in one call; the oracles take the prompt in pieces of 128 rows."""
    args, w, model = engine_1b_bf16 if dtype == "bf16" else engine_1b_q4
    prompts = [long_prompt(args, 7000 + rows + b, rows) for b in range(2)]
    _check("1b+norm", dtype, model, prompts, expect=_expect(args.n_audio_codebooks, 2), capsys=capsys, block=BLOCK)


# ----------------------------------------------------------------------------- reload of the norm tensors alone
def _reload_norms(which, dtype, B, prompts):
    """An engine on the plain (all-ones) weights that has run a frame, then given the rigged norm tensors alone."""
    from csm_mlx.generation import FrameCache
    from csm_mlx.sampling import Sampler
    args, plain = _weights(which)
    _, _, model = build_model((args, plain), dtype, B)
    cache = FrameCache(model, len(prompts), Sampler(0.0, 0), [0] * len(prompts))
    for b, (t, m) in enumerate(prompts):
        cache.prefill(b, t, m)
    cache.run(1)
    del cache
    rigged = norm_rig(args, plain)
    norms = {n: v for n, v in rigged.items() if is_norm(n)}
    assert norms and all(not np.array_equal(v, plain[n]) for n, v in norms.items())
    model.load_weights(norms, strict=False)
    return args, model


def test_reload_tiny(capsys):
    """tiny bf16, B = 9: the same bar against the rigged reference as a fresh engine's."""
    args, _ = _weights("tiny")
    prompts = _tiny_prompts(args, 9, 4000 + 97 * 9)
    _, model = _reload_norms("tiny", "bf16", 9, prompts)
    _check("tiny+norm", "bf16", model, prompts, capsys=capsys)
    del model


def test_reload_1b_persistent(capsys):
    """csm_1b bf16, B = 1 on bb_step + dec_frame: decoder.layers.0's norms raise proj_tab_dirty (the folded QKV
    table is rebuilt at the next frame); every other norm is copied into the buffer the kernels already read --
    the persistent kernels' argument blocks and the captured graphs hold pointers, not values."""
    args, _ = _weights("1b")
    prompts = _prompts_1b(1)
    _, model = _reload_norms("1b", "bf16", 1, prompts)
    K = args.n_audio_codebooks
    _check("1b+norm", "bf16", model, prompts, expect=_expect(K, 1, dec_frame=True, bb_step=True), capsys=capsys)
    _check("1b+norm", "bf16", model, prompts, options=("bb_step", "dec_frame"), expect=_expect(K, 1), capsys=capsys)
    del model


# ----------------------------------------------------------------------------- bf16 bits in
def test_tiny_bf16_bits_in(capsys):
    """Every tensor of the rigged dict handed over as bf16 bits (uint16): the engine holds what a bf16 checkpoint
    holds, norm weights included (converted to fp32 exactly).  Reference: the oracle on the bf16-rounded dict."""
    from csm_mlx.weights import bf16_bits, bf16_round
    key = "tiny+norm+bf16_bits"
    args, w = _weights("tiny+norm")
    if key not in taps._W:
        taps._W[key] = (args, {n: bf16_round(v) for n, v in w.items()})
    rounded = taps._W[key][1]
    assert any(is_norm(n) and not np.array_equal(rounded[n], w[n]) for n in w)
    bits = {n: bf16_bits(v) for n, v in w.items()}
    assert all(v.dtype == np.uint16 for v in bits.values())
    _, _, model = build_model((args, bits), "bf16", 9)
    _check(key, "bf16", model, _tiny_prompts(args, 9, 4000 + 97 * 9), capsys=capsys)
    del model


# ----------------------------------------------------------------------------- scoring
@pytest.mark.parametrize("per_sample,mismatch", [(False, False), (True, False), (False, True)])
def test_compute_loss(per_sample, mismatch):
    """csm_frame_forced over whole sequences (tests/test_scoring_gpu.py's batch and tolerance), rigged fp32."""
    from csm_mlx.scoring import compute_loss
    from oracle.csm_oracle import compute_loss_ref
    from test_scoring_gpu import _batch
    args, w, model = _engine("tiny+norm", "float32", 2)
    batch = _batch(args)
    got = compute_loss(model, batch, per_sample=per_sample, cause_mismatch=mismatch)
    ref = compute_loss_ref(oracle_for(args, w), batch, per_sample=per_sample, cause_mismatch=mismatch)
    assert np.all(np.isfinite(got)) and np.shape(got) == np.shape(ref)
    np.testing.assert_allclose(got, ref, rtol=1e-4)


# ----------------------------------------------------------------------------- a running batch
def test_greedy_queue_matches_oracle():
    """generate_queue over the 14 slot prompts through 4 slots, greedy, tiny bf16: every utterance bit-exact against
    OracleCSM.generate_codes alone on its prompt (as tests/test_slots_gpu.py).  The norm rig sits on the EOS-capable
    weights, so utterances end at different frames and slots turn over."""
    from csm_mlx import generate_queue
    from helpers import eos_weights
    args, base = eos_weights("tiny")
    w = norm_rig(args, base)
    _, _, model = build_model((args, w), "bf16", max_batch=4)
    prompts = slot_prompts(args.n_audio_codebooks)
    o = oracle_for(args, w, bf16=True)
    want = [o.generate_codes(t, m, CAP) for t, m in prompts]
    print("oracle frame counts (greedy, norm rig):", [len(r) for r in want])
    assert len({len(r) for r in want}) > 2
    got = generate_queue(model, prompts, slots=4, max_audio_frames=[CAP] * N_TINY, decode=False)
    assert len(got) == len(want)
    for i, (g, r) in enumerate(zip(got, want)):
        d = first_divergence(g, r)
        assert d is None and len(g) == len(r), f"utterance {i}: {len(g)} frames vs {len(r)}, first divergence {d}"
    del model
