"""Per-utterance sampling parameters in a running SlotBatch (csm_slot_set_sampling, ``SlotBatch.submit(sampler=,
logits_processors=)``): every utterance's codes are those it gets alone with its own sampler and processors,
whatever the other slots sample with and whatever plan (greedy / sampled / filtered, with or without the c0
processors pass) the batch runs while it is resident.

The reference for codes is always ``OracleCSM.generate_codes`` run alone on each prompt with that prompt's own
parameters; nothing is compared against another run of the slot path.  Comparison is bit-exact.

The oracle's ``filter_keep`` warns that a top-p or min-p boundary within float32 rounding of its cut may fall
differently on the GPU, which sums the same float32 values in another order.  Every top-p / min-p utterance here
is therefore checked on the CPU oracle first (``assert_clear_of_the_cuts``): over all of its frames and
codebooks, no kept entry's ascending cumulative probability lies within TOP_P_MARGIN of float32(1 - top_p), and
no kept entry's log-probability within MIN_P_MARGIN of the min-p threshold.  The margins come from the number
format, not from the GPU: an n-term float32 sum differs between two summation orders by at most 2 n u S (u =
2^-24, S the sum: here <= the cut 0.1 .. 0.3, n <= 67 kept entries in the tiny model and <= 50 after top-k in
csm_1b), i.e. <= 2.4e-6, plus the 1 - 2 ulp of expf per term (<= 4e-8 S); TOP_P_MARGIN = 1e-5 is four times
that.  A log-probability carries the error of lse (an n-term sum inside a log: <= n u = 4e-6 relative on the
sum, so 4e-6 absolute, plus an ulp of lse ~ 1e-6); MIN_P_MARGIN = 1e-4 is twenty times that.  A seed that fails
the check is replaced by another seed, never by a wider comparison."""
import ctypes

import numpy as np
import pytest

from helpers import csm_weights, eos_weights, first_divergence, oracle_for, prompt_ids
from rigs import CAP, N_TINY, SEEDS, build_model, slot_prompts

pytestmark = pytest.mark.gpu

F32 = np.float32
TOP_P_MARGIN, MIN_P_MARGIN = 1e-5, 1e-4


@pytest.fixture(scope="module")
def tiny():
    args, w, model = build_model(eos_weights("tiny"), "bf16", max_batch=8)
    yield args, w, model, oracle_for(args, w, bf16=True), slot_prompts(args.n_audio_codebooks)
    del model


def assert_exact(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, r) in enumerate(zip(got, want)):
        d = first_divergence(g, r)
        assert d is None and len(g) == len(r), f"{what} utterance {i}: {len(g)} frames vs {len(r)}, first divergence {d}"


# ----------------------------------------------------------------------------- the oracle's side
def oracle_kw(smp, procs=None):
    kw = dict(temperature=smp.temp, top_k=smp.top_k)
    if not smp.greedy:
        kw.update(top_p=smp.top_p, min_p=smp.min_p, min_keep=smp.min_tokens_to_keep)
    if procs:
        kw["processors"] = procs
    return kw


def cut_margins(logits, smp):
    """(distance of the nearest kept entry's ascending cumulative probability to float32(1 - top_p), distance of
    the nearest kept entry's log-probability to the min-p threshold) of one row, by ``filter_keep``'s own
    float32 steps; inf where the filter is off."""
    from oracle.csm_oracle import topk_threshold
    l = np.asarray(logits, F32)
    n = l.shape[-1]
    keep = l >= topk_threshold(l, smp.top_k)
    mx = l.max()
    lse = F32(mx + F32(np.log(np.sum(np.exp(l - mx, dtype=F32), dtype=F32))))
    lp = (l - lse).astype(F32)
    order = np.lexsort((np.arange(n), -lp.astype(np.float64)))
    dp = dm = np.inf
    if 0.0 < smp.top_p < 1.0:
        p_desc = np.where(keep[order], np.exp(lp[order]), F32(0)).astype(F32)
        cum = np.cumsum(p_desc[::-1], dtype=F32)[::-1]
        cut = F32(1.0 - smp.top_p)
        dp = float(np.abs(cum[keep[order]].astype(np.float64) - float(cut)).min())
        kp = np.zeros(n, bool)
        kp[order] = cum > cut
        keep = keep & kp
    if smp.min_p != 0.0 and keep.any():
        tmin = F32(lp[keep].max() + F32(np.log(smp.min_p)))
        dm = float(np.abs(lp[keep].astype(np.float64) - float(tmin)).min())
    return dp, dm


def reference(o, prompt, cap, smp, seed, procs=None):
    """The oracle alone on one prompt with its own parameters; a filtered utterance is checked clear of the
    cuts on the way (module docstring).  The c0 processors act before the sampler: their logits are what the
    filters see, and ``collect_logits`` hands back exactly those."""
    if smp.greedy or not smp.filtered:
        return o.generate_codes(*prompt, cap, seed=seed, **oracle_kw(smp, procs))
    codes, logs = o.generate_codes(*prompt, cap, seed=seed, collect_logits=True, **oracle_kw(smp, procs))
    for f, (c0, ci) in enumerate(logs):
        for cb, row in enumerate([c0, *ci]):
            dp, dm = cut_margins(row, smp)
            assert dp > TOP_P_MARGIN and dm > MIN_P_MARGIN, \
                f"seed {seed}, frame {f}, codebook {cb}: a boundary {dp:.3g} / {dm:.3g} from its cut -- take another seed"
    return codes


_REFS = {}


def refs(key, o, prompts, caps, samplers, seeds, procs=None):
    """The references of one case, computed once and shared."""
    if key not in _REFS:
        procs = procs or [None] * len(prompts)
        _REFS[key] = [reference(o, prompts[i], caps[i], samplers[i], seeds[i], procs[i]) for i in range(len(prompts))]
    return _REFS[key]


# ----------------------------------------------------------------------------- 1. mixed samplers
def mixed_samplers():
    from csm_mlx.sampling import Sampler
    kinds = [Sampler(0.0, 0), Sampler(0.8, 50), Sampler(1.2, 5), Sampler(0.7, 0, 0.9, 0.05)]
    return [kinds[i % 4] for i in range(N_TINY)]


# (the seeds of rigs.SEEDS, 1234 + i; an utterance whose top-p / min-p check fails there gets another)
MIXED_SEEDS = list(SEEDS)


@pytest.mark.parametrize("slots", [4, 8])
def test_mixed_samplers_match_their_oracles(tiny, slots):
    """Prompt i samples with entry i % 4 of greedy / 0.8, top-k 50 / 1.2, top-k 5 / 0.7, top-p 0.9, min-p 0.05
    over a greedy batch: 4 slots run the GEMV paths, 8 the matrix cores.  The frame counts are spread, so slots
    change owner between sampler kinds and the plan class changes while the batch runs."""
    from csm_mlx import generate_queue
    _, _, model, o, prompts = tiny
    smp = mixed_samplers()
    want = refs("mixed", o, prompts, [CAP] * N_TINY, smp, MIXED_SEEDS)
    print("oracle frame counts (mixed):", [len(r) for r in want])
    assert len({len(r) for r in want}) > 4                                   # slots turn over at many frames
    for kind in range(4):                                                    # ... and every kind runs some frames
        assert any(len(want[i]) > 0 for i in range(kind, N_TINY, 4)), kind
    got = generate_queue(model, prompts, slots=slots, seeds=MIXED_SEEDS, max_audio_frames=[CAP] * N_TINY, decode=False,
                         samplers=[None if s.greedy else s for s in smp])
    assert_exact(got, want, f"mixed, {slots} slots:")


# ----------------------------------------------------------------------------- 2. defaults and no leak
def test_defaults_and_no_leak(tiny):
    """The batch samples at 0.8 / top-k 50; every third prompt is greedy with logit_bias {0: -2}, a repetition
    penalty of 1.5 over 8 codes.  Those equal their oracle; the others equal the oracle at the default -- a slot
    that held an override forgets it at the restart, and its bias row does not reach the next utterance."""
    from csm_mlx import generate_queue
    from csm_mlx.sampling import Sampler, make_logits_processors
    _, _, model, o, prompts = tiny
    procs = make_logits_processors(logit_bias={0: -2.0}, repetition_penalty=1.5, repetition_context_size=8)
    caps = [(5, 9, 14, 24)[i % 4] for i in range(N_TINY)]
    own = [i % 3 == 0 for i in range(N_TINY)]
    smp = [Sampler(0.0, 0) if own[i] else Sampler(0.8, 50) for i in range(N_TINY)]
    want = refs("leak", o, prompts, caps, smp, SEEDS, [procs if own[i] else None for i in range(N_TINY)])
    print("oracle frame counts (defaults):", [len(r) for r in want])
    got = generate_queue(model, prompts, slots=4, temperature=0.8, top_k=50, seeds=SEEDS, max_audio_frames=caps,
                         decode=False, samplers=[Sampler(0.0, 0) if own[i] else None for i in range(N_TINY)],
                         prompt_processors=[procs if own[i] else None for i in range(N_TINY)])
    assert_exact(got, want, "defaults:")


# ----------------------------------------------------------------------------- 3. plan-independence
# the two utterances that change the plan: a long sampled one (resident from the first boundary: the sampled
# plan) and a top-p one that joins midway (the filtered plan); (prompt index, seed)
LONG, TOP_P = (9, 4321), (1, 979)


def beside(tiny, order, chunk):
    """The 14 greedy prompts in ``order`` beside the long sampled utterance (submitted first) and the top-p one
    (submitted in the middle of the queue).  Returns (greedy codes by prompt, sampled codes, top-p codes)."""
    from csm_mlx import SlotBatch
    from csm_mlx.sampling import Sampler
    _, _, model, _, prompts = tiny
    batch = SlotBatch(model, 4, sampler=Sampler(0.0, 0), chunk=chunk)
    t_long = batch.submit(*prompts[LONG[0]], CAP, LONG[1], sampler=Sampler(0.8, 50))
    tickets, t_top_p = {}, None
    for n, i in enumerate(order):
        if n == N_TINY // 2:
            t_top_p = batch.submit(*prompts[TOP_P[0]], CAP, TOP_P[1], sampler=Sampler(0.7, 0, 0.9))
        tickets[batch.submit(*prompts[i], CAP, 0)] = i
    got = dict(batch.run())
    return [got[t] for t in sorted(tickets, key=tickets.get)], got[t_long], got[t_top_p]


def test_greedy_codes_do_not_depend_on_the_plan(tiny):
    """The 14 prompts, all greedy: alone as a greedy batch, then beside a long sampled utterance (the sampled
    plan: the greedy rows' arg-max runs in the sample kernels) with a top-p utterance joining midway (the
    filtered kernel for all rows): the oracle's greedy codes every time, also in reversed order at chunk 1."""
    from csm_mlx import generate_queue
    from csm_mlx.sampling import Sampler
    _, _, model, o, prompts = tiny
    greedy = [Sampler(0.0, 0)] * N_TINY
    want = refs("greedy", o, prompts, [CAP] * N_TINY, greedy, [0] * N_TINY)
    long_ref = reference(o, prompts[LONG[0]], CAP, Sampler(0.8, 50), LONG[1])
    top_p_ref = reference(o, prompts[TOP_P[0]], CAP, Sampler(0.7, 0, 0.9), TOP_P[1])
    print("oracle frame counts: greedy", [len(r) for r in want], "sampled", len(long_ref), "top-p", len(top_p_ref))
    # the sampled utterance outlasts the queue's first half, the top-p one runs some frames beside the rest
    assert len(long_ref) >= 30 and len(top_p_ref) >= 4
    got = generate_queue(model, prompts, slots=4, seeds=[0] * N_TINY, max_audio_frames=[CAP] * N_TINY, decode=False)
    assert_exact(got, want, "greedy alone:")
    for order, chunk in ((list(range(N_TINY)), 8), (list(reversed(range(N_TINY))), 1)):
        g, s, t = beside(tiny, order, chunk)
        assert_exact(g, want, f"greedy beside sampled and top-p, chunk {chunk}:")
        assert_exact([s, t], [long_ref, top_p_ref], f"the sampled and the top-p utterance, chunk {chunk}:")


# ----------------------------------------------------------------------------- 4. ABI refusals
def test_abi_refusals(tiny):
    from csm_mlx import SlotBatch, _lib, generate_batch
    from csm_mlx.generation import FrameCache
    from csm_mlx.sampling import Sampler
    args, _, model, o, prompts = tiny
    L, V = _lib.lib(), args.n_audio_vocab
    greedy = refs("greedy", o, prompts, [CAP] * N_TINY, [Sampler(0.0, 0)] * N_TINY, [0] * N_TINY)
    before = generate_batch(model, prompts[:8], 12 * 80, decode=False)
    assert_exact(before, [r[:12] for r in greedy[:8]], "static before:")

    def sampling(idx=(), val=(), penalty=0.0, context=0):
        i, v = np.asarray(idx, np.int32), np.asarray(val, np.float32)
        s = _lib.CsmSampling(0.8, 50, 0.0, 0.0, 1, len(i), i.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                             v.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), penalty, context)
        s._keep = (i, v)
        return s

    def call(b, s):
        return L.csm_slot_set_sampling(model.engine, b, ctypes.byref(s) if s is not None else None)
    cache = FrameCache(model, 4, Sampler(0.0, 0), [0] * 4)
    assert call(0, sampling()) == _lib.CSM_ERR_STATE                   # csm_begin alone is not slot mode
    del cache
    batch = SlotBatch(model, 4, sampler=Sampler(0.0, 0))
    eng = batch._eng
    eng.restart(0, 0)
    for b in (2, 3):
        eng.release(b)
    eng.restart(1, 0)
    assert call(4, sampling()) == _lib.CSM_ERR_STATE                   # b >= B
    assert call(2, sampling()) == _lib.CSM_ERR_STATE                   # a parked slot holds no utterance
    assert call(1, sampling(idx=[V], val=[1.0])) == _lib.CSM_ERR_ARG   # bias index = V
    assert call(1, sampling(penalty=1.5, context=257)) == _lib.CSM_ERR_ARG
    assert call(1, sampling(penalty=-1.0, context=8)) == _lib.CSM_ERR_ARG
    assert call(1, sampling(idx=[V - 1], val=[1.0], penalty=1.5, context=256)) == _lib.CSM_OK
    assert call(1, None) == _lib.CSM_OK                                # the batch's again
    eng.prefill([(0, *prompts[2]), (1, *prompts[3])])
    eng.run(1)
    assert call(0, sampling()) == _lib.CSM_ERR_STATE                   # its utterance has run a frame
    assert b"already run a frame" in L.csm_last_error()
    eng.run(3)
    assert_exact([eng.read(0, 4), eng.read(1, 4)], [greedy[2][:4], greedy[3][:4]], "after the refusals:")
    after = generate_batch(model, prompts[:8], 12 * 80, decode=False)
    assert_exact(after, before, "static after:")


# ----------------------------------------------------------------------------- 5. csm_1b: the persistent batched step
@pytest.fixture(scope="module")
def weights_1b():
    return csm_weights("1b")


def prompts_1b(n, K):
    from csm_mlx.tokenizers import tokenize_text_segment
    return [tokenize_text_segment(prompt_ids(1000 + i), 0, K) for i in range(n)]


SEEDS_1B = [1234 + i for i in range(10)]
CAPS_1B = [(2, 3, 4)[i % 3] for i in range(10)]


def run_1b(weights_1b, dtype, smp, seeds):
    from csm_mlx import generate_queue
    args, w = weights_1b
    prompts = prompts_1b(10, args.n_audio_codebooks)
    model = build_model(weights_1b, dtype, max_batch=8)[2]
    got = generate_queue(model, prompts, slots=8, seeds=seeds, max_audio_frames=CAPS_1B, decode=False,
                         samplers=[None if s.greedy else s for s in smp])
    del model
    o = oracle_for(args, w, bf16=True) if dtype == "bf16" else oracle_for(args, w, q4=True)
    want = [reference(o, prompts[i], CAPS_1B[i], smp[i], seeds[i]) for i in range(10)]
    assert_exact(got, want, f"csm_1b {dtype}:")


def test_csm_1b_bf16_greedy_beside_sampled(weights_1b):
    """bf16 through 8 slots, prompts alternating greedy and 0.8 / top-k 50 over a greedy batch: dec_step_xs's
    fused sampler (role_s) with greedy and sampled rows in one launch."""
    from csm_mlx.sampling import Sampler
    run_1b(weights_1b, "bf16", [Sampler(0.0, 0) if i % 2 == 0 else Sampler(0.8, 50) for i in range(10)], SEEDS_1B)


def test_csm_1b_q4_with_top_p(weights_1b):
    """int4: the same mix with prompts 5 and 7 (caps 4 and 3) at 0.8 / top-k 50 / top-p 0.9, which put the whole
    batch on sample_filtered_kernel while they are resident (greedy rows and rows with both filters off among
    them).  Their seeds are not 1234 + i: at 1239 and 1241 a top-p boundary lies 2e-7 and 9e-6 from the cut on
    the oracle; at 2052 and 2073 the nearest is 3.4e-5 and 5.8e-5 away."""
    from csm_mlx.sampling import Sampler
    smp = [Sampler(0.0, 0) if i % 2 == 0 else Sampler(0.8, 50) for i in range(10)]
    smp[5] = smp[7] = Sampler(0.8, 50, 0.9)
    seeds = list(SEEDS_1B)
    seeds[5], seeds[7] = 2052, 2073
    run_1b(weights_1b, "q4", smp, seeds)
