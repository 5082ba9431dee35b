"""Continuous batching (csm_mlx.batching, csrc/csm_engine_slots.hip): utterances join and leave a running
batch of slots, and every utterance's codes depend only on its prompt, its seed, the sampler and the
processors -- not on the slot, on when it joined, on who ran beside it or on what ran in the slot before.

The reference for codes is always ``OracleCSM.generate_codes`` run alone on each prompt (bf16-rounded or
int4 weights through ``helpers.oracle_for``); nothing is compared against another run of the slot path.

Tiny cases: ``helpers.eos_weights("tiny")`` (K = 4, V = 67, utterances can end), 14 prompts of 4..10 rows,
a cap of 40 frames.  The oracle's frame counts are spread over 0..40 (several utterances end at frame 0:
the empty-result edge), so slots turn over at many different frames; the tests recompute them."""
import ctypes

import numpy as np
import pytest

from helpers import csm_weights, eos_weights, first_divergence, oracle_for, prompt_ids
from rigs import CAP, N_TINY, SEEDS, build_model, slot_prompts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    args, w, model = build_model(eos_weights("tiny"), "bf16", max_batch=8)
    yield args, w, model, oracle_for(args, w, bf16=True), slot_prompts(args.n_audio_codebooks)
    del model


_REFS = {}


def refs(o, prompts, key, caps, **kw):
    """The oracle alone on each prompt, computed once per case and shared."""
    if key not in _REFS:
        seeds = kw.pop("seeds", None)
        _REFS[key] = [o.generate_codes(t, m, caps[i], **kw, **({"seed": seeds[i]} if seeds else {}))
                      for i, (t, m) in enumerate(prompts)]
    return _REFS[key]


def greedy_refs(tiny):
    _, _, _, o, prompts = tiny
    return refs(o, prompts, "greedy", [CAP] * N_TINY)


def assert_exact(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, r) in enumerate(zip(got, want)):
        d = first_divergence(g, r)
        assert d is None and len(g) == len(r), f"{what} utterance {i}: {len(g)} frames vs {len(r)}, first divergence {d}"


@pytest.mark.parametrize("slots", [4, 8])
def test_greedy_queue_matches_oracle(tiny, slots):
    """4 slots run the GEMV paths, 8 slots every projection on the matrix cores; result order = prompt order."""
    from csm_mlx import generate_queue
    _, _, model, _, prompts = tiny
    want = greedy_refs(tiny)
    print("oracle frame counts (greedy):", [len(r) for r in want])
    assert len({len(r) for r in want}) > 4 and any(len(r) == 0 for r in want)     # slots turn over at many frames
    got = generate_queue(model, prompts, slots=slots, max_audio_frames=[CAP] * N_TINY, decode=False)
    assert_exact(got, want, f"{slots} slots:")


def test_sampled_queue_matches_oracle(tiny):
    """temperature 0.8, top-k 50, seeds 1234 + i: bit-exact against the oracle's restatement of the RNG, whose
    counter is the utterance's own frame index -- a sampler keyed on the global frame counter fails here."""
    from csm_mlx import generate_queue
    _, _, model, o, prompts = tiny
    want = refs(o, prompts, "sampled", [CAP] * N_TINY, temperature=0.8, top_k=50, seeds=SEEDS)
    print("oracle frame counts (sampled):", [len(r) for r in want])
    got = generate_queue(model, prompts, slots=8, temperature=0.8, top_k=50, seeds=SEEDS,
                         max_audio_frames=[CAP] * N_TINY, decode=False)
    assert_exact(got, want, "sampled:")
    got = generate_queue(model, prompts, slots=8, temperature=0.8, top_k=50, seeds=1234,      # scalar s: s + i
                         max_audio_frames=[CAP] * N_TINY, decode=False)
    assert_exact(got, want, "sampled, scalar seed:")


def test_ring_history(tiny):
    """A 48-frame history: the session runs well over 48 global frames (the 40-frame utterances alone take
    more than that through 4 slots), every utterance still bit-exact; a cap above 48 is refused."""
    from csm_mlx import SlotBatch, _lib, generate_queue
    from csm_mlx.models import CSM
    from csm_mlx.sampling import Sampler
    args, w, _, _, prompts = tiny
    want = greedy_refs(tiny)
    assert sum(len(r) for r in want) > 4 * 48
    model = CSM(args, dtype="bf16", max_batch=4, max_frames=48)
    model.load_weights(w)
    got = generate_queue(model, prompts, slots=4, max_audio_frames=[CAP] * N_TINY, decode=False)
    frames_run = ctypes.c_int(0)
    _lib.check(_lib.lib().csm_read_codes(model.engine, None, None, None, ctypes.byref(frames_run)))
    print("global frames run:", frames_run.value)
    assert frames_run.value > 48 + 8       # utterances ran across the wrap
    assert_exact(got, want, "ring:")
    batch = SlotBatch(model, 4, sampler=Sampler(0.0, 0))
    with pytest.raises(_lib.CsmHipError) as ei:
        batch.submit(*prompts[0], 49)
    assert ei.value.code == _lib.CSM_ERR_STATE
    # the engine's own refusal: frames that would take a slot's utterance past the history
    eng = batch._eng
    eng.restart(0, 0)
    for b in (1, 2, 3):
        eng.release(b)
    eng.prefill([(0, *prompts[2])])
    eng.run(48)
    with pytest.raises(_lib.CsmHipError) as ei:
        eng.run(1)
    assert ei.value.code == _lib.CSM_ERR_STATE
    hist = np.zeros((48, 4, args.n_audio_codebooks), np.int32)
    assert _lib.lib().csm_read_codes(model.engine, _lib.ptr(hist), None, None, None) == _lib.CSM_ERR_STATE
    del model


def test_processors_across_a_restart(tiny):
    """logit_bias + repetition penalty over the last 8 c0 codes, per-prompt caps cycling 5, 9, 14, 24: the
    window of a new utterance never holds its predecessor's codes in the same slot (on the oracle, seeding the
    window with a previous utterance's last 8 c0 codes changes the first frames of 8 of these 14)."""
    from csm_mlx import generate_queue
    from csm_mlx.sampling import make_logits_processors
    _, _, model, o, prompts = tiny
    procs = make_logits_processors(logit_bias={0: -2.0}, repetition_penalty=1.5, repetition_context_size=8)
    caps = [(5, 9, 14, 24)[i % 4] for i in range(N_TINY)]
    want = refs(o, prompts, "procs", caps, processors=procs)
    print("oracle frame counts (processors):", [len(r) for r in want])
    got = generate_queue(model, prompts, slots=4, max_audio_frames=caps, decode=False, logits_processors=procs)
    assert_exact(got, want, "processors:")


@pytest.mark.parametrize("chunk", [1, 5])
def test_independent_of_arrival(tiny, chunk):
    """Reversed submission order and other chunk lengths: the per-ticket codes are the oracle's (test 1's)."""
    from csm_mlx import SlotBatch
    from csm_mlx.sampling import Sampler
    _, _, model, _, prompts = tiny
    want = greedy_refs(tiny)
    batch = SlotBatch(model, 4, sampler=Sampler(0.0, 0), chunk=chunk)
    order = list(reversed(range(N_TINY)))
    tickets = {batch.submit(*prompts[i], CAP, 0): i for i in order}
    got = {tickets[t]: c for t, c in batch.run()}
    assert sorted(got) == list(range(N_TINY))
    assert_exact([got[i] for i in range(N_TINY)], want, f"reversed, chunk {chunk}:")


def test_static_behaviour_untouched(tiny):
    """A plain generate_batch after a SlotBatch gives the codes it gave before; the old SlotBatch is then
    superseded; a parked slot's position stays 0."""
    from csm_mlx import SlotBatch, _lib, generate_batch
    from csm_mlx.sampling import Sampler
    _, _, model, _, prompts = tiny
    before = generate_batch(model, prompts[:8], 12 * 80, decode=False)
    assert_exact(before, [r[:12] for r in greedy_refs(tiny)[:8]], "static before slots:")
    batch = SlotBatch(model, 4, sampler=Sampler(0.0, 0))
    batch.submit(*prompts[2], 10, 0)                      # one utterance: slots 1..3 are parked
    run = batch.run()
    eng = batch._eng
    # drive one boundary by hand to look at the parked slots while slot 0 runs
    list(batch._fill())
    pos = np.zeros(4, np.int32)
    for _ in range(10):
        eng.run(1)
        _lib.check(_lib.lib().csm_debug_read(model.engine, b"pos", _lib.ptr(pos), pos.nbytes, None))
        assert list(pos[1:]) == [0, 0, 0], pos
    assert pos[0] == len(prompts[2][0]) - 1 + 9
    n, done = eng.poll()
    assert list(done[1:]) == [True] * 3 and list(n[1:]) == [0] * 3
    after = generate_batch(model, prompts[:8], 12 * 80, decode=False)
    assert_exact(after, before, "static after slots:")
    with pytest.raises(RuntimeError, match="superseded"):
        next(run)


# ----------------------------------------------------------------------------- csm_1b: the persistent batched step
@pytest.fixture(scope="module")
def weights_1b():
    return csm_weights("1b")


def prompts_1b(n, K):
    from csm_mlx.tokenizers import tokenize_text_segment
    return [tokenize_text_segment(prompt_ids(1000 + i), 0, K) for i in range(n)]


def test_csm_1b_bf16_greedy(weights_1b):
    """bf16 greedy through 8 slots: 12 prompts, caps cycling 2, 3, 4, 5 (codebook steps >= 2 on dec_step_xs)."""
    from csm_mlx import generate_queue
    args, w = weights_1b
    prompts = prompts_1b(12, args.n_audio_codebooks)
    caps = [(2, 3, 4, 5)[i % 4] for i in range(12)]
    model = build_model(weights_1b, "bf16", max_batch=8)[2]
    got = generate_queue(model, prompts, slots=8, max_audio_frames=caps, decode=False)
    del model
    o = oracle_for(args, w, bf16=True)
    want = [o.generate_codes(t, m, caps[i]) for i, (t, m) in enumerate(prompts)]
    assert_exact(got, want, "csm_1b bf16:")


def test_csm_1b_q4_sampled(weights_1b):
    """int4 sampled (temperature 0.8, top-k 50: the sampler inside the persistent step's launch) through 8
    slots: 10 prompts, caps cycling 2, 3, 4."""
    from csm_mlx import generate_queue
    args, w = weights_1b
    prompts = prompts_1b(10, args.n_audio_codebooks)
    caps = [(2, 3, 4)[i % 3] for i in range(10)]
    seeds = [1234 + i for i in range(10)]
    model = build_model(weights_1b, "q4", max_batch=8)[2]
    got = generate_queue(model, prompts, slots=8, temperature=0.8, top_k=50, seeds=seeds, max_audio_frames=caps,
                         decode=False)
    del model
    o = oracle_for(args, w, q4=True)
    want = [o.generate_codes(t, m, caps[i], temperature=0.8, top_k=50, seed=seeds[i]) for i, (t, m) in enumerate(prompts)]
    assert_exact(got, want, "csm_1b int4 sampled:")
