"""Shared context prefixes (csrc/csm_engine_prefix.hip, csm_mlx/prefix.py): the backbone K / V of a prompt's first
rows saved once (csm_prefix_save) and copied into any utterance or slot that begins with them (csm_prefix_load),
which then prefills only the rows that follow.

What is held:
  * the copy is exact and goes nowhere else: the loaded rows equal the saved source bit for bit in every layer, K
    and V (read through csm_kv_read); the rows behind them, the other slots and their positions are untouched;
  * codes are those of the whole prompt: always ``OracleCSM.generate_codes`` alone on prefix + suffix
    (``helpers.oracle_for``), bit-exact, never another engine run -- B = 1, 4 (mixed None / prefix entries, two
    utterances sharing one prefix) and 8 (matrix cores), through 4 and 8 slots, with ``keep_rows``;
  * the taps against float64 on the whole prompt under the project's bar, helpers.BAR_MARGIN (2) x e32, e32 from
    the two references alone.  A missing or misplaced key measures >= 1825 x e32, so the
    unchanged bar separates a wrong copy from a right one; engine / e32 is printed per tap;
  * csm_1b: the same bar, and the persistent kernels' epochs move as they do after a whole-prompt prefill (+80 per
    decode row, +498 per frame): the load has not pushed the frame off its fast path;
  * the window counts prefix + suffix rows; refusals change nothing.

The window (csm_engine_abi.hip require_window; tests/test_f64_long_gpu.py confirmed it on the GPU): after L rows
nframes <= max_seq_len + 1 - L are admitted.  A prefix of max_seq_len - 8 rows + a 5-row suffix is L = max_seq_len
- 3, so FOUR frames run and the fifth is CSM_ERR_TOO_LONG -- exactly what the whole prompt of that length is
admitted (the issue's text says three; by the rule it cites it is four, and a prefix must not change it).  The
reference's own guard (generation.py:131-137, L >= max_seq_len - max_audio_frames) is stricter and refuses that
prompt with a cap of 4 frames, through ``generate`` and ``submit`` alike."""
import ctypes

import numpy as np
import pytest

from helpers import (BAR_MARGIN, TAPS, csm_weights, eos_weights, f64_reference, first_divergence, long_prompt,
                     mimi_pcm_clip, oracle_for, rms, tap_errors)
from rigs import (CAP, N_TINY, SEEDS, TAP_NAMES, build_model, epoch, frame_taps, handoffs, read_taps, slot_prompts,
                  synchronize)

pytestmark = pytest.mark.gpu

FRAMES = 12
PCM_RMS = 1e-4
PAIRS = [(1, 5), (63, 1), (64, 20), (65, 70), (130, 5)]        # (prefix rows, suffix rows)


def greedy():
    from csm_mlx.sampling import Sampler
    return Sampler(0.0, 0)


def cat(*prompts):
    return (np.concatenate([t for t, _ in prompts], 0).astype(np.int32),
            np.concatenate([np.asarray(m).astype(bool) for _, m in prompts], 0))


def cut(prompt, a, b=None):
    return prompt[0][a:b], prompt[1][a:b]


def assert_exact(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, r) in enumerate(zip(got, want)):
        d = first_divergence(g, r)
        assert d is None and len(g) == len(r), f"{what} utterance {i}: {len(g)} frames vs {len(r)}, first divergence {d}"


# ----------------------------------------------------------------------------- raw calls
def lib():
    from csm_mlx import _lib
    return _lib


def rc_load(model, utts, ids):
    u, i = np.asarray(utts, np.int32), np.asarray(ids, np.int32)
    return lib().lib().csm_prefix_load(model.engine, len(u), lib().ptr(u), lib().ptr(i))


def rc_save(model, b, rows):
    h = ctypes.c_int(-1)
    return lib().lib().csm_prefix_save(model.engine, b, rows, ctypes.byref(h)), h.value


def rc_run(model, n=1):
    done = ctypes.c_int(0)
    return lib().lib().csm_run_frames(model.engine, n, ctypes.byref(done))


def positions(model, B):
    pos = np.zeros(B, np.int32)
    lib().check(lib().lib().csm_debug_read(model.engine, b"pos", lib().ptr(pos), pos.nbytes, None))
    return pos


def kv_read(model, b, first, rows):
    """(layers, 2, Hkv, rows, hd) float32: K and V of positions first .. first+rows-1 of utterance b."""
    a = model.backbone.args
    out = np.zeros((a.num_hidden_layers, 2, a.num_key_value_heads, rows, a.head_dim), np.float32)
    for layer in range(a.num_hidden_layers):
        k, v = np.zeros(out.shape[2:], np.float32), np.zeros(out.shape[2:], np.float32)
        lib().check(lib().lib().csm_kv_read(model.engine, b, layer, first, rows, lib().ptr(k), lib().ptr(v)))
        out[layer, 0], out[layer, 1] = k, v
    return out


# ----------------------------------------------------------------------------- 1. the copy
def test_copy_is_exact_and_goes_nowhere_else():
    from csm_mlx.generation import FrameCache
    args, w, model = build_model(eos_weights("tiny"), "float32", max_batch=4)
    src_prompt, p3, p2 = (long_prompt(args, 700 + L, L) for L in (130, 140, 20))
    cache = FrameCache(model, 4, greedy(), [0] * 4)
    cache.prefill(1, *src_prompt)
    src = kv_read(model, 1, 0, 130)
    assert np.abs(src).max() > 0 and np.isfinite(src).all()
    rows_list = (1, 63, 64, 65, 130)
    saved = {rows: cache.save_prefix(1, rows, *cut(src_prompt, 0, rows)) for rows in rows_list}
    for rows, p in saved.items():
        L, H, hd = args_dims(model)
        assert (p.rows, p.nbytes) == (rows, 2 * L * H * rows * hd * 4)
    assert np.array_equal(kv_read(model, 1, 0, 130), src)                   # a save leaves its source alone
    cache.prefill(3, *p3)
    cache.prefill(2, *p2)
    for rows in rows_list:
        cache = FrameCache(model, 4, greedy(), [0] * 4)                      # csm_begin: every position -1
        before = {3: kv_read(model, 3, 0, 140), 2: kv_read(model, 2, 0, 20), 1: kv_read(model, 1, 0, 130)}
        pos0 = positions(model, 4)
        cache.load_prefix([(3, saved[rows])])
        after = {3: kv_read(model, 3, 0, 140), 2: kv_read(model, 2, 0, 20), 1: kv_read(model, 1, 0, 130)}
        assert after[3][:, :, :, :rows].tobytes() == src[:, :, :, :rows].tobytes(), f"{rows} rows: not the saved bits"
        assert np.array_equal(after[3][:, :, :, rows: rows + 8], before[3][:, :, :, rows: rows + 8]), f"{rows}: rows behind"
        assert np.array_equal(after[2], before[2]) and np.array_equal(after[1], before[1]), f"{rows}: another slot"
        pos = positions(model, 4)
        assert pos[3] == rows - 1 and np.array_equal(pos[:3], pos0[:3]), (rows, pos0, pos)
    del model


def args_dims(model):
    a = model.backbone.args
    return a.num_hidden_layers, a.num_key_value_heads, a.head_dim


# ----------------------------------------------------------------------------- 2. codes of the whole prompt
@pytest.fixture(scope="module")
def tiny():
    """tiny bf16 with EOS-capable weights, the tiny codec registered, the (prefix, suffix) cases and their
    prefixes, and a second suffix behind the 65-row prefix (two utterances sharing one prefix)."""
    from csm_mlx import cache_context
    from csm_mlx.config import MIMI_CONFIGURATION
    from csm_mlx.mimi import MimiCodec
    from csm_mlx.tokenizers import set_audio_tokenizer
    from csm_mlx.weights import synthetic_mimi_weights
    args, w, model = build_model(eos_weights("tiny"), "bf16", max_batch=8)
    mm = MIMI_CONFIGURATION["tiny"]
    codec = MimiCodec(mm, max_batch=8, max_frames=CAP)
    codec.load_weights(synthetic_mimi_weights(mm))
    set_audio_tokenizer(codec, args.n_audio_codebooks)
    whole = [long_prompt(args, 800 + i, P + S) for i, (P, S) in enumerate(PAIRS)]
    whole.append(cat(cut(whole[3], 0, 65), cut(long_prompt(args, 850, 40), 9, 40)))     # 65 shared + 31 other rows
    cuts = [P for P, _ in PAIRS] + [65]
    prefixes = [cache_context(model, cut(whole[i], 0, cuts[i])) for i in range(len(PAIRS))]
    prefixes.append(prefixes[3])
    case = dict(args=args, w=w, model=model, o=oracle_for(args, w, bf16=True), whole=whole, cuts=cuts, prefixes=prefixes,
                suffix=[cut(whole[i], cuts[i]) for i in range(len(whole))])
    yield case
    del model


SAMPLERS = {"greedy": dict(), "sampled": dict(temperature=0.8, top_k=50)}
_REFS = {}


def refs(o, key, prompts, frames, seeds=None, **kw):
    """The oracle alone on each whole prompt, once per key."""
    if key not in _REFS:
        _REFS[key] = [o.generate_codes(t, m, frames, **kw, **({"seed": seeds[i]} if seeds is not None else {}))
                      for i, (t, m) in enumerate(prompts)]
    return _REFS[key]


def batch_codes(model, prompts, prefixes, frames, how, seeds):
    from csm_mlx.generation import generate_codes_batch
    from csm_mlx.sampling import Sampler
    smp = Sampler(SAMPLERS[how].get("temperature", 0.0), SAMPLERS[how].get("top_k", 0))
    hist, n, _ = generate_codes_batch(model, prompts, frames, sampler=smp, seeds=seeds, prefixes=prefixes)
    return [hist[: n[b], b].copy() for b in range(len(prompts))]


@pytest.mark.parametrize("how", list(SAMPLERS))
def test_codes_are_the_whole_prompts(tiny, how):
    model, o, whole, suffix, prefixes = (tiny[k] for k in ("model", "o", "whole", "suffix", "prefixes"))
    n = len(whole)
    seeds = [4321 + i for i in range(n)]
    want = refs(o, how, whole, FRAMES, seeds if how == "sampled" else None, **SAMPLERS[how])
    print(f"oracle frame counts ({how}):", [len(r) for r in want])
    for i in range(len(PAIRS)):                                           # B = 1: csm_prefill of the suffix
        got = batch_codes(model, [suffix[i]], [prefixes[i]], FRAMES, how, [seeds[i]])
        assert_exact(got, [want[i]], f"B=1 {PAIRS[i]}:")
    # B = 4: prefix / whole prompt / the two utterances that share the 65-row prefix
    idx, use = [2, 0, 3, 5], [True, False, True, True]
    got = batch_codes(model, [suffix[i] if u else whole[i] for i, u in zip(idx, use)],
                      [prefixes[i] if u else None for i, u in zip(idx, use)], FRAMES, how, [seeds[i] for i in idx])
    assert_exact(got, [want[i] for i in idx], "B=4:")
    # B = 8 (every projection on the matrix cores): all six with their prefixes, two whole
    idx, use = [0, 1, 2, 3, 4, 5, 1, 4], [True] * 6 + [False] * 2
    got = batch_codes(model, [suffix[i] if u else whole[i] for i, u in zip(idx, use)],
                      [prefixes[i] if u else None for i, u in zip(idx, use)], FRAMES, how, [seeds[i] for i in idx])
    assert_exact(got, [want[i] for i in idx], "B=8:")


# ----------------------------------------------------------------------------- 3. float64 taps
def hold(tag, key, variant, prompts, codes, got, capsys):
    args, w = csm_weights(key)
    t64, e32 = f64_reference(args, w, variant, prompts, codes)
    err = tap_errors(got, t64)
    line = f"prefix-f64 {key} {variant} {tag}: " + " ".join(
        f"{t}={float(err[t].max()):.2e}({float(err[t].max()) / e32[t]:.2f}x)" for t in TAPS) + " | e32 " + " ".join(
        f"{t}={e32[t]:.2e}" for t in TAPS)
    with capsys.disabled():
        print("\n" + line)
    bad = [f"{t}: {float(err[t].max()):.3e} > {BAR_MARGIN} x e32 = {BAR_MARGIN * e32[t]:.3e}" for t in TAPS
           if not float(err[t].max()) <= BAR_MARGIN * e32[t]]
    assert not bad, line + "\n" + "\n".join(bad)


def prefix_taps(model, args, cuts, suffix_seeds, frames, batched):
    """Whole prompts = a shared ``cuts[i]``-row context (one per distinct length) + a 13..14-row suffix of its own;
    each context cached once, loaded in one call, the suffixes prefilled.  Returns (prompts, codes, taps)."""
    from csm_mlx import cache_context
    ctx = {P: long_prompt(args, 900 + P, P) for P in sorted(set(cuts))}
    saved = {P: cache_context(model, ctx[P]) for P in ctx}
    sfx = [cut(long_prompt(args, s, 40), 40 - n, 40) for s, n in suffix_seeds]
    prompts = [cat(ctx[P], s) for P, s in zip(cuts, sfx)]

    def feed(cache):
        cache.load_prefix([(b, saved[P]) for b, P in enumerate(cuts)])
        if batched:
            cache.prefill_batch([(b, *s) for b, s in enumerate(sfx)])
        else:
            for b, s in enumerate(sfx):
                cache.prefill(b, *s)
    hist, n, taps = frame_taps(model, prompts, frames, greedy(), [0] * len(prompts), TAP_NAMES, prefill=feed)
    synchronize(model)
    assert hist.shape[0] == frames and (n == frames).all(), "an utterance ended inside the window"
    return prompts, hist, tuple(taps[t] for t in TAP_NAMES)


@pytest.fixture(scope="module", params=["float32", "bf16", "q4"])
def tiny_plain(request):
    args, w, model = build_model("tiny", request.param, 9)
    yield request.param, args, model
    del model


@pytest.mark.parametrize("case", ["B1-65", "B1-511", "B9"])
def test_taps_against_float64(tiny_plain, case, capsys):
    dtype, args, model = tiny_plain
    cuts = {"B1-65": [65], "B1-511": [511], "B9": [65, 511, 65, 511, 511, 65, 65, 511, 65]}[case]
    prompts, codes, got = prefix_taps(model, args, cuts, [(950 + b, 13) for b in range(len(cuts))], 2, case == "B9")
    hold(case, "tiny", {"float32": "fp32"}.get(dtype, dtype), prompts, codes, got, capsys)


@pytest.mark.parametrize("dtype", ["bf16", "q4"])
def test_1b_stays_on_the_persistent_kernels(dtype, capsys):
    """csm_1b, B = 1: a 200-row prefix + 14 rows, 2 frames."""
    args, w, model = build_model("1b", dtype, 1)
    K = args.n_audio_codebooks
    names = ("dec_frame", "dec_xsd", "bb_step")

    def epochs():
        return {n: epoch(model, n) for n in names}
    e0 = epochs()                      # (caching the context runs no frame: the epochs move in the two frames alone)
    prompts, codes, got = prefix_taps(model, args, [200], [(990, 14)], 2, False)
    e1 = epochs()
    delta = {n: e1[n] - e0[n] for n in names}
    expect = {"dec_frame": handoffs("dec_frame", K) * 2, "dec_xsd": 0, "bb_step": handoffs("bb_step", K) * 1}
    assert delta == expect, f"kernels that ran (epoch deltas) {delta}, expected {expect}"
    hold("200+14", "1b", dtype, prompts, codes, got, capsys)
    del model


# ----------------------------------------------------------------------------- 4. the window's edge
def state_of(model, cache, B):
    hist, n, done = cache.codes()
    taps = read_taps(model, cache, B, TAP_NAMES)
    return [hist.tobytes(), n.tobytes(), done.tobytes(), positions(model, B).tobytes()] + [taps[t].tobytes() for t in TAP_NAMES]


def test_window_counts_prefix_and_suffix():
    from csm_mlx import SlotBatch, cache_context, generate
    from csm_mlx.generation import FrameCache
    args, w, model = build_model(eos_weights("tiny"), "float32", max_batch=2)
    S = model.max_seq_len
    whole = long_prompt(args, 1100, S - 3)
    prefix = cache_context(model, cut(whole, 0, S - 8))
    assert prefix.rows == S - 8
    cache = FrameCache(model, 1, greedy(), [0])
    cache.load_prefix([(0, prefix)])
    cache.prefill(0, *cut(whole, S - 8))
    admitted = S + 1 - (S - 3)                                            # require_window: 4
    for f in range(admitted):
        assert rc_run(model) == 0, (f, lib().lib().csm_last_error())
    synchronize(model)
    before = state_of(model, cache, 1)
    assert rc_run(model) == lib().CSM_ERR_TOO_LONG
    synchronize(model)
    assert state_of(model, cache, 1) == before
    hist, n, _ = cache.codes()
    # (the oracle's own guard is the reference's stricter one: lifted, its arithmetic is the same up to position S - 1)
    want = oracle_for(args, w).generate_codes(*whole, admitted, max_seq_len=S + admitted + 1)
    assert_exact([hist[: n[0], 0]], [want], "at the window's edge:")
    # the reference's guard on prefix + suffix rows: S - 3 >= S - 4
    ids = [int(x) for x in whole[0][S - 8:, -1]]
    text_rows = (np.ascontiguousarray(whole[0][S - 8:]), np.ascontiguousarray(whole[1][S - 8:]))
    with pytest.raises(ValueError, match="Inputs too long"):
        generate(model, ids, 0, prefix, max_audio_length_ms=4 * 80, temperature=0.0)
    batch = SlotBatch(model, 2, sampler=greedy())
    with pytest.raises(ValueError, match="Inputs too long"):
        batch.submit(*text_rows, 4, prefix=prefix)
    # a prefix of max_seq_len rows: saved, never loadable
    full = long_prompt(args, 1101, S)
    cache = FrameCache(model, 1, greedy(), [0])
    cache.prefill(0, *full)
    too_long = cache.save_prefix(0, S, *full)
    cache = FrameCache(model, 1, greedy(), [0])
    assert rc_load(model, [0], [too_long.handle]) == lib().CSM_ERR_TOO_LONG
    assert rc_run(model) == lib().CSM_ERR_STATE                           # still empty: nothing landed
    cache.prefill(0, *cut(whole, 0, 20))
    assert rc_run(model) == 0
    del model


# ----------------------------------------------------------------------------- 5. slots
@pytest.fixture(scope="module")
def queue(tiny):
    """The 14 slot prompts, each behind one of three shared contexts (65, 130, 17 rows) or none."""
    from csm_mlx import cache_context
    args, model = tiny["args"], tiny["model"]
    sp = slot_prompts(args.n_audio_codebooks)
    ctx = [long_prompt(args, 1200 + P, P) for P in (65, 130, 17)]
    voice = [i % 4 if i % 4 < 3 else None for i in range(N_TINY)]
    whole = [sp[i] if v is None else cat(ctx[v], sp[i]) for i, v in enumerate(voice)]
    saved = [cache_context(model, c) for c in ctx]
    return dict(sp=sp, ctx=ctx, voice=voice, whole=whole, saved=saved)


def queue_refs(tiny, queue, how):
    return refs(tiny["o"], "queue-" + how, queue["whole"], CAP, SEEDS if how == "sampled" else None, **SAMPLERS[how])


@pytest.mark.parametrize("how", list(SAMPLERS))
@pytest.mark.parametrize("slots", [4, 8])
def test_queue_with_shared_prefixes(tiny, queue, slots, how):
    from csm_mlx import generate_queue
    want = queue_refs(tiny, queue, how)
    print(f"oracle frame counts ({how}):", [len(r) for r in want])
    assert len({len(r) for r in want}) > 3                                 # slots turn over at different frames
    prefixes = [None if v is None else queue["saved"][v] for v in queue["voice"]]
    got = generate_queue(tiny["model"], queue["sp"], slots=slots, max_audio_frames=[CAP] * N_TINY, decode=False,
                         seeds=SEEDS, prefixes=prefixes, **SAMPLERS[how])
    assert_exact(got, want, f"{slots} slots, {how}:")


def test_keep_rows_pays_for_the_later_sentences(tiny, queue):
    """The first utterance of each voice is submitted whole with keep_rows = its context; the later ones join
    while run() is in progress, behind batch.kept(ticket)."""
    from csm_mlx import SlotBatch
    want = queue_refs(tiny, queue, "greedy")
    batch = SlotBatch(tiny["model"], 4, sampler=greedy())
    tickets, keeper = {}, {}
    for i in range(4):                                                     # voices 0, 1, 2 and a prompt without context
        v = queue["voice"][i]
        keep = 0 if v is None else queue["ctx"][v][0].shape[0]
        tickets[i] = batch.submit(*queue["whole"][i], CAP, SEEDS[i], keep_rows=keep)
        if v is not None:
            keeper[v] = tickets[i]
    with pytest.raises(ValueError):
        batch.kept(tickets[3])                                             # submitted without keep_rows
    with pytest.raises(RuntimeError):
        batch.kept(tickets[0])                                             # not joined yet
    got, later = {}, False
    for ticket, codes in batch.run():
        got[ticket] = codes
        if not later:                                                      # the batch is running: the rest join it
            later = True
            for i in range(4, N_TINY):
                v = queue["voice"][i]
                if v is None:
                    tickets[i] = batch.submit(*queue["whole"][i], CAP, SEEDS[i])
                else:
                    kept = batch.kept(keeper[v])
                    assert kept.rows == queue["ctx"][v][0].shape[0] and np.array_equal(kept.tokens, queue["ctx"][v][0])
                    tickets[i] = batch.submit(*queue["sp"][i], CAP, SEEDS[i], prefix=kept)
    assert_exact([got[tickets[i]] for i in range(N_TINY)], want, "keep_rows:")


def segments(args, n):
    from csm_mlx import Segment
    return [Segment(s % 2, [998, 20 + s, 30 + s, 999], audio=mimi_pcm_clip(9600 + 1920 * s, seed=60 + s)) for s in range(n)]


def test_stream_queue_matches_stream_generate(tiny):
    """PCM per utterance = stream_generate's for that utterance alone with the list context (RMS within the
    project's decode_step bar; the same number of frames)."""
    from csm_mlx import cache_context, stream_generate, stream_generate_queue
    from csm_mlx.tokenizers import tokenize_text_segment
    args, model = tiny["args"], tiny["model"]
    segs = segments(args, 2)
    texts = [[998, 100 + i, 200 + i, 300 + i, 999] for i in range(5)]
    alone = [np.concatenate([np.zeros((0,), np.float32)] + list(
        stream_generate(model, ids, 0, segs, max_audio_length_ms=10 * 80, temperature=0.0))) for ids in texts]
    print("frames per utterance:", [len(a) // 1920 for a in alone])
    prefix = cache_context(model, segs)
    got = {i: [] for i in range(len(texts))}
    for i, pcm, final in stream_generate_queue(model, [tokenize_text_segment(ids, 0, args.n_audio_codebooks) for ids in texts],
                                               slots=4, max_audio_frames=[10] * len(texts), prefixes=[prefix] * len(texts)):
        got[i].append(pcm)
    for i, ref in enumerate(alone):
        mine = np.concatenate(got[i])
        assert len(mine) == len(ref), (i, len(mine) // 1920, len(ref) // 1920)
        assert rms(mine, ref) <= PCM_RMS, (i, rms(mine, ref))


# ----------------------------------------------------------------------------- 6. drop-in
def test_generate_with_a_cached_context(tiny):
    from csm_mlx import cache_context, generate
    from csm_mlx.generation import build_prompt
    args, model, o = tiny["args"], tiny["model"], tiny["o"]
    segs = segments(args, 3)
    ids = [998, 41, 42, 43, 999]
    for n in (2, 3):
        whole = build_prompt(model, ids, 0, segs[:n])
        want = o.generate_codes(*whole, FRAMES)
        ref = generate(model, ids, 0, segs[:n], max_audio_length_ms=FRAMES * 80, temperature=0.0)
        prefix = cache_context(model, segs[:2]) if n == 2 else prefix.extend([segs[2]])
        text = build_prompt(model, ids, 0, prefix)
        assert prefix.rows + text[0].shape[0] == whole[0].shape[0] and text[0].shape[0] == len(ids)
        assert np.array_equal(np.concatenate([prefix.tokens, text[0]]), whole[0])
        assert np.array_equal(np.concatenate([prefix.mask, text[1]]), whole[1])
        got = batch_codes(model, [text], [prefix], FRAMES, "greedy", [0])
        assert_exact(got, [want], f"{n} segments:")
        pcm = generate(model, ids, 0, prefix, max_audio_length_ms=FRAMES * 80, temperature=0.0)
        assert pcm.shape == ref.shape == (len(want) * 1920,)
        assert rms(pcm, ref) <= PCM_RMS, (n, rms(pcm, ref))


# ----------------------------------------------------------------------------- 7. refusals
def test_refusals_change_nothing():
    """Every refused call sits inside a batch that is then completed and run for two frames; codes, taps and
    positions equal, byte for byte, those of the same batch without the refused calls."""
    from csm_mlx import cache_context
    from csm_mlx.generation import FrameCache
    args, w, model = build_model(eos_weights("tiny"), "float32", max_batch=3)
    whole = [long_prompt(args, 1300 + i, L) for i, L in enumerate((78, 30, 21))]
    prefix = cache_context(model, cut(whole[0], 0, 65))
    gone = cache_context(model, cut(whole[1], 0, 10))
    gone_handle = gone.handle
    gone.free()
    ARG, STATE = lib().CSM_ERR_ARG, lib().CSM_ERR_STATE

    def run(refusals):
        cache = FrameCache(model, 3, greedy(), [0] * 3)
        if refusals:
            assert rc_save(model, 0, 1)[0] == STATE                        # a save from an empty slot
            assert rc_load(model, [0, 0], [prefix.handle] * 2) == ARG      # a repeated slot
            assert rc_load(model, [0, 1], [prefix.handle, gone_handle]) == ARG      # a freed handle
            with pytest.raises(RuntimeError, match="freed"):
                cache.load_prefix([(1, gone)])
        cache.prefill(1, *whole[1])
        if refusals:
            assert rc_load(model, [0, 1], [prefix.handle] * 2) == STATE    # slot 1 already holds rows
            assert rc_save(model, 1, 31)[0] == ARG                         # more rows than the source holds
            assert rc_save(model, 1, 0)[0] == ARG
        cache.load_prefix([(0, prefix)])
        cache.prefill(2, *whole[2])
        if refusals:
            assert rc_run(model) == STATE                                  # slot 0: a load, no suffix yet
            assert b"csm_prefill not called" in lib().lib().csm_last_error()
        cache.prefill(0, *cut(whole[0], 65))
        cache.run(2)
        synchronize(model)
        return state_of(model, cache, 3)
    clean = run(False)
    assert run(True) == clean
    hist = np.frombuffer(clean[0], np.int32).reshape(2, 3, args.n_audio_codebooks)
    o = oracle_for(args, w)
    for b in range(3):
        want = o.generate_codes(*whole[b], 2)
        assert np.array_equal(hist[: len(want), b], want), b
    del model


@pytest.mark.parametrize("change", ["load_tensor", "quantize"])
def test_stale_prefix_is_refused(change):
    from csm_mlx import cache_context, nn
    from csm_mlx.generation import FrameCache
    args, w, model = build_model(eos_weights("tiny"), "bf16", max_batch=2)
    whole = long_prompt(args, 1400, 40)
    prefix = cache_context(model, cut(whole, 0, 30))
    if change == "load_tensor":
        name = "backbone.layers.0.self_attn.q_proj.weight"
        model.load_weights({name: w[name]}, strict=False)                  # the same values: only the epoch moves
    else:
        nn.quantize(model, 64, 4)
    cache = FrameCache(model, 2, greedy(), [0, 0])
    assert rc_load(model, [0], [prefix.handle]) == lib().CSM_ERR_STATE
    assert b"stale" in lib().lib().csm_last_error()
    with pytest.raises(lib().CsmHipError, match="stale"):
        cache.load_prefix([(1, prefix)])
    rows, nbytes = ctypes.c_int(0), ctypes.c_int64(0)
    lib().check(lib().lib().csm_prefix_info(model.engine, prefix.handle, ctypes.byref(rows), ctypes.byref(nbytes)))
    assert rows.value == 30 and nbytes.value == prefix.nbytes              # info still answers
    cache.prefill(0, *whole)                                               # the slots are as they were: empty
    cache.prefill(1, *whole)
    cache.run(2)
    synchronize(model)
    after_refusal = state_of(model, cache, 2)
    cache = FrameCache(model, 2, greedy(), [0, 0])                         # the same batch without the refused calls
    cache.prefill(0, *whole)
    cache.prefill(1, *whole)
    cache.run(2)
    synchronize(model)
    assert state_of(model, cache, 2) == after_refusal
    hist, n, _ = cache.codes()
    if change == "load_tensor":                                            # (the same values: the bf16 oracle still holds)
        want = oracle_for(args, w, bf16=True).generate_codes(*whole, 2)
    else:                      # in-place int4 of bf16 weights has no oracle here: the engine's own whole-prompt codes
        want = hist[: n[0], 0].copy()
    assert_exact([hist[: n[b], b] for b in range(2)], [want, want], f"after {change}:")
    prefix.free()                                                          # and free still frees
    assert lib().lib().csm_prefix_info(model.engine, prefix.handle, None, None) == lib().CSM_ERR_ARG
    fresh = cache_context(model, cut(whole, 0, 30))                        # a prefix of the new weights loads
    cache = FrameCache(model, 2, greedy(), [0, 0])
    cache.load_prefix([(0, fresh)])
    cache.prefill(0, *cut(whole, 30))
    cache.prefill(1, *whole)
    cache.run(2)
    hist, n, _ = cache.codes()
    assert_exact([hist[: n[b], b] for b in range(2)], [want, want], f"fresh prefix after {change}:")
    del model
