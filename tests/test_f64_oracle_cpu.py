"""The float64 evaluation of the oracle (OracleCSM dtype=np.float64, frame(forced=...)) and the bar the GPU
taps are held to (tests/test_f64_taps_gpu.py).

Unit: max over the vocabulary (over D for h_last) of |value - float64| / the row's largest |float64 value|.
e32 = the float32 oracle's error in that unit, forced on the float64 oracle's codes, maximum over rows,
codebook steps and frames, per tap (h_last, c0, ci).  bar = helpers.BAR_MARGIN (2) x e32.

What makes the bar mean something (test_degraded_oracle_is_detectable): a float32 oracle whose
projections see only the hi + mid parts of their activations (16 significant bits: the matrix-core paths'
hi + mid + lo split, csrc/xs.h split3, with lo lost) must miss the bar by 2x at least, on EVERY row,
step and frame of every tap behind the degraded stack -- degraded everywhere, and in one projection kind
of one stack at a time.  Both matmul inputs are cut; bf16 values and dequantized int4 weights have at most 16
significant bits, so there only the activations change (fp32 weights lose bits too: the tiny fp32 figures are
about twice the others).  The smallest figure, in units of e32 (2 frames, minimum over rows / steps / frames):
tiny bf16 4.8 and tiny q4 5.2 (the backbone's down_proj seen from ci), 5.3 / 6.1 for the decoder's down_proj;
all projections: 18-42 (tiny), 9.1-19 (csm_1b).  That is why the margin is 2 and not 4 (helpers.BAR_MARGIN).
Nothing here is a constant: e32 and the degraded errors are computed each run."""
import contextlib

import numpy as np
import pytest

from helpers import (BAR_MARGIN, csm_weights, cut16, f64_reference, oracle_batch, oracle_for, oracle_taps, prompt_ids,
                     tap_errors, tiny_prompt_ids)

FRAMES = 2
MODELS = [pytest.param("tiny", v, id=f"tiny-{v}") for v in ("fp32", "bf16", "q4")] + \
         [pytest.param("1b", v, id=f"1b-{v}", marks=pytest.mark.slow) for v in ("bf16", "q4")]
KINDS = {"qkv": ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), "o": ("self_attn.o_proj",),
         "gate_up": ("mlp.gate_proj", "mlp.up_proj"), "down": ("mlp.down_proj",)}
BEHIND = {"backbone": ("h_last", "c0", "ci"), "decoder": ("ci",), "all": ("h_last", "c0", "ci")}


def _prompts(key, args):
    from csm_mlx.tokenizers import tokenize_text_segment
    K = args.n_audio_codebooks
    if key == "tiny":
        return [tokenize_text_segment(tiny_prompt_ids(40 + b, 5 + b % 3), 0, K) for b in range(3)]
    return [tokenize_text_segment(prompt_ids(40 + b, 10 + b), 0, K) for b in range(2)]     # 12 and 13 rows


_CASES = {}


def _case(key, variant):
    """(args, w, prompts, the float64 oracle's own greedy codes (F, B, K), its free-run logits)."""
    if (key, variant) not in _CASES:
        args, w = csm_weights(key)
        prompts = _prompts(key, args)
        o64 = oracle_for(args, w, bf16=variant == "bf16", q4=variant == "q4", f64=True)
        free = oracle_batch(o64, prompts, FRAMES, collect_logits=True)
        o64.drop_upcasts()
        codes = np.stack([c for c, _ in free], 1)
        assert codes.shape == (FRAMES, len(prompts), args.n_audio_codebooks)
        _CASES[key, variant] = (args, w, prompts, codes, [logs for _, logs in free])
    return _CASES[key, variant]


_REFS = {}


def _reference(key, variant):
    """(float64 taps, e32) of the case, computed once and left unchanged."""
    if (key, variant) not in _REFS:
        args, w, prompts, codes, _ = _case(key, variant)
        _REFS[key, variant] = f64_reference(args, w, variant, prompts, codes)
    return _REFS[key, variant]


@pytest.mark.parametrize("key,variant", MODELS)
def test_f64_forced_on_own_codes_equals_free_run(key, variant):
    args, w, prompts, codes, free_logs = _case(key, variant)
    o64 = oracle_for(args, w, bf16=variant == "bf16", q4=variant == "q4", f64=True)
    h, c0, ci = oracle_taps(o64, prompts, codes)
    assert h.dtype == c0.dtype == ci.dtype == np.float64
    for b, logs in enumerate(free_logs):
        for f, (c0f, cif) in enumerate(logs):
            assert c0f.dtype == np.float64
            assert np.array_equal(c0[f, b], c0f) and np.array_equal(ci[f, b], cif), (b, f)
            # greedy = first-index arg-max of the float64 logits themselves
            assert codes[f, b, 0] == np.argmax(c0f) and np.array_equal(codes[f, b, 1:], np.argmax(cif, -1))


@pytest.mark.parametrize("key,variant", MODELS)
def test_float32_oracle_error_e32(key, variant, capsys):
    """e32 per tap: the float32 oracle forced on the float64 oracle's codes, against float64.  It is a few
    float32 roundings (2^-24 = 6e-8) deep; were it to reach 2^-17, the mean size of the 16-bit cut itself, no
    multiple of it could separate a healthy path from a degraded one."""
    _, e32 = _reference(key, variant)
    with capsys.disabled():
        print(f"\n{key} {variant}: e32 " + " ".join(f"{t}={e32[t]:.2e}" for t in e32))
    assert set(e32) == {"h_last", "c0", "ci"}
    assert all(2.0 ** -24 < v < 2.0 ** -17 for v in e32.values()), e32


def test_f64_q4_starts_from_the_stored_triple():
    """The float64 int4 weight is scale*q + bias evaluated in float64 from (packed, scales, biases), not the
    float32 dequantize result converted; the float32 one is the float64 one rounded once."""
    from oracle.quant_oracle import QuantMatrix, affine_quantize, dequantize, unpack
    w = np.random.default_rng(0).standard_normal((24, 256)).astype(np.float32)
    p, s, b = affine_quantize(w)
    d64 = dequantize(p, s, b, dtype=np.float64)
    exact = np.repeat(s.astype(np.float64), 64, 1) * unpack(p) + np.repeat(b.astype(np.float64), 64, 1)
    assert d64.dtype == np.float64 and np.array_equal(d64, exact)
    d32 = dequantize(p, s, b)
    assert d32.dtype == np.float32 and np.array_equal(d32, d64.astype(np.float32))    # scale * q is exact
    qm = QuantMatrix(p, s, b)
    idx = np.array([[3, 0], [23, 3]])
    assert np.array_equal(qm.rows(idx, np.float64), d64[idx]) and np.array_equal(qm.dense(), d32)
    args, wt = csm_weights("tiny")
    o64 = oracle_for(args, wt, q4=True, f64=True)
    assert isinstance(o64.w["backbone.layers.0.mlp.down_proj.weight"], QuantMatrix)
    assert o64.w["audio_head"].dtype == np.float32                      # not quantized; converted where used


@contextlib.contextmanager
def _degraded(monkeypatch, o, select):
    """oracle.csm_oracle.linear with its activations cut to 16 significant bits for the stored matrices whose
    name ``select`` accepts."""
    import oracle.csm_oracle as co
    ids = {id(v) for k, v in o.w.items() if select(k)}
    plain = co.linear
    cut_w = {}            # bf16 values and dequantized int4 weights have <= 16 significant bits: cut once, keep
                          # the matrix itself where the cut changes nothing

    def linear(x, w):
        if id(w) not in ids:
            return plain(x, w)
        if id(w) not in cut_w:
            c = cut16(w)
            cut_w[id(w)] = w if np.array_equal(c, w) else c
        return plain(cut16(x), cut_w[id(w)])
    with monkeypatch.context() as m:
        m.setattr(co, "linear", linear)
        yield len(ids)


def _selectors(form):
    if form == "all":
        return {"all": lambda n: n != "audio_head"}
    sel = {}
    for stack in ("backbone", "decoder"):
        for kind, names in KINDS.items():
            sel[f"{stack}:{kind}"] = (lambda n, s=stack, nm=names: n.startswith(s + ".layers.")
                                      and any(n.endswith(x + ".weight") for x in nm))
    return sel


# one projection kind at a time on tiny, where a run takes a fraction of a second (the same code runs the
# projection in every layer of csm_1b)
DEGRADED = [pytest.param(*p.values, "all", id=p.id + "-all", marks=p.marks) for p in MODELS] + \
           [pytest.param(*p.values, "kinds", id=p.id + "-kinds") for p in MODELS if p.values[0] == "tiny"]


@pytest.mark.parametrize("key,variant,form", DEGRADED)
def test_degraded_oracle_is_detectable(key, variant, form, monkeypatch, capsys):
    args, w, prompts, codes, _ = _case(key, variant)
    t64, e32 = _reference(key, variant)
    o32 = oracle_for(args, w, bf16=variant == "bf16", q4=variant == "q4")
    bad, lines = [], [f"{key} {variant}: e32 " + " ".join(f"{t}={e32[t]:.2e}" for t in e32)]
    for tag, select in _selectors(form).items():
        with _degraded(monkeypatch, o32, select) as n:
            assert n > 0, tag
            err = tap_errors(oracle_taps(o32, prompts, codes), t64)
        for tap in BEHIND[tag.split(":")[0]]:
            worst = float(err[tap].min())                    # the row / step / frame that shows the least
            lines.append(f"  {tag:18s} {tap:6s} min {worst:.2e} = {worst / e32[tap]:6.1f} x e32")
            if not worst >= 2 * BAR_MARGIN * e32[tap]:
                bad.append(lines[-1])
    # the undegraded oracle is back, bit for bit
    again = tap_errors(oracle_taps(o32, prompts, codes), t64)
    assert all(float(again[t].max()) == e32[t] for t in e32)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not bad, f"bar = {BAR_MARGIN} x e32 is over half of a degraded error:\n" + "\n".join(bad)
