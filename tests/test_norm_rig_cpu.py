"""What the bars of tests/test_norm_rig_gpu.py and the rigged cases of tests/test_mimi_f64_gpu.py mean: on the
rigged weights (helpers.norm_rig, helpers.mimi_affine_rig) a single wrong norm operand misses the bar.  The
oracles only; nothing here comes from the engine.

CSM (tiny; fp32 / bf16 / q4; the float32 oracle's own two frames on three prompts).  Each defect is applied to
the float32 oracle's weights, one tensor at a time, and its taps are held against the float64 reference of the
TRUE rigged weights, in the unit of tests/test_f64_taps_gpu.py.  It must miss 2 x helpers.BAR_MARGIN x e32 on at
least one tap behind the tensor (the "2 x bar" rule of tests/test_f64_oracle_cpu.py):
  * a norm tensor replaced by ones (a norm weight not applied);
  * n1[l] <-> n2[l];  n1[l] <-> n1[l + 1];  the last layer's n2 <-> the stack's final norm (the wrong layer);
  * a norm tensor rolled by 8 elements (the wrong offset).
The int4 split "s sum(q nw x) + b sum(x)" -- half-group sums taken of x, not of x * nw -- is restated for one
projection from its quant triple, in the unit of helpers.linear_f64_bar.
The rig may not cost the bar its meaning: e32 on the rigged weights is at most 4 x e32 on the all-ones weights.

Mimi (tiny, both attention modes; helpers.mimi_errors' unit, bar = helpers.MIMI_BAR_MARGIN x e32): norm1 <->
norm2 weights, one bias zeroed, layer_scale_1 <-> layer_scale_2 (decoder: rows and pcm of the decode case;
encoder: the latent rows of the encode clip), cluster usage ignored, and the clamp at 1e-6 instead of 1e-5 on
codes that hold the two clamped bins of every codebook.
Nothing is a constant: e32 and every defect's figure are computed each run and printed."""
import numpy as np
import pytest

from helpers import (BAR_MARGIN, MIMI_BAR_MARGIN, _quant_for, csm_weights, f64_reference, is_norm, linear_err,
                     linear_f64_bar, mimi_affine_rig, mimi_clamped_bins, mimi_errors, mimi_pair, mimi_pcm_clip,
                     mimi_place_clamped, norm_weights, oracle_batch, oracle_for, oracle_taps, tap_errors, tiny_prompt_ids)

FRAMES = 2
VARIANTS = ["fp32", "bf16", "q4"]
TAPS_BEHIND = {"backbone": ("h_last", "c0", "ci"), "decoder": ("ci",)}


def _kw(variant):
    return dict(bf16=variant == "bf16", q4=variant == "q4")


def _prompts(args):
    from csm_mlx.tokenizers import tokenize_text_segment
    return [tokenize_text_segment(tiny_prompt_ids(40 + b, 5 + b % 3), 0, args.n_audio_codebooks) for b in range(3)]


_CASES = {}


def _case(variant, rigged=True):
    """(args, w, prompts, the float32 oracle's own greedy codes (F, B, K), float64 taps, e32), computed once."""
    if (variant, rigged) not in _CASES:
        args, w = norm_weights("tiny") if rigged else csm_weights("tiny")
        prompts = _prompts(args)
        free = oracle_batch(oracle_for(args, w, **_kw(variant)), prompts, FRAMES)
        assert all(c.shape == (FRAMES, args.n_audio_codebooks) for c, _ in free), "an utterance ended inside the window"
        codes = np.stack([c for c, _ in free], 1)
        t64, e32 = f64_reference(args, w, variant, prompts, codes)
        _CASES[variant, rigged] = (args, w, prompts, codes, t64, e32)
    return _CASES[variant, rigged]


def _norm_names(w, stack):
    return sorted(n for n in w if is_norm(n) and n.startswith(stack + "."))


def _defects(args, w):
    """{label: (stack, {name: replacement})} -- every single-tensor defect of the module docstring."""
    from csm_mlx.config import BACKBONE_CONFIGURATION as BB, DECODER_CONFIGURATION as DC
    out = {}
    for stack, L in (("backbone", BB[args.backbone_name].num_hidden_layers),
                     ("decoder", DC[args.decoder_name].num_hidden_layers)):
        n1 = [f"{stack}.layers.{l}.input_layernorm.weight" for l in range(L)]
        n2 = [f"{stack}.layers.{l}.post_attention_layernorm.weight" for l in range(L)]
        fin = f"{stack}.norm.weight"
        assert sorted(n1 + n2 + [fin]) == _norm_names(w, stack)
        for n in n1 + n2 + [fin]:
            out[f"ones {n}"] = (stack, {n: np.ones_like(w[n])})
            out[f"roll8 {n}"] = (stack, {n: np.roll(w[n], 8)})
        swaps = [(n1[l], n2[l]) for l in range(L)] + [(n1[l], n1[l + 1]) for l in range(L - 1)] + [(n2[L - 1], fin)]
        for a, b in swaps:
            out[f"swap {a} <-> {b}"] = (stack, {a: w[b], b: w[a]})
    return out


@pytest.mark.parametrize("variant", VARIANTS)
def test_rig_leaves_the_window_alive_and_e32_in_place(variant, capsys):
    """No utterance ends and no code is 0 within the window; e32 on the rigged weights is within 4 x of e32 on the
    all-ones weights, per tap (measured: 1.6-2.9 x), and still a few float32 roundings deep."""
    args, w, prompts, codes, _, e32 = _case(variant)
    assert codes.shape == (FRAMES, 3, args.n_audio_codebooks) and (codes != 0).all(), "a code is 0 inside the window"
    _, _, _, _, _, ones = _case(variant, rigged=False)
    with capsys.disabled():
        print(f"\nnorm-rig tiny {variant}: e32 " + " ".join(f"{t}={e32[t]:.2e}({e32[t] / ones[t]:.2f}x ones {ones[t]:.2e})"
                                                            for t in e32))
    assert all(e32[t] <= 4 * ones[t] for t in e32), (e32, ones)
    assert all(2.0 ** -24 < v < 2.0 ** -17 for v in e32.values()), e32


def test_rig_draws():
    """Every norm tensor has its own draw: 2^U(-2, 2) magnitudes, some negative, no two tensors alike; every other
    tensor is the base dict's own array; the rig is memoised (oracle_for's id cache depends on it)."""
    args, w = norm_weights("tiny")
    _, base = csm_weights("tiny")
    assert norm_weights("tiny")[1] is w
    names = [n for n in w if is_norm(n)]
    assert len(names) == 10
    for n in w:
        if not is_norm(n):
            assert w[n] is base[n], n
            continue
        a = w[n]
        assert a.dtype == np.float32 and a.shape == base[n].shape and (base[n] == 1).all()
        assert 0.25 <= np.abs(a).min() and np.abs(a).max() <= 4 and 0.02 < (a < 0).mean() < 0.25, n
    assert all(not np.array_equal(w[a], w[b]) for i, a in enumerate(names) for b in names[:i])


def test_bf16_oracle_keeps_norm_weights_as_given():
    """The engine's rule: RMSNorm weights are stored fp32 exactly as given.  The bf16 oracle variant
    rounds every tensor but those; an oracle on a dict rounded beforehand (what a bf16 checkpoint holds) has
    bf16-exact norms either way."""
    from csm_mlx.weights import bf16_round
    args, w = norm_weights("tiny")
    o = oracle_for(args, w, bf16=True)
    for n, v in o.w.items():
        if is_norm(n):
            assert np.array_equal(v, w[n]) and not np.array_equal(v, bf16_round(v)), n
        else:
            assert np.array_equal(v, bf16_round(v)), n
    assert np.array_equal(o.w["projection.weight"], oracle_for(args, csm_weights("tiny")[1], bf16=True).w["projection.weight"])


@pytest.mark.parametrize("variant", VARIANTS)
def test_wrong_norm_is_detectable(variant, capsys):
    from oracle.csm_oracle import OracleCSM
    from csm_mlx.config import BACKBONE_CONFIGURATION as BB, DECODER_CONFIGURATION as DC
    args, w, prompts, codes, t64, e32 = _case(variant)
    o32 = oracle_for(args, w, **_kw(variant))
    cfg = (BB[args.backbone_name], DC[args.decoder_name])
    bad, lines, least = [], [], {}
    for label, (stack, repl) in _defects(args, w).items():
        wd = dict(o32.w)
        assert all(np.array_equal(wd[n], w[n]) for n in repl)          # every variant holds the norms as given
        wd.update(repl)
        err = tap_errors(oracle_taps(OracleCSM(args, wd, *cfg), prompts, codes), t64)
        ratio = max(float(err[t].max()) / e32[t] for t in TAPS_BEHIND[stack])
        kind = label.split()[0]
        least[kind] = min(least.get(kind, np.inf), ratio)
        lines.append(f"  {label}: {ratio:.3g} x e32")
        if not ratio >= 2 * BAR_MARGIN:
            bad.append(lines[-1])
    with capsys.disabled():
        print(f"\nnorm-rig tiny {variant}: smallest defect over all norm tensors, in e32: "
              + " ".join(f"{k}={v:.3g}" for k, v in least.items()))
    assert not bad, f"bar = {BAR_MARGIN} x e32 is over half of a wrong norm's error:\n" + "\n".join(bad)


def test_q4_half_group_sums_before_the_norm_weight(capsys):
    """The int4 kernels split y = sum (s q + b) nw x per group of 64 into s sum(q nw x) + b sum(nw x).  Taking
    the half-group sums of x instead of nw x is invisible when nw = 1.  One projection (the backbone's layer-0
    q_proj), restated from its quant triple, in helpers.linear_f64_bar's unit: the defect misses 2 x the bar."""
    from oracle.quant_oracle import unpack
    args, w = norm_weights("tiny")
    name = "backbone.layers.0.self_attn.q_proj.weight"
    qm = _quant_for(w)[name]
    packed, scales, biases = qm.packed, qm.scales, qm.biases
    q = unpack(packed).astype(np.float64)
    N, K = q.shape
    G = K // scales.shape[1]
    assert G == 64
    nw = w["backbone.layers.0.input_layernorm.weight"]
    x = np.random.default_rng(11).standard_normal((5, K)).astype(np.float32)
    xn = (x * nw).astype(np.float32)
    wd = (np.repeat(scales.astype(np.float64), G, 1) * q + np.repeat(biases.astype(np.float64), G, 1)).astype(np.float32)
    y64, S, bar, _ = linear_f64_bar(xn, wd, n_cols=N)
    s64, b64 = scales.astype(np.float64), biases.astype(np.float64)
    qx = np.einsum("ngk,mgk->mng", q.reshape(N, -1, G), xn.astype(np.float64).reshape(5, -1, G))
    right = (s64[None] * qx + b64[None] * xn.astype(np.float64).reshape(5, 1, -1, G).sum(-1)).sum(-1)
    wrong = (s64[None] * qx + b64[None] * x.astype(np.float64).reshape(5, 1, -1, G).sum(-1)).sum(-1)
    e_right, e_wrong = float(linear_err(right, y64, S)), float(linear_err(wrong, y64, S))
    with capsys.disabled():
        print(f"\nnorm-rig q4 half-group sums of x: {e_wrong:.2e} = {e_wrong / bar:.3g} x bar {bar:.2e} (the split itself {e_right:.1e})")
    assert e_right <= bar and e_wrong >= 2 * bar


def test_rms_norm_is_torch_rms_norm():
    """oracle.csm_oracle.rms_norm against torch.nn.functional.rms_norm, float64, on a rigged weight row."""
    import torch
    from oracle.csm_oracle import rms_norm
    _, w = norm_weights("tiny")
    nw = w["backbone.layers.1.post_attention_layernorm.weight"].astype(np.float64)
    x = np.random.default_rng(3).standard_normal((7, nw.shape[0])) * 3
    ref = torch.nn.functional.rms_norm(torch.from_numpy(x), (nw.shape[0],), torch.from_numpy(nw), 1e-5).numpy()
    got = rms_norm(x, nw, 1e-5)
    assert got.dtype == np.float64
    np.testing.assert_allclose(got, ref, rtol=1e-13, atol=0)


# ----------------------------------------------------------------------------- Mimi
MODES = ["mlx", "causal"]


def mimi_rig_codes(m):
    """The decode case's codes (tests/test_mimi_f64_gpu.py), the two clamped bins placed in every codebook."""
    codes = np.random.default_rng(5).integers(0, m.bins, (2, m.n_q, 12)).astype(np.int32)
    return mimi_place_clamped(m, codes)


def _clip():
    return np.stack([mimi_pcm_clip(24000 * 2 + 480, 1), mimi_pcm_clip(24000 * 2 + 480, 2)])[:, None, :]


def _mimi_run(o, codes, pcm):
    out = {"pcm": o.decode(codes)}
    out["rows"] = o.taps["rows"]
    if pcm is not None:
        out["codes"] = o.encode(pcm)
        out["enc_rows"] = o.taps["rows"]
    return out


def _mimi_figs(got, r64, fs):
    return {"pcm": mimi_errors(got["pcm"], r64["pcm"], fs), "rows": mimi_errors(got["rows"], r64["rows"]),
            **({"enc_rows": mimi_errors(got["enc_rows"], r64["enc_rows"])} if "enc_rows" in got else {})}


@pytest.mark.parametrize("mode", MODES)
def test_mimi_rig_defects_miss_the_bar(mode, capsys):
    from csm_mlx.weights import mimi_codebook
    from oracle.mimi_oracle import OracleMimi
    m, w, o32, o64 = mimi_pair("tiny", mode, rig=mimi_affine_rig)
    _, _, p32, p64 = mimi_pair("tiny", mode)
    codes, pcm = mimi_rig_codes(m), _clip()
    for k in range(m.n_q):
        lo = mimi_clamped_bins(m, "rvq_first" if k == 0 else "rvq_rest", max(k - 1, 0))
        assert set(lo) <= set(codes[:, k].reshape(-1).tolist()), k
    r64, r32 = _mimi_run(o64, codes, pcm), _mimi_run(o32, codes, pcm)
    e32 = {t: float(e.max()) for t, e in _mimi_figs(r32, r64, m.frame_size).items()}
    ones = {t: float(e.max()) for t, e in _mimi_figs(_mimi_run(p32, codes, pcm), _mimi_run(p64, codes, pcm),
                                                     m.frame_size).items()}
    assert all(e32[t] <= 4 * ones[t] for t in e32), (e32, ones)
    # the references alone need no near-tie exception on this clip
    assert np.array_equal(r32["codes"], r64["codes"]), np.argwhere(r32["codes"] != r64["codes"])[:4].tolist()

    def swapped(a, b):
        return {a: w[b], b: w[a]}
    dec, enc = "decoder_transformer.transformer.layers.1", "encoder_transformer.transformer.layers.0"
    defects = {}
    for side, p in (("decoder", dec), ("encoder", enc)):
        defects[f"{side} norm1 <-> norm2"] = swapped(f"{p}.norm1.weight", f"{p}.norm2.weight")
        defects[f"{side} norm2.bias zeroed"] = {f"{p}.norm2.bias": np.zeros_like(w[f"{p}.norm2.bias"])}
        defects[f"{side} ls1 <-> ls2"] = swapped(f"{p}.layer_scale_1.scale", f"{p}.layer_scale_2.scale")
    defects["decoder usage ignored"] = {n: np.ones_like(v) for n, v in w.items() if n.endswith(".cluster_usage")}
    lines = [f"mimi-rig tiny-{mode}: e32 " + " ".join(f"{t}={e32[t]:.2e}({e32[t] / ones[t]:.2f}x ones)" for t in e32)]
    bad = []

    def hold(what, got, taps):
        figs = _mimi_figs(got, r64, m.frame_size)
        ratio = max(float(figs[t].max()) / e32[t] for t in taps)
        lines.append(f"  {what}: {ratio:.3g} x e32")
        if not ratio >= 2 * MIMI_BAR_MARGIN:
            bad.append(lines[-1])
    for what, repl in defects.items():
        od = OracleMimi(m, {**w, **repl})
        if what.startswith("decoder"):
            hold(what, _mimi_run(od, codes, None), ("pcm", "rows"))
        else:
            od.encode(pcm)
            hold(what, {"pcm": r32["pcm"], "rows": r32["rows"], "enc_rows": od.taps["rows"]}, ("enc_rows",))
    od = OracleMimi(m, w)
    od.cb_first = [mimi_codebook(od.w, "rvq_first", 0, eps=1e-6)]
    od.cb_rest = [mimi_codebook(od.w, "rvq_rest", k, eps=1e-6) for k in range(m.n_q - 1)]
    hold("decoder clamp 1e-6", _mimi_run(od, codes, None), ("pcm", "rows"))
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not bad, f"bar = {MIMI_BAR_MARGIN} x e32 is over half of a defect's error:\n" + "\n".join(bad)


def test_mimi_rig_draws():
    from csm_mlx.weights import mimi_codebook
    m, w, _, _ = mimi_pair("tiny", "mlx", rig=mimi_affine_rig)
    _, base, _, _ = mimi_pair("tiny", "mlx")
    p = "decoder_transformer.transformer.layers.0"
    assert not np.array_equal(w[f"{p}.norm1.weight"], w[f"{p}.norm2.weight"]) and (w[f"{p}.norm1.weight"] < 0).any()
    assert not np.array_equal(w[f"{p}.layer_scale_1.scale"], w[f"{p}.layer_scale_2.scale"])
    assert np.abs(w[f"{p}.norm1.bias"]).max() > 0.5
    for q, k in (("rvq_first", 0), ("rvq_rest", 2)):
        u = w[f"quantizer.{q}.vq.layers.{k}._codebook.cluster_usage"]
        lo = mimi_clamped_bins(m, q, k)
        assert u[lo[0]] == 0 and u[lo[1]] == np.float32(1e-6) and (np.delete(u, lo) >= 0.25).all()
        eff, plain = mimi_codebook(w, q, k), mimi_codebook(base, q, k)
        np.testing.assert_allclose(eff, plain, rtol=1e-6)               # the effective rows keep their scale
        assert np.abs(mimi_codebook(w, q, k, eps=1e-6)[lo]).max() > 5 * np.abs(eff[lo]).max()
