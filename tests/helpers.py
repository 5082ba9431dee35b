"""Shared builders for the parity tests (test infrastructure)."""
import dataclasses
import functools
import zlib

import numpy as np

from csm_mlx.config import BACKBONE_CONFIGURATION as BB, DECODER_CONFIGURATION as DC
from csm_mlx.weights import bf16_round, synthetic_csm_weights


@functools.lru_cache(maxsize=4)
def csm_weights(args_key, seed=0):
    from csm_mlx.models import csm_1b, csm_tiny
    args = {"tiny": csm_tiny, "1b": csm_1b}[args_key]()
    return args, synthetic_csm_weights(args, seed)


_ORACLES = {}


def oracle_for(args, weights, bf16=False, q4=False, f64=False):
    """bf16: every weight rounded to bf16 (CSM dtype "bf16").  q4: nn.quantize'd CSM (dtype "q4"):
    Linear / Embedding weights quantize->dequantize (oracle/quant_oracle.py), audio_head bf16.
    f64: the float64 evaluation (OracleCSM dtype=np.float64) of the same stored parameters: it shares the
    float32 oracle's arrays (bf16 / fp32) or starts from the int4 triples (q4), never a float64 model.
    Memoised per weight dict (the csm_weights dicts are cached): the csm_1b bf16 / int4 conversions
    take 10-45 s each (6 GB of fp32 per variant)."""
    key = (id(weights), bool(bf16), bool(q4), bool(f64))
    if key not in _ORACLES:
        _ORACLES[key] = _oracle_for(args, weights, bf16, q4, f64)
    return _ORACLES[key]


_QUANT = {}


def _quant_for(weights):
    from oracle.quant_oracle import quantize_weights
    weights = _RIG_BASE.get(id(weights), weights)                    # a norm rig quantizes nothing anew
    if id(weights) not in _QUANT:
        _QUANT[id(weights)] = quantize_weights(weights)
    return _QUANT[id(weights)]


def _oracle_for(args, weights, bf16, q4, f64=False):
    from oracle.csm_oracle import OracleCSM
    from oracle.quant_oracle import quantize_dequantize_weights
    cfg = (BB[args.backbone_name], DC[args.decoder_name])
    if f64:
        w = dict(oracle_for(args, weights, bf16, q4).w)              # the float32 oracle's own arrays
        if q4:
            w.update(_quant_for(weights))                            # (packed, scales, biases): exact in float64
        return OracleCSM(args, w, *cfg, dtype=np.float64)
    base = _RIG_BASE.get(id(weights))
    if base is not None:                                             # norm_rig: the base dict's conversions, its own norms
        w = dict(oracle_for(args, base, bf16, q4).w)
        w.update({k: v for k, v in weights.items() if is_norm(k)})
        return OracleCSM(args, w, *cfg)
    # the engine keeps RMSNorm weights as given (fp32 in, fp32 kept: DESIGN.md "RMSNorm weights fp32"), so the
    # bf16 variant rounds every tensor but those
    w = {k: v if is_norm(k) else bf16_round(v) for k, v in weights.items()} if bf16 else weights
    if q4:
        w = quantize_dequantize_weights(weights, quant=_quant_for(weights))
        w["audio_head"] = bf16_round(weights["audio_head"])
    return OracleCSM(args, w, *cfg)


def oracle_taps(o, prompts, codes, block=None):
    """Teacher-forced taps of oracle ``o`` (either precision): prompts (tokens, mask) of any lengths, codes
    (F, B, K) forced per frame.  Returns h_last (F, B, D), c0_logits (F, B, V), ci_logits (F, B, K-1, V)
    in the oracle's precision.  Utterances of equal prompt length run as one batch.
    block: a prompt of more rows reaches the backbone in pieces of ``block`` rows (the KV cache appends; the
    last piece, of 1..block rows, is the first frame's), so the (heads, T, S) score temporaries of a long prompt
    stay small: the same arithmetic up to the matrix products' blocking (tests/test_f64_long_cpu.py)."""
    codes = np.asarray(codes)
    F, B, K = codes.shape
    assert B == len(prompts)
    groups = {}
    for i, (t, _) in enumerate(prompts):
        groups.setdefault(t.shape[0], []).append(i)
    out = None
    for idx in groups.values():
        toks = np.stack([prompts[i][0] for i in idx]).astype(np.int64)
        msk = np.stack([prompts[i][1] for i in idx]).astype(bool)
        cache = o.new_backbone_cache()
        if block is not None and toks.shape[1] > block:
            ahead = (toks.shape[1] - 1) // block * block
            for r in range(0, ahead, block):
                o.backbone(o.embed_rows(toks[:, r:r + block], msk[:, r:r + block]), cache)
            toks, msk = toks[:, ahead:], msk[:, ahead:]
        for f in range(F):
            s = o.frame(toks, msk, cache, forced=codes[f, idx])
            taps = [o.debug["h_last"], o.debug["c0_logits"], o.debug["ci_logits"]]
            if out is None:
                out = [np.zeros((F, B) + t.shape[1:], t.dtype) for t in taps]
            for dst, t in zip(out, taps):
                dst[f, idx] = t
            toks = np.concatenate([s, np.zeros((len(idx), 1), np.int32)], 1)[:, None, :].astype(np.int64)
            msk = np.concatenate([np.ones_like(s, bool), np.zeros((len(idx), 1), bool)], 1)[:, None, :]
    if hasattr(o, "drop_upcasts"):
        o.drop_upcasts()
    return tuple(out)


def prompt_ids(seed: int, n_mid: int = 12, vocab: int = 128000, bos: int = 128000, eos: int = 128001):
    """SURVEY 8(d) prompt recipe: BOS + n ids ~ U[0, vocab) + EOS."""
    rng = np.random.default_rng(seed)
    return [bos] + [int(x) for x in rng.integers(0, vocab, n_mid)] + [eos]


def b32_prompt_ids():
    """The ids of configs[3]'s 32 utterances: tests/test_batched_long_gpu.py runs them, tests/golden/make_golden.py
    computed their fixtures -- one list, so the two cannot part."""
    return [prompt_ids(1 if g == 0 else 1000 + g) for g in range(32)]


def tiny_prompt_ids(seed: int, n_mid: int = 5):
    rng = np.random.default_rng(seed)
    return [998] + [int(x) for x in rng.integers(0, 990, n_mid)] + [999]


def long_prompt(args, seed: int, rows: int):
    """A seeded prompt of exactly ``rows`` rows laid out as a context segment before the text to speak: text
    rows, then rows // 3 audio rows (codes 1 .. bins - 1 in every codebook: no row is the all-zero frame),
    then text rows.  Returns (tokens (rows, K+1) int32, mask (rows, K+1) bool)."""
    K, rng = args.n_audio_codebooks, np.random.default_rng(seed)
    n_audio = rows // 3
    a0 = (rows - n_audio) // 2
    tokens = np.zeros((rows, K + 1), np.int32)
    mask = np.zeros((rows, K + 1), bool)
    audio = np.zeros(rows, bool)
    audio[a0:a0 + n_audio] = True
    tokens[~audio, K] = rng.integers(0, args.n_text_vocab, rows - n_audio)
    mask[~audio, K] = True
    tokens[audio, :K] = rng.integers(1, args.n_audio_vocab - 3, (n_audio, K))
    mask[audio, :K] = True
    return tokens, mask


def rms(a, b):
    """Root mean square of a - b over every element (0 for empty arrays); the shapes must agree."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.sqrt(np.mean((a - b) ** 2))) if a.size else 0.0


def free_port():
    """A TCP port that was free a moment ago (the multi-process tests' rendezvous)."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def first_divergence(a: np.ndarray, b: np.ndarray):
    n = min(len(a), len(b))
    for i in range(n):
        if not np.array_equal(a[i], b[i]):
            return i
    return None if len(a) == len(b) else n


def make_adapters(model_handle, weights, fine_tune_type="lora", keys=("attn",), rank=4, scale=2.0,
                  seed=7, b_std=0.05):
    """Synthetic trained adapters for ``keys`` (mlx_lm LoRALinear naming: <module>.lora_a (in, r),
    .lora_b (r, out); LoRAEmbedding: lora_a (n, r), lora_b (r, d); DoRA adds .m).  Returns
    (adapter_config dict, flat tensors for adapters.safetensors, oracle adapters {path: dict})."""
    from csm_mlx.adapters import converted_modules
    rng = np.random.default_rng(seed)
    tensors, oracle_ad = {}, {}
    for path, kind in converted_modules(model_handle, list(keys)).items():
        w = np.asarray(weights[path + ".weight"], np.float32)
        n_in = w.shape[1] if kind == "linear" else w.shape[0]
        n_out = w.shape[0] if kind == "linear" else w.shape[1]
        bound = 1.0 / np.sqrt(n_in) if kind == "linear" else 1.0 / np.sqrt(rank)
        a = rng.uniform(-bound, bound, (n_in, rank)).astype(np.float32)
        b = (rng.standard_normal((rank, n_out)) * b_std).astype(np.float32)
        tensors[path + ".lora_a"], tensors[path + ".lora_b"] = a, b
        ad = {"a": a, "b": b, "scale": scale, "m": None}
        if fine_tune_type == "dora":
            m = (np.linalg.norm(w, axis=1) * rng.uniform(0.8, 1.2, w.shape[0])).astype(np.float32)
            tensors[path + ".m"] = m
            ad["m"] = m
        oracle_ad[path] = ad
    config = {"fine_tune_type": fine_tune_type,
              "lora_parameters": {"rank": rank, "scale": scale, "dropout": 0.0, "keys": list(keys)}}
    return config, tensors, oracle_ad


def write_adapter_dir(path, config, tensors):
    import json
    from safetensors.numpy import save_file
    path.mkdir(parents=True, exist_ok=True)
    (path / "adapter_config.json").write_text(json.dumps(config))
    save_file({k: np.ascontiguousarray(v) for k, v in tensors.items()}, str(path / "adapters.safetensors"))
    return path


def oracle_batch(o, prompts, frames, collect_logits=False, temperature=0.0, top_k=0, seeds=None, **flt):
    """Greedy oracle frames for many utterances at once: prompts (tokens, mask) of equal length run as
    one (B, L, 33) batch through OracleCSM.frame (the reference's generate_frame is batch-agnostic,
    generation.py:21-92).  Returns per utterance (codes (F_b, K), [(c0, ci) per frame] or None);
    an utterance that reaches EOS is re-run alone so its frame count follows generation.py:151.
    Sampling (temperature > 0) uses the oracle's restatement of the engine's counter-based RNG with
    one seed per utterance."""
    seeds = [0] * len(prompts) if seeds is None else list(seeds)
    groups = {}
    for i, (t, _) in enumerate(prompts):
        groups.setdefault(t.shape[0], []).append(i)
    out = [None] * len(prompts)
    for L, idx in groups.items():
        toks = np.stack([prompts[i][0] for i in idx]).astype(np.int64)
        msk = np.stack([prompts[i][1] for i in idx]).astype(bool)
        cache = o.new_backbone_cache()
        codes, logs = [], []
        for f in range(frames):
            s = o.frame(toks, msk, cache, temperature, top_k, [seeds[i] for i in idx], f, **flt)
            codes.append(s)
            if collect_logits:
                logs.append((o.debug["c0_logits"].copy(), o.debug["ci_logits"].copy()))
            toks = np.concatenate([s, np.zeros((len(idx), 1), np.int32)], 1)[:, None, :].astype(np.int64)
            msk = np.concatenate([np.ones_like(s, bool), np.zeros((len(idx), 1), bool)], 1)[:, None, :]
        codes = np.stack(codes, 1)                                    # (b, F, K)
        for j, i in enumerate(idx):
            if not codes[j].any(-1).all():                            # EOS inside the window: run alone
                res = o.generate_codes(prompts[i][0], prompts[i][1], frames, temperature, top_k, seeds[i],
                                       collect_logits=collect_logits, **flt)
                out[i] = res if collect_logits else (res, None)
            else:
                out[i] = (codes[j], [(c0[j], ci[j]) for c0, ci in logs] if collect_logits else None)
    return out


# ----------------------------------------------------------------------------- EOS-capable weights
EOS_RIG = dict(alpha=2.5, emb_norm=20.0, head_gain=0.5, seed=77)


def eos_rig(args, w, alpha=EOS_RIG["alpha"], emb_norm=EOS_RIG["emb_norm"], head_gain=EOS_RIG["head_gain"],
            seed=EOS_RIG["seed"]):
    """Seeded synthetic weights in which an utterance CAN end (test infrastructure).

    The reference stops an utterance at the first all-zero frame (generation.py:151).  With plain random
    weights all 32 codes are never 0 together, so EOS is never exercised.  The rig (documented here and
    in DESIGN.md; nothing else changes):
      * audio_embeddings row ``0 + V*j`` (code 0 of codebook j, j < K-1) = ``emb_norm`` x a seeded unit
        vector u_j -- ~20x a normal row, so when c_j = 0 the decoder's residual stream at the next step
        is dominated by projection(u_j);
      * audio_head[j][:, 0] (code 0 of codebook j+1) = ``head_gain`` x the unit direction of
        projection(u_j) -- logit 0 then leads by ~10 whenever c_j = 0: a zero code chains to the end of
        the frame (greedy and sampled alike);
      * codebook0_head row 0 scaled by ``alpha`` -- c0 = 0 (and so the all-zero frame) becomes an
        occasional event whose timing depends on the utterance.
    Returns a new dict (the input is not modified)."""
    V, K = args.n_audio_vocab, args.n_audio_codebooks
    rng = np.random.default_rng(seed)
    out = dict(w)
    emb = np.array(w["audio_embeddings.weight"], np.float32)
    ah = np.array(w["audio_head"], np.float32)
    wp = np.asarray(w["projection.weight"], np.float32)
    for j in range(K - 1):
        u = rng.standard_normal(emb.shape[1]).astype(np.float32)
        u *= emb_norm / np.linalg.norm(u)
        emb[j * V] = u
        d = wp @ u
        ah[j][:, 0] = head_gain * d / np.linalg.norm(d)
    c0 = np.array(w["codebook0_head.weight"], np.float32)
    c0[0] *= alpha
    out["audio_embeddings.weight"], out["audio_head"], out["codebook0_head.weight"] = emb, ah, c0
    return out


@functools.lru_cache(maxsize=2)
def eos_weights(args_key="1b", seed=0):
    args, w = csm_weights(args_key, seed)
    return args, eos_rig(args, w)


# ----------------------------------------------------------------------------- norms that are not all ones
def is_norm(name):
    """A CSM RMSNorm weight: input_layernorm / post_attention_layernorm of a layer, or a stack's final norm."""
    return name.endswith("norm.weight")


def _rig_rng(seed, name):
    return np.random.default_rng([seed, zlib.crc32(name.encode())])


def _pow2(rng, shape, lo, hi, negate=0.0):
    """2^U(lo, hi) per element, a fraction ``negate`` of them negated."""
    v = np.exp2(rng.uniform(lo, hi, shape))
    return (v * np.where(rng.random(shape) < negate, -1.0, 1.0)).astype(np.float32)


_RIG_BASE = {}          # id(rigged dict) -> the dict it was made from (kept alive by _NORM_RIGS)
_NORM_RIGS = {}


def norm_rig(args, w, seed=0):
    """Seeded weights whose RMSNorm weights can be told apart (test infrastructure): every norm tensor of ``w``
    (``is_norm``) gets its own draw, keyed by (seed, name): magnitude 2^U(-2, 2) per element, about 10 % of the
    elements negated.  With the synthetic all-ones norms n1[l], n1[l + 1], n2[l] and the final norm are
    interchangeable and sum(x * nw) = sum(x); with these a norm weight that is skipped, applied twice, taken
    from another layer, read at an offset or left stale moves the taps by 1e5 x the bar
    (tests/test_norm_rig_cpu.py).  Nothing else changes.  Returns a new dict, memoised per (dict, seed) so that
    ``oracle_for``'s cache holds; ``oracle_for`` reuses ``w``'s bf16 / int4 conversions for every other tensor."""
    key = (id(w), seed)
    if key not in _NORM_RIGS:
        out = dict(w)
        for name, v in w.items():
            if is_norm(name):
                out[name] = _pow2(_rig_rng(seed, name), v.shape, -2, 2, 0.1)
        _RIG_BASE[id(out)] = w
        _NORM_RIGS[key] = out
    return _NORM_RIGS[key]


def norm_weights(args_key, seed=0):
    """(args, norm_rig of the ``csm_weights`` dict)."""
    args, w = csm_weights(args_key)
    return args, norm_rig(args, w, seed)


MIMI_CLAMP = 1e-5       # EuclideanCodebook: embedding_sum / max(cluster_usage, 1e-5)


def mimi_clamped_bins(m, q, k, seed=0):
    """The two bins of codebook (q, k) that ``mimi_affine_rig`` puts under the clamp (usage 0, usage 1e-6)."""
    name = f"quantizer.{q}.vq.layers.{k}._codebook.clamped"
    return _rig_rng(seed, name).choice(m.bins, 2, replace=False)


def mimi_place_clamped(m, codes, seed=0):
    """``codes`` (B >= 2, n_q, F >= 2) with each codebook's two clamped bins placed once: utterance 0 frame 0 and
    the last utterance's frame 1.  Returns a copy."""
    codes = np.array(codes, np.int32)
    for k in range(m.n_q):
        lo = mimi_clamped_bins(m, "rvq_first" if k == 0 else "rvq_rest", 0 if k == 0 else k - 1, seed)
        codes[0, k, 0], codes[-1, k, 1] = lo
    return codes


def mimi_affine_rig(m, w, seed=0):
    """Seeded Mimi weights whose LayerNorm affine terms, layer scales and cluster usages can be told apart:
      * norm1/2.weight = 2^U(-1, 1), about 10 % negated;  norm1/2.bias = 0.5 N(0, 1);
      * layer_scale_1/2.scale = m.layer_scale x 2^U(-2, 2) per channel, separate draws for 1 and 2;
      * cluster_usage = 2^U(-2, 2) with the embedding_sum row multiplied by the same factor (the effective rows
        keep their scale); per codebook two bins (``mimi_clamped_bins``) sit under the clamp, usage 0 and 1e-6,
        their embedding_sum rows scaled by 1e-5 so that sum / 1e-5 stays O(0.1).
    Returns a new dict."""
    out = dict(w)
    for name, v in w.items():
        rng = _rig_rng(seed, name)
        if name.endswith((".norm1.weight", ".norm2.weight")):
            out[name] = _pow2(rng, v.shape, -1, 1, 0.1)
        elif name.endswith((".norm1.bias", ".norm2.bias")):
            out[name] = (0.5 * rng.standard_normal(v.shape)).astype(np.float32)
        elif name.endswith((".layer_scale_1.scale", ".layer_scale_2.scale")):
            out[name] = (np.float32(m.layer_scale) * _pow2(rng, v.shape, -2, 2)).astype(np.float32)
        elif name.endswith("._codebook.cluster_usage"):
            p = name[:-len(".cluster_usage")]
            q, k = p.split(".")[1], int(p.split(".")[4])
            f = _pow2(rng, v.shape, -2, 2)
            rows = (np.asarray(w[p + ".embedding_sum"], np.float32) * f[:, None]).astype(np.float32)
            lo = mimi_clamped_bins(m, q, k, seed)
            f[lo] = (0.0, 1e-6)
            rows[lo] = (np.asarray(w[p + ".embedding_sum"], np.float32)[lo] * np.float32(MIMI_CLAMP)).astype(np.float32)
            out[name], out[p + ".embedding_sum"] = f, rows
    return out


# ----------------------------------------------------------------------------- float64 taps: errors and the bar
TAPS = ("h_last", "c0", "ci")
# bar = BAR_MARGIN x e32.  Two float32 evaluations of the same arithmetic with different blocking and exp / rsqrt
# implementations differ from the truth by the same order, so a healthy engine sits near 1 x e32 (measured on
# the MI355X: 0.3-1.1 x over every path).  The margin is capped from above by what the
# bar has to catch (tests/test_f64_oracle_cpu.py): 2 x bar must stay under the error of an evaluation that
# loses the low activation bits of ONE projection kind of one stack, on the row / step that shows it least --
# that error is 4.8 x e32 at its smallest (tiny, bf16 weights, the backbone's down_proj seen from ci), so a
# margin of 4 would be over the cap; 2 holds it with room on both sides.
BAR_MARGIN = 2.0


def tap_errors(got, ref64):
    """got / ref64: (h_last, c0_logits, ci_logits) as ``oracle_taps`` returns them.  Per tap the array of
    max |got - float64| over the vocabulary (over D for h_last) / that row's largest |float64 value|:
    one figure per frame and row (and codebook step for ci)."""
    out = {}
    for tap, g, r in zip(TAPS, got, ref64):
        r = np.asarray(r, np.float64)
        out[tap] = np.abs(np.asarray(g, np.float64) - r).max(-1) / np.abs(r).max(-1)
    return out


def f64_reference(args, weights, variant, prompts, codes, block=None):
    """(float64 taps, e32) of a case: both oracles forced on ``codes`` (F, B, K); e32[tap] = the float32
    oracle's largest error over rows, steps and frames -- measured from the references alone.
    block: ``oracle_taps``' (both oracles)."""
    kw = dict(bf16=variant == "bf16", q4=variant == "q4")
    t64 = oracle_taps(oracle_for(args, weights, f64=True, **kw), prompts, codes, block)
    t32 = oracle_taps(oracle_for(args, weights, **kw), prompts, codes, block)
    return t64, {tap: float(e.max()) for tap, e in tap_errors(t32, t64).items()}


# ----------------------------------------------------------------------------- the Mimi codec against float64
# bar = MIMI_BAR_MARGIN x e32 on every frame of every utterance (tests/test_mimi_f64_gpu.py).  The margin starts
# from the CSM taps' and is capped the same way (tests/test_mimi_f64_cpu.py asserts it): it may not exceed half
# the smallest defect that the bar has to catch, in units of e32.
MIMI_BAR_MARGIN = BAR_MARGIN


def mimi_pair(name, mode, rig=None, context=None):
    """(MimiArgs, synthetic weights, float32 oracle, float64 oracle) of a codec config, memoised.
    rig: a function (m, w) -> new weights applied to the synthetic ones (``mimi_affine_rig``);
    context: the attention window in place of the config's (tests/test_mimi_window_*.py)."""
    key = ("mimi", name, mode, rig, context)
    if key not in _ORACLES:
        from csm_mlx.config import MIMI_CONFIGURATION
        from csm_mlx.weights import synthetic_mimi_weights
        from oracle.mimi_oracle import OracleMimi
        m = dataclasses.replace(MIMI_CONFIGURATION[name], attn_mode=mode)
        if context is not None:
            m = dataclasses.replace(m, context=context)
        w = synthetic_mimi_weights(m)
        if rig is not None:
            w = rig(m, w)
        _ORACLES[key] = (m, w, OracleMimi(m, w), OracleMimi(m, w, dtype=np.float64))
    return _ORACLES[key]


def mimi_errors(got, ref64, frame=None):
    """got / ref64 (B, ..., n): a waveform (B, 1, F * frame), or rows (B, T, D) with frame None.  Per
    utterance and per frame of ``frame`` samples (per row): max |got - float64| / the utterance's largest
    |float64 value|.  Returns (B, F) or (B, T)."""
    r = np.asarray(ref64, np.float64)
    g = np.asarray(got, np.float64)
    B = r.shape[0]
    assert g.shape == r.shape, (g.shape, r.shape)
    if frame is not None:
        g, r = g.reshape(B, -1, frame), r.reshape(B, -1, frame)
    return np.abs(g - r).max(-1) / np.abs(r).reshape(B, -1).max(-1)[:, None]


def mimi_pcm_clip(n, seed=0, amp=0.1):
    """The encode tests' clip: three seeded sines plus noise."""
    t = np.arange(n) / 24000.0
    rng = np.random.default_rng(seed)
    f = rng.uniform(100, 400, 3)
    x = amp * sum(np.sin(2 * np.pi * fi * t + rng.uniform(0, 6.28)) for fi in f) + rng.normal(0, 0.01, n)
    return x.astype(np.float32)


# ----------------------------------------------------------------------------- one projection against float64
def cut16(a):
    """hi + mid of the matrix-core paths' activation split (csrc/xs.h split3): two truncations to bf16, the
    second on the remainder -- what a path that loses the lo part computes with (16 significant bits)."""
    a = np.ascontiguousarray(a, np.float32)
    hi = (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    r = (a - hi).astype(np.float32)
    mid = (r.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    return (hi + mid).astype(np.float32)


def linear_f64_bar(x, w, n_cols=64, seed=0):
    """For y = x @ w.T (x (M, K), w (N, K) float32): (y64, S, bar, defect) with y64 the float64 product,
    S = sum |x||w| per output (the unit every error is divided by), bar = 1.5 x the largest error of a
    left-to-right float32 accumulation of the float32 products -- the least favourable plain order --
    over ``n_cols`` sampled output columns and every row, and defect = the largest error of the exact
    product with x cut to 16 significant bits (``cut16``).  All from numpy, nothing from the engine."""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    y64 = x64 @ w64.T
    S = np.abs(x64) @ np.abs(w64).T
    cols = np.sort(np.random.default_rng(seed).choice(w.shape[0], min(n_cols, w.shape[0]), replace=False))
    prods = x[:, None, :] * w[None, cols, :]                                    # (M, cols, K) float32 products
    lr = np.cumsum(prods, axis=-1, dtype=np.float32)[..., -1]                   # summed k = 0, 1, 2, ... in float32
    bar = 1.5 * float(linear_err(lr, y64[:, cols], S[:, cols]))
    defect = float(linear_err(cut16(x).astype(np.float64) @ w64.T, y64, S))
    return y64, S, bar, defect


def linear_err(y, y64, S):
    """Largest |y - y64| / S; an output whose S is 0 (an all-zero weight row: padding) must be exactly 0."""
    d = np.abs(np.asarray(y, np.float64) - y64)
    return np.where(S > 0, d / np.where(S > 0, S, 1.0), np.where(d > 0, np.inf, 0.0)).max()


# ----------------------------------------------------------------------------- SlotBatch against a stub engine
STUB_K = 4


class StubEngine:
    """The engine's side of a ``SlotBatch`` (csm_mlx.batching._EngineSlots' methods) as a small object that
    records every call.  eos[seed] = the frame at which the utterance submitted with that seed produces its
    all-zero frame (absent: never); a slot's codes are (seed + 1, its own frame index + 1, 1, 1).

    ``StubEngine(slots, eos)`` is what ``SlotBatch.run`` may use: it has its own ``log``, logs ("run", n), and
    its ``wait`` and ``ring`` fail -- ``run`` must not call them.  With ``F_cap`` (and a ``log`` to share with
    a stub codec) it is the streaming engine: ``run`` writes the frames' codes into a ring [F_cap][B][K] over
    the global frame index (every other cell written in a frame is -1) and logs ("run", n, global frame
    index), ``wait`` is logged, ``ring`` hands out the stub itself as the "device pointer"; ``pending`` holds
    from a ``run(n, sync=False)`` to its ``wait`` and no other call may fall inside."""

    def __init__(self, slots, eos, F_cap=None, log=None):
        self.B, self.eos, self.F_cap, self.log = slots, eos, F_cap, [] if log is None else log
        self.seed = [None] * slots
        self.frame = [0] * slots           # the slot's own frame index
        self.n = [0] * slots
        self.done = [True] * slots
        self.prompt = [False] * slots
        self.rows = [[] for _ in range(slots)]
        self.hist = None if F_cap is None else np.full((F_cap, slots, STUB_K), -7, np.int32)
        self.frames_run = 0
        self.pending = False

    def restart(self, b, seed):
        assert not self.pending
        self.log.append(("restart", b, seed))
        self.seed[b], self.frame[b], self.n[b], self.done[b], self.prompt[b], self.rows[b] = seed, 0, 0, False, False, []

    def release(self, b):
        assert not self.pending
        self.log.append(("release", b))
        self.seed[b], self.done[b], self.n[b], self.prompt[b] = None, True, 0, True

    def prefill(self, items):
        self.log.append(("prefill", tuple(b for b, _, _ in items)))
        for b, t, m in items:
            assert self.seed[b] is not None and not self.prompt[b]
            self.prompt[b] = True

    def run(self, n, sync=True):
        assert all(self.prompt), "frames while a restarted slot has no prompt"
        assert not self.pending, "a chunk enqueued before the last one was waited for"
        assert sync or self.hist is not None, "SlotBatch.run enqueues and waits in one call"
        self.log.append(("run", n) if self.hist is None else ("run", n, self.frames_run))
        for _ in range(n):
            row = None
            if self.hist is not None:
                row = self.hist[self.frames_run % self.F_cap]
                row[:] = -1
            for b in range(self.B):
                if self.seed[b] is None:
                    continue
                f = self.frame[b]
                if not self.done[b]:
                    if self.eos.get(self.seed[b]) == f:
                        self.done[b] = True
                    else:
                        self.rows[b].append([self.seed[b] + 1, f + 1, 1, 1])
                        if row is not None:
                            row[b] = self.rows[b][-1]
                        self.n[b] = f + 1
                self.frame[b] = f + 1
            self.frames_run += 1
        self.pending = not sync

    def wait(self):
        assert self.hist is not None, "SlotBatch.run has nothing to wait for"
        self.log.append(("wait",))
        self.pending = False

    def ring(self):
        assert self.hist is not None, "SlotBatch.run reads no ring"
        return self, self.F_cap, self.frames_run        # the "device pointer" is the stub itself

    def poll(self):
        assert not self.pending, "polled before the wait"
        return np.array(self.n, np.int32), np.array(self.done, bool)

    def read(self, b, cap):
        assert not self.pending
        self.log.append(("read", b))
        assert self.n[b] <= cap
        return np.array(self.rows[b], np.int32).reshape(-1, STUB_K)
