"""CPU ORACLE -- numpy fp32 restatement of the reference CSM hot path.

TEST INFRASTRUCTURE ONLY.  Only ``tests/``, ``__graft_entry__.smoke()`` and the
``cpu_baseline`` leg of ``bench.py`` may import this module; the product path
(csm-mlx_amd/) never does.

Parity status: the reference (MLX, mlx-lm, moshi-mlx) cannot be imported or run
in this container (ModuleNotFoundError, no network) and
ships no tests, fixtures or golden vectors, so this restatement is
**parity unpinned** against the reference itself.  It follows the reference
sources line by line as a spec:

  * frame step            /root/reference/csm_mlx/generation.py:21-92
  * generate loop / EOS   /root/reference/csm_mlx/generation.py:95-178
  * embeddings            /root/reference/csm_mlx/models.py:79-92
  * Llama-3 scaled RoPE   /root/reference/csm_mlx/attention.py:10-177
  * GQA attention         /root/reference/csm_mlx/attention.py:180-253
  * Llama block / RMSNorm mlx_lm.models.llama (TransformerBlock, MLP) as wired
                          by /root/reference/csm_mlx/models.py:50-77
  * LoRA / DoRA adapters  mlx_lm.tuner LoRALinear / DoRALinear / LoRAEmbedding /
                          DoRAEmbedding forwards (unfused), as wrapped by
                          /root/reference/csm_mlx/finetune/utils.py:16-108

Sampling with temperature cannot reproduce MLX's RNG; it restates the build's
own counter-based Gumbel-max sampler (``gumbel_u``) so GPU sampled codes can be
checked bit-for-bit against this file.

``OracleCSM(..., dtype=np.float64)`` evaluates the same stored parameters in
float64 (the truth the float32 evaluations, this one and the GPU's, are measured
against); the default is the fp32 restatement.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import numpy as np

F32 = np.float32
F64 = np.float64


def _dt(x):
    """The evaluation precision follows the activations: float64 in, float64 arithmetic and out; anything
    else is the float32 restatement (the default, bit for bit what it always was)."""
    return F64 if getattr(x, "dtype", None) == F64 else F32


def _dense(w, dt):
    """A stored matrix as an array: lazy int4 triples (quant_oracle.QuantMatrix) dequantize in ``dt``."""
    return w.dense(dt) if hasattr(w, "dense") else w.astype(dt, copy=False)   # (explicit: a mixed matmul is slow)


# ----------------------------------------------------------------------------- RoPE
def llama3_rope_theta(dim: int, base: float, scale_factor: float, low_freq_factor: float = 1.0,
                      high_freq_factor: float = 4.0, old_context_len: int = 8192) -> np.ndarray:
    """attention.py:57-79 (rope_init) + :94-117 (apply_scaling), in float32 as MLX does."""
    expo = (np.arange(0, dim, 2, dtype=F32)[: dim // 2] / F32(dim)).astype(F32)
    freqs = (F32(1.0) / np.power(F32(base), expo, dtype=F32)).astype(F32)
    low_freq_wavelen = old_context_len / low_freq_factor
    high_freq_wavelen = old_context_len / high_freq_factor
    out = []
    for freq in freqs:
        wavelen = F32(2 * math.pi) / freq                      # mx float32 scalar math
        if wavelen < high_freq_wavelen:
            out.append(freq)
        elif wavelen > low_freq_wavelen:
            out.append(freq / F32(scale_factor))
        else:
            smooth = (F32(old_context_len) / wavelen - F32(low_freq_factor)) / F32(high_freq_factor - low_freq_factor)
            out.append((F32(1) - smooth) * freq / F32(scale_factor) + smooth * freq)
    return np.array(out, dtype=F32)


def rope_cache(theta: np.ndarray, max_seq_len: int = 2048) -> np.ndarray:
    """attention.py:81-92 -> (max_seq_len, dim//2, 2) = [cos, sin]."""
    seq = np.arange(max_seq_len, dtype=F32)
    idx_theta = np.outer(seq, theta).astype(F32)
    return np.stack([np.cos(idx_theta), np.sin(idx_theta)], axis=-1).astype(F32)


def rope_apply(x: np.ndarray, cache: np.ndarray, offset: int) -> np.ndarray:
    """attention.py:119-177: interleaved pairs (2i, 2i+1), fp32.  x: (B, T, H, hd).
    A float64 x is rotated in float64 by the same float32 table (the table is input data)."""
    dt = _dt(x)
    b, t, h, hd = x.shape
    if offset + t > cache.shape[0]:
        raise ValueError("RoPE position beyond the cached 2048-position table (attention.py:152)")
    c = cache[offset: offset + t].reshape(1, t, 1, hd // 2, 2)
    xs = x.astype(dt).reshape(b, t, h, hd // 2, 2)
    x0, x1 = xs[..., 0], xs[..., 1]
    out = np.stack([x0 * c[..., 0] - x1 * c[..., 1], x1 * c[..., 0] + x0 * c[..., 1]], axis=-1)
    return out.reshape(b, t, h, hd).astype(dt)


# ----------------------------------------------------------------------------- blocks
def rms_norm(x: np.ndarray, w: np.ndarray, eps: float) -> np.ndarray:
    """mlx fast.rms_norm: x * rsqrt(mean(x^2) + eps) * w, fp32 internally."""
    dt = _dt(x)
    x = x.astype(dt)
    ms = np.mean(x * x, axis=-1, keepdims=True, dtype=dt)
    return (x * (dt(1) / np.sqrt(ms + dt(eps))) * w).astype(dt)


def linear(x: np.ndarray, w: np.ndarray) -> np.ndarray:
    """nn.Linear without bias: y = x @ W.T with W (out, in)."""
    dt = _dt(x)
    return np.matmul(x, _dense(w, dt).T).astype(dt)


def adapted_linear(x: np.ndarray, w: np.ndarray, ad: Optional[dict]) -> np.ndarray:
    """mlx_lm LoRALinear / DoRALinear forward, unfused (finetune/utils.py:33-50 wraps the layer):
    LoRA  y = x W^T + scale (x A) B;  DoRA  y = (m / ||W + scale B^T A^T||_row) (x W^T + scale (x A) B).
    ad: {"a": (in, r), "b": (r, out), "scale": s, "m": (out,) or None}."""
    y = linear(x, w)
    if ad is None:
        return y
    dt = _dt(x)
    z = (y + dt(ad["scale"]) * np.matmul(np.matmul(x, ad["a"]), ad["b"])).astype(dt)
    if ad.get("m") is not None:
        wf = _dense(w, dt) + (dt(ad["scale"]) * ad["b"].T) @ ad["a"].T
        z = (ad["m"] / np.linalg.norm(wf, axis=1).astype(dt)).astype(dt) * z
    return z.astype(dt)


def adapted_embedding(idx: np.ndarray, w: np.ndarray, ad: Optional[dict], dt=F32) -> np.ndarray:
    """mlx_lm LoRAEmbedding / DoRAEmbedding forward: y = E[i] + scale A[i] B, DoRA rows rescaled
    by m[i] / ||E[i] + scale A[i] B||.  ``dt``: the evaluation precision (the rows convert exactly)."""
    y = w.rows(idx, dt) if hasattr(w, "rows") else w[idx].astype(dt, copy=False)
    if ad is None:
        return y
    z = (y + np.matmul(ad["a"][idx], dt(ad["scale"]) * ad["b"])).astype(dt)
    if ad.get("m") is not None:
        z = (ad["m"][idx] / np.linalg.norm(z, axis=-1).astype(dt))[..., None] * z
    return z.astype(dt)


def silu(x):
    dt = _dt(x)
    return (x / (dt(1) + np.exp(-x))).astype(dt)


def sdpa(q, k, v, scale, causal_offset: Optional[int]):
    """softmax(q k^T * scale + mask) v; q (B,H,T,hd), k/v (B,H,S,hd); causal iff T>1."""
    dt = _dt(q)
    s = np.matmul(q, np.swapaxes(k, -1, -2)).astype(dt) * dt(scale)
    T, S = q.shape[2], k.shape[2]
    if causal_offset is not None and T > 1:
        qi = np.arange(T)[:, None] + causal_offset
        kj = np.arange(S)[None, :]
        s = np.where(kj <= qi, s, dt(-np.inf))
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(-1, keepdims=True)
    return np.matmul(p.astype(dt), v).astype(dt)


class KVCacheRef:
    """mlx_lm KVCache semantics: append at offset, return the [:offset] view."""

    def __init__(self):
        self.k = None
        self.v = None
        self.offset = 0

    def update_and_fetch(self, k, v):
        self.k = k if self.k is None else np.concatenate([self.k, k], axis=2)
        self.v = v if self.v is None else np.concatenate([self.v, v], axis=2)
        self.offset = self.k.shape[2]
        return self.k, self.v


class LlamaRef:
    """mlx_lm LlamaModel with embed_tokens=Identity and the reference Attention patched in."""

    def __init__(self, w: Dict[str, np.ndarray], prefix: str, args, adapters: Optional[Dict[str, dict]] = None,
                 dtype=F32, mat=None):
        """dtype: the evaluation precision (float32, or float64 on the same stored parameters);
        mat: name -> the matrix handed to ``linear`` (OracleCSM.mat; default: the stored one)."""
        self.w, self.p, self.a = w, prefix, args
        self.adapters = adapters or {}
        self.dt = dtype
        self.mat = mat or w.__getitem__
        rs = args.rope_scaling
        theta = llama3_rope_theta(args.head_dim, args.rope_theta, rs.get("factor", 1.0),
                                  1.0, 4.0, 8192)   # attention.py:201-205 passes only base/scale_factor
        self.rope = rope_cache(theta, 2048)

    def attention(self, i, x, cache: KVCacheRef):
        a, w, p = self.a, self.w, f"{self.p}.layers.{i}.self_attn"
        b, t, _ = x.shape
        hd, H, Hkv = a.head_dim, a.num_attention_heads, a.num_key_value_heads
        q = self.lin(x, f"{p}.q_proj").reshape(b, t, H, hd)
        k = self.lin(x, f"{p}.k_proj").reshape(b, t, Hkv, hd)
        v = self.lin(x, f"{p}.v_proj").reshape(b, t, Hkv, hd)
        off = cache.offset
        q = rope_apply(q, self.rope, off)
        k = rope_apply(k, self.rope, off)
        q, k, v = (np.swapaxes(z, 1, 2) for z in (q, k, v))
        k, v = cache.update_and_fetch(k, v)
        rep = H // Hkv
        k = np.repeat(k, rep, axis=1)
        v = np.repeat(v, rep, axis=1)
        o = sdpa(q, k, v, hd ** -0.5, off)
        o = np.swapaxes(o, 1, 2).reshape(b, t, H * hd)
        return self.lin(o, f"{p}.o_proj")

    def lin(self, x, path):
        return adapted_linear(x, self.mat(path + ".weight"), self.adapters.get(path))

    def __call__(self, x, caches: List[KVCacheRef]):
        a, w = self.a, self.w
        dt = self.dt
        h = x.astype(dt)
        for i in range(a.num_hidden_layers):
            p = f"{self.p}.layers.{i}"
            r = self.attention(i, rms_norm(h, w[f"{p}.input_layernorm.weight"], a.rms_norm_eps), caches[i])
            h = (h + r).astype(dt)
            n = rms_norm(h, w[f"{p}.post_attention_layernorm.weight"], a.rms_norm_eps)
            g = self.lin(n, f"{p}.mlp.gate_proj")
            u = self.lin(n, f"{p}.mlp.up_proj")
            h = (h + self.lin((silu(g) * u).astype(dt), f"{p}.mlp.down_proj")).astype(dt)
        return rms_norm(h, w[f"{self.p}.norm.weight"], a.rms_norm_eps)


# ----------------------------------------------------------------------------- sampler (build's own RNG)
MASK64 = (1 << 64) - 1


def splitmix64(x: np.ndarray) -> np.ndarray:
    x = (x + np.uint64(0x9E3779B97F4A7C15)) & np.uint64(MASK64)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def gumbel_u(seed: int, step: int, n: int) -> np.ndarray:
    """Uniform (0,1) doubles for vocab indices 0..n-1 of one sampling event.

    key = splitmix64(splitmix64(seed) ^ step) ; u_v = ((splitmix64(key ^ v) >> 11) + 0.5) * 2^-53
    (csm-mlx_amd/csrc/csm_kernels.hip ``sample_gumbel`` implements the same).
    """
    with np.errstate(over="ignore"):
        k = splitmix64(np.array([seed & MASK64], dtype=np.uint64))
        k = splitmix64(k ^ np.uint64(step & MASK64))
        h = splitmix64(k ^ np.arange(n, dtype=np.uint64))
    return ((h >> np.uint64(11)).astype(np.float64) + 0.5) * (2.0 ** -53)


def topk_threshold(logits: np.ndarray, k: int) -> float:
    """k-th largest value; every logit >= it is kept (ties at the boundary all kept)."""
    if k <= 0 or k >= logits.shape[-1]:
        return -np.inf
    return float(np.sort(logits)[::-1][k - 1])


def filter_keep(logits: np.ndarray, top_k: int, top_p: float, min_p: float, min_keep: int) -> np.ndarray:
    """The kept set of mlx_lm ``make_sampler``'s filter chain (sample_utils: apply_top_k, then
    apply_top_p, then apply_min_p, then categorical_sampling), restated on the log-probabilities
    ``lp = logits - logsumexp(logits)`` that mlx_lm's generate hands its sampler:

      * top_k: keep lp >= the k-th largest (ties at the k-th value kept; mlx argpartition breaks them
        arbitrarily);
      * top_p: probs = exp(lp) (0 where masked, not renormalised), cumulative sum in ascending
        order; keep where it exceeds float32(1 - top_p);
      * min_p: keep lp >= max(kept lp) + float32(log(min_p)), and always the first min_keep entries
        of the descending order (if still kept).
    Order for the sorts: lp descending, equal values by index ascending (ascending = its reverse).
    Sums are float32 (np.cumsum order); the GPU sums the same values in a parallel order, so a
    top_p boundary within float32 rounding of 1 - top_p may fall differently (never seen in tests).
    The same holds for min_p: lse (np.sum order here, a DPP / wave-ordered sum on the GPU) enters every
    lp, so an entry within float32 rounding of the min_p threshold may be kept on one side only.
    If every entry is removed the arg-max is kept (mlx would sample from an all -inf row).
    Parity of this chain against mlx_lm itself is unpinned (mlx_lm is not importable here and the
    reference holds no sampler fixture; its generate() samples with plain categorical,
    generation.py:51-54)."""
    l = logits.astype(F32)
    n = l.shape[-1]
    keep = l >= topk_threshold(l, top_k)
    if (0.0 < top_p < 1.0) or min_p != 0.0:
        mx_ = l.max()
        lse = F32(mx_ + F32(np.log(np.sum(np.exp(l - mx_, dtype=F32), dtype=F32))))
        lp = (l - lse).astype(F32)
        order = np.lexsort((np.arange(n), -lp.astype(np.float64)))        # lp desc, index asc
        if 0.0 < top_p < 1.0:
            p_desc = np.where(keep[order], np.exp(lp[order]), F32(0)).astype(F32)
            cum_asc = np.cumsum(p_desc[::-1], dtype=F32)[::-1]           # ascending cumsum, back in desc order
            kp = np.zeros(n, bool)
            kp[order] = cum_asc > F32(1.0 - top_p)
            keep &= kp
        if min_p != 0.0 and keep.any():
            top = lp[keep].max()
            tmin = F32(top + F32(math.log(min_p)))
            rank = np.empty(n, np.int64)
            rank[order] = np.arange(n)
            keep &= ~(lp < tmin) | (rank < min_keep)
    if not keep.any():
        keep[int(np.argmax(l))] = True
    return keep


def sample_one(logits: np.ndarray, temperature: float, top_k: int, seed: int, step: int,
               top_p: float = 0.0, min_p: float = 0.0, min_keep: int = 1) -> int:
    """Greedy = first max (mx.argmax); else Gumbel-max of logits*(1/temp) over the kept set
    (top-k; with top_p / min_p the mlx_lm filter chain, ``filter_keep``)."""
    if temperature == 0:
        return int(np.argmax(logits.astype(_dt(logits))))
    logits = logits.astype(F32)
    keep = filter_keep(logits, top_k, top_p, min_p, min_keep)
    scaled = (logits * (F32(1.0) / F32(temperature))).astype(F32).astype(np.float64)
    u = gumbel_u(seed, step, logits.shape[-1])
    g = -np.log(-np.log(u))
    val = np.where(keep, scaled + g, -np.inf)
    return int(np.argmax(val))


# ----------------------------------------------------------------------------- CSM
class OracleCSM:
    """Restatement of ``CSM`` (models.py:31-92) + ``generate_frame`` (generation.py:21-92)."""

    def __init__(self, args, weights: Dict[str, np.ndarray], bb_args, dec_args,
                 adapters: Optional[Dict[str, dict]] = None, dtype=np.float32):
        """adapters: module path -> LoRA/DoRA tensors (see ``adapted_linear``), applied unfused.
        dtype: np.float32 (the restatement) or np.float64: every operation (embedding sums, RMSNorm,
        matmuls, RoPE application, SDPA, SiLU, heads) in float64 on the SAME stored parameters, converted
        exactly where they are used -- the truth the float32 paths (this oracle's and the GPU's) are
        measured against.  The RoPE table stays the float32 table the engine is given (input data).
        A weight may be a ``quant_oracle.QuantMatrix`` (packed, scales, biases): it dequantizes in the
        evaluation precision, so the float64 reference of an int4 model is exact ``scale*q + bias``."""
        if dtype not in (np.float32, np.float64):
            raise ValueError("dtype must be np.float32 or np.float64")
        self.args = args
        self.dt = dtype
        self.w = {k: v if hasattr(v, "dense") else np.asarray(v, dtype=F32) for k, v in weights.items()}
        self.ad = adapters or {}
        self._up = {}
        self.backbone = LlamaRef(self.w, "backbone", bb_args, self.ad, dtype, self.mat)
        self.decoder = LlamaRef(self.w, "decoder", dec_args, self.ad, dtype, self.mat)
        self.bb_args, self.dec_args = bb_args, dec_args
        self.V, self.K = args.n_audio_vocab, args.n_audio_codebooks
        self.debug = {}

    def mat(self, name: str):
        """The matrix ``linear`` multiplies by.  float32: the stored array.  float64: the stored array too
        (``linear`` converts it exactly for the product, a temporary), except the depth decoder's and the
        projection's, which every codebook step reuses: those are kept converted (~0.9 GB for csm_1b)
        until ``drop_upcasts``.  No float64 copy of the whole model is ever held."""
        w = self.w[name]
        if self.dt is F32 or not (name.startswith("decoder.") or name == "projection.weight"):
            return w
        if name not in self._up:
            self._up[name] = np.ascontiguousarray(_dense(w, F64), dtype=F64)
        return self._up[name]

    def drop_upcasts(self):
        self._up.clear()

    def new_backbone_cache(self):
        return [KVCacheRef() for _ in range(self.bb_args.num_hidden_layers)]

    def embed_audio(self, codebook: int, tokens: np.ndarray) -> np.ndarray:
        return adapted_embedding(tokens + codebook * self.V, self.w["audio_embeddings.weight"],
                                 self.ad.get("audio_embeddings"), self.dt)           # models.py:79-80

    def embed_tokens(self, tokens: np.ndarray) -> np.ndarray:                   # models.py:82-92
        text = adapted_embedding(tokens[:, :, -1], self.w["text_embeddings.weight"],
                                 self.ad.get("text_embeddings"), self.dt)[:, :, None, :]
        audio_tokens = tokens[:, :, :-1] + self.V * np.arange(self.K)
        audio = adapted_embedding(audio_tokens.reshape(-1), self.w["audio_embeddings.weight"],
                                  self.ad.get("audio_embeddings"), self.dt).reshape(*tokens.shape[:2], self.K, -1)
        return np.concatenate([audio, text], axis=-2)

    def embed_rows(self, tokens, mask) -> np.ndarray:
        """generation.py:34-36: the backbone's input rows (B, T, D) of tokens / mask (B, T, K+1)."""
        emb = self.embed_tokens(tokens) * mask[..., None].astype(self.dt)          # :34-35
        x = np.zeros(emb.shape[:2] + emb.shape[3:], self.dt)
        for j in range(emb.shape[2]):                                              # :36 sum over 33, in order
            x = x + emb[:, :, j]
        return x

    def frame(self, tokens, mask, cache, temperature=0.0, top_k=0, seeds=None, frame_idx=0,
              processors=None, c0_history=None, top_p=0.0, min_p=0.0, min_keep=1, sampler=None, forced=None):
        """generation.py:21-92.  tokens/mask (B,T,33).  Returns codes (B,K) int32.
        processors: logits processors on c0 (:44-49), called with (stack(c0_history) or zeros((0,)),
        logits); c0 (B,1) is appended to c0_history when it is a list (:60-61).
        sampler: a callable logits (B, V) -> codes (B,) used for every codebook instead of the built-in
        greedy / Gumbel sampler (the sampler= keyword of the reference CLI, cli/generate.py:197-199).
        forced: codes (B, K) fed forward at every codebook instead of the sampled ones (teacher forcing:
        the logits are computed as always; the frame returns ``forced``)."""
        B = tokens.shape[0]
        dt = self.dt
        if forced is not None:
            forced = np.asarray(forced, np.int64).reshape(B, self.K)
        h = self.backbone(self.embed_rows(tokens, mask), cache)                    # :39
        h_last = h[:, -1, :]                                                       # :40
        c0_logits = adapted_linear(h_last, self.w["codebook0_head.weight"], self.ad.get("codebook0_head"))  # :42
        for proc in processors or []:                                              # :44-49
            hist = np.stack(c0_history, 0) if c0_history else np.zeros((0,), np.int32)
            c0_logits = np.asarray(proc(hist, c0_logits), dt)
        self.debug["c0_logits"] = c0_logits
        self.debug["h_last"] = h_last
        seeds = seeds if seeds is not None else [0] * B
        flt = dict(top_p=top_p, min_p=min_p, min_keep=min_keep)
        if forced is not None:
            c0 = forced[:, 0]
        elif sampler is not None:
            c0 = np.asarray(sampler(c0_logits), np.int64).reshape(B)
        else:
            c0 = np.array([sample_one(c0_logits[b], temperature, top_k, seeds[b], frame_idx * self.K, **flt)
                           for b in range(B)], dtype=np.int64)                    # :51-54
        out = np.zeros((B, self.K), np.int32)
        out[:, 0] = c0
        if c0_history is not None:
            c0_history.append(c0[:, None].astype(np.int32))
        dec_in = np.stack([h_last, self.embed_audio(0, c0)], axis=1)               # :57-64
        dcache = [KVCacheRef() for _ in range(self.dec_args.num_hidden_layers)]   # :70 fresh per frame
        ci_logits_all = []
        for i in range(1, self.K):                                                 # :72
            z = self.decoder(adapted_linear(dec_in, self.w["projection.weight"], self.ad.get("projection")),
                             dcache)                                               # :74-77
            head = self.w["audio_head"][i - 1].astype(dt, copy=False)
            logits = np.matmul(z[:, -1, :], head).astype(dt)                       # :79 (in,out) layout
            ci_logits_all.append(logits)
            if forced is not None:
                ci = forced[:, i]
            elif sampler is not None:
                ci = np.asarray(sampler(logits), np.int64).reshape(B)
            else:
                ci = np.array([sample_one(logits[b], temperature, top_k, seeds[b], frame_idx * self.K + i, **flt)
                               for b in range(B)], dtype=np.int64)
            out[:, i] = ci
            dec_in = self.embed_audio(i, ci)[:, None, :]                          # :87-89
        self.debug["ci_logits"] = np.stack(ci_logits_all, axis=1)
        return out

    def generate_codes(self, prompt_tokens: np.ndarray, prompt_mask: np.ndarray, max_frames: int,
                       temperature=0.0, top_k=0, seed=0, max_seq_len=2048, collect_logits=False,
                       processors=None, top_p=0.0, min_p=0.0, min_keep=1, sampler=None):
        """generation.py:95-178 up to (not including) decode_audio.  prompt (L,33).

        Returns (codes (F,K) int32 up to EOS, logits list if requested)."""
        L = prompt_tokens.shape[0]
        if L >= max_seq_len - max_frames:                                          # :132-137
            raise ValueError(f"Inputs too long ({L}), must be below max_seq_len - max_audio_frames: "
                             f"{max_seq_len - max_frames}")
        cache = self.new_backbone_cache()
        inp, msk = prompt_tokens[None].astype(np.int64), prompt_mask[None].astype(bool)
        samples, logs, c0_history = [], [], []                                     # :128
        for f in range(max_frames):                                                # :139
            s = self.frame(inp, msk, cache, temperature, top_k, [seed], f, processors, c0_history,
                           top_p=top_p, min_p=min_p, min_keep=min_keep, sampler=sampler)
            if collect_logits:
                logs.append((self.debug["c0_logits"][0].copy(), self.debug["ci_logits"][0].copy()))
            if not s.any():                                                        # :151 EOS
                break
            samples.append(s[0])
            inp = np.concatenate([s, np.zeros((1, 1), np.int32)], axis=1)[:, None, :].astype(np.int64)   # :156
            msk = np.concatenate([np.ones_like(s, bool), np.zeros((1, 1), bool)], axis=1)[:, None, :]   # :159
        codes = np.stack(samples) if samples else np.zeros((0, self.K), np.int32)
        return (codes, logs) if collect_logits else codes


def text_frame(ids, n_codebooks: int = 32) -> (np.ndarray, np.ndarray):
    """tokenizers.py:43-58 given already-tokenized ids: (n,K+1) tokens with ids in the last col."""
    ids = np.asarray(ids, dtype=np.int32)
    t = np.zeros((len(ids), n_codebooks + 1), np.int32)
    m = np.zeros((len(ids), n_codebooks + 1), bool)
    t[:, -1] = ids
    m[:, -1] = True
    return t, m


def audio_frame(codes_kt: np.ndarray) -> (np.ndarray, np.ndarray):
    """tokenizers.py:69-85: (K,T) codes -> append EOS zero frame -> (T+1, 33) rows, mask cols 0..K-1."""
    K, T = codes_kt.shape
    c = np.concatenate([codes_kt, np.zeros((K, 1), codes_kt.dtype)], axis=1)
    t = np.zeros((T + 1, K + 1), np.int32)
    m = np.zeros((T + 1, K + 1), bool)
    t[:, :-1] = c.T
    m[:, :-1] = True
    return t, m


# ----------------------------------------------------------------------------- compute_loss
def compute_loss_ref(o: "OracleCSM", batch, per_sample: bool = False, cause_mismatch: bool = False):
    """/root/reference/csm_mlx/finetune/trainer.py:203-318, whole-sequence form: one causal backbone
    call over rows [0, S-1), codebook0_head on every position, one causal decoder call over the
    (B*(S-1), K+1) rows [h_t, E_0(c_0), ..., E_{K-1}(c_{K-1})] of the next frame, masked means of
    the cross entropies."""
    tokens = np.asarray(batch["tokens"]).astype(np.int64)
    masks = np.asarray(batch["masks"]).astype(bool)
    loss_masks = np.asarray(batch["loss_masks"]).astype(bool)
    w0 = F32(batch["first_codebook_weight_multiplier"])
    B, S, n_cb = tokens.shape
    K = n_cb - 1
    tgt = tokens[:, 1:, :K]                                                        # :220-221
    lm = masks[:, 1:, :K] & loss_masks[:, 1:, :K]                                  # :263-265
    emb = o.embed_tokens(tokens) * masks[..., None].astype(F32)                    # :232-233
    x = np.zeros(emb.shape[:2] + emb.shape[3:], F32)
    for j in range(emb.shape[2]):
        x = x + emb[:, :, j]
    h = o.backbone(x[:, :-1], o.new_backbone_cache())                              # :234-239
    c0_logits = adapted_linear(h, o.w["codebook0_head.weight"], o.ad.get("codebook0_head"))
    ci = np.stack([o.embed_audio(i, tgt[:, :, i]) for i in range(K)], axis=-2)     # :243-249
    dec_in = np.concatenate([h[:, :, None, :], ci], axis=-2).reshape(-1, n_cb, h.shape[-1])
    dcache = [KVCacheRef() for _ in range(o.dec_args.num_hidden_layers)]
    proj = adapted_linear(dec_in, o.w["projection.weight"], o.ad.get("projection"))
    dh = o.decoder(proj, dcache).reshape(B, S - 1, n_cb, -1)[:, :, 1:-1, :]        # :257-262
    if cause_mismatch:                                                             # :266-269
        tgt = np.concatenate([tgt[:, 1:], tgt[:, :1]], axis=1)

    def ce(logits, t):
        lg = logits.astype(np.float64)
        m = lg.max(-1, keepdims=True)
        lse = np.log(np.exp(lg - m).sum(-1)) + m[..., 0]
        return lse - np.take_along_axis(lg, t[..., None], -1)[..., 0]

    def masked_mean(v, msk):
        return (v * msk).sum(-1) / msk.sum(-1) if per_sample else (v * msk).sum() / msk.sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        total = masked_mean(ce(c0_logits, tgt[:, :, 0]), lm[:, :, 0]) * w0 / K         # :271-289
        for i in range(1, K):                                                          # :291-312
            logits = np.matmul(dh[:, :, i - 1, :], o.w["audio_head"][i - 1])
            total = total + masked_mean(ce(logits, tgt[:, :, i]), lm[:, :, i]) / K
    return total
