"""Regenerate the committed golden fixtures from the numpy oracle (test infrastructure).

    python tests/golden/make_golden.py

Fixtures are small .npz files (ids, codes, logit slices, waveform samples) produced from
seeded synthetic weights; they pin the oracle (and, through the GPU tests, the HIP path)
against silent regressions.  Nothing here comes from the reference (which cannot run here).
"""
import dataclasses
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "csm-mlx_amd"), ROOT]

from csm_mlx.config import BACKBONE_CONFIGURATION as BB, DECODER_CONFIGURATION as DC, MIMI_CONFIGURATION  # noqa
from csm_mlx.models import csm_tiny  # noqa: E402
from csm_mlx.weights import synthetic_csm_weights, synthetic_mimi_weights  # noqa: E402
from oracle.csm_oracle import OracleCSM, text_frame  # noqa: E402
from oracle.mimi_oracle import OracleMimi  # noqa: E402

TINY_IDS = [998, 17, 401, 77, 912, 3, 999]

# configs[1] prompt (bench.py prompt_ids(0)): BOS + 12 ids ~ U[0, 128000) (seed 1) + EOS
CONFIG1_IDS = [128000] + [int(x) for x in np.random.default_rng(1).integers(0, 128000, 12)] + [128001]
# configs[0] "[0]Hello from Sesame." under the Llama-3.2 BPE + BOS/EOS template (tokenizers.py:24-58).
# UNVERIFIED: the tokenizer assets (unsloth/Llama-3.2-1B) are not available offline.  The ids are the
# cl100k-compatible pieces "[", "0", "]", "Hello", " from", " Ses", "ame", "." recalled by hand; only
# the plumbing (prompt -> 125 frames -> Mimi decode) is pinned by this fixture, not the tokenizer.
CONFIG0_IDS = [128000, 58, 15, 60, 9906, 505, 23720, 373, 13, 128001]
LONG_FRAMES = (0, 63, 64, 100, 124)   # frames whose logits are kept (attention crosses 64-key chunks)
LONG_CI = (1, 2, 16, 31)              # codebooks whose ci logits are kept


def pcm_fixture(n=9600, seed=3):
    t = np.arange(n) / 24000.0
    rng = np.random.default_rng(seed)
    x = 0.1 * (np.sin(2 * np.pi * 150 * t) + np.sin(2 * np.pi * 230 * t) + np.sin(2 * np.pi * 370 * t))
    return (x + rng.normal(0, 0.01, n)).astype(np.float32)


def csm_golden():
    args = csm_tiny()
    o = OracleCSM(args, synthetic_csm_weights(args, 0), BB["tiny"], DC["tiny"])
    t, m = text_frame(TINY_IDS, args.n_audio_codebooks)
    codes, logs = o.generate_codes(t, m, 8, collect_logits=True)
    scodes = o.generate_codes(t, m, 8, temperature=0.8, top_k=5, seed=1234)
    return dict(ids=np.array(TINY_IDS, np.int32), codes=codes, c0_logits=np.stack([l[0] for l in logs]),
                ci_logits=np.stack([l[1] for l in logs]), sampled_codes=scodes)


def _oracle(args, w, bf16):
    from csm_mlx.weights import bf16_round
    ww = {k: bf16_round(v) for k, v in w.items()} if bf16 else w
    return OracleCSM(args, ww, BB[args.backbone_name], DC[args.decoder_name])


def csm_1b_long_golden():
    """configs[1] at full length: csm_1b B=1 greedy, 125 frames from the 14-row prompt (backbone
    attention reaches S = 139 keys: three 64-key chunks), fp32 weights and bf16-rounded weights."""
    from csm_mlx.models import csm_1b
    args = csm_1b()
    w = synthetic_csm_weights(args, 0)
    out = dict(ids=np.array(CONFIG1_IDS, np.int32), frames=np.array(LONG_FRAMES), ci_codebooks=np.array(LONG_CI))
    for tag, bf16 in (("fp32", False), ("bf16", True)):
        codes, logs = _oracle(args, w, bf16).generate_codes(*text_frame(CONFIG1_IDS, 32), 125, collect_logits=True)
        out[f"{tag}_codes"] = codes
        out[f"{tag}_c0"] = np.stack([logs[f][0] for f in LONG_FRAMES])
        out[f"{tag}_ci"] = np.stack([logs[f][1][[c - 1 for c in LONG_CI]] for f in LONG_FRAMES])
        print(tag, "codes", codes.shape, flush=True)
    return out


def config0_golden():
    """configs[0] plumbing: generate("[0]Hello from Sesame." ids (unverified), speaker 0, no context,
    10 s, greedy) on the fp32 oracle -> 125 frames; the Mimi oracle's decode of them (rms + head)."""
    from csm_mlx.models import csm_1b
    args = csm_1b()
    w = synthetic_csm_weights(args, 0)
    codes = _oracle(args, w, False).generate_codes(*text_frame(CONFIG0_IDS, 32), 125)
    m = MIMI_CONFIGURATION["mimi_202407"]
    y = OracleMimi(m, synthetic_mimi_weights(m, 0)).decode(np.ascontiguousarray(codes.T[None]))
    return dict(ids=np.array(CONFIG0_IDS, np.int32), codes=codes, pcm_head=y[0, 0, :1920],
                pcm_rms=np.array(np.sqrt(np.mean(y.astype(np.float64) ** 2))), n_samples=np.array(y.shape[-1]))


def tiny_long_prompt(seed=11):
    """A >= 200-row tiny prompt: text, 100 audio rows + EOS row, text, 100 audio rows + EOS row, text
    (tokenize_segment layout, tokenizers.py:61-102) -- prefill and decode past three 64-key chunks."""
    from oracle.csm_oracle import audio_frame
    rng = np.random.default_rng(seed)
    parts = []
    for i in range(3):
        parts.append(text_frame([998] + [int(x) for x in rng.integers(0, 990, 6)] + [999], 4))
        if i < 2:
            parts.append(audio_frame(rng.integers(0, 64, (4, 100)).astype(np.int32)))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


TINY_LONG_FRAMES = (0, 20, 39)


def tiny_long_golden():
    args = csm_tiny()
    w = synthetic_csm_weights(args, 0)
    t, m = tiny_long_prompt()
    out = dict(tokens=t, mask=m, frames=np.array(TINY_LONG_FRAMES))
    for tag, bf16 in (("fp32", False), ("bf16", True)):
        codes, logs = _oracle(args, w, bf16).generate_codes(t, m, 40, collect_logits=True)
        out[f"{tag}_codes"] = codes
        out[f"{tag}_c0"] = np.stack([logs[f][0] for f in TINY_LONG_FRAMES])
        out[f"{tag}_ci"] = np.stack([logs[f][1] for f in TINY_LONG_FRAMES])
    return out


def mimi_golden():
    out = {}
    for mode in ("mlx", "causal"):
        m = dataclasses.replace(MIMI_CONFIGURATION["tiny"], attn_mode=mode)
        o = OracleMimi(m, synthetic_mimi_weights(m, 0))
        pcm = pcm_fixture()
        codes = o.encode(pcm[None, None])
        y = o.decode(codes)
        out[f"{mode}_codes"] = codes
        out[f"{mode}_pcm_head"] = y[0, 0, :512]
        out[f"{mode}_pcm_rms"] = np.array(np.sqrt(np.mean(y.astype(np.float64) ** 2)))
    return out


# ----------------------------------------------------------------------------- batched, full length
# configs[3]'s per-GPU shard (B = 32 bf16 greedy, 125 frames) and configs[2] (B = 32, temperature 0.8,
# top-k 50, streamed) on the EOS-capable rig of the seed-0 weights (tests/helpers.py eos_rig): prompts
# as bench.py's prompt_ids(g), g = 0..31; sampling seeds 1234 + g.
B32_FRAMES = (0, 64, 100, 124)      # frames whose logits are kept (past the backbone's first 64-key chunk)
B32_CI = (1, 16, 31)                # codebooks whose ci logits are kept
B32_LOGIT_UTTS = 4                  # logits kept for the first 4 utterances that run all frames (size)
B32_PROJ = 4                        # random unit vectors per streamed chunk's projection statistics


def _b32_prompts():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import b32_prompt_ids
    return [text_frame(ids, 32) for ids in b32_prompt_ids()]


def _b32_run(frames, temperature=0.0, top_k=0, keep_logits=True):
    """One (32, L, 33) batch through the oracle frame by frame (utterances are independent, so each one's
    codes up to its EOS frame are those of a run alone, generation.py:139-161).  Returns codes (32, F, K),
    n_frames (first all-zero frame, or F), c0 (F, 32, V), ci (F, 32, K-1, V) logits."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import eos_weights, oracle_for
    args, w = eos_weights("1b")
    o = oracle_for(args, w, bf16=True)
    prompts = _b32_prompts()
    toks = np.stack([t for t, _ in prompts]).astype(np.int64)
    msk = np.stack([m for _, m in prompts]).astype(bool)
    seeds = [1234 + g for g in range(32)]
    cache = o.new_backbone_cache()
    codes, c0s, cis = [], [], []
    for f in range(frames):
        s = o.frame(toks, msk, cache, temperature, top_k, seeds, f)
        codes.append(s)
        if keep_logits:
            c0s.append(o.debug["c0_logits"].copy())
            cis.append(o.debug["ci_logits"].copy())
        toks = np.concatenate([s, np.zeros((32, 1), np.int32)], 1)[:, None, :].astype(np.int64)
        msk = np.concatenate([np.ones_like(s, bool), np.zeros((32, 1), bool)], 1)[:, None, :]
        print("frame", f, "zero frames so far", int((~np.stack(codes, 1).any(-1)).any(-1).sum()), flush=True)
    codes = np.stack(codes, 1)
    zero = ~codes.any(-1)                                        # (32, F) all-zero frames
    n = np.array([int(np.argmax(z)) if z.any() else frames for z in zero], np.int32)
    return codes, n, (np.stack(c0s) if keep_logits else None), (np.stack(cis) if keep_logits else None)


def config4_b32_golden():
    """configs[3]'s shard: B = 32 bf16 greedy, 125 frames; codes up to each utterance's EOS; c0 logits at
    B32_FRAMES and ci logits of B32_CI for every utterance still running there (and at each EOS frame)."""
    codes, n, c0, ci = _b32_run(125)
    print("n_frames", n.tolist(), flush=True)
    out = dict(codes=codes, n_frames=n, frames=np.array(B32_FRAMES), ci_codebooks=np.array(B32_CI))
    utts = [b for b in range(32) if n[b] == 125][:B32_LOGIT_UTTS]
    out["logit_utts"] = np.array(utts, np.int32)
    out["c0"] = np.stack([c0[f][utts] for f in B32_FRAMES])                      # (4 frames, 4 utts, V)
    out["ci"] = np.stack([ci[f][utts][:, [c - 1 for c in B32_CI]] for f in B32_FRAMES])   # (4, 4, 3, V)
    eos = [b for b in range(32) if n[b] < 125]
    out["eos_utts"] = np.array(eos, np.int32)
    out["eos_c0"] = np.stack([c0[n[b], b] for b in eos]) if eos else np.zeros((0, c0.shape[-1]), np.float32)
    return out


def config3_b32_golden(frames=125):
    """configs[2]: B = 32, temperature 0.8, top-k 50 (the oracle's restatement of the engine's counter-based
    RNG), all 125 frames; the Mimi oracle's streaming decode_step of every frame: per (utterance, frame) RMS,
    mean and B32_PROJ projections on seeded unit vectors, and whole chunks: utterance 0's first 8 and
    each ending utterance's last 4 before its EOS."""
    from csm_mlx.weights import synthetic_mimi_weights
    codes, n, _, _ = _b32_run(frames, 0.8, 50, keep_logits=False)
    print("n_frames", n.tolist(), flush=True)
    m = MIMI_CONFIGURATION["mimi_202407"]
    om = OracleMimi(m, synthetic_mimi_weights(m, 0))
    om.reset_state()
    vec = np.random.default_rng(5).standard_normal((B32_PROJ, 1920))
    vec /= np.linalg.norm(vec, axis=1, keepdims=True)
    keep = [0] + [b for b in range(32) if n[b] < frames]
    rms, mean, proj = [], [], []
    pcm = {b: [] for b in keep}
    for f in range(frames):
        y = om.decode_step(np.ascontiguousarray(codes[:, f, :, None]), window=12)[:, 0].astype(np.float64)  # (32, 1920)
        rms.append(np.sqrt(np.mean(y ** 2, axis=1)))
        mean.append(y.mean(axis=1))
        proj.append(y @ vec.T)
        for b in keep:
            if f < n[b]:
                pcm[b].append(y[b].astype(np.float32))
        print("mimi frame", f, flush=True)
    out = dict(codes=codes, n_frames=n, rms=np.stack(rms, 1), mean=np.stack(mean, 1), proj=np.stack(proj, 1),
               proj_vec=vec, pcm_utts=np.array(keep, np.int32))
    for b in keep:   # (size) utterance 0's first 8 chunks; an ending utterance's last 4 before its EOS
        st = 0 if b == 0 else max(0, len(pcm[b]) - 4)
        sl = pcm[b][:8] if b == 0 else pcm[b][st:]
        out[f"pcm_{b}"] = np.stack(sl) if sl else np.zeros((0, 1920), np.float32)
        out[f"pcm_start_{b}"] = np.array(st, np.int32)
    return out


C5_UTTS = tuple(range(8)) + tuple(range(56, 64))   # configs[4] utterances pinned at full length (of the GPU
#                     test's B = 64): both 32-row tiles of the 64-row int4 GEMMs
C5_LOGIT_FRAMES = (0, 64, 124)      # frames whose c0 / ci logits are kept, for the first and last pinned utterance
C5_CI = (1, 16, 31)
RVQ_TIE = 3e-6                      # RVQ margin (oracle vq_margin: gap / (|latent| |c1 - c2|)) below which a context
#                                     code is a near-tie: the fixture carries the oracle's other outcome (a variant
#                                     prompt) and its frames.  The oracle's own latents move by 1.2-1.4e-6 (relative)
#                                     between two BLAS call shapes (one segment vs 24 per call), so a margin this small
#                                     is decided by summation order, not by the codec
RVQ_LIST = 1e-5                     # context codes with a margin below this are listed in the fixture (report)


def config5_q4_contexts(utts=C5_UTTS):
    """configs[4]'s context codes for utterances `utts` (bench.py context_segments: 3 Segments, 5 s of
    bench.context_audio each) by the codec oracle, with every code's RVQ margin (OracleMimi.vq_margin).
    Returns codes (U, 3, 32, 63), margins (U, 3, 32, 63)."""
    import bench
    m = MIMI_CONFIGURATION["mimi_202407"]
    om = OracleMimi(m, synthetic_mimi_weights(m, 0))
    # one segment per encode call (a variant prompt re-encodes its segment alone: the same BLAS call shapes, so
    # the same latents bit for bit)
    pcm = np.stack([bench.context_audio(g, seg) for g in utts for seg in range(3)])[:, None]
    codes, mg = [], []
    for i in range(len(pcm)):
        c, mm = om.encode(pcm[i:i + 1], with_margins=True)
        codes.append(c)
        mg.append(mm)
    print("encoded", len(pcm), "segments", flush=True)
    U = len(utts)
    codes = np.concatenate(codes).reshape(U, 3, 32, -1)
    return codes, np.concatenate(mg).reshape(U, 3, 32, -1), om


def config5_q4_prompt(g, seg_codes):
    """One configs[4] prompt (bench.py context_prompts): per context Segment the text row of 12 ids (speaker
    seg % 2) and its audio frames (tokenize_audio: codes + the EOS zero frame), then the utterance's text."""
    from bench import prompt_ids
    from csm_mlx.tokenizers import audio_codes_to_frames, tokenize_text_segment
    parts = []
    for seg in range(3):
        parts.append(tokenize_text_segment(prompt_ids(10_000 + 10 * g + seg), seg % 2, 32))
        parts.append(audio_codes_to_frames(seg_codes[seg]))
    parts.append(tokenize_text_segment(prompt_ids(g), 0, 32))
    return np.concatenate([t for t, _ in parts]).astype(np.int32), np.concatenate([mm for _, mm in parts])


def _margins(ref):
    """The oracle's top-2 logit margin of every code, relative to max|logit| (U, F, 32): where it is at fp32
    resolution (~1e-7) another summation order may pick the other code."""
    F = max(r[0].shape[0] for r in ref)
    margin = np.ones((len(ref), F, 32), np.float32)
    for b, r in enumerate(ref):
        for f in range(r[0].shape[0]):
            lg = [r[1][f][0]] + [r[1][f][1][k] for k in range(31)]
            for k, l in enumerate(lg):
                top = np.sort(l)[-2:]
                margin[b, f, k] = (top[1] - top[0]) / max(float(np.abs(l).max()), 1e-30)
    return margin


def config5_q4_golden(utts=C5_UTTS, frames=125):
    """configs[4] at full length for 16 of its 64 utterances (0-7 and 56-63: both 32-row tiles of the batched
    int4 GEMMs): int4 group-64 weights (nn.quantize of the seed-0 weights; the oracle on the dequantized weights),
    the Mimi-encoded 3-segment contexts (248 rows), 125 greedy frames.  Stored: the prompts, the context codes'
    RVQ near-ties (margin < RVQ_LIST: utterance, segment, codebook, frame, margin), codes, frame counts, every
    code's top-2 logit margin, c0 / ci logit slices at C5_LOGIT_FRAMES for the first and last utterance; and for
    every context code with an RVQ margin below RVQ_TIE the oracle's OTHER outcome -- the runner-up code there, the
    residual chain continued from it (OracleMimi.encode force=) -- as a variant prompt with its own 125 frames and
    margins, so a GPU encode that takes the other side of such a tie is still checked frame for frame."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import csm_weights, oracle_batch, oracle_for
    import bench
    ctx, cmg, om = config5_q4_contexts(utts)
    prompts = [config5_q4_prompt(g, ctx[u]) for u, g in enumerate(utts)]
    near = np.argwhere(cmg < RVQ_LIST)
    ties = [tuple(int(v) for v in x) for x in np.argwhere(cmg < RVQ_TIE)]           # (u, seg, k, t)
    print("context codes below RVQ_LIST:", len(near), "below RVQ_TIE:", ties, flush=True)
    var_prompts, var_meta = [], []
    for (u, seg, k, t) in ties:
        g = utts[u]
        vc = om.encode(bench.context_audio(g, seg)[None, None], force=[(0, k, t)])[0]
        assert (vc != ctx[u, seg]).any(), "the forced runner-up changed nothing"
        sc = [ctx[u, s] if s != seg else vc for s in range(3)]
        var_prompts.append(config5_q4_prompt(g, sc))
        var_meta.append((u, seg, k, t))
    args, w = csm_weights("1b")
    o = oracle_for(args, w, q4=True)
    ref = oracle_batch(o, prompts + var_prompts, frames, collect_logits=True)
    n = np.array([r[0].shape[0] for r in ref], np.int32)
    print("n_frames", n.tolist(), flush=True)
    codes = np.zeros((len(ref), frames, 32), np.int32)
    for b, r in enumerate(ref):
        codes[b, :n[b]] = r[0]
    margin = _margins(ref)
    U = len(utts)
    print("codes with a relative top-2 margin < 1e-5:", [tuple(int(v) for v in x) for x in np.argwhere(margin < 1e-5)],
          flush=True)
    keep = [0, U - 1]
    c0 = np.stack([[ref[b][1][f][0] for f in C5_LOGIT_FRAMES] for b in keep])                     # (2, 3, V)
    ci = np.stack([[ref[b][1][f][1][[c - 1 for c in C5_CI]] for f in C5_LOGIT_FRAMES] for b in keep])  # (2, 3, 3, V)
    nv = len(var_prompts)
    return dict(utts=np.array(utts, np.int32), codes=codes[:U], n_frames=n[:U],
                tokens=np.stack([t for t, _ in prompts]), masks=np.stack([m for _, m in prompts]),
                logit_utts=np.array(keep, np.int32), frames=np.array(C5_LOGIT_FRAMES), ci_codebooks=np.array(C5_CI),
                c0=c0, ci=ci, margin=margin[:U],
                rvq_near=near.astype(np.int32).reshape(-1, 4),
                rvq_near_margin=cmg[tuple(near.T)].astype(np.float64) if len(near) else np.zeros(0),
                rvq_tie=np.array(RVQ_TIE), var_of=np.array(var_meta, np.int32).reshape(nv, 4),
                var_margin=np.array([cmg[x] for x in var_meta], np.float64),
                var_tokens=np.stack([t for t, _ in var_prompts]) if nv else np.zeros((0,) + prompts[0][0].shape, np.int32),
                var_codes=codes[U:], var_n_frames=n[U:], var_frame_margin=margin[U:])


def csm_1b_q4_stream_golden(frames=125):
    """The reference demo's path (run_streaming_csm_mlx.py:811-818, :844-852: nn.quantize(model, 64, 4), then
    stream_generate) at configs[1]'s utterance, greedy: csm_1b int4 g64 B = 1, 125 frames, the oracle on the
    dequantized weights; codes, every code's top-2 logit margin, c0 / ci logit slices at C5_LOGIT_FRAMES, and
    per frame the Mimi oracle's streaming decode_step chunk (RMS, mean, 4 projections; the first 8 and last 4
    chunks whole)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import csm_weights, oracle_for
    from csm_mlx.models import csm_1b  # noqa: F401
    args, w = csm_weights("1b")
    o = oracle_for(args, w, q4=True)
    codes, logs = o.generate_codes(*text_frame(CONFIG1_IDS, 32), frames, collect_logits=True)
    margin = _margins([(codes, logs)])[0]
    print("q4 B=1 codes", codes.shape, "margins < 1e-5:", [tuple(int(v) for v in x) for x in np.argwhere(margin < 1e-5)],
          flush=True)
    m = MIMI_CONFIGURATION["mimi_202407"]
    om = OracleMimi(m, synthetic_mimi_weights(m, 0))
    om.reset_state()
    vec = np.random.default_rng(5).standard_normal((B32_PROJ, 1920))
    vec /= np.linalg.norm(vec, axis=1, keepdims=True)
    rms, mean, proj, whole = [], [], [], {}
    F = codes.shape[0]
    for f in range(F):
        y = om.decode_step(np.ascontiguousarray(codes[None, f, :, None]), window=12)[0, 0].astype(np.float64)
        rms.append(np.sqrt(np.mean(y ** 2)))
        mean.append(y.mean())
        proj.append(y @ vec.T)
        if f < 8 or f >= F - 4:
            whole[f] = y.astype(np.float32)
    return dict(ids=np.array(CONFIG1_IDS, np.int32), codes=codes, margin=margin, frames=np.array(C5_LOGIT_FRAMES),
                ci_codebooks=np.array(C5_CI), c0=np.stack([logs[f][0] for f in C5_LOGIT_FRAMES]),
                ci=np.stack([logs[f][1][[c - 1 for c in C5_CI]] for f in C5_LOGIT_FRAMES]),
                rms=np.array(rms), mean=np.array(mean), proj=np.stack(proj), proj_vec=vec,
                pcm_frames=np.array(sorted(whole), np.int32), pcm=np.stack([whole[f] for f in sorted(whole)]))


FIXTURES = {
    "csm_tiny_oracle.npz": csm_golden,
    "mimi_tiny_oracle.npz": mimi_golden,
    "tiny_long_prompt.npz": tiny_long_golden,
    "csm_1b_greedy_125.npz": csm_1b_long_golden,
    "config0_plumbing.npz": config0_golden,
    "config4_b32_greedy_125.npz": config4_b32_golden,
    "config3_b32_stream_125.npz": config3_b32_golden,
    "config5_q4_b16_greedy_125.npz": config5_q4_golden,
    "csm_1b_q4_stream_125.npz": csm_1b_q4_stream_golden,
}

if __name__ == "__main__":
    # python tests/golden/make_golden.py [fixture ...]   (default: all; the csm_1b ones take minutes)
    for name in (sys.argv[1:] or list(FIXTURES)):
        np.savez_compressed(os.path.join(HERE, name), **FIXTURES[name]())
        print("wrote", name, flush=True)
