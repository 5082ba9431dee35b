"""A SHA-256 per execution path of the depth decoder's attention: a record to compare two builds of the
library bit for bit.

csm_1b with synthetic weights (tests/helpers.py), two frames per case (one frame runs every decoder position
0..31: n = 1 and 2, the 16 / 17 boundary of the key halves, n = 32); per case the digest covers the codes and
the h_last / c0_logits / ci_logits taps of every frame.  The cases switch the engine's options so that
attn_short_kernel (with and without the layer-0 table gather, with split outputs and half-group sums),
dec_frame's phase_attn and dec_step_xs's role_a (one and two row tiles) each run; csrc/attn32.h holds the
arithmetic they share.

  usage: path_digest.py

Run it once per library, each in a fresh process (``CSM_HIP_LIB`` names the other build), twice on one
library first (a case whose two digests differ is not deterministic), and ``diff`` the outputs
(profiles/attn_fold_digest.txt)."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csm-mlx_amd"), os.path.join(ROOT, "tests"), ROOT]

import numpy as np  # noqa: E402

from csm_mlx.sampling import Sampler  # noqa: E402
from csm_mlx.tokenizers import tokenize_text_segment  # noqa: E402
from helpers import prompt_ids  # noqa: E402
from rigs import TAP_NAMES, build_model, epoch, frame_taps, set_option, synchronize  # noqa: E402

FRAMES = 2
KERNELS = ("dec_frame", "dec_xsd", "bb_step")
GREEDY, SAMPLED = (0.0, 0), (0.8, 50)
LAUNCHES = ("dec_frame", "bb_step")
# (dtype, B, sampler, options switched off)
CASES = [(d, 1, GREEDY, off) for d in ("bf16", "q4") for off in ((), LAUNCHES, LAUNCHES + ("qkv0_tab",))]
CASES += [("bf16", 1, SAMPLED, ())]
CASES += [(d, 8, GREEDY, off) for d in ("bf16", "q4") for off in ((), ("dec_xsd",), ("dec_xsd", "gemm_xs"))]
CASES += [("q4", 40, GREEDY, ())]


def prompts(B):
    return [tokenize_text_segment(prompt_ids(3000 + 97 * B + b, 10 + b % 3), 0, 32) for b in range(B)]


def run(model, B, sampler, off):
    """-> (the persistent kernels' hand-off counts over the case: which of them ran, the digest)"""
    for name in off:
        set_option(model, name, 0)
    try:
        e0 = [epoch(model, k) for k in KERNELS]
        hist, n, taps = frame_taps(model, prompts(B), FRAMES, Sampler(*sampler), list(range(B)), TAP_NAMES)
        synchronize(model)
        ran = " ".join(f"{k}+{epoch(model, k) - e}" for k, e in zip(KERNELS, e0))
    finally:
        for name in off:
            set_option(model, name, 1)
    assert hist.shape[0] == FRAMES and (n == FRAMES).all(), "an utterance ended inside the window"
    h = hashlib.sha256()
    for a in (hist, *(taps[t] for t in TAP_NAMES)):
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype}{list(a.shape)}".encode() + a.tobytes())
    return ran, h.hexdigest()


for dtype, max_batch in (("bf16", 32), ("q4", 64)):
    model = build_model("1b", dtype, max_batch)[2]
    for d, B, sampler, off in CASES:
        if d == dtype:
            kind = "greedy" if sampler == GREEDY else "sampled %g / top-k %d" % sampler
            ran, sha = run(model, B, sampler, off)
            print(f"{dtype} B={B} {kind} off={','.join(off) or '-'} ({ran}): {sha}", flush=True)
    del model
