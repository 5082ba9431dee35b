"""The sequence of C calls the Python package makes, per entry point: a record to compare two versions of the
package against one library.

The object ``_lib.lib()`` returns is wrapped in a proxy that logs every call -- the function name, its scalar
arguments, and for array arguments (what ``_lib.ptr`` was given) the dtype and shape.  csm_tiny with the
seeded synthetic weights of the EOS rig (tests/helpers.py) and the tiny Mimi codec; per scenario the trace and
a SHA-256 of everything the call returned (codes, PCM, logits, losses).

  usage: abi_trace.py [directory that holds the csm_mlx package; default this tree's csm-mlx_amd]

Run it once per package version, each in a fresh process, with ``CSM_HIP_LIB`` naming the same library, and
``diff`` the two outputs (profiles/host_fold_trace.txt)."""
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "csm-mlx_amd")
sys.path[:0] = [PKG, os.path.join(ROOT, "tests"), ROOT]

import numpy as np  # noqa: E402

import csm_mlx  # noqa: E402
from csm_mlx import _lib, batching, generation, scoring  # noqa: E402
from csm_mlx.config import MIMI_CONFIGURATION  # noqa: E402
from csm_mlx.mimi import MimiCodec  # noqa: E402
from csm_mlx.models import CSM, csm_tiny  # noqa: E402
from csm_mlx.sampling import make_logits_processors  # noqa: E402
from csm_mlx.tokenizers import set_audio_tokenizer, tokenize_text_segment  # noqa: E402
from csm_mlx.weights import synthetic_csm_weights, synthetic_mimi_weights  # noqa: E402
from helpers import eos_rig  # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(csm_mlx.__file__))) == PKG, csm_mlx.__file__
TRACE = None        # the open scenario's lines


class ArrayPtr(ctypes.c_void_p):
    """What ``_lib.ptr`` hands out while tracing: the pointer, and what it points to."""


def traced_ptr(a):
    p = ArrayPtr(a.ctypes.data)
    p.what = f"{a.dtype}{list(a.shape)}"
    return p


def show(a):
    if isinstance(a, ArrayPtr):
        return a.what
    if isinstance(a, ctypes.c_void_p):
        return "handle"
    if isinstance(a, ctypes.Array):
        return f"{a._type_.__name__}[{len(a)}]"
    if isinstance(a, ctypes._SimpleCData):
        return f"{type(a).__name__}({a.value})"
    if a is None or isinstance(a, (int, float, bytes)):
        return repr(a)
    return "byref"                                   # (its repr holds an address)


class TracedLib:
    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            if TRACE is not None:
                TRACE.append(f"  {name}({', '.join(show(a) for a in args)})")
            return fn(*args)
        return call


def digest(x, h=None):
    h = hashlib.sha256() if h is None else h
    if isinstance(x, (list, tuple)):
        h.update(f"[{len(x)}]".encode())
        for y in x:
            digest(y, h)
    elif x is None or isinstance(x, (bool, int)):
        h.update(repr(x).encode())
    else:
        a = np.ascontiguousarray(x)
        h.update(f"{a.dtype}{list(a.shape)}".encode() + a.tobytes())
    return h


def scenario(name, fn):
    global TRACE
    TRACE = []
    out = fn()
    lines, TRACE = TRACE, None
    print(f"== {name}: {len(lines)} calls")
    print("\n".join(lines))
    print(f"  sha256 {digest(out).hexdigest()}", flush=True)


args = csm_tiny()
K = args.n_audio_codebooks
model = CSM(args, dtype="float32", max_batch=4, max_frames=64)
model.load_weights(eos_rig(args, synthetic_csm_weights(args, 0)))
mm = MIMI_CONFIGURATION["tiny"]
codec = MimiCodec(mm, max_batch=4, max_frames=64)
codec.load_weights(synthetic_mimi_weights(mm))
set_audio_tokenizer(codec, K)
model.engine                                          # created before the first trace
_lib._lib = TracedLib(_lib.lib())
_lib.ptr = traced_ptr

IDS = [[998, 12, 34, 56, 999], [998, 7, 8, 999], [998, 3, 1, 4, 1, 5, 999], [998, 2, 7, 1, 999], [998, 9, 999]]
PROMPTS = [tokenize_text_segment(ids, 0, K) for ids in IDS]
MS = 6 * 80


def plain_processor(tokens, logits):
    out = np.array(logits, np.float32, copy=True)
    out[:, 1] += 0.5 + 0.25 * len(tokens)
    return out


def callable_sampler(logits):
    return np.asarray(logits).argmax(-1)


def device_list():
    return make_logits_processors(logit_bias={3: -2.0, 7: 1.5}, repetition_penalty=1.3, repetition_context_size=4)


MODES = {"plain": dict(temperature=0.8, seed=5),
         "host processor": dict(temperature=0.8, seed=5, logits_processors=[plain_processor]),
         "host sampler": dict(sampler=callable_sampler, logits_processors=[plain_processor])}

scenario("generate greedy", lambda: csm_mlx.generate(model, IDS[0], 0, [], MS, temperature=0.0))
scenario("generate sampled", lambda: csm_mlx.generate(model, IDS[0], 0, [], MS, temperature=0.8, seed=7))
scenario("generate make_logits_processors",
         lambda: csm_mlx.generate(model, IDS[0], 0, [], MS, temperature=0.8, seed=7, logits_processors=device_list()))
scenario("generate callable processor",
         lambda: csm_mlx.generate(model, IDS[0], 0, [], MS, temperature=0.8, seed=7,
                                  logits_processors=[plain_processor]))
scenario("generate callable sampler", lambda: csm_mlx.generate(model, IDS[0], 0, [], MS, sampler=callable_sampler))
scenario("generate_batch B=3", lambda: csm_mlx.generate_batch(model, PROMPTS[:3], MS, temperature=0.8, top_k=5,
                                                              seeds=[1, 2, 3], with_codes=True))
for mode, kw in MODES.items():
    scenario(f"stream_generate {mode}", lambda: list(csm_mlx.stream_generate(model, IDS[1], 0, [], MS, **kw)))
for B in (1, 3):
    scenario(f"stream_generate_batch B={B}",
             lambda: list(generation.stream_generate_batch(model, PROMPTS[:B], MS, temperature=0.8, top_k=5,
                                                           seeds=list(range(B)))))


def frames_on_a_kept_cache(temperature=0.8, seed=None, sampler=None, logits_processors=None):
    cache = generation.make_frame_cache(model, 1, temperature=temperature, sampler=sampler, seed=seed)
    hist, out = [], []
    tokens, mask = PROMPTS[0][0][None], PROMPTS[0][1][None]
    for _ in range(3):
        codes = csm_mlx.generate_frame(model, tokens, temperature=temperature, token_mask=mask, cache=cache,
                                       logits_processors=logits_processors, c0_history=hist, sampler=sampler)
        out.append(codes)
        tokens = np.concatenate([codes, np.zeros((1, 1), np.int32)], 1)[:, None, :]
        mask = np.concatenate([np.ones((1, K), bool), np.zeros((1, 1), bool)], 1)[:, None, :]
    return out + hist


for mode, kw in MODES.items():
    scenario(f"generate_frame {mode}", lambda: frames_on_a_kept_cache(**kw))
scenario("generate_frame plain, no c0_history",
         lambda: [csm_mlx.generate_frame(model, PROMPTS[0][0][None], temperature=0.0, seed=0)])

CAPS = [5, 0, 7, 2, 4]
scenario("generate_queue", lambda: csm_mlx.generate_queue(model, PROMPTS, slots=2, temperature=0.8, top_k=5, seeds=11,
                                                          max_audio_frames=CAPS, chunk=3, with_codes=True))
scenario("stream_generate_queue",
         lambda: [list(ev) for ev in csm_mlx.stream_generate_queue(model, PROMPTS, slots=2, temperature=0.8, top_k=5,
                                                                   seeds=11, max_audio_frames=CAPS, chunk=3)])

rng = np.random.default_rng(3)
FORCED = [rng.integers(0, args.n_audio_vocab, (n, K)).astype(np.int32) for n in (4, 2)]
scenario("score_frames logits", lambda: scoring.score_frames(model, PROMPTS[:2], FORCED))
scenario("score_frames cross entropy", lambda: scoring.score_frames(model, PROMPTS[:2], FORCED, logits=False))


def loss_batch():
    """Two utterances: (text, audio, text, audio), whose text rows after the first scored row send it through
    ``_score_utterance``, and (text, audio), which takes the batched path."""
    def audio(n):
        t = np.zeros((n + 1, K + 1), np.int32)
        t[:n, :K] = rng.integers(1, args.n_audio_vocab, (n, K))
        m = np.zeros((n + 1, K + 1), bool)
        m[:, :K] = True
        return t, m
    utts = []
    for spec in ([(0, 3), (1, 2)], [(0, 4)]):
        parts = [p for i, (spk, n) in enumerate(spec) for p in (tokenize_text_segment(IDS[i], spk, K), audio(n))]
        utts.append((np.concatenate([t for t, _ in parts]), np.concatenate([m for _, m in parts])))
    S = max(len(t) for t, _ in utts)
    T, M = np.zeros((2, S, K + 1), np.int32), np.zeros((2, S, K + 1), bool)
    for b, (t, m) in enumerate(utts):
        T[b, : len(t)], M[b, : len(t)] = t, m
    return {"tokens": T, "masks": M, "loss_masks": M.copy(), "first_codebook_weight_multiplier": 1.5}


BATCH = loss_batch()
assert scoring._split(BATCH["tokens"], BATCH["masks"], BATCH["loss_masks"], K)[1] == [False, True]
scenario("compute_loss", lambda: scoring.compute_loss(model, BATCH, per_sample=True))
scenario("compute_loss cause_mismatch", lambda: scoring.compute_loss(model, BATCH, cause_mismatch=True))
