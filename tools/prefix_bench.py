"""Shared context prefixes against whole-prompt prefills (csm_mlx.prefix, csrc/csm_engine_prefix.hip): csm_1b bf16
synthetic weights, a 248-row context (config 5's context length) in front of 14 text rows, greedy.  Both ways run
in this one process, alternating, after a warm-up; medians with the spread (min .. max).

  (a) join cost    32 slots restarted at one boundary: csm_slot_restart x 32 .. the end of the prefill, synchronized.
                   whole: one csm_prefill_batch of 32 x 262 rows (the code path without prefixes, unchanged);
                   prefix: one csm_prefix_load of the shared context into 32 slots + csm_prefill_batch of 32 x 14 rows
  (b) queue        generate_queue, 96 such utterances through 32 slots, caps seeded uniform 12..125: useful frames/s
  (c) first frame  B = 1, from the call to the first frame's codes, the context as three Segments with audio
                   (mimi_202407, synthetic weights): whole = build_prompt (three Mimi encodes) + prefill of every row
                   + one frame; prefix = cache_context once (not timed), then text rows + load + prefill + one frame
  (d) copy         the copy kernel alone (csm_bench_prefix_load, HIP events) at 248 and 2046 rows: bytes read +
                   written / time, against the MI355X's 8 TB/s HBM peak

usage: prefix_bench.py [repeats of (a), default 24]   Every step runs under its own time limit; a step that
exceeds it ends the process (nothing more is started on the GPU)."""
import ctypes
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csm-mlx_amd"), ROOT]

import numpy as np  # noqa: E402

from csm_mlx import Segment, _lib, cache_context, generate_queue  # noqa: E402
from csm_mlx.batching import _EngineSlots  # noqa: E402
from csm_mlx.generation import FrameCache, build_prompt, generate_codes_batch  # noqa: E402
from csm_mlx.models import CSM, csm_1b  # noqa: E402
from csm_mlx.sampling import Sampler  # noqa: E402
from csm_mlx.tokenizers import tokenize_text_segment  # noqa: E402
from csm_mlx.weights import bf16_bits, synthetic_csm_weights  # noqa: E402

SLOTS, N, CTX, TEXT = 32, 96, 248, 14
REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 24
GREEDY = Sampler(0.0, 0)


def step(name, seconds, fn):
    def late(*_):
        print(f"{name}: over its {seconds} s limit -- ending here", flush=True)
        os._exit(124)
    signal.signal(signal.SIGALRM, late)
    signal.alarm(seconds)
    t = time.perf_counter()
    out = fn()
    signal.alarm(0)
    print(f"[{name}: {time.perf_counter() - t:.1f} s]", flush=True)
    return out


def spread(ms):
    a = np.asarray(ms)
    return f"median {np.median(a):8.3f}  min {a.min():8.3f}  max {a.max():8.3f}  (n = {len(a)})"


def text_rows(i):
    ids = [128000] + [int(x) for x in np.random.default_rng(1000 + i).integers(0, 128000, TEXT - 2)] + [128001]
    return ids, tokenize_text_segment(ids, 0, 32)


def context_rows():
    """248 rows laid out as three segments: 3 text rows + 79 audio rows + the segment's zero frame each, one short."""
    rng = np.random.default_rng(5)
    t = np.zeros((CTX, 33), np.int32)
    m = np.zeros((CTX, 33), bool)
    r = 0
    for s, n_audio in enumerate((80, 80, 79)):
        t[r:r + 3, 32] = rng.integers(0, 128000, 3)
        m[r:r + 3, 32] = True
        r += 3
        t[r:r + n_audio - 1, :32] = rng.integers(1, 2048, (n_audio - 1, 32))
        m[r:r + n_audio, :32] = True
        r += n_audio
    assert r == CTX
    return t, m


def long_rows(rows):
    rng = np.random.default_rng(rows)
    t = np.zeros((rows, 33), np.int32)
    m = np.zeros((rows, 33), bool)
    t[:, 32] = rng.integers(0, 128000, rows)
    m[:, 32] = True
    return t, m


def sync(model):
    _lib.check(_lib.lib().csm_synchronize(model.engine))


def main():
    args = csm_1b()
    model = CSM(args, dtype="bf16", max_batch=SLOTS)
    step("load", 300, lambda: model.load_weights({k: bf16_bits(v) for k, v in synthetic_csm_weights(args, 0).items()}))
    ctx = context_rows()
    texts = [text_rows(i) for i in range(N)]
    whole = [(np.concatenate([ctx[0], t]), np.concatenate([ctx[1], m])) for _, (t, m) in texts]
    prefix = step("cache_context (248 rows)", 120, lambda: cache_context(model, ctx))
    print(f"context {prefix.rows} rows = {prefix.nbytes / 1e6:.1f} MB of K / V; {TEXT} text rows; {SLOTS} slots", flush=True)

    # ---------------------------------------------------------------- (a)
    def join_cost():
        eng = _EngineSlots(model, SLOTS, GREEDY, None)
        out = {"whole": [], "prefix": []}

        def boundary(way):
            sync(model)
            t = time.perf_counter()
            for b in range(SLOTS):
                eng.restart(b, b)
            if way == "prefix":
                eng.load_prefix([(b, prefix) for b in range(SLOTS)])
                eng.prefill([(b, *texts[b][1]) for b in range(SLOTS)])
            else:
                eng.prefill([(b, *whole[b]) for b in range(SLOTS)])
            sync(model)
            return (time.perf_counter() - t) * 1e3
        for way in ("whole", "prefix", "whole", "prefix"):                 # warm-up
            boundary(way)
        for _ in range(REPEATS):
            for way in ("whole", "prefix"):
                out[way].append(boundary(way))
        for way in out:
            print(f"(a) join boundary, {SLOTS} joins, {way:6s}: ms {spread(out[way])}", flush=True)
        print(f"(a) prefix / whole (medians): {np.median(out['prefix']) / np.median(out['whole']):.3f}", flush=True)
    step("(a)", 240, join_cost)

    # ---------------------------------------------------------------- (b)
    caps = [int(c) for c in np.random.default_rng(7).integers(12, 126, N)]
    useful = sum(caps)

    def queue():
        ref = None
        runs = {"whole": [], "prefix": []}
        generate_queue(model, whole[:SLOTS], slots=SLOTS, max_audio_frames=[4] * SLOTS, decode=False)     # warm-up
        generate_queue(model, [t for _, t in texts[:SLOTS]], slots=SLOTS, max_audio_frames=[4] * SLOTS, decode=False,
                       prefixes=[prefix] * SLOTS)
        for r in range(3):
            for way in ("whole", "prefix"):
                t = time.perf_counter()
                if way == "whole":
                    codes = generate_queue(model, whole, slots=SLOTS, max_audio_frames=caps, decode=False)
                else:
                    codes = generate_queue(model, [t_ for _, t_ in texts], slots=SLOTS, max_audio_frames=caps, decode=False,
                                           prefixes=[prefix] * N)
                dt = time.perf_counter() - t
                assert [len(c) for c in codes] == caps
                ref = codes if ref is None else ref
                same = sum(np.array_equal(a, b) for a, b in zip(codes, ref))
                runs[way].append(useful / dt)
                print(f"(b) generate_queue {way:6s} run {r}: {useful / dt:8.1f} useful frames/s  {dt:6.3f} s  "
                      f"utterances with the first run's codes: {same} / {N}", flush=True)
        for way in runs:
            print(f"(b) {way:6s}: useful frames/s {spread(runs[way])}", flush=True)
    step("(b)", 300, queue)

    # ---------------------------------------------------------------- (c)
    def first_frame():
        from csm_mlx.config import MIMI_CONFIGURATION
        from csm_mlx.mimi import MimiCodec
        from csm_mlx.tokenizers import set_audio_tokenizer
        from csm_mlx.weights import synthetic_mimi_weights
        mm = MIMI_CONFIGURATION["mimi_202407"]
        codec = MimiCodec(mm, max_batch=1, max_frames=128)
        codec.load_weights(synthetic_mimi_weights(mm))
        set_audio_tokenizer(codec, 32)
        rng = np.random.default_rng(11)
        tt = np.arange(int(6.32 * 24000)) / 24000.0
        segs = [Segment(s % 2, [128000, 100 + s, 128001],
                        audio=(0.1 * np.sin(2 * np.pi * (150 + 40 * s) * tt) + rng.normal(0, 0.01, len(tt))).astype(np.float32))
                for s in range(3)]
        pre = cache_context(model, segs)
        print(f"(c) three Segments -> {pre.rows} context rows", flush=True)
        out = {"whole": [], "prefix": []}

        def one(way, i):
            ids = texts[i][0]
            sync(model)
            t = time.perf_counter()
            ctxt = segs if way == "whole" else pre
            prompt = build_prompt(model, ids, 0, ctxt)
            hist, n, _ = generate_codes_batch(model, [prompt], 1, sampler=GREEDY, seeds=[0],
                                              prefixes=None if way == "whole" else [pre])
            return (time.perf_counter() - t) * 1e3, hist[0, 0].copy()
        for way in ("whole", "prefix"):
            one(way, 0)
        for i in range(10):
            a, ca = one("whole", i)
            b, cb = one("prefix", i)
            out["whole"].append(a)
            out["prefix"].append(b)
            assert np.array_equal(ca, cb), i
        for way in out:
            print(f"(c) B = 1 call -> first frame's codes, {way:6s}: ms {spread(out[way])}", flush=True)
    step("(c)", 240, first_frame)

    # ---------------------------------------------------------------- (d)
    def copy_bandwidth():
        for rows in (CTX, 2046):
            if rows == CTX:
                p = prefix
            else:
                p = cache_context(model, long_rows(rows))
            res = []
            for _ in range(5):
                FrameCache(model, 1, GREEDY, [0])                          # csm_begin: utterance 0 is empty again
                us, nb = ctypes.c_float(0), ctypes.c_double(0)
                _lib.check(_lib.lib().csm_bench_prefix_load(model.engine, 0, p.handle, 50, ctypes.byref(us), ctypes.byref(nb)))
                res.append(us.value)
            med = float(np.median(res))
            print(f"(d) copy kernel, {rows:4d} rows ({p.nbytes / 1e6:6.1f} MB read + written = {nb.value / 1e6:6.1f} MB): us "
                  f"{spread(res)}  -> {nb.value / med / 1e6:6.2f} TB/s = {nb.value / med / 1e6 / 8 * 100:4.1f} % of 8 TB/s", flush=True)
    step("(d)", 240, copy_bandwidth)


if __name__ == "__main__":
    main()
