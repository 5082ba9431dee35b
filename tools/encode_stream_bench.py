#!/usr/bin/env python3
"""Streaming encode microbench: synchronous MimiCodec.encode_slots passes of n frames for B slots (synthetic
mimi_202407 weights, seeded audio), alone on the GPU -- the per-tick codec cost of a duplex serving loop's ingest
side, with the codec's kernel launches per pass (the host counter behind mimi_debug_read "launches").  Beside
them the one-shot encode of a 10 s clip at B = 1: the cost streaming takes off the turn boundary.
A pass of one frame has to stay under the 80 ms frame interval (12.5 Hz) for streaming to keep up.
usage: python tools/encode_stream_bench.py [calls]     (default 200 per shape, after a warm-up of every shape)"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csm-mlx_amd"), ROOT]
import numpy as np  # noqa: E402
from csm_mlx import _lib  # noqa: E402
from csm_mlx.config import MIMI_CONFIGURATION  # noqa: E402
from csm_mlx.mimi import MimiCodec  # noqa: E402
from csm_mlx.weights import synthetic_mimi_weights  # noqa: E402

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
SHAPES = [(1, 1), (1, 4), (32, 1), (32, 4)]
WARM = 5
m = MIMI_CONFIGURATION["mimi_202407"]
fs = m.frame_size
codec = MimiCodec(m, max_batch=32, max_frames=(CALLS + WARM) * 4 + 8)
codec.load_weights(synthetic_mimi_weights(m))
rng = np.random.default_rng(0)


def launches():
    v = ctypes.c_int64(0)
    _lib.check(_lib.lib().mimi_debug_read(codec._h, b"launches", ctypes.byref(v), 8, None))
    return v.value


def run(B, n, calls):
    pcm = rng.normal(0, 0.1, (B, n * fs)).astype(np.float32)
    for b in range(B):
        codec.encode_slot_reset(b)
    l0, t = launches(), []
    for _ in range(calls):
        t0 = time.perf_counter()
        codec.encode_slots(pcm)
        t.append(time.perf_counter() - t0)
    return np.array(t) * 1e3, (launches() - l0 - B) / calls    # (the B resets are launches too)


for B, n in SHAPES:
    run(B, n, WARM)
for B, n in SHAPES:
    t, per = run(B, n, CALLS)
    print(f"encode_slots B={B:2d} n={n}: median {np.median(t):7.3f} ms  mean {t.mean():7.3f}  p95 "
          f"{np.percentile(t, 95):7.3f}  ({np.median(t) / n:6.3f} ms per frame tick of 80 ms)  launches/pass {per:.1f}  "
          f"over {CALLS} calls", flush=True)
clip = rng.normal(0, 0.1, (1, 1, 10 * 24000)).astype(np.float32)
codec.encode(clip)
t = []
for _ in range(10):
    t0 = time.perf_counter()
    codec.encode(clip)
    t.append(time.perf_counter() - t0)
print(f"one-shot encode B=1 10 s clip: median {np.median(t) * 1e3:.3f} ms over 10 calls", flush=True)
