"""``MimiCodec`` -- the GPU Mimi codec (drop-in for moshi_mlx ``Mimi`` as the reference uses it).

Methods mirror the calls the reference makes (/root/reference/csm_mlx/tokenizers.py:16-19, 70,
150; generation.py:225, 251, 258): ``load_pytorch_weights``, ``encode``, ``decode``,
``decode_step``, ``reset_state``.  All compute runs in libcsm_hip.so (mimi_* C ABI); codec
weights are kept in fp32 (waveform parity target 1e-4 RMS).
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Iterable, Optional, Tuple, Union

import numpy as np

from . import _lib
from .config import MimiArgs
from .rope import mimi_rope_table


def _dims(m: MimiArgs) -> _lib.MimiDims:
    r = (ctypes.c_int * 8)(*list(m.ratios) + [0] * (8 - len(m.ratios)))
    return _lib.MimiDims(m.channels, m.dimension, m.n_filters, len(m.ratios), r, m.kernel_size,
                         m.residual_kernel_size, m.last_kernel_size, m.compress, m.num_heads, m.num_layers,
                         m.dim_feedforward, m.context, m.n_q, m.bins, m.codebook_dim, m.downsample_stride,
                         m.norm_eps, 1 if m.gelu == "erf" else 0, 0 if m.attn_mode == "mlx" else 1)


_SLOTS = "slots"    # MimiCodec._stream in slot mode (slot_reset)


class MimiCodec:
    def __init__(self, m: MimiArgs, *, device: Optional[int] = None, max_batch: int = 1, max_frames: int = 1200):
        from .models import default_device
        self.m = m
        self.device = default_device() if device is None else device
        self.max_batch = max_batch
        self.max_frames = max_frames
        L = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(L.mimi_create(ctypes.byref(_dims(m)), self.device, max_batch, max_frames, ctypes.byref(h)))
        self._h = h
        n_pos = 2 * max_frames * m.downsample_stride + 64
        t = mimi_rope_table(m, n_pos)
        _lib.check(L.mimi_set_rope_table(h, _lib.ptr(t), t.shape[0], t.shape[1] * 2))
        self._stream = None    # the streaming state: None, the batch size of a decode_step stream, or _SLOTS
        self._enc_stream = None    # the batch size of the encode_step streams (rows 0..B-1 of the encode slots)

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None:
                _lib.lib().mimi_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def load_weights(self, weights: Union[Dict[str, np.ndarray], Iterable[Tuple[str, np.ndarray]]], strict=True):
        L = _lib.lib()
        items = weights.items() if isinstance(weights, dict) else weights
        for name, arr in items:
            a, dt = _lib.host_tensor(arr)
            rc = L.mimi_load_tensor(self._h, name.encode(), _lib.ptr(a), dt, _lib.shape_arr(a.shape), a.ndim)
            if rc != 0 and not strict:
                continue
            _lib.check(rc)
        if strict:
            _lib.check(L.mimi_weights_ready(self._h))
        return self

    def load_pytorch_weights(self, path: str):
        """Kyutai PyTorch checkpoint (safetensors), as moshi_mlx ``Mimi.load_pytorch_weights``
        (tokenizers.py:19).  Weight-normalised convs (weight_g / weight_v) are folded to plain
        weights, ``in_projs.0`` / ``out_projs.0`` spellings are aliased, unknown keys ignored."""
        from safetensors import safe_open
        raw = {}
        with safe_open(path, framework="pt") as f:
            for k in f.keys():
                raw[k] = f.get_tensor(k).float().numpy()
        out = {}
        for k, v in raw.items():
            if k.endswith(".weight_g"):
                continue
            if k.endswith(".weight_v"):
                g = raw[k[:-1] + "g"]
                norm = np.sqrt((v.astype(np.float64) ** 2).sum(axis=tuple(range(1, v.ndim)), keepdims=True))
                k, v = k[:-2], (g * v / norm).astype(np.float32)
            k = k.replace(".self_attn.in_projs.0.weight", ".self_attn.in_proj_weight")
            k = k.replace(".self_attn.out_projs.0.weight", ".self_attn.out_proj.weight")
            out[k] = v
        self.load_weights(out, strict=False)
        _lib.check(_lib.lib().mimi_weights_ready(self._h))
        return self

    # ------------------------------------------------------------------ codec
    def encode(self, pcm: np.ndarray) -> np.ndarray:
        """(B, 1, N) or (B, N) float32 -> (B, n_q, Tf) int32."""
        x = np.asarray(pcm, np.float32)
        if x.ndim == 3:
            x = x[:, 0, :]
        B, N = x.shape

        def part(b0, nb, codes, got):
            xb = np.ascontiguousarray(x[b0: b0 + nb])
            return _lib.lib().mimi_encode(self._h, nb, N, _lib.ptr(xb), codes, got)
        return self._encode_chunks(B, N, part)

    def _encode_chunks(self, B: int, N: int, part) -> np.ndarray:
        """The loop of both encodes: B clips of N samples in chunks of <= ``max_batch`` rows, each through
        ``part(first row, rows, codes pointer, frame count pointer)``, its codes trimmed to the frames the
        library reports."""
        Tf = int(np.ceil(N / self.m.frame_size)) + 2
        out = []
        for b0 in range(0, B, self.max_batch):
            nb = min(self.max_batch, B - b0)
            codes = np.zeros((nb, self.m.n_q, Tf), np.int32)
            got = ctypes.c_int(0)
            _lib.check(part(b0, nb, _lib.ptr(codes), ctypes.byref(got)))
            out.append(codes.reshape(-1)[: nb * self.m.n_q * got.value].reshape(nb, self.m.n_q, got.value))
        return np.concatenate(out, 0)

    def encode_rows(self, rows) -> np.ndarray:
        """Same-length 1-D float32 clips -> (B, n_q, Tf) int32, as ``encode(np.stack(rows))`` without the
        stacking copy (each clip is uploaded into its slot: mimi_encode_rows)."""
        xs = [np.ascontiguousarray(r, np.float32).reshape(-1) for r in rows]
        if not xs or len({x.shape[0] for x in xs}) != 1:
            raise ValueError("encode_rows: same-length clips only")
        N = xs[0].shape[0]

        def part(b0, nb, codes, got):
            ptrs = (ctypes.c_void_p * nb)(*[x.ctypes.data for x in xs[b0: b0 + nb]])
            return _lib.lib().mimi_encode_rows(self._h, nb, N, None, ptrs, codes, got)
        return self._encode_chunks(len(xs), N, part)

    def decode(self, codes: np.ndarray) -> np.ndarray:
        """(B, n_q, F) int32 -> (B, 1, F*frame_size) float32.  Resets streaming state (moshi_mlx)."""
        c = np.asarray(codes, np.int32)
        B, K, F = c.shape
        if K != self.m.n_q:
            raise ValueError(f"expected {self.m.n_q} codebooks, got {K}")
        out = []
        for b0 in range(0, B, self.max_batch):
            cb = np.ascontiguousarray(c[b0: b0 + self.max_batch])
            nb = cb.shape[0]
            pcm = np.zeros((nb, F * self.m.frame_size), np.float32)
            _lib.check(_lib.lib().mimi_decode(self._h, nb, F, _lib.ptr(cb), 0, 0, _lib.ptr(pcm), 0))
            out.append(pcm)
        self._stream = None
        return np.concatenate(out, 0)[:, None, :]

    def debug_rows(self) -> np.ndarray:
        """The engine's row buffer (rows, dimension) as the last call left it (mimi_debug_read "rows"):
        after ``encode`` the pre-RVQ latent, row = b * Tf + t; after ``decode`` / ``decode_step`` the decoder
        transformer's output, row = b * n_lat + t.  Of the last ``max_batch`` chunk of a chunked call."""
        need = ctypes.c_int64(0)
        _lib.check(_lib.lib().mimi_debug_read(self._h, b"rows", None, 0, ctypes.byref(need)))
        out = np.zeros((need.value // (4 * self.m.dimension), self.m.dimension), np.float32)
        _lib.check(_lib.lib().mimi_debug_read(self._h, b"rows", _lib.ptr(out), out.nbytes, ctypes.byref(need)))
        return out

    def reset_state(self, batch_size: int = 1):
        _lib.check(_lib.lib().mimi_reset_state(self._h, batch_size))
        self._stream = batch_size
        self._enc_stream = None    # encode_step's streams start again too (moshi: one reset for both halves)

    def decode_step(self, codes: np.ndarray) -> np.ndarray:
        """One frame: (B, n_q, 1) or (B, n_q) -> (B, 1, frame_size)."""
        c = np.asarray(codes, np.int32)
        if c.ndim == 3:
            c = c[:, :, 0]
        B = c.shape[0]
        if self._stream not in (B, _SLOTS):    # (slot mode: refused by the library, not silently reset)
            self.reset_state(B)
        c = np.ascontiguousarray(c)
        pcm = np.zeros((B, self.m.frame_size), np.float32)
        _lib.check(_lib.lib().mimi_decode_step(self._h, B, _lib.ptr(c), _lib.ptr(pcm)))
        return pcm[:, None, :]

    # ------------------------------------------------------------------ slot streaming
    def slot_reset(self, b: int):
        """Row b of the streaming state starts a new stream (mimi_slot_reset; enqueued, not waited for).  The
        first call puts the codec in slot mode, ``reset_state`` and ``decode`` leave it."""
        _lib.check(_lib.lib().mimi_slot_reset(self._h, int(b)))
        self._stream = _SLOTS

    def decode_slots(self, hist, n: int, first_row: int, active, F_cap: Optional[int] = None,
                     on_device: bool = False) -> np.ndarray:
        """n frames of every slot in one pass (mimi_decode_slots): codes from the ring ``hist``
        (F_cap, B, n_q) int32 -- a numpy array, or with ``on_device`` a device pointer in that layout (the
        engine's code history) -- at rows (first_row + f) % F_cap.  ``active`` (B,): the slots whose streams
        advance.  Returns (B, n * frame_size) float32; an inactive slot's row is not audio."""
        act = np.ascontiguousarray(np.asarray(active).astype(bool), np.uint8)
        B = act.shape[0]
        if on_device:
            if F_cap is None:
                raise ValueError("decode_slots(on_device=True) needs F_cap")
            src = ctypes.c_void_p(int(hist))
        else:
            ring = np.ascontiguousarray(hist, np.int32)
            if ring.ndim != 3 or ring.shape[1] != B or ring.shape[2] != self.m.n_q:
                raise ValueError(f"expected a ring (F_cap, {B}, {self.m.n_q}), got {ring.shape}")
            if F_cap is not None and F_cap != ring.shape[0]:
                raise ValueError(f"F_cap {F_cap} differs from the ring's {ring.shape[0]} rows")
            F_cap, src = ring.shape[0], _lib.ptr(ring)
        pcm = np.zeros((B, max(int(n), 0) * self.m.frame_size), np.float32)
        _lib.check(_lib.lib().mimi_decode_slots(self._h, B, int(n), src, 1 if on_device else 0, int(F_cap),
                                                int(first_row), _lib.ptr(act), _lib.ptr(pcm)))
        return pcm

    # ------------------------------------------------------------------ streaming encode
    def encode_slot_reset(self, b: int):
        """Row b of the streaming encoder starts a new stream (mimi_encode_slot_reset; enqueued, not waited
        for).  The encoder's slots are independent of the decoder's streaming state."""
        _lib.check(_lib.lib().mimi_encode_slot_reset(self._h, int(b)))

    def encode_slots(self, pcm: np.ndarray, active=None) -> np.ndarray:
        """n whole frames of every slot in one pass (mimi_encode_slots): (B, n * frame_size) or
        (B, 1, n * frame_size) float32 -> (B, n_q, n) int32, row b continuing slot b's stream.  ``active``
        (B,), default all: an inactive slot's row is not codes, and its stream stays where it was."""
        x = np.asarray(pcm, np.float32)
        if x.ndim == 3:
            x = x[:, 0, :]
        if x.ndim != 2:
            raise ValueError(f"expected pcm (B, n * {self.m.frame_size}), got {x.shape}")
        B, N = x.shape
        if N % self.m.frame_size:
            raise ValueError(f"encode_slots takes whole frames: {N} samples is no multiple of {self.m.frame_size}")
        n = N // self.m.frame_size
        act = np.ones(B, np.uint8) if active is None else np.ascontiguousarray(np.asarray(active).astype(bool), np.uint8)
        if act.shape != (B,):
            raise ValueError(f"expected an active mask ({B},), got {act.shape}")
        x = np.ascontiguousarray(x)
        codes = np.zeros((B, self.m.n_q, n), np.int32)
        _lib.check(_lib.lib().mimi_encode_slots(self._h, B, n, _lib.ptr(x), _lib.ptr(act), _lib.ptr(codes)))
        return codes

    def encode_step(self, pcm: np.ndarray) -> np.ndarray:
        """moshi ``Mimi.encode_step``: (B, 1, n * frame_size) or (B, n * frame_size) -> (B, n_q, n), rows
        0..B-1 continuing their streams.  A change of B, or ``reset_state``, starts them again."""
        x = np.asarray(pcm, np.float32)
        B = x.shape[0]
        if self._enc_stream != B:
            for b in range(B):
                self.encode_slot_reset(b)
            self._enc_stream = B
        return self.encode_slots(x)
