"""``StreamEncoder`` -- audio streamed *into* the codec: the ingest side of a duplex serving loop.

Microphone audio arrives in blocks of any length while the model speaks.  Every caller holds a slot of the
codec's streaming encoder (``MimiCodec.encode_slots``); one ``push`` per tick encodes the whole frames all
callers have pending in shared passes, each slot at its own position, so a turn's codes are complete the
moment it ends and ``rows`` hands them on as the prompt rows ``tokenize_segment`` would have built from a
one-shot encode of the clip (ready for ``cache_context``, ``ContextPrefix.extend`` and ``SlotBatch.submit``).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np

from .tokenizers import audio_codes_to_frames, get_audio_tokenizer, tokenize_text_segment


class _Stream:
    def __init__(self, slot: int, n_q: int):
        self.slot = slot
        self.pending = np.zeros(0, np.float32)    # samples not yet encoded (whole frames and the remainder)
        self.codes: List[np.ndarray] = [np.zeros((n_q, 0), np.int32)]


class StreamEncoder:
    """Per-caller streaming Mimi encode over the slots of one codec.

    ``codec`` defaults to the registered audio tokenizer of ``n_audio_codebooks``; ``slots`` (default: the
    codec's ``max_batch``) is how many streams may be open at once.  A stream is bounded by the codec's
    ``max_frames``, as decode streams are.

    A trailing partial frame is never encoded: a live stream has no end-of-clip padding (the one-shot
    ``encode`` pads a clip's last frame on the right; here the remainder waits on the host for the samples
    that complete it, and is dropped by ``close``).
    """

    def __init__(self, codec=None, slots: Optional[int] = None, *, n_audio_codebooks: int = 32):
        self.codec = get_audio_tokenizer(n_audio_codebooks) if codec is None else codec
        self.slots = int(slots if slots is not None else self.codec.max_batch)
        if self.slots < 1:
            raise ValueError("StreamEncoder needs at least one slot")
        self.frame_size = int(self.codec.m.frame_size)
        self.n_q = int(self.codec.m.n_q)
        self._free = list(range(self.slots))
        self._streams: Dict[int, _Stream] = {}
        self._next = 0

    def open(self) -> int:
        """A handle for a new stream on a free slot (the lowest), reset to position 0."""
        if not self._free:
            raise RuntimeError(f"all {self.slots} encoder slots are in use")
        slot = self._free.pop(0)
        self.codec.encode_slot_reset(slot)
        handle, self._next = self._next, self._next + 1
        self._streams[handle] = _Stream(slot, self.n_q)
        return handle

    def close(self, handle: int):
        """Free the handle's slot (its pending remainder is dropped)."""
        st = self._streams.pop(handle)
        self._free.append(st.slot)
        self._free.sort()

    def push(self, chunks: Dict[int, np.ndarray]) -> Dict[int, np.ndarray]:
        """Append 1-D float32 samples (any lengths) to the given streams and encode every whole frame
        pending: {handle: the new codes (n_q, v)}, v >= 0.  Each pass encodes the smallest positive pending
        frame count for all streams with frames pending; the rest of the slots are inactive in it."""
        for h, x in chunks.items():
            st = self._streams[h]
            x = np.asarray(x, np.float32).reshape(-1)
            st.pending = np.concatenate([st.pending, x]) if st.pending.size else x.copy()
        new = {h: [] for h in chunks}
        fs = self.frame_size
        while True:
            due = {h: st.pending.size // fs for h, st in self._streams.items() if st.pending.size >= fs}
            if not due:
                break
            n = min(due.values())
            B = max(self._streams[h].slot for h in due) + 1
            pcm = np.zeros((B, n * fs), np.float32)
            active = np.zeros(B, bool)
            for h in due:
                st = self._streams[h]
                pcm[st.slot] = st.pending[: n * fs]
                active[st.slot] = True
            codes = np.asarray(self.codec.encode_slots(pcm, active))
            for h in due:    # (only after the pass went through: a refused pass leaves host and device alike)
                st = self._streams[h]
                st.pending = st.pending[n * fs:]
                c = codes[st.slot].astype(np.int32)
                st.codes.append(c)
                new.setdefault(h, []).append(c)
        empty = np.zeros((self.n_q, 0), np.int32)
        return {h: np.concatenate(v, axis=1) if v else empty for h, v in new.items()}

    def codes(self, handle: int) -> np.ndarray:
        """The stream's codes so far, (n_q, frames)."""
        st = self._streams[handle]
        if len(st.codes) > 1:
            st.codes = [np.concatenate(st.codes, axis=1)]
        return st.codes[0]

    def pending(self, handle: int) -> int:
        """Samples of the stream waiting for the rest of their frame."""
        return int(self._streams[handle].pending.size)

    def rows(self, handle: int, text, speaker: int):
        """(tokens, mask) of the turn as ``tokenize_segment`` lays out a ``Segment(speaker, text, audio)``:
        the text rows, the audio frames of the codes so far, the EOS zero frame."""
        t_tok, t_mask = tokenize_text_segment(text, speaker, self.n_q)
        a_tok, a_mask = audio_codes_to_frames(self.codes(handle))
        return np.concatenate([t_tok, a_tok], 0).astype(np.int32), np.concatenate([t_mask, a_mask], 0).astype(bool)
