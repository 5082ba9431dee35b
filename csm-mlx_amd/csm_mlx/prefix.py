"""Shared context prefixes: a conversation's context is prefilled once.

Every utterance begins by prefilling its whole prompt, and in every real use of CSM that prompt is mostly
context that does not change between sentences (run_streaming_csm_mlx.py ``tts_worker`` passes the same
segments to ``stream_generate`` for every sentence of a turn; the reference's ``generate`` Mimi-encodes and
prefills them again each time, generation.py:108-125).  Attention is causal, so the backbone K / V of a
prompt's first rows depend on those rows alone: ``cache_context`` prefills a context once and keeps its K / V
on the GPU as a ``ContextPrefix`` (csm_prefix_save, csrc/csm_engine_prefix.hip); ``generate`` /
``stream_generate`` take it in place of the segment list, the batch entry points take ``prefixes=``, and
``SlotBatch.submit`` takes ``prefix=``.  The rows are then copied into the utterance's cache
(csm_prefix_load) and only the rows that follow -- the text segment -- run through the backbone.

No reference counterpart.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple, Union

import numpy as np

from .segment import Segment


class ContextPrefix:
    """The saved backbone K / V of a prompt's first ``rows`` rows on ``model``'s engine (``nbytes`` of GPU
    memory until ``free`` or garbage collection), with the ``(rows, K+1)`` ``tokens`` and ``mask`` it stands
    for.  Valid for the weights it was computed with: after a weight change (``load_weights``,
    ``load_adapters``, ``nn.quantize``) loading it raises; so does using it after ``free`` or with another
    model."""

    def __init__(self, model, handle: int, rows: int, nbytes: int, tokens, mask,
                 release: Optional[Callable[[int], None]] = None):
        self.model = model
        self.handle = int(handle)
        self.rows = int(rows)
        self.nbytes = int(nbytes)
        self.tokens = np.ascontiguousarray(tokens, np.int32)
        self.mask = np.ascontiguousarray(np.asarray(mask).astype(bool))
        if self.tokens.shape[0] != self.rows or self.mask.shape != self.tokens.shape:
            raise ValueError(f"a prefix of {self.rows} rows needs tokens and mask of ({self.rows}, K+1), got "
                             f"{self.tokens.shape} and {self.mask.shape}")
        self._release = release
        self.freed = False

    def require(self, model):
        """Raise unless this prefix can be loaded into ``model``'s engine (staleness is the engine's check)."""
        if self.freed:
            raise RuntimeError("this ContextPrefix was freed")
        if model is not self.model:
            raise ValueError("this ContextPrefix belongs to another model: its K / V were computed with that "
                             "model's weights and live on its engine")

    def free(self):
        """Release the GPU buffer (waits for a load still in flight).  Idempotent."""
        if self.freed:
            return
        self.freed = True
        if self._release is not None:
            self._release(self.handle)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def extend(self, segments_or_prompt) -> "ContextPrefix":
        """A longer prefix: this one plus the rows of more ``Segment``s (or of a ready ``(tokens, mask)``
        pair) -- the growing conversation, with no old row recomputed: this prefix is loaded, the new rows
        are prefilled after it and the whole is saved.  This prefix stays valid.  Like ``cache_context`` it
        starts a new batch on the model (a running generation is superseded)."""
        from .generation import FrameCache
        from .sampling import Sampler
        self.require(self.model)
        t, m = context_rows(self.model, segments_or_prompt)
        cache = FrameCache(self.model, 1, Sampler(0.0, 0), [0])
        cache.load_prefix([(0, self)])
        cache.prefill(0, t, m)
        return cache.save_prefix(0, self.rows + t.shape[0], np.concatenate([self.tokens, t], 0),
                                 np.concatenate([self.mask, m], 0))

    def __repr__(self):
        return f"ContextPrefix(rows={self.rows}, nbytes={self.nbytes}, handle={self.handle}{', freed' if self.freed else ''})"


def context_rows(model, context: Union[Sequence[Segment], Tuple[np.ndarray, np.ndarray]]):
    """(tokens (L, K+1) int32, mask bool) of a context: ``Segment``s tokenized in order (this is where the
    Mimi encode of their audio is paid), or a ready (tokens, mask) pair."""
    if isinstance(context, tuple) and len(context) == 2 and not isinstance(context[0], Segment):
        t, m = context
        return np.ascontiguousarray(t, np.int32), np.asarray(m).astype(bool)
    from .tokenizers import tokenize_segment
    segs = list(context)
    if not segs:
        raise ValueError("an empty context has no rows to cache")
    parts = [tokenize_segment(seg, n_audio_codebooks=model.n_audio_codebooks) for seg in segs]
    return (np.concatenate([t for t, _ in parts], 0).astype(np.int32),
            np.concatenate([m for _, m in parts], 0).astype(bool))


def cache_context(model, context: Union[Sequence[Segment], Tuple[np.ndarray, np.ndarray]]) -> ContextPrefix:
    """Prefill ``context`` -- a list of ``Segment``s, or a ready (tokens, mask) pair -- once and keep its
    backbone K / V as a ``ContextPrefix``: ``generate(model, text, speaker, context=prefix)`` then returns
    what ``generate(model, text, speaker, context=segments)`` returns, without encoding or prefilling the
    segments again.

    The prefill runs in a one-utterance ``FrameCache``, so like every ``FrameCache`` it supersedes a running
    generation of the model; a running ``SlotBatch`` saves a prefix without stopping through
    ``submit(..., keep_rows=)`` instead."""
    from .generation import FrameCache
    from .sampling import Sampler
    t, m = context_rows(model, context)
    if t.shape[0] < 1:
        raise ValueError("an empty context has no rows to cache")
    cache = FrameCache(model, 1, Sampler(0.0, 0), [0])
    cache.prefill(0, t, m)
    return cache.save_prefix(0, t.shape[0], t, m)
