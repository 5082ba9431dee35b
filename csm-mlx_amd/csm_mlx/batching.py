"""Continuous batching: utterances join and leave a running batch.

``generate_batch`` runs B utterances as one indivisible generation: they start together and every frame
runs all B rows until the slowest ends.  ``SlotBatch`` runs the same frame graphs over B *slots*: a slot
whose utterance reached EOS (or its frame cap) is read, then restarted with the next queued prompt at the
next frame boundary -- or parked when the queue is empty -- while the other slots go on
(csm_slot_restart / csm_slot_release / csm_slot_read, csrc/csm_engine_slots.hip).  The codes of an
utterance depend only on its prompt, its seed, the sampler and the processors: not on the slot, on when it
joined, on who ran beside it or on what ran in the slot before.

No reference counterpart: the reference speaks one sentence per ``stream_generate`` call
(run_streaming_csm_mlx.py ``tts_worker``); this is what a server with several such conversations on one
GPU puts between them and the engine.

``SlotBatch.stream`` is the same loop with audio coming out while it runs: each slot has its own streaming
Mimi decoder state (mimi_slot_reset / mimi_decode_slots, csrc/mimi_engine.hip), a chunk of frames is decoded
for every slot in one codec pass that reads the codes from the engine's ring history on the device, and the
PCM of chunk c is handed out per utterance while chunk c + 1 runs on the engine's stream.
"""
from __future__ import annotations

import collections
import ctypes
from typing import Callable, Generator, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .generation import (FrameCache, _check_window, _decode_batch, _resolve_sampler, _seed_list,
                         device_processors, processor_args)
from .models import CSM
from .prefix import ContextPrefix
from .sampling import HostSampler, Sampler

DEFAULT_CHUNK = 8


class StreamChunk(NamedTuple):
    """One event of ``SlotBatch.stream``: the ``len(pcm) // 1920`` new frames of utterance ``ticket``.
    ``final`` marks the utterance's last event, which alone carries its ``codes`` (F, K) int32."""
    ticket: int
    pcm: np.ndarray
    final: bool
    codes: Optional[np.ndarray] = None


class _EngineSlots:
    """The engine's side of a ``SlotBatch``: one ``FrameCache`` (csm_begin, the sampler filters, the c0
    processors, the superseded check, the prefix calls) plus the slot calls.  ``SlotBatch`` only talks to these
    methods, so its scheduling is testable against a stub with the same ones (``set_sampling`` only for a job
    that brings its own sampler or processors: a stub without it serves every other queue)."""

    def __init__(self, model: CSM, slots: int, sampler: Sampler, processors):
        self.model = model
        self.processors = processors
        self.cache = FrameCache(model, slots, sampler, np.zeros(slots, np.uint64), processors)
        self._call = self.cache._call

    def restart(self, b: int, seed: int):
        self._call("csm_slot_restart", b, ctypes.c_uint64(int(seed) & ((1 << 64) - 1)))

    def release(self, b: int):
        self._call("csm_slot_release", b)

    def set_sampling(self, b: int, sampler: Optional[Sampler], processors):
        """Slot b's utterance samples with ``sampler`` and the ``device_processors`` pair ``processors``
        instead of the batch's (csm_slot_set_sampling); None for either: the batch's.  Right after
        ``restart(b)``."""
        smp = self.cache.sampler if sampler is None else sampler
        idx, val, penalty, context = processor_args(self.processors if processors is None else processors,
                                                    self.model.n_audio_vocab)
        s = _lib.CsmSampling(smp.temp, smp.top_k, smp.top_p, smp.min_p, smp.min_tokens_to_keep, len(idx),
                             idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                             val.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), penalty, context)
        self._call("csm_slot_set_sampling", b, ctypes.byref(s))

    def prefill(self, items: Sequence[Tuple[int, np.ndarray, np.ndarray]]):
        self.cache.prefill_batch(items)

    def load_prefix(self, items: Sequence[Tuple[int, ContextPrefix]]):
        """(slot, prefix) of every join of a boundary that has one: one csm_prefix_load, before ``prefill``."""
        self.cache.load_prefix(items)

    def save_prefix(self, b: int, rows: int, tokens, mask) -> ContextPrefix:
        """The first ``rows`` rows slot b holds, kept as a ``ContextPrefix`` (after the boundary's ``prefill``)."""
        return self.cache.save_prefix(b, rows, tokens, mask)

    def run(self, nframes: int, sync: bool = True):
        """nframes frames for every slot, waited for (the wait also checks the persistent kernels'
        hand-off error flags: all three); ``sync=False``: enqueued only, ``wait`` does the rest."""
        self.cache.run(nframes, sync=sync)

    def wait(self):
        """Wait for the enqueued frames and check the three hand-off error flags, as ``run`` does."""
        self._call("csm_synchronize")

    def ring(self) -> Tuple[int, int, int]:
        """(device pointer of the code history [F_cap][B][K], F_cap, global frames run): frame g of the
        session is ring row g % F_cap."""
        p = ctypes.c_void_p()
        self._call("csm_codes_device_ptr", ctypes.byref(p))
        return int(p.value), int(self.model.max_frames), int(self.cache.frames)

    def poll(self) -> Tuple[np.ndarray, np.ndarray]:
        """(n_frames [B], done [B]) of the slots' current utterances."""
        n = np.zeros(self.cache.B, np.int32)
        d = np.zeros(self.cache.B, np.uint8)
        self._call("csm_read_codes", None, _lib.ptr(n), _lib.ptr(d), None)
        return n, d.astype(bool)

    def read(self, b: int, cap: int) -> np.ndarray:
        """codes (F, K) int32 of slot b's utterance (EOS excluded)."""
        out = np.zeros((max(cap, 1), self.model.n_audio_codebooks), np.int32)
        n = ctypes.c_int(0)
        d = ctypes.c_uint8(0)
        self._call("csm_slot_read", b, _lib.ptr(out), cap, ctypes.byref(n), ctypes.byref(d))
        return out[: n.value].copy()


class _Job:
    __slots__ = ("ticket", "tokens", "mask", "cap", "seed", "ran", "prefix", "keep_rows", "sampling")

    def __init__(self, ticket, tokens, mask, cap, seed, prefix=None, keep_rows=0, sampling=None):
        self.ticket, self.tokens, self.mask, self.cap, self.seed, self.ran = ticket, tokens, mask, cap, seed, 0
        self.prefix, self.keep_rows = prefix, keep_rows
        self.sampling = sampling      # (sampler or None, device_processors pair or None) of an override; else None


class SlotBatch:
    """A batch of ``slots`` slots over ``model``'s engine, each holding at most one utterance.

    ``submit`` queues a prompt; ``run`` is a generator that yields ``(ticket, codes (F, K) int32)`` as
    utterances finish and ends when the queue and the slots are empty (more can be submitted while it
    runs: they join at the next frame boundary).  Every chunk runs ``min(chunk, smallest remaining frame
    budget among the active slots)`` frames, then waits and polls, so no slot ever runs past its own cap
    and the reference's window guard (prompt rows < max_seq_len - max_audio_frames) stays the only
    admission rule; a slot runs at most ``chunk - 1`` frames past its EOS, which are discarded.

    The sampler runs on the GPU, and so must the processors (``device_processors``): a ``HostSampler`` or
    any other processor list pauses every frame for the host and has nothing to batch -- ``ValueError``.
    Creating a SlotBatch supersedes older ``FrameCache``s (and SlotBatches) of the model exactly as a new
    ``FrameCache`` does.

    ``stream`` is ``run`` with audio: it yields each utterance's PCM chunk by chunk while the queue runs."""

    def __init__(self, model, slots: int, *, sampler, logits_processors: Optional[List[Callable]] = None,
                 chunk: int = DEFAULT_CHUNK, _engine=None):
        if slots < 1:
            raise ValueError("a SlotBatch needs at least one slot")
        if chunk < 1:
            raise ValueError("chunk must be >= 1")
        on_device = self._on_device(sampler, logits_processors)
        self.model = model
        self.slots = slots
        self.chunk = chunk
        self.max_frames = int(getattr(model, "max_frames", 0) or model.max_seq_len)
        self._eng = _engine if _engine is not None else _EngineSlots(model, slots, sampler, on_device)
        self._queue: collections.deque = collections.deque()
        self._active: List[Optional[_Job]] = [None] * slots
        self._parked = [False] * slots
        self._joined: List[int] = []     # the slots the last ``_fill`` restarted
        self._tickets = 0
        self._kept: dict = {}            # ticket -> ContextPrefix (None until its utterance has joined)

    @staticmethod
    def _on_device(sampler, logits_processors):
        """The ``device_processors`` pair of a sampler and a processor list the GPU can run (None: no
        processors), for the batch or for one utterance; ``ValueError`` for anything that needs the host."""
        if isinstance(sampler, HostSampler) or not isinstance(sampler, Sampler):
            raise ValueError("SlotBatch samples on the GPU: pass a csm_mlx.sampling.Sampler (a host sampler "
                             "callable pauses every frame for the host and has nothing to batch)")
        on_device = device_processors(logits_processors, sampler)
        if logits_processors and on_device is None:
            raise ValueError("SlotBatch runs logits processors on the GPU only: at most one logit_bias followed "
                             "by at most one repetition_penalty (make_logits_processors); other lists pause "
                             "every frame for the host")
        return on_device

    def submit(self, tokens, mask, max_audio_frames: int, seed: int = 0, *, prefix: Optional[ContextPrefix] = None,
               keep_rows: int = 0, sampler: Optional[Sampler] = None,
               logits_processors: Optional[List[Callable]] = None) -> int:
        """Queue one utterance: prompt (L, K+1) tokens / mask, at most ``max_audio_frames`` frames, its
        sampling seed.  Returns the ticket ``run`` yields its codes under.

        ``sampler`` / ``logits_processors``: this utterance's own, as the reference's ``generate()`` takes them
        per call; None (each on its own) means the batch's, an empty processor list means none.  Both run on
        the GPU under the constructor's rules (``ValueError`` otherwise).  The utterance's codes are those it
        gets alone with these parameters, whatever its neighbours sample with (csm_slot_set_sampling).

        ``prefix``: a ``ContextPrefix`` the prompt begins with; ``tokens`` / ``mask`` are then only the rows
        that follow it (at least one).  Its K / V are copied into the slot when the utterance joins, and only
        the given rows run through the backbone.  ``keep_rows`` > 0: right after the prefill of the boundary
        at which this utterance joins, the first ``keep_rows`` rows of its whole prompt (prefix + given rows)
        are saved as a ``ContextPrefix`` that ``kept(ticket)`` returns -- the first sentence in a new voice
        pays for the later ones without the batch stopping.  The window guard and the frame-history check
        count the whole prompt."""
        tokens = np.ascontiguousarray(tokens, np.int32)
        mask = np.ascontiguousarray(np.asarray(mask).astype(bool), np.uint8)
        cap = int(max_audio_frames)
        if cap < 0:
            raise ValueError("max_audio_frames must be >= 0")
        if prefix is not None:
            prefix.require(self.model)
            if tokens.shape[0] < 1:
                raise ValueError("a prompt with a prefix needs at least one row after it")
        total = tokens.shape[0] + (prefix.rows if prefix is not None else 0)
        keep_rows = int(keep_rows)
        if not 0 <= keep_rows <= total:
            raise ValueError(f"keep_rows {keep_rows} outside the prompt's {total} rows")
        _check_window(self.model, total, cap)                                    # generation.py:131-137
        if cap > self.max_frames:     # the engine would refuse the frames that take it there (CSM_ERR_STATE)
            raise _lib.CsmHipError(_lib.CSM_ERR_STATE, f"an utterance of up to {cap} frames does not fit the engine's "
                                   f"{self.max_frames}-frame code history (CSM(..., max_frames=))")
        sampling = None
        if sampler is not None or logits_processors is not None:
            pair = self._on_device(Sampler() if sampler is None else sampler, logits_processors)
            V = self.model.n_audio_vocab
            if pair and pair[0] and not all(0 <= i < V for i in pair[0].indices):    # not at the join, mid-run
                raise ValueError(f"logit_bias index outside [0, {V}): {pair[0].indices}")
            sampling = (sampler, None if logits_processors is None else (pair or (None, None)))
        ticket = self._tickets
        self._tickets += 1
        self._queue.append(_Job(ticket, tokens, mask, cap, seed, prefix, keep_rows if cap > 0 else 0, sampling))
        if keep_rows and cap > 0:
            self._kept[ticket] = None
        return ticket

    def kept(self, ticket: int) -> ContextPrefix:
        """The ``ContextPrefix`` saved for a ticket submitted with ``keep_rows`` (available once its utterance
        has joined the batch: from the first event ``run`` / ``stream`` yields after that boundary on)."""
        if ticket not in self._kept:
            raise ValueError(f"ticket {ticket} was not submitted with keep_rows (or generates no frames)")
        if self._kept[ticket] is None:
            raise RuntimeError(f"ticket {ticket} has not joined the batch yet: its rows are not prefilled")
        return self._kept[ticket]

    def _fill(self) -> Generator[Tuple[int, np.ndarray], None, None]:
        """A frame boundary: free slots take the next queued prompts (all of the boundary's joins in one
        batched prefill, after one load of all their prefixes; then the ``keep_rows`` saves); slots left
        without work are parked."""
        K = self.model.n_audio_codebooks
        joins, loads, saves = [], [], []
        self._joined = []
        for b in range(self.slots):
            if self._active[b] is not None:
                continue
            while self._queue and self._queue[0].cap == 0:      # nothing to generate: an empty result
                yield self._queue.popleft().ticket, np.zeros((0, K), np.int32)
            if self._queue:
                job = self._queue.popleft()
                self._eng.restart(b, job.seed)
                if job.sampling is not None:        # (a restart puts the slot back on the batch's)
                    self._eng.set_sampling(b, *job.sampling)
                self._active[b] = job
                self._parked[b] = False
                joins.append((b, job.tokens, job.mask))
                if job.prefix is not None:
                    loads.append((b, job.prefix))
                if job.keep_rows:
                    saves.append((b, job))
                self._joined.append(b)
            elif not self._parked[b]:
                self._eng.release(b)
                self._parked[b] = True
        if loads:
            self._eng.load_prefix(loads)
        if joins:
            self._eng.prefill(joins)
        for b, job in saves:
            t, m = job.tokens, job.mask.astype(bool)
            if job.prefix is not None:
                t, m = np.concatenate([job.prefix.tokens, t], 0), np.concatenate([job.prefix.mask, m], 0)
            self._kept[job.ticket] = self._eng.save_prefix(b, job.keep_rows, t[: job.keep_rows], m[: job.keep_rows])

    def _chunk_frames(self) -> int:
        """The frames of the next chunk: ``chunk``, shortened to the smallest remaining budget among the
        active slots; 0 when no slot is active (with every slot free, ``_fill`` has emptied the queue)."""
        left = [j.cap - j.ran for j in self._active if j is not None]
        return min(self.chunk, min(left)) if left else 0

    def _advance(self, n: int, done) -> Generator[Tuple[int, int, bool, Optional[np.ndarray]], None, None]:
        """After a chunk of n frames and its poll: (slot, ticket, final, codes) of every active slot in
        slot order.  ``final``: the utterance reached EOS or its cap -- its slot is read (``codes``, else
        None) and freed for the next ``_fill``."""
        for b, job in enumerate(self._active):
            if job is None:
                continue
            job.ran += n
            final = bool(done[b]) or job.ran >= job.cap
            codes = None
            if final:
                codes = self._eng.read(b, job.cap)
                self._active[b] = None
            yield b, job.ticket, final, codes

    def run(self) -> Generator[Tuple[int, np.ndarray], None, None]:
        while True:
            yield from self._fill()
            n = self._chunk_frames()
            if not n:
                return
            self._eng.run(n)
            _, done = self._eng.poll()
            for _, ticket, final, codes in self._advance(n, done):
                if final:
                    yield ticket, codes

    def stream(self, codec=None) -> Generator[StreamChunk, None, None]:
        """``run`` with audio: yields ``StreamChunk(ticket, pcm, final, codes)`` as the frames of each
        utterance are decoded -- ``pcm`` the (v * 1920,) float32 samples of its v >= 0 new frames, ``final``
        on its last event, which also carries its codes (F, K).  The concatenated ``pcm`` of a ticket is what
        ``stream_generate`` yields for that utterance alone; an utterance without frames gives one empty
        final event.

        Chunk c + 1 is enqueued on the engine's stream, then chunk c is decoded on the codec's (one
        ``decode_slots`` pass for all slots, codes read from the engine's ring history on the device) and its
        events yielded, then chunk c + 1 is waited for and polled.  A slot restarted at a boundary has its
        codec state reset (``slot_reset``) after the decode of the chunk that holds its previous utterance's
        last frames and before the decode of the first chunk of the new one: the resets travel with the
        chunk record.  ``codec``: default the registered audio tokenizer of the model's codebook count."""
        K = self.model.n_audio_codebooks
        if codec is None:
            from .tokenizers import get_audio_tokenizer
            codec = get_audio_tokenizer(K)
        if 2 * self.chunk > self.max_frames:    # a chunk's ring rows must outlive the next chunk
            raise ValueError(f"streaming needs 2 * chunk <= max_frames: chunk {self.chunk}, the engine's code "
                             f"history holds {self.max_frames} frames")
        if codec.max_batch < self.slots:
            raise ValueError(f"the codec serves {codec.max_batch} streams, the batch has {self.slots} slots "
                             f"(MimiCodec(..., max_batch=))")
        cap = max([j.cap for j in self._queue] + [j.cap for j in self._active if j is not None] + [0])
        if codec.max_frames < cap:
            raise ValueError(f"the codec holds streams of {codec.max_frames} frames, the longest utterance may "
                             f"take {cap} (MimiCodec(..., max_frames=))")
        fs = int(codec.m.frame_size)
        empty = np.zeros((0,), np.float32)

        def events(rec):
            """Decode one finished chunk and yield its utterances' events."""
            for b in rec["resets"]:
                codec.slot_reset(b)
            rows = rec["rows"]           # (slot, ticket, valid frames, final, codes)
            pcm = None
            if any(v > 0 for _, _, v, _, _ in rows):
                active = np.zeros(self.slots, bool)
                active[[b for b, _, _, _, _ in rows]] = True
                pcm = codec.decode_slots(rec["ptr"], rec["n"], rec["first_row"], active, F_cap=rec["F_cap"],
                                         on_device=True)
            for b, ticket, v, final, codes in rows:
                yield StreamChunk(ticket, pcm[b, : v * fs].copy() if v > 0 else empty, final, codes)

        prev = None
        delivered = [0] * self.slots         # frames of the slot's current utterance already in a chunk record
        while True:
            for ticket, codes in self._fill():                      # cap 0: nothing to generate
                yield StreamChunk(ticket, empty, True, codes)
            for b in self._joined:
                delivered[b] = 0
            resets = list(self._joined)
            n = self._chunk_frames()
            if not n:
                break
            ptr, F_cap, g0 = self._eng.ring()
            self._eng.run(n, sync=False)
            if prev is not None:
                yield from events(prev)
            self._eng.wait()
            n_frames, done = self._eng.poll()
            rows = []
            for b, ticket, final, codes in self._advance(n, done):
                valid = max(0, min(n, int(n_frames[b]) - delivered[b]))
                delivered[b] += valid
                rows.append((b, ticket, valid, final, codes))
            prev = {"resets": resets, "rows": rows, "ptr": ptr, "F_cap": F_cap, "first_row": g0 % F_cap, "n": n}
        if prev is not None:
            yield from events(prev)


def _queued(model, prompts, max_audio_length_ms, slots, temperature, top_k, sampler, seeds, max_audio_frames,
            logits_processors, chunk, prefixes=None, samplers=None, prompt_processors=None
            ) -> Tuple[SlotBatch, List[int]]:
    """What both queue entry points begin with: a ``SlotBatch`` with every prompt submitted under its frame
    cap, seed, prefix and its own sampler / processors.  Returns (batch, the tickets in prompt order)."""
    smp = _resolve_sampler(temperature, sampler, top_k)
    n = len(prompts)
    caps = [int(max_audio_length_ms / 80)] * n if max_audio_frames is None else [int(c) for c in max_audio_frames]
    if len(caps) != n:
        raise ValueError("need one frame cap per prompt")
    if prefixes is None:
        prefixes = [None] * n
    if len(prefixes) != n:
        raise ValueError("need one prefix (or None) per prompt")
    if samplers is None:
        samplers = [None] * n
    if len(samplers) != n:
        raise ValueError("need one sampler (or None) per prompt")
    if prompt_processors is None:
        prompt_processors = [None] * n
    if len(prompt_processors) != n:
        raise ValueError("need one logits processor list (or None) per prompt")
    seed_list = _seed_list(seeds, n)
    batch = SlotBatch(model, slots, sampler=smp, logits_processors=logits_processors, chunk=chunk)
    return batch, [batch.submit(t, m, caps[i], int(seed_list[i]), prefix=prefixes[i], sampler=samplers[i],
                                logits_processors=prompt_processors[i]) for i, (t, m) in enumerate(prompts)]


def generate_queue(model: CSM, prompts: Sequence[Tuple[np.ndarray, np.ndarray]], max_audio_length_ms: float = 10_000,
                   *, slots: int, temperature: float = 0.0, top_k: int = 0, sampler=None, seeds=None,
                   max_audio_frames: Optional[Sequence[int]] = None, decode: bool = True, with_codes: bool = False,
                   logits_processors: Optional[List[Callable]] = None, chunk: int = DEFAULT_CHUNK,
                   prefixes: Optional[Sequence[Optional[ContextPrefix]]] = None,
                   samplers: Optional[Sequence[Optional[Sampler]]] = None,
                   prompt_processors: Optional[Sequence[Optional[List[Callable]]]] = None):
    """``generate_batch`` for any number of prompts through ``slots`` slots: list of waveforms in prompt
    order (or codes if decode=False; (codes, waveforms) with ``with_codes``).  ``max_audio_frames``: one
    frame cap per prompt (default: ``max_audio_length_ms`` for all).  Seeds follow ``generate_batch``: a
    scalar s gives s + i for prompt i.  ``prefixes``: one ``ContextPrefix`` (or None) per prompt, which then
    holds only the rows after it (``SlotBatch.submit``).  ``samplers`` / ``prompt_processors``: one
    ``Sampler`` / one processor list (or None: the batch's ``sampler`` / ``logits_processors``) per prompt."""
    batch, tickets = _queued(model, prompts, max_audio_length_ms, slots, temperature, top_k, sampler, seeds,
                             max_audio_frames, logits_processors, chunk, prefixes, samplers, prompt_processors)
    got = dict(batch.run())
    codes = [got[t] for t in tickets]
    if not decode:
        return codes
    n = len(prompts)
    n_frames = np.array([len(c) for c in codes], np.int32)
    hist = np.zeros((int(n_frames.max()) if n else 0, n, model.n_audio_codebooks), np.int32)
    for i, c in enumerate(codes):
        hist[: len(c), i] = c
    pcm = _decode_batch(model, hist, n_frames)
    return (codes, pcm) if with_codes else pcm


def stream_generate_queue(model: CSM, prompts: Sequence[Tuple[np.ndarray, np.ndarray]],
                          max_audio_length_ms: float = 10_000, *, slots: int, temperature: float = 0.0,
                          top_k: int = 0, sampler=None, seeds=None, max_audio_frames: Optional[Sequence[int]] = None,
                          logits_processors: Optional[List[Callable]] = None, chunk: int = DEFAULT_CHUNK,
                          prefixes: Optional[Sequence[Optional[ContextPrefix]]] = None,
                          samplers: Optional[Sequence[Optional[Sampler]]] = None,
                          prompt_processors: Optional[Sequence[Optional[List[Callable]]]] = None
                          ) -> Generator[Tuple[int, np.ndarray, bool], None, None]:
    """``generate_queue`` as a stream: yields ``(prompt index, pcm, final)`` while the queue runs -- ``pcm``
    the new (v * 1920,) float32 samples of that prompt's utterance (v >= 0), ``final`` on its last event.  The
    concatenation per prompt is what ``stream_generate`` yields for it alone.  The registered audio tokenizer
    needs ``max_batch >= slots`` and ``max_frames >=`` the largest frame cap.  ``samplers`` /
    ``prompt_processors``: per prompt, as in ``generate_queue``."""
    batch, tickets = _queued(model, prompts, max_audio_length_ms, slots, temperature, top_k, sampler, seeds,
                             max_audio_frames, logits_processors, chunk, prefixes, samplers, prompt_processors)
    index = {t: i for i, t in enumerate(tickets)}
    for ev in batch.stream():
        yield index[ev.ticket], ev.pcm, ev.final
