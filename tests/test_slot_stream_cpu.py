"""``SlotBatch.stream`` (csm_mlx.batching) against a stub engine and a recording stub codec -- the order of
the calls on the two streams, the codec resets around a restart, the valid-frame accounting, the flush of
the last chunk, the ValueErrors -- and the slot codec ABI's checks that need no GPU."""
import numpy as np
import pytest

from helpers import STUB_K as K, StubEngine

FS = 4          # the stub codec's samples per frame


class StubCodec:
    """Records slot_reset / decode_slots; a frame's PCM is FS copies of 1000 * code 0 + code 1 (utterance and
    frame), read from the ring when the decode is called -- as the GPU codec reads the engine's history."""

    class m:
        frame_size = FS

    def __init__(self, max_batch, max_frames, log):
        self.max_batch, self.max_frames, self.log = max_batch, max_frames, log

    def slot_reset(self, b):
        self.log.append(("reset", b))

    def decode_slots(self, hist, n, first_row, active, F_cap=None, on_device=False):
        assert on_device and F_cap == hist.F_cap and 0 <= first_row < F_cap and 1 <= n <= F_cap
        self.log.append(("decode", first_row, n, tuple(bool(a) for a in active)))
        out = np.zeros((len(active), n * FS), np.float32)
        for f in range(n):
            row = hist.hist[(first_row + f) % F_cap]
            out[:, f * FS: (f + 1) * FS] = (1000.0 * row[:, 0] + row[:, 1])[:, None]
        return out


def handle(**kw):
    from csm_mlx.models import CSM, csm_tiny
    return CSM(csm_tiny(), **kw)


def prompt(L=5):
    return np.zeros((L, K + 1), np.int32), np.ones((L, K + 1), bool)


def scheduler(slots, eos, chunk=8, max_frames=64, codec_rows=None, codec_frames=64):
    from csm_mlx.batching import SlotBatch
    from csm_mlx.sampling import Sampler
    log = []
    stub = StubEngine(slots, eos, max_frames, log)
    batch = SlotBatch(handle(max_frames=max_frames), slots, sampler=Sampler(0.0, 0), chunk=chunk, _engine=stub)
    return batch, stub, StubCodec(slots if codec_rows is None else codec_rows, codec_frames, log), log


def expected_pcm(seed, cap, eos):
    n = min(cap, eos.get(seed, cap))
    return np.repeat(np.array([1000.0 * (seed + 1) + f + 1 for f in range(n)], np.float32), FS)


def collect(batch, codec):
    evs = list(batch.stream(codec))
    by = {}
    for e in evs:
        by.setdefault(e.ticket, []).append(e)
    return evs, by


CAPS = [3, 20, 11, 8, 5, 30, 0, 6]
EOS = {1: 13, 5: 2, 7: 0}


def test_every_utterance_gets_exactly_its_frames():
    """EOS inside a chunk (utterances 1 and 5), at frame 0 (7), a cap of 0 (6): the frames after an EOS are
    never yielded, each utterance has one final event, the last, which alone carries the codes."""
    batch, stub, codec, log = scheduler(3, EOS, chunk=4)
    tickets = [batch.submit(*prompt(), CAPS[i], i) for i in range(len(CAPS))]
    evs, by = collect(batch, codec)
    assert sorted(by) == tickets
    for i, t in enumerate(tickets):
        e = by[t]
        assert [x.final for x in e] == [False] * (len(e) - 1) + [True], i
        assert all(x.codes is None for x in e[:-1]), i
        want = expected_pcm(i, CAPS[i], EOS)
        got = np.concatenate([x.pcm for x in e])
        assert got.dtype == np.float32 and np.array_equal(got, want), (i, got, want)
        assert len(e[-1].codes) == len(want) // FS, i
        assert all(len(x.pcm) % FS == 0 for x in e), i
    for i in (6, 7):                                   # nothing generated: one empty final event
        assert len(by[tickets[i]]) == 1 and len(by[tickets[i]][0].pcm) == 0
    assert by[tickets[1]][-1].codes.shape == (13, K)


def test_call_order_one_chunk_behind():
    """run(chunk c + 1), decode(chunk c), wait -- and the last chunk is decoded after the loop."""
    batch, stub, codec, log = scheduler(2, {}, chunk=4)
    for i in range(3):
        batch.submit(*prompt(), 10, i)
    collect(batch, codec)
    seq = [e for e in log if e[0] in ("run", "decode", "wait")]
    runs = [e for e in seq if e[0] == "run"]
    decodes = [e for e in seq if e[0] == "decode"]
    assert len(runs) == len(decodes) and len(runs) >= 4
    assert [e[0] for e in seq[:2]] == ["run", "wait"]                         # nothing to decode yet
    body = seq[2:-1]
    assert [e[0] for e in body] == ["run", "decode", "wait"] * (len(runs) - 1), body
    assert seq[-1][0] == "decode"                                             # the flush
    for r, d in zip(runs, decodes):                                           # decode c reads run c's rows
        assert d[1] == r[2] % stub.F_cap and d[2] == r[1], (r, d)


def test_codec_reset_sits_between_the_two_utterances_of_a_slot():
    """Each slot_reset(b) falls after the decode of the chunk that ends b's previous utterance and before the
    decode of the first chunk of the new one -- with the engine's restart of b already a chunk ahead."""
    batch, stub, codec, log = scheduler(2, {0: 5, 3: 1}, chunk=4)
    caps = [9, 3, 6, 7, 2]
    for i, c in enumerate(caps):
        batch.submit(*prompt(), c, i)
    evs, by = collect(batch, codec)
    # replay: which chunk (by its run index) holds the first / last frames of each slot's utterances
    chunk_of_run, owner, spans = -1, {}, []          # spans: (slot, first chunk, last chunk)
    open_span = {}
    for e in log:
        if e[0] == "restart":
            open_span[e[1]] = [e[1], None, None]
        elif e[0] == "run":
            chunk_of_run += 1
            for b, s in open_span.items():
                if s[1] is None:
                    s[1] = chunk_of_run
                s[2] = chunk_of_run
        elif e[0] == "read":
            spans.append(tuple(open_span.pop(e[1])))
    assert len(spans) == len(caps)
    # position of every decode and reset in the log, decodes numbered like the runs
    where_decode, resets = {}, []
    d = -1
    for i, e in enumerate(log):
        if e[0] == "decode":
            d += 1
            where_decode[d] = i
        elif e[0] == "reset":
            resets.append((i, e[1]))
    assert len(resets) == len(caps)                                           # one per utterance that ran
    per_slot = {}
    for s in spans:
        per_slot.setdefault(s[0], []).append(s)
    for b, ss in per_slot.items():
        mine = [i for i, rb in resets if rb == b]
        assert len(mine) == len(ss)
        for j, (_, first, last) in enumerate(ss):
            assert mine[j] < where_decode[first], (b, j)                      # before its first chunk's decode
            if j > 0:
                assert mine[j] > where_decode[ss[j - 1][2]], (b, j)           # after the previous one's last
    # and the restart of the engine slot came before the decode of the previous utterance's last chunk
    restarts = [i for i, e in enumerate(log) if e[0] == "restart" and e[1] == 0]
    assert restarts[1] < where_decode[per_slot[0][0][2]]
    # the decode's active mask names exactly the slots that held an utterance in that chunk
    d = -1
    for e in log:
        if e[0] == "decode":
            d += 1
            want = tuple(any(s[0] == b and s[1] <= d <= s[2] for s in spans) for b in range(2))
            assert e[3] == want, (d, e, want)


def test_ring_rows_outlive_the_next_chunk():
    """A 16-frame history under chunks of 8: every chunk is decoded after the next one has been written."""
    batch, stub, codec, log = scheduler(2, {}, chunk=8, max_frames=16, codec_frames=16)
    for i in range(5):
        batch.submit(*prompt(), 16, i)
    evs, by = collect(batch, codec)
    assert stub.frames_run > 2 * 16
    for i in range(5):
        assert np.array_equal(np.concatenate([x.pcm for x in by[i]]), expected_pcm(i, 16, {})), i


def test_value_errors():
    batch, _, codec, _ = scheduler(2, {}, chunk=5, max_frames=9)
    batch.submit(*prompt(), 4, 0)
    with pytest.raises(ValueError, match="5.*9"):                             # 2 * chunk > max_frames
        next(batch.stream(codec))
    batch, _, codec, _ = scheduler(4, {}, codec_rows=3)
    batch.submit(*prompt(), 4, 0)
    with pytest.raises(ValueError, match="3.*4"):                             # codec rows < slots
        next(batch.stream(codec))
    batch, _, codec, _ = scheduler(2, {}, codec_frames=10)
    batch.submit(*prompt(), 11, 0)
    with pytest.raises(ValueError, match="10.*11"):                           # codec frames < the largest cap
        next(batch.stream(codec))
    batch, _, codec, log = scheduler(2, {}, chunk=4, max_frames=8, codec_frames=8)      # 2 * chunk == max_frames
    batch.submit(*prompt(), 8, 0)
    assert sum(len(e.pcm) for e in batch.stream(codec)) == 8 * FS
    assert list(batch.stream(codec)) == []                                    # nothing queued: ends at once


def test_stream_generate_queue_orders_by_prompt(monkeypatch):
    from csm_mlx import batching, tokenizers
    eos = {1235: 1}
    log = []
    monkeypatch.setattr(batching, "_EngineSlots", lambda model, slots, sampler, processors: StubEngine(slots, eos, 64, log))
    monkeypatch.setattr(tokenizers, "get_audio_tokenizer", lambda K: StubCodec(2, 64, log))
    caps = [5, 7, 2, 4, 3]
    got, finals = {}, {}
    for i, pcm, final in batching.stream_generate_queue(handle(max_frames=64), [prompt(3 + i) for i in range(5)],
                                                        slots=2, seeds=1234, max_audio_frames=caps, chunk=2):
        got.setdefault(i, []).append(pcm)
        finals.setdefault(i, []).append(final)
    for i in range(5):                                 # scalar seed s: s + i for prompt i
        assert np.array_equal(np.concatenate(got[i]), expected_pcm(1234 + i, caps[i], eos)), i
        assert finals[i][-1] and not any(finals[i][:-1])


def test_exports_and_abi():
    """The new calls are declared, exported and bound, and refuse a null codec before touching a device."""
    import csm_mlx
    from csm_mlx import _lib
    from csm_mlx.mimi import MimiCodec
    assert {"mimi_slot_reset", "mimi_decode_slots"} <= set(_lib.declared_symbols())
    L = _lib.lib()
    assert hasattr(L, "mimi_slot_reset") and hasattr(L, "mimi_decode_slots")
    assert L.mimi_slot_reset(None, 0) == _lib.CSM_ERR_ARG
    assert b"null codec" in L.csm_last_error()
    assert L.mimi_decode_slots(None, 1, 1, None, 0, 8, 0, None, None) == _lib.CSM_ERR_ARG
    with pytest.raises(ValueError):
        _lib.check(L.mimi_slot_reset(None, 0))
    assert callable(MimiCodec.slot_reset) and callable(MimiCodec.decode_slots)
    for name in ("StreamChunk", "stream_generate_queue", "SlotBatch", "generate_queue"):
        assert name in csm_mlx.__all__ and hasattr(csm_mlx, name)
    ev = csm_mlx.StreamChunk(3, np.zeros(0, np.float32), True)
    assert ev.ticket == 3 and ev.final and ev.codes is None
