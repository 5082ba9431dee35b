"""The frame loops of csm_mlx.generation -- ``generate_codes_batch``, ``stream_generate_batch``,
``stream_generate`` in their three modes (plain, host logits processors, host sampler) -- against a recording
stub ``FrameCache`` and a recording stub codec: the order of the calls, where EOS is tested, the codec resets,
the window guard.  No engine is created; only the public functions are driven."""
import numpy as np
import pytest

from csm_mlx import generation
from csm_mlx.sampling import HostSampler, Sampler

FRAMES = 4                      # the frame budget of every case unless it says otherwise
ENDS = (1, 2)                   # utterance b produces its all-zero frame at frame ENDS[b]: all done at frame 2
LOG = []


class StubCache(generation.FrameCache):
    """``FrameCache`` with every engine-touching method replaced: each logs itself with the index of the frame
    it ran.  The codes of frame f are all f; utterance b is done from frame ENDS[b] on."""

    def __init__(self, model, batch_size, sampler, seeds=None, processors=None):
        self.model, self.B, self.sampler, self.seeds, self.frames = model, batch_size, sampler, seeds, 0
        LOG.append(("begin", batch_size, processors))

    def _done(self, frames):
        return np.array([frames > e for e in ENDS[: self.B]], bool)

    def prefill(self, b, tokens, mask):
        LOG.append(("prefill", b))

    def prefill_batch(self, items):
        LOG.append(("prefill_batch", tuple(b for b, _, _ in items)))

    def run(self, nframes, sync=True):
        assert nframes == 1
        LOG.append(("run", self.frames, sync))
        self.frames += 1
        return bool(sync and self._done(self.frames).all())

    def run_ahead(self, nframes):
        prev = None if self.frames == 0 else bool(self._done(self.frames).all())
        LOG.append(("run_ahead", nframes, prev))
        self.frames += nframes
        return prev

    def run_processed(self, processors, c0_history):
        LOG.append(("processed", self.frames, tuple(processors), len(c0_history)))
        self.frames += 1
        c0_history.append(self.last_codes()[:, :1])
        return bool(self._done(self.frames).all())

    def run_host_sampled(self, sampler, processors=(), c0_history=None):
        LOG.append(("host_sampled", self.frames, sampler, tuple(processors), len(c0_history)))
        self.frames += 1
        c0_history.append(self.last_codes()[:, :1])
        return bool(self._done(self.frames).all())

    def codes(self):
        K = self.model.n_audio_codebooks
        n = np.minimum(self.frames, np.array(ENDS[: self.B])).astype(np.int32)
        return np.zeros((self.frames, self.B, K), np.int32), n, self._done(self.frames).astype(np.uint8)

    def done(self):
        LOG.append(("poll", self.frames - 1))
        return self._done(self.frames)

    def last_codes(self):
        return np.full((self.B, self.model.n_audio_codebooks), self.frames - 1, np.int32)


class StubCodec:
    def reset_state(self, batch_size=1):
        LOG.append(("reset", batch_size))

    def decode_step(self, codes):
        assert (codes == codes[0, 0]).all()
        LOG.append(("decode", int(codes[0, 0])))
        return np.full((codes.shape[0], 1, 1920), float(codes[0, 0]), np.float32)


@pytest.fixture
def model(monkeypatch):
    from csm_mlx.models import CSM, csm_tiny
    LOG.clear()
    monkeypatch.setattr(generation, "FrameCache", StubCache)
    monkeypatch.setattr(generation, "get_audio_tokenizer", lambda K: StubCodec())
    return CSM(csm_tiny())         # a host-side handle: no engine is created without a compute call


def prompts(model, B=2, L=5):
    K = model.n_audio_codebooks
    return [(np.zeros((L + b, K + 1), np.int32), np.ones((L + b, K + 1), bool)) for b in range(B)]


def keep(*kinds):
    return [e for e in LOG if e[0] in kinds]


def host_processor(tokens, logits):
    return logits


def host_sampler(logits):
    return logits.argmax(-1)


def test_stream_batch_plain_runs_one_frame_ahead(model):
    evs = list(generation.stream_generate_batch(model, prompts(model), FRAMES * 80, sampler=Sampler(0.0, 0)))
    assert LOG[:3] == [("begin", 2, None), ("prefill_batch", (0, 1)), ("reset", 2)]
    # enqueue f + 1, decode f, poll -- and frame 2, at which every utterance is done, is never decoded
    assert LOG[3:-1] == [("run", 0, False), ("poll", 0),
                         ("run", 1, False), ("decode", 0), ("poll", 1),
                         ("run", 2, False), ("decode", 1), ("poll", 2)]
    assert LOG[-1] == ("reset", 2) and len(keep("reset")) == 2
    assert len(evs) == 2
    for f, (pcm, done) in enumerate(evs):
        assert pcm.shape == (2, 1920) and pcm.dtype == np.float32 and (pcm == f).all()
        assert done.tolist() == [f >= 1, False]


def test_stream_batch_resets_the_codec_when_closed_early(model):
    gen = generation.stream_generate_batch(model, prompts(model), FRAMES * 80, sampler=Sampler(0.0, 0))
    next(gen)
    assert keep("reset") == [("reset", 2)]
    gen.close()
    assert keep("reset") == [("reset", 2)] * 2 and LOG[-1] == ("reset", 2)
    assert keep("decode") == [("decode", 0)]


@pytest.mark.parametrize("mode", ["processed", "host_sampled"])
def test_stream_batch_host_modes_test_eos_before_the_decode(model, mode):
    smp = Sampler(0.0, 0) if mode == "processed" else HostSampler(host_sampler)
    evs = list(generation.stream_generate_batch(model, prompts(model), FRAMES * 80, sampler=smp,
                                                logits_processors=[host_processor]))
    assert LOG[:3] == [("begin", 2, None), ("prefill_batch", (0, 1)), ("reset", 2)] and LOG[-1] == ("reset", 2)
    assert [e[:2] for e in LOG[3:-1]] == [(mode, 0), ("decode", 0), ("poll", 0),
                                           (mode, 1), ("decode", 1), ("poll", 1),
                                           (mode, 2)]                  # once per frame; all done: no decode
    frames = keep(mode)
    assert [e[-1] for e in frames] == [0, 1, 2]                        # one c0 history through the frames
    assert all(e[-2] == (host_processor,) for e in frames)
    if mode == "host_sampled":
        assert all(e[2] is smp for e in frames)
    assert len(evs) == 2 and [d.tolist() for _, d in evs] == [[False, False], [True, False]]
    assert not keep("run", "run_ahead")


def test_stream_batch_host_sampler_without_processors(model):
    list(generation.stream_generate_batch(model, prompts(model), FRAMES * 80, sampler=host_sampler))
    frames = keep("host_sampled")
    assert len(frames) == 3 and all(isinstance(e[2], HostSampler) and e[3] == () for e in frames)
    assert not keep("processed", "run")


@pytest.mark.parametrize("chunk,budget,want", [
    (1, FRAMES, [(1, None), (1, False), (1, False), (1, True)]),       # the report is one chunk behind
    (3, FRAMES, [(3, None), (1, True)]),                               # the last chunk shortened to the budget
    (1, 8, [(1, None), (1, False), (1, False), (1, True)]),            # stops after the chunk that reports it
    (2, 8, [(2, None), (2, False), (2, True)]),
])
def test_codes_batch_plain_polls_one_chunk_behind(model, chunk, budget, want):
    hist, n_frames, cache = generation.generate_codes_batch(model, prompts(model), budget, sampler=Sampler(0.0, 0),
                                                            chunk=chunk)
    assert LOG[:2] == [("begin", 2, None), ("prefill_batch", (0, 1))]
    assert [e[1:] for e in LOG[2:]] == want and not keep("run", "processed", "host_sampled")
    assert isinstance(cache, StubCache) and n_frames.tolist() == [1, 2] and hist.shape[0] == cache.frames


@pytest.mark.parametrize("mode", ["processed", "host_sampled"])
def test_codes_batch_host_modes_stop_at_the_first_all_done_frame(model, mode):
    smp = Sampler(0.0, 0) if mode == "processed" else HostSampler(host_sampler)
    _, n_frames, cache = generation.generate_codes_batch(model, prompts(model), FRAMES, sampler=smp,
                                                         logits_processors=[host_processor])
    assert [e[:2] for e in LOG[2:]] == [(mode, 0), (mode, 1), (mode, 2)]
    assert cache.frames == 3 and n_frames.tolist() == [1, 2]


def test_codes_batch_of_one_prompt_prefills_it_alone(model):
    generation.generate_codes_batch(model, prompts(model, 1), FRAMES, sampler=Sampler(0.0, 0))
    assert LOG[:2] == [("begin", 1, None), ("prefill", 0)]


@pytest.mark.parametrize("mode", ["plain", "processed", "host_sampled"])
def test_stream_generate_yields_the_rows_of_the_same_loop(model, mode):
    kw = {"plain": dict(), "processed": dict(logits_processors=[host_processor]),
          "host_sampled": dict(sampler=host_sampler)}[mode]
    gen = generation.stream_generate(model, [998, 5, 17, 999], 0, [], FRAMES * 80, temperature=0.0, **kw)
    rows = list(gen)
    assert LOG[:3] == [("begin", 1, None), ("prefill", 0), ("reset", 1)] and LOG[-1] == ("reset", 1)
    assert len(rows) == 1 and rows[0].shape == (1920,) and rows[0].dtype == np.float32   # done at frame 1
    assert keep("decode") == [("decode", 0)]
    if mode == "plain":
        assert LOG[3:-1] == [("run", 0, False), ("poll", 0), ("run", 1, False), ("decode", 0), ("poll", 1)]
    else:
        assert [e[:2] for e in LOG[3:-1]] == [(mode, 0), ("decode", 0), ("poll", 0), (mode, 1)]


def test_stream_generate_resets_the_codec_when_closed_early(model, monkeypatch):
    monkeypatch.setattr(StubCache, "_done", lambda self, frames: np.zeros(self.B, bool))     # never ends
    gen = generation.stream_generate(model, [998, 5, 17, 999], 0, [], FRAMES * 80, temperature=0.0)
    next(gen)
    gen.close()
    assert keep("reset") == [("reset", 1)] * 2 and LOG[-1] == ("reset", 1)


def test_device_processors_leave_the_plain_loop(model):
    from csm_mlx import make_logits_processors
    procs = make_logits_processors(logit_bias={3: -1.0}, repetition_penalty=1.2, repetition_context_size=4)
    evs = list(generation.stream_generate_batch(model, prompts(model), FRAMES * 80, sampler=Sampler(0.8, 10),
                                                logits_processors=procs))
    assert LOG[0][:2] == ("begin", 2) and LOG[0][2] is not None and len(LOG[0][2]) == 2
    assert len(evs) == 2 and len(keep("run")) == 3 and not keep("processed", "host_sampled")


def test_window_guard_comes_before_any_call(model):
    K = model.n_audio_codebooks
    L = model.max_seq_len - FRAMES
    bad = prompts(model) + [(np.zeros((L, K + 1), np.int32), np.ones((L, K + 1), bool))]
    with pytest.raises(ValueError, match="Inputs too long"):
        next(generation.stream_generate_batch(model, bad, FRAMES * 80, sampler=Sampler(0.0, 0)))
    with pytest.raises(ValueError, match="Inputs too long"):
        generation.generate_codes_batch(model, bad, FRAMES, sampler=Sampler(0.0, 0))
    with pytest.raises(ValueError, match="Inputs too long"):
        generation.generate_batch(model, bad, FRAMES * 80)
    with pytest.raises(ValueError, match="Inputs too long"):
        next(generation.stream_generate(model, [998] + [5] * L + [999], 0, [], FRAMES * 80))
    assert LOG == []
