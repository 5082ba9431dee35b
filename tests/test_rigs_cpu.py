"""The shared rigs of the GPU tests (tests/rigs.py) against stub objects, without a GPU or the built library: a
rig that quietly stopped checking would weaken every file that calls it.

* ``ab`` runs the off leg, then the on leg, and fails unless the epoch moved by exactly the count it was given;
* ``frame_taps`` cuts the padded vocabulary (V = 5 in rows of Vp = 8), reads only the kept frames, lets a
  ``step`` stand in for ``cache.run(1)`` and a ``prefill`` for the prompt feeding, and returns copies;
* ``codes_per_utterance`` cuts every utterance at its own frame count;
* ``handoffs`` holds the literals the test files used to carry (through test_f64_taps_gpu._expect)."""
import ctypes
import itertools

import numpy as np
import pytest

from rigs import TAP_NAMES, ab, codes_per_utterance, frame_taps, handoffs

B, K, V, D = 2, 3, 5, 4
PAD = -777.0                                      # what the stub writes into the padding columns


class StubModel:
    n_audio_codebooks, n_audio_vocab, n_backbone_embedding, engine = K, V, D, None


def tap_value(what, f):
    """The stub engine's tap after frame f, in the engine's own layout, without padding."""
    b, v, d, i = np.arange(B), np.arange(V), np.arange(D), np.arange(K - 1)
    if what == "h_last":
        return (1000 * f + 500 + 10 * b[:, None] + d[None, :]).astype(np.float32)                             # (B, D)
    if what == "c0_logits":
        return (1000 * f + 10 * b[:, None] + v[None, :]).astype(np.float32)                                   # (B, V)
    return (1000 * f + 100 * (i[:, None, None] + 1) + 10 * b[None, :, None] + v[None, None, :]).astype(np.float32)


class StubCache:
    """FrameCache as ``frame_taps`` uses it; every call is logged, every buffer handed out is kept."""
    made = []

    def __init__(self, model, batch_size, sampler, seeds=None, processors=None):
        self.args = (batch_size, sampler, seeds, processors)
        self.frame, self.log, self.bufs = -1, [], []
        StubCache.made.append(self)

    def prefill(self, b, tokens, mask):
        self.log.append(("prefill", b))

    def prefill_batch(self, items):
        self.log.append(("prefill_batch", [b for b, _, _ in items]))

    def run(self, n):
        assert n == 1
        self.frame += 1
        self.log.append(("run", self.frame))

    def debug(self, what, shape):
        self.log.append((what, self.frame))
        buf = np.full(shape, PAD, np.float32)
        val = tap_value(what, self.frame)
        buf[..., : val.shape[-1]] = val
        self.bufs.append(buf)
        return buf

    def codes(self):
        F = self.frame + 1
        return np.arange(F * B * K, dtype=np.int32).reshape(F, B, K), np.full(B, F, np.int32), np.zeros(B, np.uint8)


@pytest.fixture
def cache(monkeypatch):
    from csm_mlx import generation
    monkeypatch.setattr(generation, "FrameCache", StubCache)
    StubCache.made.clear()
    return StubCache


PROMPTS = [(np.zeros((3, K + 1), np.int32), np.ones((3, K + 1), bool))] * B


def test_frame_taps_cut_the_padding_and_keep_the_layout(cache):
    hist, n, taps = frame_taps(StubModel, PROMPTS, 3, "sampler", [11, 12], TAP_NAMES)
    c = cache.made[0]
    assert len(cache.made) == 1 and c.args == (B, "sampler", [11, 12], None)
    assert c.log[:2] == [("prefill", 0), ("prefill", 1)]
    assert hist.shape == (3, B, K) and list(n) == [3, 3]
    assert taps["h_last"].shape == (3, B, D) and taps["c0_logits"].shape == (3, B, V)
    assert taps["ci_logits"].shape == (3, B, K - 1, V)
    for f in range(3):
        assert np.array_equal(taps["h_last"][f], tap_value("h_last", f))
        assert np.array_equal(taps["c0_logits"][f], tap_value("c0_logits", f))
        assert np.array_equal(taps["ci_logits"][f], tap_value("ci_logits", f).transpose(1, 0, 2))
    assert all(PAD not in t for t in taps.values())
    assert all(b.shape[-1] == 8 for b in c.bufs if b.shape[-1] != D), "the stub was not asked for rows of Vp = 8"
    # taps are read in the engine's order after every frame
    assert c.log[2:] == [x for f in range(3) for x in [("run", f)] + [(t, f) for t in TAP_NAMES]]


def test_frame_taps_read_only_the_kept_frames_and_taps(cache):
    hist, n, taps = frame_taps(StubModel, PROMPTS, 3, "sampler", None, ("ci_logits", "c0_logits"), keep={1})
    assert sorted(taps) == ["c0_logits", "ci_logits"]
    assert taps["c0_logits"].shape == (1, B, V) and taps["ci_logits"].shape == (1, B, K - 1, V)
    assert np.array_equal(taps["c0_logits"][0], tap_value("c0_logits", 1))
    assert np.array_equal(taps["ci_logits"][0], tap_value("ci_logits", 1).transpose(1, 0, 2))
    assert [x for x in cache.made[0].log if x[0] in TAP_NAMES] == [("c0_logits", 1), ("ci_logits", 1)]
    assert hist.shape[0] == 3                                        # every frame ran
    with pytest.raises(AssertionError):
        frame_taps(StubModel, PROMPTS, 1, "sampler", None, ("c1_logits",))


def test_frame_taps_return_copies(cache):
    _, _, taps = frame_taps(StubModel, PROMPTS, 2, "sampler", None, TAP_NAMES)
    want = {t: a.copy() for t, a in taps.items()}
    for buf in cache.made[0].bufs:
        buf[...] = PAD
    assert all(np.array_equal(taps[t], want[t]) and taps[t].flags.owndata for t in taps)


def test_frame_taps_step_and_batched_prefill(cache):
    stepped = []

    def step(c, f):
        stepped.append(f)
        c.frame += 1
    _, _, taps = frame_taps(StubModel, PROMPTS, 2, "sampler", None, ("c0_logits",), step=step, processors=("bias", "pen"),
                            prefill_batch=True)
    c = cache.made[0]
    assert stepped == [0, 1] and not [x for x in c.log if x[0] == "run"]
    assert c.args[3] == ("bias", "pen") and c.log[0] == ("prefill_batch", [0, 1])
    assert np.array_equal(taps["c0_logits"][1], tap_value("c0_logits", 1))


def test_codes_per_utterance_cuts_each_at_its_own_length(monkeypatch):
    from csm_mlx import generation
    hist = np.arange(4 * 3 * K, dtype=np.int32).reshape(4, 3, K)
    seen = {}

    def stub(model, prompts, frames, *, sampler, seeds=None, logits_processors=None):
        seen.update(frames=frames, sampler=sampler, seeds=seeds, procs=logits_processors, n=len(prompts))
        return hist, np.array([0, 1, 4], np.int32), None
    monkeypatch.setattr(generation, "generate_codes_batch", stub)
    got = codes_per_utterance(StubModel, ["p0", "p1", "p2"], 4, "sampler", [5, 6, 7], ["proc"])
    assert seen == dict(frames=4, sampler="sampler", seeds=[5, 6, 7], procs=["proc"], n=3)
    assert [len(g) for g in got] == [0, 1, 4] and got[0].shape == (0, K)
    assert np.array_equal(got[1], hist[:1, 1]) and np.array_equal(got[2], hist[:, 2])
    want = hist.copy()
    hist[...] = -1
    assert np.array_equal(got[2], want[:, 2]), "the codes are views of the engine's history"
    codes_per_utterance(StubModel, ["p0", "p1", "p2"], 4, "sampler")
    assert seen["seeds"] is None and seen["procs"] is None


class StubLib:
    """csm_set_option / csm_debug_read of an engine whose kernel, with its option on, moves its epoch by
    ``per_run`` in every run."""

    def __init__(self, per_run):
        self.per_run, self.options, self.epochs, self.log = per_run, {}, {"dec_xsd_epoch": 4_000_000_000}, []

    def csm_set_option(self, engine, key, value):
        self.options[key.decode()] = value
        self.log.append(("set", key.decode(), value))
        return 0

    def csm_debug_read(self, engine, name, ptr, nbytes, _):
        assert nbytes == 4
        ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint32))[0] = self.epochs[name.decode()]
        return 0

    def run(self):
        on = self.options["dec_xsd"]
        self.log.append(("run", on))
        if on:
            self.epochs["dec_xsd_epoch"] += self.per_run
        return "on" if on else "off"


@pytest.mark.parametrize("per_run", [60, 59, 61, 0])
def test_ab_holds_the_epoch_to_the_exact_count(monkeypatch, per_run):
    from csm_mlx import _lib
    stub = StubLib(per_run)
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    if per_run == 60:
        assert ab(StubModel, "dec_xsd", stub.run, 60) == ("off", "on")
    else:
        with pytest.raises(AssertionError, match="dec_xsd"):
            ab(StubModel, "dec_xsd", stub.run, 60)
    assert stub.log == [("set", "dec_xsd", 0), ("run", 0), ("set", "dec_xsd", 1), ("run", 1)]     # off, then on; left on
    with pytest.raises(TypeError):
        ab(StubModel, "dec_xsd", stub.run)                          # the count has no default


@pytest.mark.parametrize("K_,B_", [(32, 1), (32, 8), (4, 2)])
def test_handoff_table_matches_the_literals(K_, B_):
    """The counts as the test files wrote them before the table: 498 per dec_frame frame, 80 per backbone
    step, K - 2 per dec_xsd frame; test_f64_taps_gpu._expect over its 2 frames."""
    from test_f64_taps_gpu import FRAMES, _expect
    assert FRAMES == 2
    assert (handoffs("dec_frame", K_), handoffs("bb_step", K_), handoffs("dec_xsd", K_)) == (498, 80, K_ - 2)
    for df, xsd, bb in itertools.product([False, True], repeat=3):
        old = {"dec_frame_epoch": 498 * 2 if df else 0, "dec_xsd_epoch": (K_ - 2) * 2 if xsd else 0,
               "bb_step_epoch": 80 * (2 - 1) * B_ if bb else 0}
        assert _expect(K_, B_, dec_frame=df, dec_xsd=xsd, bb_step=bb) == old
    with pytest.raises(KeyError):
        handoffs("bb_xs", K_)


def test_frame_taps_custom_prefill(cache):
    fed = []
    _, _, taps = frame_taps(StubModel, PROMPTS, 1, "sampler", None, ("h_last",), prefill=fed.append)
    c = cache.made[0]
    assert fed == [c] and not [x for x in c.log if x[0].startswith("prefill")]
    assert np.array_equal(taps["h_last"][0], tap_value("h_last", 0))
