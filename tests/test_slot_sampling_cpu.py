"""Per-utterance sampling parameters in the SlotBatch scheduler (csm_mlx.batching) against a stub engine that
logs ``set_sampling``, and the new ABI call's prototype against the header: no GPU."""
import ctypes
import re

import numpy as np
import pytest

from helpers import STUB_K as K, StubEngine


class SamplingStub(StubEngine):
    """``StubEngine`` plus the call a job with an override makes right after its slot's restart."""

    def set_sampling(self, b, sampler, processors):
        assert not self.pending
        assert self.seed[b] is not None and not self.prompt[b], "set_sampling belongs between restart and prefill"
        self.log.append(("set_sampling", b, sampler, processors))


def handle():
    from csm_mlx.models import CSM, csm_tiny
    return CSM(csm_tiny())                 # a host-side handle: no engine is created without a compute call


def prompt(L=5):
    return np.zeros((L, K + 1), np.int32), np.ones((L, K + 1), bool)


def test_set_sampling_follows_the_restart_of_its_slot_and_only_for_overrides():
    from csm_mlx import make_logits_processors
    from csm_mlx.batching import SlotBatch
    from csm_mlx.generation import device_processors
    from csm_mlx.sampling import Sampler
    stub = SamplingStub(2, {})
    batch = SlotBatch(handle(), 2, sampler=Sampler(0.0, 0), chunk=4, _engine=stub)
    hot, procs = Sampler(0.8, 50), make_logits_processors(logit_bias={0: -2.0}, repetition_penalty=1.5,
                                                           repetition_context_size=8)
    over = {1: (hot, None), 3: (None, device_processors(procs, hot)), 4: (hot, (None, None))}
    for i in range(6):                      # seeds 0..5; 1, 3 and 4 carry an override
        kw = {}
        if i in over:
            kw = {"sampler": over[i][0], "logits_processors": {1: None, 3: procs, 4: []}[i]}
        batch.submit(*prompt(), 4, i, **kw)
    assert len(dict(batch.run())) == 6
    seen = {}
    for j, ev in enumerate(stub.log):
        if ev[0] == "set_sampling":
            prev = stub.log[j - 1]
            assert prev[0] == "restart" and prev[1] == ev[1], (prev, ev)      # right after its own slot's restart
            seen[prev[2]] = ev[2:]
    assert seen == over                     # jobs without an override make no call; None means the batch's


def test_generate_queue_maps_samplers_and_processors_to_prompts(monkeypatch):
    from csm_mlx import batching, make_logits_processors
    from csm_mlx.sampling import Sampler
    made = []

    def stub_engine(model, slots, sampler, processors):
        made.append(SamplingStub(slots, {}))
        return made[-1]
    monkeypatch.setattr(batching, "_EngineSlots", stub_engine)
    samplers = [None, Sampler(0.8, 50), None, Sampler(1.2, 5), Sampler(0.7, 0, 0.9, 0.05)]
    procs = [None, None, make_logits_processors(logit_bias={3: 1.0}), None, None]
    out = batching.generate_queue(handle(), [prompt(3 + i) for i in range(5)], slots=2, seeds=100, decode=False,
                                  max_audio_frames=[3] * 5, samplers=samplers, prompt_processors=procs)
    assert len(out) == 5
    log = made[0].log
    by_seed = {log[j - 1][2]: ev for j, ev in enumerate(log) if ev[0] == "set_sampling"}
    assert sorted(by_seed) == [101, 102, 103, 104]                     # prompt i runs under seed 100 + i
    for i in (1, 3, 4):
        assert by_seed[100 + i][2] is samplers[i] and by_seed[100 + i][3] is None
    assert by_seed[102][2] is None and by_seed[102][3][0].indices == (3,) and by_seed[102][3][1] is None
    for kw in ({"samplers": samplers[:4]}, {"prompt_processors": procs + [None]}):
        with pytest.raises(ValueError, match="per prompt"):
            batching.generate_queue(handle(), [prompt() for _ in range(5)], slots=2, decode=False, **kw)
    with pytest.raises(ValueError, match="per prompt"):
        list(batching.stream_generate_queue(handle(), [prompt() for _ in range(5)], slots=2, samplers=samplers[:2]))


def test_submit_refuses_what_the_gpu_cannot_run():
    from csm_mlx import make_logits_processors, make_sampler
    from csm_mlx.batching import SlotBatch
    from csm_mlx.sampling import HostSampler, Sampler
    batch = SlotBatch(handle(), 2, sampler=Sampler(0.0, 0), _engine=SamplingStub(2, {}))
    host = make_sampler(0.8, xtc_probability=0.1)
    assert isinstance(host, HostSampler)
    with pytest.raises(ValueError, match="samples on the GPU"):
        batch.submit(*prompt(), 4, sampler=host)
    with pytest.raises(ValueError, match="samples on the GPU"):
        batch.submit(*prompt(), 4, sampler=lambda lp: lp.argmax(-1))
    both = make_logits_processors(logit_bias={0: -2.0}, repetition_penalty=1.5, repetition_context_size=8)
    with pytest.raises(ValueError, match="on the GPU only"):           # penalty before bias: not mlx_lm's order
        batch.submit(*prompt(), 4, logits_processors=both[::-1])
    with pytest.raises(ValueError, match="on the GPU only"):
        batch.submit(*prompt(), 4, logits_processors=[lambda t, l: l])
    with pytest.raises(ValueError, match="logit_bias index"):
        batch.submit(*prompt(), 4, logits_processors=make_logits_processors(logit_bias={10 ** 6: 1.0}))
    assert not batch._queue                                             # nothing refused was queued
    assert batch.submit(*prompt(), 4, sampler=Sampler(0.8, 50), logits_processors=both) == 0


def test_prototype_matches_the_header():
    """csm_slot_set_sampling is declared, bound with one ctypes argument per C parameter, and _lib.CsmSampling
    lists csm_sampling's fields in the header's order with the header's types."""
    from csm_mlx import _lib
    assert "csm_slot_set_sampling" in _lib.declared_symbols()
    text = open(_lib.HEADER_PATH).read()
    params = re.search(r"int\s+csm_slot_set_sampling\s*\(([^)]*)\)", text).group(1).split(",")
    assert [p.split()[-1].lstrip("*") for p in params] == ["e", "b", "s"]
    fn = _lib.lib().csm_slot_set_sampling
    assert fn.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(_lib.CsmSampling)] and fn.restype is ctypes.c_int
    body = re.search(r"typedef struct csm_sampling\s*\{(.*?)\}\s*csm_sampling;", text, re.S).group(1)
    ctype = {"float": ctypes.c_float, "int": ctypes.c_int, "double": ctypes.c_double,
             "const int32_t*": ctypes.POINTER(ctypes.c_int32), "const float*": ctypes.POINTER(ctypes.c_float)}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        typ, names = re.match(r"((?:const\s+)?\w+\*?)\s+(.*)", decl).groups()
        fields += [(n.strip(), ctype[typ]) for n in names.split(",")]
    assert fields == list(_lib.CsmSampling._fields_)
    assert fn(None, 0, None) == _lib.CSM_ERR_ARG and b"null engine" in _lib.lib().csm_last_error()
