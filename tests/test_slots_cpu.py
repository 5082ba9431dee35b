"""The SlotBatch scheduler (csm_mlx.batching) against a stub engine -- a small object with the slot calls and
scripted EOS frames -- and the slot ABI's argument checks that need no GPU."""
import numpy as np
import pytest

from helpers import STUB_K as K, StubEngine


def handle():
    from csm_mlx.models import CSM, csm_tiny
    return CSM(csm_tiny())                 # a host-side handle: no engine is created without a compute call


def prompt(L=5):
    return np.zeros((L, K + 1), np.int32), np.ones((L, K + 1), bool)


def scheduler(slots, eos, chunk=8):
    from csm_mlx.batching import SlotBatch
    from csm_mlx.sampling import Sampler
    stub = StubEngine(slots, eos)
    return SlotBatch(handle(), slots, sampler=Sampler(0.0, 0), chunk=chunk, _engine=stub), stub


def expected(seed, cap, eos):
    n = min(cap, eos.get(seed, cap))
    return np.array([[seed + 1, f + 1, 1, 1] for f in range(n)], np.int32).reshape(-1, K)


def test_chunks_stop_at_the_nearest_cap_and_no_slot_passes_its_cap():
    caps = [3, 20, 11, 8, 5, 30]
    eos = {1: 13, 5: 2}
    batch, stub = scheduler(3, eos, chunk=8)
    tickets = [batch.submit(*prompt(), caps[i], i) for i in range(len(caps))]
    out = dict(batch.run())
    for i, t in enumerate(tickets):
        assert np.array_equal(out[t], expected(i, caps[i], eos)), (i, out[t])
    # replay the log: frames each utterance ran
    ran, slot_seed = {}, {}
    for ev in stub.log:
        if ev[0] == "restart":
            slot_seed[ev[1]] = ev[2]
            ran[ev[2]] = 0
        elif ev[0] == "release":
            slot_seed.pop(ev[1], None)
        elif ev[0] == "read":
            slot_seed.pop(ev[1])
        elif ev[0] == "run":
            assert 1 <= ev[1] <= 8
            for s in slot_seed.values():
                ran[s] += ev[1]
                assert ran[s] <= caps[s], f"utterance {s} stepped past its cap"
    assert ran[0] == 3 and stub.log[[e[0] for e in stub.log].index("run")] == ("run", 3)   # shortened to the cap of 3
    for s, c in enumerate(caps):                   # at most chunk - 1 frames past EOS, never past the cap
        assert ran[s] <= min(c, eos.get(s, c) + 1 + 7)


def test_joins_of_a_boundary_share_one_prefill():
    batch, stub = scheduler(4, {}, chunk=4)
    for i in range(10):
        batch.submit(*prompt(), 4, i)
    out = dict(batch.run())
    assert len(out) == 10
    kinds = [e[0] for e in stub.log]
    # between two runs there is at most one prefill, and it names every slot restarted at that boundary
    boundary = []
    for ev in stub.log + [("run", 0)]:
        if ev[0] == "run":
            restarted = tuple(e[1] for e in boundary if e[0] == "restart")
            prefills = [e[1] for e in boundary if e[0] == "prefill"]
            assert prefills == ([restarted] if restarted else []), boundary
            boundary = []
        else:
            boundary.append(ev)
    assert stub.log[:5] == [("restart", 0, 0), ("restart", 1, 1), ("restart", 2, 2), ("restart", 3, 3),
                            ("prefill", (0, 1, 2, 3))]
    assert kinds.count("prefill") == 3             # 4 + 4 + 2 joins


def test_result_order_and_queue_shorter_than_the_slots():
    batch, stub = scheduler(8, {0: 0}, chunk=8)
    tickets = [batch.submit(*prompt(), c, s) for s, c in enumerate((6, 2, 9))]
    got = list(batch.run())                        # terminates with 5 slots never used
    assert sorted(t for t, _ in got) == tickets
    assert [e for e in stub.log if e[0] == "release"][:5] == [("release", b) for b in range(3, 8)]
    out = dict(got)
    assert len(out[tickets[0]]) == 0               # EOS at its first frame: the empty result
    assert len(out[tickets[1]]) == 2 and len(out[tickets[2]]) == 9
    assert list(batch.run()) == []                 # nothing queued: ends at once


def test_generate_queue_orders_by_prompt(monkeypatch):
    from csm_mlx import batching
    eos = {1235: 1}
    made = []

    def stub_engine(model, slots, sampler, processors):
        made.append(StubEngine(slots, eos))
        return made[-1]
    monkeypatch.setattr(batching, "_EngineSlots", stub_engine)
    caps = [5, 7, 2, 4, 3]
    out = batching.generate_queue(handle(), [prompt(3 + i) for i in range(5)], slots=2, seeds=1234,
                                  max_audio_frames=caps, decode=False)
    for i, c in enumerate(out):                    # scalar seed s: s + i for prompt i
        assert np.array_equal(c, expected(1234 + i, caps[i], eos)), (i, c)


def test_host_samplers_and_host_processors_are_refused():
    from csm_mlx import make_logits_processors, make_sampler
    from csm_mlx.batching import SlotBatch, generate_queue
    from csm_mlx.sampling import HostSampler, Sampler
    m = handle()
    host = make_sampler(0.8, xtc_probability=0.1)
    assert isinstance(host, HostSampler)
    with pytest.raises(ValueError):
        SlotBatch(m, 2, sampler=host, _engine=StubEngine(2, {}))
    with pytest.raises(ValueError):
        SlotBatch(m, 2, sampler=Sampler(0.0, 0), logits_processors=[lambda t, l: l], _engine=StubEngine(2, {}))
    with pytest.raises(ValueError):                # context 0 is the whole history: the host's
        SlotBatch(m, 2, sampler=Sampler(0.0, 0), _engine=StubEngine(2, {}),
                  logits_processors=make_logits_processors(repetition_penalty=1.3, repetition_context_size=0))
    with pytest.raises(ValueError):
        generate_queue(m, [prompt()], slots=2, sampler=lambda lp: lp.argmax(-1))
    ok = SlotBatch(m, 2, sampler=Sampler(0.8, 50), _engine=StubEngine(2, {}),
                   logits_processors=make_logits_processors(logit_bias={0: -2.0}, repetition_penalty=1.5,
                                                            repetition_context_size=8))
    with pytest.raises(ValueError):                # the reference's window guard is the admission rule
        ok.submit(*prompt(2000), 100)
    with pytest.raises(ValueError):
        SlotBatch(m, 0, sampler=Sampler(0.0, 0), _engine=StubEngine(1, {}))


def test_cap_beyond_the_history_is_a_state_error():
    from csm_mlx import _lib
    from csm_mlx.batching import SlotBatch
    from csm_mlx.models import CSM, csm_tiny
    from csm_mlx.sampling import Sampler
    m = CSM(csm_tiny(), max_frames=48)
    batch = SlotBatch(m, 2, sampler=Sampler(0.0, 0), _engine=StubEngine(2, {}))
    batch.submit(*prompt(), 48)
    with pytest.raises(_lib.CsmHipError) as ei:
        batch.submit(*prompt(), 49)
    assert ei.value.code == _lib.CSM_ERR_STATE
    with pytest.raises(ValueError):
        CSM(csm_tiny(), max_frames=0)


def test_slot_abi_argument_checks():
    """Null engines are refused before anything touches a device; the calls are declared and bound."""
    import ctypes
    from csm_mlx import _lib
    L = _lib.lib()
    assert {"csm_slot_restart", "csm_slot_release", "csm_slot_read"} <= set(_lib.declared_symbols())
    n, d = ctypes.c_int(0), ctypes.c_uint8(0)
    assert L.csm_slot_restart(None, 0, 1) == _lib.CSM_ERR_ARG
    assert b"null engine" in L.csm_last_error()
    assert L.csm_slot_release(None, 0) == _lib.CSM_ERR_ARG
    assert L.csm_slot_read(None, 0, None, 0, ctypes.byref(n), ctypes.byref(d)) == _lib.CSM_ERR_ARG
    with pytest.raises(ValueError):
        _lib.check(L.csm_slot_restart(None, 0, 1))
