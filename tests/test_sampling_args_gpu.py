"""The engine's value checks on sampling parameters, pinned on both ways a row's sampler and c0 processors
reach it: the batch's calls (csm_begin, csm_set_sampler_filters, csm_set_c0_processors) and the slot's
(csm_slot_set_sampling).  Every bad value is refused by both with the same exception type and the same
message, and a logit_bias that names an index twice takes the last value on both.

The C calls are made directly: the package checks bias indices itself before the engine sees them.  csm_tiny,
two rows; no frame runs except the one whose processed c0 logits are read back."""
import ctypes

import numpy as np
import pytest

from helpers import tiny_prompt_ids
from rigs import build_model, read_taps

pytestmark = pytest.mark.gpu

I32, F32 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope="module")
def tiny():
    args, _, model = build_model("tiny", "float32", max_batch=2)
    yield args, model
    del model


def arrays(idx, val):
    """(int32 indices, float32 values) of a bias, None for a null pointer"""
    return (None if idx is None else np.asarray(idx, np.int32)), (None if val is None else np.asarray(val, np.float32))


def sampling(temperature=0.8, top_k=5, top_p=0.0, min_p=0.0, min_keep=1, n_bias=None, idx=(), val=(), penalty=0.0,
             context=0):
    """A csm_sampling; n_bias defaults to the length of idx, idx / val None is a null pointer."""
    from csm_mlx import _lib
    i, v = arrays(idx, val)
    s = _lib.CsmSampling(temperature, top_k, top_p, min_p, min_keep, len(i) if n_bias is None else n_bias,
                         i.ctypes.data_as(I32) if i is not None else I32(), v.ctypes.data_as(F32) if v is not None else F32(),
                         penalty, context)
    s._keep = (i, v)
    return s


def begin(model, temperature=0.8, top_k=5):
    """A fresh batch of two rows through the package, so that older caches of the model are superseded."""
    from csm_mlx.generation import FrameCache
    from csm_mlx.sampling import Sampler
    return FrameCache(model, 2, Sampler(temperature, top_k), [7, 8])


def slots(model, temperature=0.8, top_k=5):
    """A fresh batch of two slots, both holding a new utterance."""
    from csm_mlx.batching import _EngineSlots
    from csm_mlx.sampling import Sampler
    eng = _EngineSlots(model, 2, Sampler(temperature, top_k), None)
    eng.restart(0, 7)
    eng.restart(1, 8)
    return eng


def set_filters(top_p=0.0, min_p=0.0, min_keep=1):
    return lambda model: begin(model)._call("csm_set_sampler_filters", top_p, min_p, min_keep)


def set_processors(n_bias=None, idx=(), val=(), penalty=0.0, context=0):
    def call(model):
        from csm_mlx import _lib
        i, v = arrays(idx, val)
        begin(model)._call("csm_set_c0_processors", len(i) if n_bias is None else n_bias,
                           None if i is None else _lib.ptr(i), None if v is None else _lib.ptr(v), penalty, context)
    return call


def begin_at(temperature):
    def call(model):
        from csm_mlx import _lib
        begin(model)          # (the engine exists and is this model's current batch)
        seeds = np.zeros(2, np.uint64)
        _lib.check(_lib.lib().csm_begin(model.engine, 2, _lib.ptr(seeds), temperature, 0))
    return call


# tests/test_logits_processors_gpu.py and csrc/csm_kernels.h: the device cap of the repetition window
C0_WINDOW_MAX = 256

# (name, the batch's call with the bad value, the same value as csm_sampling fields; V stands for the vocabulary size)
BAD = [
    ("top_p -0.1", set_filters(top_p=-0.1), dict(top_p=-0.1)),
    ("top_p 1.5", set_filters(top_p=1.5), dict(top_p=1.5)),
    ("min_p 1.5", set_filters(min_p=1.5), dict(min_p=1.5)),
    ("min_tokens_to_keep 0", set_filters(min_keep=0), dict(min_keep=0)),
    ("n_bias -1", set_processors(n_bias=-1), dict(n_bias=-1)),
    ("n_bias 1, null pointers", set_processors(n_bias=1, idx=None, val=None), dict(n_bias=1, idx=None, val=None)),
    ("bias index -1", set_processors(idx=[3, -1], val=[1.0, 1.0]), dict(idx=[3, -1], val=[1.0, 1.0])),
    ("bias index V", "V", "V"),
    ("penalty -1", set_processors(penalty=-1.0, context=8), dict(penalty=-1.0, context=8)),
    ("context -1", set_processors(penalty=1.5, context=-1), dict(penalty=1.5, context=-1)),
    ("context C0_WINDOW_MAX + 1", set_processors(penalty=1.5, context=C0_WINDOW_MAX + 1),
     dict(penalty=1.5, context=C0_WINDOW_MAX + 1)),
    ("temperature -1", begin_at(-1.0), dict(temperature=-1.0)),
    ("temperature NaN", begin_at(float("nan")), dict(temperature=float("nan"))),
]


@pytest.mark.parametrize("name,batch_call,fields", BAD, ids=[b[0] for b in BAD])
def test_bad_value_is_refused_alike_by_the_batch_and_the_slot(tiny, name, batch_call, fields):
    from csm_mlx.sampling import C0_WINDOW_MAX as package_cap
    args, model = tiny
    assert package_cap == C0_WINDOW_MAX
    if batch_call == "V":
        V = model.n_audio_vocab
        batch_call, fields = set_processors(idx=[V], val=[1.0]), dict(idx=[V], val=[1.0])
    with pytest.raises(ValueError) as of_batch:
        batch_call(model)
    eng = slots(model)
    with pytest.raises(ValueError) as of_slot:
        eng._call("csm_slot_set_sampling", 0, ctypes.byref(sampling(**fields)))
    print(f"{name}: batch {str(of_batch.value)!r}, slot {str(of_slot.value)!r}")
    assert type(of_batch.value) is type(of_slot.value) is ValueError
    assert str(of_batch.value) == str(of_slot.value) != ""


# ----------------------------------------------------------------------------- a repeated bias index
REPEATED = ([5, 9, 5], [1.0, 0.25, -3.0])    # index 5 twice: -3.0, the later value, counts


def prompts(args):
    from csm_mlx.tokenizers import tokenize_text_segment
    return [tokenize_text_segment(tiny_prompt_ids(s), 0, args.n_audio_codebooks) for s in (41, 42)]


def batch_c0(args, model, bias):
    """Frame 0's c0 logits (2, V) as the sampler saw them, with ``bias`` (idx, val) set for the batch"""
    from csm_mlx import _lib
    cache = begin(model)
    if bias:
        i, v = arrays(*bias)
        cache._call("csm_set_c0_processors", len(i), _lib.ptr(i), _lib.ptr(v), 0.0, 0)
    for b, (t, m) in enumerate(prompts(args)):
        cache.prefill(b, t, m)
    cache.run(1)
    return read_taps(model, cache, 2, ("c0_logits",))["c0_logits"]


def slot_c0(args, model, bias):
    """The same with ``bias`` set for slot 0's utterance alone"""
    eng = slots(model)
    if bias:
        eng._call("csm_slot_set_sampling", 0, ctypes.byref(sampling(idx=bias[0], val=bias[1])))
    eng.prefill([(b, t, m) for b, (t, m) in enumerate(prompts(args))])
    eng.run(1)
    return read_taps(model, eng.cache, 2, ("c0_logits",))["c0_logits"]


def test_repeated_bias_index_takes_its_last_value_on_both_paths(tiny):
    """The processed c0 row against ``LogitBias`` -- the processor the oracle runs -- on the unprocessed row of
    the same path, with each index once and the repeated one at its last value: the same bits (one float32
    addition per biased logit).  The batch samples (0.8 / top-k 5), so the head stores its logits either way."""
    from csm_mlx.sampling import LogitBias
    args, model = tiny
    once = LogitBias((5, 9), (-3.0, 0.25))
    for path, c0 in (("batch", batch_c0), ("slot", slot_c0)):
        raw, got = c0(args, model, None), c0(args, model, REPEATED)
        want = once(None, raw)
        assert not np.array_equal(want[0], raw[0])
        assert np.array_equal(got[0], want[0]), f"{path}: index 5 moved by {got[0, 5] - raw[0, 5]}, not by -3"
        if path == "batch":
            assert np.array_equal(got[1], want[1]), "batch: row 1"
        else:
            assert np.array_equal(got[1], raw[1]), "slot: slot 0's bias reached slot 1"
