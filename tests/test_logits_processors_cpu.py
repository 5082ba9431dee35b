"""``make_logits_processors`` on the host: the numpy callables of the two descriptors against hand-worked
float32 rows, the factory's surface (mlx_lm's ``make_logits_processors``), and the predicate that decides
which ``logits_processors`` lists run inside the frame on the GPU."""
import numpy as np
import pytest

from csm_mlx.generation import device_processors
from csm_mlx.sampling import (C0_WINDOW_MAX, HostSampler, LogitBias, RepetitionPenalty, Sampler,
                              make_logits_processors)

f32 = np.float32


def hist(*frames):
    """Stacked c0 history (F, B, 1) from per-frame rows of B codes."""
    return np.array(frames, np.int32)[:, :, None]


def test_bias_add():
    logits = np.array([[0.5, -1.25, 2.0, 0.0], [1.0, 1.0, 1.0, 1.0]], f32)
    out = LogitBias((1, 3), (4.0, -0.1))(np.zeros((0,), np.int32), logits)
    assert out.dtype == f32
    assert np.array_equal(out, np.array([[0.5, 2.75, 2.0, f32(0.0) + f32(-0.1)], [1.0, 5.0, 1.0, f32(1.0) + f32(-0.1)]], f32))
    assert np.array_equal(logits[0], np.array([0.5, -1.25, 2.0, 0.0], f32))      # the input is not modified


def test_penalty_signs_zero_and_inf():
    # codes 0..3 are in the window: positive / pen, negative * pen, zero stays zero, -inf stays -inf
    logits = np.array([[3.0, -3.0, 0.0, -np.inf, 7.0]], f32)
    out = RepetitionPenalty(1.3, 20)(hist([0], [1], [2], [3]), logits)
    want = np.array([[f32(3.0) / f32(1.3), f32(-3.0) * f32(1.3), 0.0, -np.inf, 7.0]], f32)
    assert out.dtype == f32 and np.array_equal(out, want)
    assert out[0, 0] == f32(2.3076923)                                            # the correctly rounded float32 quotient


def test_penalty_duplicate_penalised_once():
    logits = np.array([[8.0, -2.0, 1.0]], f32)
    out = RepetitionPenalty(4.0, 20)(hist([0], [0], [1], [0], [1]), logits)
    assert np.array_equal(out, np.array([[2.0, -8.0, 1.0]], f32))                # not 8 / 4 / 4 / 4


def test_penalty_window_slice_and_rows():
    # context 2: only the last two frames count; row b sees utterance b's own codes
    logits = np.array([[4.0, 4.0, 4.0, 4.0], [4.0, 4.0, 4.0, 4.0]], f32)
    h = hist([0, 3], [1, 3], [2, 0])
    out = RepetitionPenalty(2.0, 2)(h, logits)
    assert np.array_equal(out, np.array([[4.0, 2.0, 2.0, 4.0], [2.0, 4.0, 4.0, 2.0]], f32))
    assert np.array_equal(RepetitionPenalty(2.0, 1)(h, logits), np.array([[4.0, 4.0, 2.0, 4.0], [2.0, 4.0, 4.0, 4.0]], f32))


def test_penalty_empty_history_is_noop():
    logits = np.array([[1.0, -1.0]], f32)
    assert np.array_equal(RepetitionPenalty(3.0, 20)(np.zeros((0,), np.int32), logits), logits)


def test_bias_then_penalty_order_on_flipped_sign():
    # entry 1 is -1: bias + 5 first makes it 4 (then / 2 = 2); penalty first would give -2 + 5 = 3
    logits = np.array([[0.0, -1.0, 0.5]], f32)
    procs = make_logits_processors({1: 5.0}, 2.0, 20)
    assert [type(p) for p in procs] == [LogitBias, RepetitionPenalty]
    out = logits
    for p in procs:
        out = p(hist([1]), out)
    assert np.array_equal(out, np.array([[0.0, 2.0, 0.5]], f32))


def test_make_logits_processors_surface():
    from csm_mlx import make_logits_processors as exported
    assert exported is make_logits_processors
    assert make_logits_processors() == []
    assert make_logits_processors(None, None) == []
    assert make_logits_processors({}, 0.0) == []
    assert make_logits_processors({0: 4}) == [LogitBias((0,), (4.0,))]
    assert make_logits_processors(repetition_penalty=1.1) == [RepetitionPenalty(1.1, 20)]
    assert make_logits_processors(repetition_penalty=2, repetition_context_size=7) == [RepetitionPenalty(2.0, 7)]
    for bad in (-1.0, -0.5, "1.1", [1.1]):
        with pytest.raises(ValueError):
            make_logits_processors(repetition_penalty=bad)
    with pytest.raises(Exception):                                                # frozen descriptors
        make_logits_processors({0: 4})[0].indices = (1,)


def test_dispatch_predicate():
    bias, bias2 = LogitBias((0,), (4.0,)), LogitBias((1,), (1.0,))
    pen = RepetitionPenalty(1.1, 20)
    greedy = Sampler(0.0, 0)
    for smp in (greedy, Sampler(0.8, 5), Sampler(0.8, 0, 0.9)):
        assert device_processors([bias], smp) == (bias, None)
        assert device_processors([pen], smp) == (None, pen)
        assert device_processors([bias, pen], smp) == (bias, pen)
    assert device_processors([RepetitionPenalty(1.1, C0_WINDOW_MAX)], greedy) is not None
    host = [[pen, bias], [bias, bias2], [bias, lambda t, l: l], [lambda t, l: l], [pen, pen], [bias, pen, pen],
            [RepetitionPenalty(1.1, C0_WINDOW_MAX + 1)], [bias, RepetitionPenalty(1.1, C0_WINDOW_MAX + 1)]]
    for procs in host:
        assert device_processors(procs, greedy) is None, procs
    assert device_processors([bias, pen], HostSampler(lambda x: x.argmax(-1))) is None
    assert device_processors(None, greedy) is None and device_processors([], greedy) is None


def test_abi_declares_the_symbol():
    from csm_mlx import _lib
    assert "csm_set_c0_processors" in _lib.declared_symbols()
