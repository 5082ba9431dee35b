"""The backbone's attention against the float64 oracle out to the window's last position, and the window's edge
through the C ABI.

Procedure, unit, e32 and bar are tests/test_f64_taps_gpu.py's: prefill, frames one at a time, h_last / c0_logits /
ci_logits read after each; both oracles forced on the engine's codes; error = max |value - float64| / the row's
largest |float64 value|; e32 from the two references alone, each run; bar = helpers.BAR_MARGIN (2) x e32 per tap,
always against float64, never against another engine path.  3 frames: a prompt of L rows gives its last row
(frame 0, L keys) and two decode rows at positions L and L + 1.

What the bar catches here is structural: a key range, a chunk loop's trip count or last partial pass, a rescale, a
combine, a RoPE row, a KV row -- tests/test_f64_long_cpu.py measures such defects at >= 1800 x e32 at every length
used here.  It claims nothing about 16-bit cuts inside attention (0.5-19 x e32 there, not separable; these kernels
have no split operands).

Tiny (float32, bf16, q4; attn_kernel<64> on decode rows, attn_prefill_kernel<64> on prompt rows): one ragged batch
of prompts of 13, 62, 63, 127, 255, 511, 700, 1023, 1500 and W rows, so the decode rows sit on both sides of 64, 128,
256, 512 and 1024 keys and end on the window's last position, at very different positions in one launch (rm.pos per
row).  Prefilled three ways -- per prompt; one prefill_batch (7300 rows: several groups of <= max_seq_len); each
prompt split in two calls, the second starting past position 0 (1500 = 1400 + 100: its tiles read 22 chunks of
cached keys) -- plus the longest prompt alone (B = 1) and the batch with option attn_prefill off (attn_block per
prompt row).

csm_1b bf16, B = 1, prompts of 511 and W rows: the persistent step (bb_step's 128-key passes and 8-wave combine:
n = 512 then 513 keys is the pass boundary where (k0 >> 6) & 7 wraps to wave 0; W is 16 passes, the last key in the
last KV row) with epochs +80 per decode row and +498 per frame, and options bb_step / dec_frame off (attn_kernel<64>
at G = 4, all four waves busy; epochs +0).  q4: 511 rows on the persistent path.  The csm_1b references feed the
prompt to the oracles in blocks of 1024 rows (helpers.oracle_taps(block=...)).

The window (csm_engine_abi.hip, confirmed by the runs below): after a prompt of L rows pos_host = L - 1;
require_window admits nframes <= max_seq_len + 1 - L; so W = max_seq_len - 2 is the longest prompt that admits 3
frames, and its last decode row sits at position max_seq_len - 1.  A prompt of max_seq_len rows is accepted and
admits one frame.  Every refusal is CSM_ERR_TOO_LONG from an argument check that returns before anything is
launched: the tests assert the code and the unchanged state, and never launch with the refused arguments."""
import ctypes
import time

import numpy as np
import pytest

from helpers import BAR_MARGIN, TAPS, csm_weights, f64_reference, long_prompt, tap_errors
from rigs import TAP_NAMES, build_model, epoch, frame_taps, handoffs, read_taps, set_option, synchronize

pytestmark = pytest.mark.gpu

FRAMES = 3
EPOCHS = ("dec_frame_epoch", "dec_xsd_epoch", "bb_step_epoch")
BLOCK_1B = 1024


def _lengths(model):
    return (13, 62, 63, 127, 255, 511, 700, 1023, 1500, model.max_seq_len - 2)


@pytest.fixture(scope="module", params=["float32", "bf16", "q4"])
def tiny(request):
    args, w, model = build_model("tiny", request.param, 10)
    assert model.max_seq_len == 2048
    yield request.param, args, model
    del model


@pytest.fixture(scope="module")
def tiny_f32():
    args, w, model = build_model("tiny", "float32", 3)
    yield args, model
    del model


@pytest.fixture(scope="module")
def engine_1b_bf16():
    args, w, model = build_model("1b", "bf16", 1)
    yield args, model
    del model


@pytest.fixture(scope="module")
def engine_1b_q4():
    args, w, model = build_model("1b", "q4", 1)
    yield args, model
    del model


def _prompts(args, lengths):
    return [long_prompt(args, 9000 + L, L) for L in lengths]


# ----------------------------------------------------------------------------- prefill modes
def _per_prompt(prompts):
    def feed(cache):
        for b, (t, m) in enumerate(prompts):
            cache.prefill(b, t, m)
    return feed


def _one_batch(prompts):
    return lambda cache: cache.prefill_batch([(b, t, m) for b, (t, m) in enumerate(prompts)])


def _cut(L):
    return 1400 if L == 1500 else L // 2


def _split(prompts):
    def feed(cache):
        for b, (t, m) in enumerate(prompts):
            s = _cut(t.shape[0])
            cache.prefill(b, t[:s], m[:s])
            cache.prefill(b, t[s:], m[s:])
    return feed


MODES = {"per_prompt": _per_prompt, "prefill_batch": _one_batch, "split": _split}


# ----------------------------------------------------------------------------- run, reference, bar
def _run(model, prompts, feed, frames=FRAMES):
    """(cache, codes (F, B, K), taps (h_last, c0, ci), seconds)."""
    from csm_mlx.sampling import Sampler
    held = []

    def prefill(cache):
        held.append(cache)
        feed(cache)
    t0 = time.perf_counter()
    hist, n, taps = frame_taps(model, prompts, frames, Sampler(0.0, 0), [0] * len(prompts), TAP_NAMES, prefill=prefill)
    synchronize(model)
    dt = time.perf_counter() - t0
    assert hist.shape[0] == frames and (n == frames).all(), "an utterance ended inside the window"
    got = tuple(taps[t] for t in TAP_NAMES)
    assert np.array_equal(hist[:, :, 0], got[1].argmax(-1)), "c0 is not the arg-max of the engine's c0 logits"
    assert np.array_equal(hist[:, :, 1:], got[2].argmax(-1)), "a code is not the arg-max of its ci logits row"
    return held[0], hist, got, dt


_REFS = {}


def _reference(key, dtype, prompts, codes, block=None):
    """(float64 taps, e32, seconds it took -- 0 when shared), memoised by (model, dtype, prompts, codes)."""
    variant = {"float32": "fp32"}.get(dtype, dtype)
    k = (key, variant, tuple(t.tobytes() for t, _ in prompts), codes.tobytes())
    dt = 0.0
    if k not in _REFS:
        args, w = csm_weights(key)
        t0 = time.perf_counter()
        _REFS[k] = f64_reference(args, w, variant, prompts, codes, block)
        dt = time.perf_counter() - t0
    return _REFS[k] + (dt,)


def _hold(tag, key, dtype, prompts, codes, got, t_engine, capsys, block=None):
    """Every tap of the case under BAR_MARGIN x e32 against float64; prints the case's f64-long line."""
    t64, e32, t_ref = _reference(key, dtype, prompts, codes, block)
    err = tap_errors(got, t64)
    ci = err["ci"]
    split = {"h_last": err["h_last"].max(), "c0": err["c0"].max(), "ci1": ci[:, :, 0].max(), "ci2+": ci[:, :, 1:].max()}
    e = {"h_last": e32["h_last"], "c0": e32["c0"], "ci1": e32["ci"], "ci2+": e32["ci"]}
    line = (f"f64-long {key} {dtype} B={len(prompts)} {tag}: "
            + " ".join(f"{t}={split[t]:.2e}({split[t] / e[t]:.2f}x)" for t in split)
            + " | e32 " + " ".join(f"{t}={e32[t]:.2e}" for t in TAPS)
            + f" | engine {t_engine:.2f} s, reference {t_ref:.1f} s")
    with capsys.disabled():
        print("\n" + line)
    bad = [f"{t}: {float(err[t].max()):.3e} > {BAR_MARGIN} x e32 = {BAR_MARGIN * e32[t]:.3e} at (frame, row[, step]) "
           f"{np.unravel_index(int(err[t].argmax()), err[t].shape)}" for t in TAPS
           if not float(err[t].max()) <= BAR_MARGIN * e32[t]]
    assert not bad, line + "\n" + "\n".join(bad)


# ----------------------------------------------------------------------------- tiny: launch-path kernels
@pytest.mark.parametrize("mode", list(MODES))
def test_tiny_ragged_batch(tiny, mode, capsys):
    dtype, args, model = tiny
    prompts = _prompts(args, _lengths(model))
    assert sum(t.shape[0] for t, _ in prompts) > 3 * model.max_seq_len            # prefill_batch: several groups
    _, codes, got, dt = _run(model, prompts, MODES[mode](prompts))
    _hold(mode, "tiny", dtype, prompts, codes, got, dt, capsys)


def test_tiny_longest_alone(tiny, capsys):
    """B = 1: the GEMV launch path with M = 1, decode rows at max_seq_len - 2 and max_seq_len - 1."""
    dtype, args, model = tiny
    prompts = _prompts(args, _lengths(model)[-1:])
    _, codes, got, dt = _run(model, prompts, _per_prompt(prompts))
    _hold("alone", "tiny", dtype, prompts, codes, got, dt, capsys)


def test_tiny_attn_prefill_off(tiny, capsys):
    """Option attn_prefill 0: attn_block per prompt row, the same bar."""
    dtype, args, model = tiny
    prompts = _prompts(args, _lengths(model))
    set_option(model, "attn_prefill", 0)
    try:
        _, codes, got, dt = _run(model, prompts, _per_prompt(prompts))
    finally:
        set_option(model, "attn_prefill", 1)
    _hold("attn_prefill=0", "tiny", dtype, prompts, codes, got, dt, capsys)


# ----------------------------------------------------------------------------- csm_1b, batch 1
def _epochs(model):
    return {name: epoch(model, name[:-len("_epoch")]) for name in EPOCHS}


def _check_1b(dtype, args, model, L, persistent, capsys):
    K = args.n_audio_codebooks
    prompts = _prompts(args, [L])
    options = () if persistent else ("bb_step", "dec_frame")
    expect = {"dec_frame_epoch": handoffs("dec_frame", K) * FRAMES if persistent else 0, "dec_xsd_epoch": 0,
              "bb_step_epoch": handoffs("bb_step", K) * (FRAMES - 1) if persistent else 0}
    for name in options:
        set_option(model, name, 0)
    try:
        e0 = _epochs(model)
        _, codes, got, dt = _run(model, prompts, _per_prompt(prompts))
        e1 = _epochs(model)
    finally:
        for name in options:
            set_option(model, name, 1)
    delta = {n: e1[n] - e0[n] for n in EPOCHS}
    assert delta == expect, f"kernels that ran (epoch deltas) {delta}, expected {expect}"
    _hold(f"L={L} off={','.join(options) or '-'}", "1b", dtype, prompts, codes, got, dt, capsys, BLOCK_1B)


@pytest.mark.parametrize("persistent", [True, False], ids=["bb_step+dec_frame", "gemv_launches"])
@pytest.mark.parametrize("L", [511, 2046])
def test_1b_bf16(L, persistent, engine_1b_bf16, capsys):
    args, model = engine_1b_bf16
    assert L in (511, model.max_seq_len - 2)
    _check_1b("bf16", args, model, L, persistent, capsys)


def test_1b_q4_persistent(engine_1b_q4, capsys):
    """bb_step_q4_kernel shares attn_rest with the bf16 step."""
    args, model = engine_1b_q4
    _check_1b("q4", args, model, 511, True, capsys)


# ----------------------------------------------------------------------------- the window's edge (tiny, float32)
def _rc_run(model, n=1):
    from csm_mlx import _lib
    done = ctypes.c_int(0)
    return _lib.lib().csm_run_frames(model.engine, n, ctypes.byref(done))


def _rc_prefill(model, b, tokens, mask):
    from csm_mlx import _lib
    t, m = np.ascontiguousarray(tokens, np.int32), np.ascontiguousarray(mask, np.uint8)
    return _lib.lib().csm_prefill(model.engine, b, t.shape[0], _lib.ptr(t), _lib.ptr(m))


def _rc_prefill_batch(model, items):
    from csm_mlx import _lib
    utts = np.array([b for b, _, _ in items], np.int32)
    Ts = np.array([t.shape[0] for _, t, _ in items], np.int32)
    toks = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int32) for _, t, _ in items]), np.int32)
    msks = np.ascontiguousarray(np.concatenate([np.asarray(m, np.uint8) for _, _, m in items]), np.uint8)
    return _lib.lib().csm_prefill_batch(model.engine, len(items), _lib.ptr(utts), _lib.ptr(Ts), _lib.ptr(toks), _lib.ptr(msks))


def _state(model, cache, B):
    """Everything a caller can read back: the code history and the three taps, as bytes."""
    hist, n, done = cache.codes()
    taps = read_taps(model, cache, B, TAP_NAMES)
    return [hist.tobytes(), n.tobytes(), done.tobytes()] + [taps[t].tobytes() for t in TAP_NAMES]


def _refused(model, cache, B, rc):
    """``rc`` is CSM_ERR_TOO_LONG; the stream is clean; returns the state read after the refusal."""
    from csm_mlx import _lib
    assert rc == _lib.CSM_ERR_TOO_LONG, (rc, _lib.lib().csm_last_error())
    synchronize(model)
    return _state(model, cache, B)


def test_last_admitted_frame_and_first_refused(tiny_f32, capsys):
    """A prompt of W = max_seq_len - 2 rows: 3 frames run and pass the float64 bar (the last decode row at position
    max_seq_len - 1); the 4th is refused and changes nothing; a fresh FrameCache reproduces the codes."""
    args, model = tiny_f32
    prompts = _prompts(args, [model.max_seq_len - 2])
    cache, codes, got, dt = _run(model, prompts, _per_prompt(prompts))
    _hold("W rows, 3 frames", "tiny", "float32", prompts, codes, got, dt, capsys)
    before = _state(model, cache, 1)
    assert _refused(model, cache, 1, _rc_run(model)) == before
    _, again, _, _ = _run(model, prompts, _per_prompt(prompts))
    assert np.array_equal(again, codes)


def test_prompt_of_max_seq_len_rows(tiny_f32, capsys):
    """Accepted; h_last at position max_seq_len - 1 (the last RoPE row and KV row, written by a prefill tile) and
    the one admitted frame's c0 / ci pass the float64 bar; the next frame is refused and changes nothing."""
    args, model = tiny_f32
    prompts = _prompts(args, [model.max_seq_len])
    cache, codes, got, dt = _run(model, prompts, _per_prompt(prompts), frames=1)
    _hold("max_seq_len rows, 1 frame", "tiny", "float32", prompts, codes, got, dt, capsys)
    before = _state(model, cache, 1)
    assert _refused(model, cache, 1, _rc_run(model)) == before


def _frame_after(model, B, feed):
    """One frame of a fresh batch fed by ``feed(cache)``: the state read back."""
    from csm_mlx.generation import FrameCache
    from csm_mlx.sampling import Sampler
    cache = FrameCache(model, B, Sampler(0.0, 0), [0] * B)
    feed(cache)
    cache.run(1)
    synchronize(model)
    return _state(model, cache, B)


def test_refused_prompts_leave_the_batch_untouched(tiny_f32):
    """A prompt of max_seq_len + 1 rows, a second prefill that would append past the window, and a prefill_batch
    with one utterance too long: each CSM_ERR_TOO_LONG; then the batch is completed with prompts that fit and one
    frame compared, byte for byte, with a batch that never saw the refused call -- so no utterance's position (its
    own or another's) moved.  The refused rows themselves are never launched."""
    from csm_mlx import _lib
    args, model = tiny_f32
    S = model.max_seq_len
    p40, p60, p100, pbig, over = (long_prompt(args, 9500 + L, L) for L in (40, 60, 100, S - 48, S + 1))
    p20, p48, p49 = (long_prompt(args, 9600 + L, L) for L in (20, 48, 49))

    def too_long_prompt(cache):
        cache.prefill(0, *p40)
        assert _rc_prefill(model, 1, *over) == _lib.CSM_ERR_TOO_LONG
        cache.prefill(1, *p100)
    clean = _frame_after(model, 2, lambda c: (c.prefill(0, *p40), c.prefill(1, *p100)))
    assert _frame_after(model, 2, too_long_prompt) == clean

    def append_past_the_window(cache):                      # S - 48 rows hold; + 49 is one row over, + 48 fits exactly
        cache.prefill(0, *p40)
        cache.prefill(1, *pbig)
        assert _rc_prefill(model, 1, *p49) == _lib.CSM_ERR_TOO_LONG
        cache.prefill(1, *p48)
    clean = _frame_after(model, 2, lambda c: (c.prefill(0, *p40), c.prefill(1, *pbig), c.prefill(1, *p48)))
    assert _frame_after(model, 2, append_past_the_window) == clean

    def batch_with_one_too_long(cache):                     # utterance 0's 20 rows are valid, and must not land either
        cache.prefill(0, *p40)
        assert _rc_prefill_batch(model, [(0,) + p20, (1,) + over, (2,) + p100]) == _lib.CSM_ERR_TOO_LONG
        cache.prefill_batch([(1,) + p60, (2,) + p100])
    clean = _frame_after(model, 3, lambda c: (c.prefill(0, *p40), c.prefill_batch([(1,) + p60, (2,) + p100])))
    assert _frame_after(model, 3, batch_with_one_too_long) == clean
