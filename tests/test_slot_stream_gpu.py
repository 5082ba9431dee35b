"""Streaming audio out of a SlotBatch: per-slot streaming Mimi decoder state (mimi_slot_reset /
mimi_decode_slots, csrc/mimi_engine.hip) and ``SlotBatch.stream`` / ``stream_generate_queue`` on top of it.

The reference is always the oracle run alone on each stream: codes from ``OracleCSM.generate_codes``, PCM from
``OracleMimi.reset_state()`` + per-frame ``decode_step`` at B = 1.  Nothing is compared against another run of
the code under test.  PCM bound: the project's bar for ``decode_step`` against the oracle, RMS <= 1e-4
(tests/test_mimi_gpu.py); codes are bit-exact."""
import dataclasses

import numpy as np
import pytest

from helpers import eos_weights, first_divergence, oracle_for, rms
from rigs import CAP, N_TINY, SEEDS, build_model, mimi_codec as mimi, slot_prompts

pytestmark = pytest.mark.gpu

PCM_RMS = 1e-4


def oracle_stream(o, codes_fk, window=0):
    """The oracle alone on one stream: codes (F, K) -> (F * frame_size,) PCM, frame by frame."""
    o.reset_state()
    out = [o.decode_step(np.ascontiguousarray(codes_fk[f][None, :, None]), window=window)[0, 0]
           for f in range(len(codes_fk))]
    return np.concatenate(out) if out else np.zeros((0,), np.float32)


# ----------------------------------------------------------------------------- 1. codec slots, tiny Mimi
# Global frames 0..14 in calls of 1, 3, 2, 5, 1, 3 frames through a ring of 8 rows (it wraps twice).
CALLS = [1, 3, 2, 5, 1, 3]
STARTS = [0, 1, 4, 6, 11, 12]
F_RING = 8
# (slot, first global frame, frames): slot 0 one stream of 14 (past the 5-frame attention window at a
# non-zero slot position); slot 1 3 frames, reset, 9 frames; slot 2 idle for two calls, reset, 8 frames
STREAMS = {"a": (0, 0, 14), "b1": (1, 0, 3), "b2": (1, 4, 9), "c": (2, 4, 8)}
_TINY_REFS = {}


def tiny_case(mode):
    """(timeline [15][3][n_q] of seeded codes, oracle PCM per stream), the oracle run once per mode."""
    if mode not in _TINY_REFS:
        from csm_mlx.config import MIMI_CONFIGURATION
        from csm_mlx.weights import synthetic_mimi_weights
        from oracle.mimi_oracle import OracleMimi
        m = dataclasses.replace(MIMI_CONFIGURATION["tiny"], attn_mode=mode)
        assert m.n_q == 4 and m.context == 10 and m.downsample_stride == 2      # a 5-frame window
        o = OracleMimi(m, synthetic_mimi_weights(m))
        line = np.random.default_rng(77).integers(0, m.bins, (sum(CALLS), 3, m.n_q)).astype(np.int32)
        ref = {k: oracle_stream(o, line[g0: g0 + F, b]) for k, (b, g0, F) in STREAMS.items()}
        _TINY_REFS[mode] = (line, ref)
    return _TINY_REFS[mode]


def drive_tiny(codec, m, line, decode):
    """The six calls of the tiny case; decode(ring, n, first_row, active) -> (3, n * frame_size)."""
    fs = m.frame_size
    ring = np.full((F_RING, 3, m.n_q), -1, np.int32)
    got = np.zeros((3, sum(CALLS) * fs), np.float32)
    codec.slot_reset(0)
    codec.slot_reset(1)
    for c, (g0, n) in enumerate(zip(STARTS, CALLS)):
        if c == 2:                       # the boundary at global frame 4: slot 1 restarts, slot 2 joins
            codec.slot_reset(1)
            codec.slot_reset(2)
        for f in range(n):
            ring[(g0 + f) % F_RING] = line[g0 + f]
        pcm = decode(ring, n, g0 % F_RING, [True, True, 2 <= c <= 4])
        assert pcm.shape == (3, n * fs) and pcm.dtype == np.float32
        got[:, g0 * fs: (g0 + n) * fs] = pcm
    return got


def check_tiny(got, ref, fs, what):
    for k, (b, g0, F) in STREAMS.items():
        e = rms(got[b, g0 * fs: (g0 + F) * fs], ref[k])
        print(f"{what} stream {k}: rms {e:.3e}")
        assert e <= PCM_RMS, (what, k, e)


@pytest.mark.parametrize("mode", ["mlx", "causal"])
def test_codec_slots_tiny(mode):
    m, codec, _ = mimi("tiny", mode, max_batch=3, max_frames=40)
    line, ref = tiny_case(mode)
    got = drive_tiny(codec, m, line, lambda ring, n, row, active: codec.decode_slots(ring, n, row, active))
    check_tiny(got, ref, m.frame_size, mode)


# The ring in device memory: a torch tensor's data_ptr().  torch has to initialise the GPU before the
# library's HIP runtime does (afterwards it finds no device in this process), so the case runs in a child
# process of its own that starts with torch; the PCM it saves is compared with the oracle here.
_DEVICE_RING_SCRIPT = r"""
import sys
import torch
torch.cuda.init()
dev = torch.zeros((8, 3, 4), dtype=torch.int32, device="cuda")
import numpy as np
sys.path[:0] = [sys.argv[3] + "/csm-mlx_amd", sys.argv[3], sys.argv[3] + "/tests"]
import test_slot_stream_gpu as t
m, codec, _ = t.mimi("tiny", "mlx", max_batch=3, max_frames=40)
line = np.load(sys.argv[1])

def decode(ring, n, row, active):
    dev.copy_(torch.from_numpy(ring))
    torch.cuda.synchronize()
    return codec.decode_slots(dev.data_ptr(), n, row, active, F_cap=t.F_RING, on_device=True)

np.save(sys.argv[2], t.drive_tiny(codec, m, line, decode))
"""


def test_codec_slots_tiny_device_ring(tmp_path):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    line, ref = tiny_case("mlx")
    src, out = str(tmp_path / "line.npy"), str(tmp_path / "pcm.npy")
    np.save(src, line)
    r = subprocess.run([sys.executable, "-c", _DEVICE_RING_SCRIPT, src, out, root], capture_output=True, text=True,
                       timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    check_tiny(np.load(out), ref, 1920, "device ring")


# ----------------------------------------------------------------------------- 2. mimi_202407 shape
def test_codec_slots_mimi_202407():
    """mlx mode, 2 slots, four calls of 2 frames, slot 1 reset after the second call."""
    m, codec, o = mimi("mimi_202407", "mlx", max_batch=2, max_frames=40)
    fs = m.frame_size
    line = np.random.default_rng(78).integers(0, m.bins, (8, 2, m.n_q)).astype(np.int32)
    got = np.zeros((2, 8 * fs), np.float32)
    codec.slot_reset(0)
    codec.slot_reset(1)
    for c in range(4):
        if c == 2:
            codec.slot_reset(1)
        got[:, 2 * c * fs: (2 * c + 2) * fs] = codec.decode_slots(line, 2, 2 * c, [True, True])
    for k, (b, g0, F) in {"a": (0, 0, 8), "b1": (1, 0, 4), "b2": (1, 4, 4)}.items():
        e = rms(got[b, g0 * fs: (g0 + F) * fs], oracle_stream(o, line[g0: g0 + F, b], window=8))
        print(f"mimi_202407 stream {k}: rms {e:.3e}")
        assert e <= PCM_RMS, (k, e)


# ----------------------------------------------------------------------------- 3-6. end to end, tiny CSM + tiny Mimi
@pytest.fixture(scope="module")
def tiny():
    from csm_mlx.config import MIMI_CONFIGURATION
    from csm_mlx.mimi import MimiCodec
    from csm_mlx.tokenizers import set_audio_tokenizer
    from csm_mlx.weights import synthetic_mimi_weights
    from oracle.mimi_oracle import OracleMimi
    args, w, model = build_model(eos_weights("tiny"), "bf16", max_batch=8)
    mm = MIMI_CONFIGURATION["tiny"]
    mw = synthetic_mimi_weights(mm)
    codec = MimiCodec(mm, max_batch=8, max_frames=CAP)
    codec.load_weights(mw)
    set_audio_tokenizer(codec, args.n_audio_codebooks)
    prompts = slot_prompts(args.n_audio_codebooks)
    yield args, w, model, oracle_for(args, w, bf16=True), prompts, OracleMimi(mm, mw), codec
    del model


_REFS = {}


def refs(tiny, key, **kw):
    """The oracles alone on each prompt, once per sampler: [(codes (F, K), pcm (F * 1920,))]."""
    if key not in _REFS:
        _, _, _, o, prompts, om, _ = tiny
        out = []
        for i, (t, m) in enumerate(prompts):
            codes = o.generate_codes(t, m, CAP, **({"seed": SEEDS[i], **kw} if kw else {}))
            out.append((codes, oracle_stream(om, codes, window=8)))
        _REFS[key] = out
    return _REFS[key]


def check_events(events, tickets, want, what):
    """events: the StreamChunks in yield order; tickets[i]: prompt i's ticket; want: refs()."""
    by = {}
    for ev in events:
        by.setdefault(ev.ticket, []).append(ev)
    assert sorted(by) == sorted(tickets), what
    for i, t in enumerate(tickets):
        evs, (codes, pcm) = by[t], want[i]
        assert [e.final for e in evs] == [False] * (len(evs) - 1) + [True], (what, i)     # one final, the last
        assert all(e.codes is None for e in evs[:-1]) and evs[-1].codes is not None, (what, i)
        assert all(e.pcm.dtype == np.float32 and e.pcm.ndim == 1 and len(e.pcm) % 1920 == 0 for e in evs), (what, i)
        d = first_divergence(evs[-1].codes, codes)
        assert d is None and len(evs[-1].codes) == len(codes), f"{what} utterance {i}: first divergence {d}"
        assert sum(len(e.pcm) // 1920 for e in evs) == len(codes), (what, i)
        if len(codes) == 0:
            assert len(evs) == 1 and len(evs[0].pcm) == 0, (what, i)                      # one empty final event
        e = rms(np.concatenate([e.pcm for e in evs]), pcm)
        assert e <= PCM_RMS, f"{what} utterance {i} ({len(codes)} frames): rms {e:.3e}"


@pytest.mark.parametrize("slots", [4, 8])
@pytest.mark.parametrize("chunk", [1, 5])
def test_stream_matches_oracle(tiny, slots, chunk):
    from csm_mlx import SlotBatch, StreamChunk
    from csm_mlx.sampling import Sampler
    _, _, model, _, prompts, _, _ = tiny
    want = refs(tiny, "greedy")
    counts = [len(c) for c, _ in want]
    print("oracle frame counts (greedy):", counts)
    assert len(set(counts)) > 4 and any(n == 0 for n in counts)          # slots turn over mid-chunk
    batch = SlotBatch(model, slots, sampler=Sampler(0.0, 0), chunk=chunk)
    tickets = [batch.submit(*prompts[i], CAP, 0) for i in range(N_TINY)]
    events = list(batch.stream())
    assert all(isinstance(e, StreamChunk) for e in events)
    check_events(events, tickets, want, f"{slots} slots, chunk {chunk}:")


def test_stream_sampled(tiny):
    """temperature 0.8, top-k 50, seeds 1234 + i through 8 slots, by the public generator."""
    from csm_mlx import stream_generate_queue
    _, _, model, _, prompts, _, _ = tiny
    want = refs(tiny, "sampled", temperature=0.8, top_k=50)
    print("oracle frame counts (sampled):", [len(c) for c, _ in want])
    got = {i: [] for i in range(N_TINY)}
    finals = {i: [] for i in range(N_TINY)}
    for i, pcm, final in stream_generate_queue(model, prompts, slots=8, temperature=0.8, top_k=50, seeds=SEEDS,
                                               max_audio_frames=[CAP] * N_TINY):
        got[i].append(pcm)
        finals[i].append(final)
    for i, (codes, pcm) in enumerate(want):
        assert finals[i] == [False] * (len(finals[i]) - 1) + [True], i
        mine = np.concatenate(got[i])
        assert len(mine) == len(codes) * 1920, (i, len(mine) // 1920, len(codes))
        e = rms(mine, pcm)
        assert e <= PCM_RMS, f"sampled utterance {i}: rms {e:.3e}"


def test_state_and_argument_errors(tiny):
    from csm_mlx import SlotBatch, _lib
    from csm_mlx.models import CSM
    from csm_mlx.sampling import Sampler
    args, w, model, _, prompts, _, _ = tiny
    m, codec, o = mimi("tiny", "mlx", max_batch=2, max_frames=40)          # 96 latent positions
    rng = np.random.default_rng(79)
    ring = rng.integers(0, m.bins, (8, 2, m.n_q)).astype(np.int32)
    with pytest.raises(_lib.CsmHipError) as ei:                             # no slot_reset yet
        codec.decode_slots(ring, 1, 0, [True, True])
    assert ei.value.code == _lib.CSM_ERR_STATE
    codec.slot_reset(0)
    with pytest.raises(_lib.CsmHipError) as ei:                             # decode_step in slot mode
        codec.decode_step(ring[0])
    assert ei.value.code == _lib.CSM_ERR_STATE
    for b in (-1, 2):
        with pytest.raises(ValueError):
            codec.slot_reset(b)
    with pytest.raises(ValueError):
        codec.decode_slots(np.zeros((8, 3, m.n_q), np.int32), 1, 0, [True] * 3)     # B > max_batch
    with pytest.raises(ValueError):
        codec.decode_slots(ring, 0, 0, [True, True])
    with pytest.raises(ValueError):
        codec.decode_slots(ring, 9, 0, [True, True])                       # n > F_cap
    # slot 0 to position 80 in 5 calls of 8 frames; a sixth would end at 96 + 4 > 96: refused before launch,
    # and the 5 frames that still fit decode as the oracle's frames 40..44 of the same stream
    line = [ring[:, 0].copy()]
    pcm = [codec.decode_slots(ring, 8, 0, [True, False])[0]]
    for _ in range(4):
        ring = rng.integers(0, m.bins, (8, 2, m.n_q)).astype(np.int32)
        line.append(ring[:, 0].copy())
        pcm.append(codec.decode_slots(ring, 8, 0, [True, False])[0])
    with pytest.raises(ValueError, match="capacity"):
        codec.decode_slots(ring, 8, 0, [True, False])
    line.append(ring[3:8, 0].copy())
    pcm.append(codec.decode_slots(ring, 5, 3, [True, False])[0])
    e = rms(np.concatenate(pcm), oracle_stream(o, np.concatenate(line), window=8))
    print(f"45 frames around a refused call: rms {e:.3e}")
    assert e <= PCM_RMS, e
    codec.reset_state(2)                                                    # leaves slot mode
    with pytest.raises(_lib.CsmHipError) as ei:
        codec.decode_slots(ring, 1, 0, [True, True])
    assert ei.value.code == _lib.CSM_ERR_STATE
    # SlotBatch.stream's own checks
    small = CSM(args, dtype="bf16", max_batch=2, max_frames=8)
    small.load_weights(w)
    batch = SlotBatch(small, 2, sampler=Sampler(0.0, 0), chunk=5)
    batch.submit(*prompts[0], 8, 0)
    with pytest.raises(ValueError, match="5.*8"):
        next(batch.stream())
    del small
    batch = SlotBatch(model, 4, sampler=Sampler(0.0, 0))
    batch.submit(*prompts[0], CAP, 0)
    with pytest.raises(ValueError, match="2.*4"):
        next(batch.stream(codec))                                           # a codec of 2 rows under 4 slots
    batch = SlotBatch(model, 2, sampler=Sampler(0.0, 0))
    batch.submit(*prompts[0], CAP + 1, 0)
    with pytest.raises(ValueError, match="40.*41"):
        next(batch.stream(codec))                                           # a cap above the codec's 40 frames


def test_run_and_stream_follow_each_other(tiny):
    from csm_mlx import SlotBatch, generate_queue
    from csm_mlx.sampling import Sampler
    _, _, model, _, prompts, _, _ = tiny
    want = refs(tiny, "greedy")

    def run_codes():
        got = generate_queue(model, prompts, slots=4, max_audio_frames=[CAP] * N_TINY, decode=False)
        for i, (g, (c, _)) in enumerate(zip(got, want)):
            assert first_divergence(g, c) is None and len(g) == len(c), i

    def stream_codes():
        batch = SlotBatch(model, 4, sampler=Sampler(0.0, 0))
        tickets = [batch.submit(*prompts[i], CAP, 0) for i in range(N_TINY)]
        check_events(list(batch.stream()), tickets, want, "stream between runs:")

    run_codes()
    stream_codes()
    run_codes()
