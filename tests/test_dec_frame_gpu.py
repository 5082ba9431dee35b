"""The persistent frame decoder (dec_frame.hip: codebook0_head + the 31 depth-decoder steps of a
batch-1 greedy bf16 frame in ONE launch, tagged-granule hand-offs between 256 resident workgroups)
against the per-projection launch path it replaces and against the oracle.

Codes must be identical to the launch path and to the oracle (both are fp32-accumulation paths over
the same bf16 weights); logits within the bf16 bar; the decoder must be deterministic run to run and
leave no hand-off timeout behind.  (tests/test_long_gpu.py's 125-frame bf16 fixture runs on it too.)"""
import numpy as np
import pytest

from helpers import first_divergence, oracle_for, prompt_ids
from rigs import ab, build_model, codes_per_utterance, epoch, frame_taps, handoffs, set_option

pytestmark = pytest.mark.gpu


def _run(model, prompt, frames):
    from csm_mlx.sampling import Sampler
    hist, n, taps = frame_taps(model, [prompt], frames, Sampler(0.0, 0), [0], ("c0_logits", "ci_logits"))
    return hist[: n[0], 0], list(zip(taps["c0_logits"][:, 0], taps["ci_logits"][:, 0]))


@pytest.mark.parametrize("dtype", ["bf16", "q4"])
def test_dec_frame_matches_launch_path_and_oracle(dtype):
    """q4: dec_frame_kernel<true> (an nn.quantize'd engine: int4 nibbles + group affine words for every
    decoder projection, codebook0_head and the projection; audio_head bf16) against the int4 GEMV launch
    path and the oracle on the dequantized weights."""
    from csm_mlx.generation import generate_codes_batch
    from csm_mlx.sampling import Sampler
    from csm_mlx.tokenizers import tokenize_text_segment
    args, w, model = build_model("1b", dtype)
    prompt = tokenize_text_segment(prompt_ids(31), 0, 32)
    (ref, ref_logs), (got, got_logs) = ab(model, "dec_frame", lambda: _run(model, prompt, 12), 12 * handoffs("dec_frame", args.n_audio_codebooks))
    assert first_divergence(got, ref) is None, f"dec_frame codes differ from the launch path at {first_divergence(got, ref)}"
    for f, ((c0a, cia), (c0b, cib)) in enumerate(zip(got_logs, ref_logs)):
        for a, b in ((c0a, c0b), (cia, cib)):
            assert np.abs(a - b).max() <= 2e-3 * np.abs(b).max(), f"frame {f}: logits differ"
    # deterministic, graph-replayed multi-frame loop (csm_run_frames of 16 frames per call)
    h1, n1, _ = generate_codes_batch(model, [prompt], 40, sampler=Sampler(0.0, 0))
    h2, n2, _ = generate_codes_batch(model, [prompt], 40, sampler=Sampler(0.0, 0))
    assert np.array_equal(h1, h2) and np.array_equal(n1, n2)
    assert first_divergence(h1[:12, 0], got) is None
    orc = oracle_for(args, w, bf16=(dtype == "bf16"), q4=(dtype == "q4")).generate_codes(*prompt, 12)
    assert first_divergence(got, orc) is None
    del model


@pytest.mark.parametrize("top_k,dtype", [(0, "bf16"), (50, "bf16"), (0, "q4"), (50, "q4")])
def test_dec_frame_sampled_matches_launch_path_and_oracle(top_k, dtype):
    """The reference's default sampler (temperature 0.8, generation.py:102, :51-54; top_k 0) and
    config 3's top-k 50 at batch 1 on the persistent frame decoder: every head hands all its logits
    to every workgroup, which runs sample_kernel's top-k radix select + Gumbel-max.  12 frames: codes
    identical to the launch path (sample_kernel) and to the oracle's restatement of the counter-based
    RNG; the decoder ran every frame (same 498 hand-offs as greedy)."""
    from csm_mlx.sampling import Sampler
    from csm_mlx.tokenizers import tokenize_text_segment
    args, w, model = build_model("1b", dtype)
    prompt = tokenize_text_segment(prompt_ids(33), 0, 32)
    smp, seed, frames = Sampler(0.8, top_k), 4242, 12

    def run():
        return codes_per_utterance(model, [prompt], frames, smp, seeds=[seed])[0]
    ref, got = ab(model, "dec_frame", run, frames * handoffs("dec_frame", args.n_audio_codebooks))
    assert len(got) == frames and first_divergence(got, ref) is None, \
        f"sampled dec_frame codes differ from the launch path at {first_divergence(got, ref)}"
    assert np.array_equal(run(), got)                                     # deterministic per seed
    orc = oracle_for(args, w, bf16=(dtype == "bf16"), q4=(dtype == "q4")).generate_codes(
        *prompt, frames, temperature=0.8, top_k=top_k, seed=seed)
    assert first_divergence(got, orc) is None
    del model


def test_dec_frame_top_k_1_equals_greedy():
    """Temperature 0.8 with top_k = 1 keeps the maximum alone, whatever the noise: the radix select runs all
    four passes with one key left to find, and the Gumbel pass and the block arg-max see one candidate.  B = 1
    bf16 on the persistent frame decoder, 4 frames: codes equal to the same engine's greedy codes and to the
    oracle's.  No head of these frames has its two largest logits equal (asserted on the oracle's logits), so
    a threshold off by one entry cannot hide behind a tie."""
    from csm_mlx.sampling import Sampler
    from csm_mlx.tokenizers import tokenize_text_segment
    args, w, model = build_model("1b", "bf16")
    prompt, frames = tokenize_text_segment(prompt_ids(31), 0, 32), 4
    orc, logs = oracle_for(args, w, bf16=True).generate_codes(*prompt, frames, collect_logits=True)
    for c0, ci in logs:
        for row in (c0, *ci):
            top = np.sort(row)[-2:]
            assert top[1] > top[0], "two equal maxima: pick another prompt"
    set_option(model, "dec_frame", 1)

    def run(smp):
        e0 = epoch(model, "dec_frame")
        got = codes_per_utterance(model, [prompt], frames, smp, seeds=[777])[0]
        assert epoch(model, "dec_frame") - e0 == frames * handoffs("dec_frame", args.n_audio_codebooks), \
            "the persistent frame decoder did not run every frame"
        return got
    greedy, got = run(Sampler(0.0, 0)), run(Sampler(0.8, 1))
    del model
    assert len(got) == frames and first_divergence(got, greedy) is None, \
        f"top_k 1 differs from greedy at frame {first_divergence(got, greedy)}"
    assert first_divergence(got, orc) is None, f"top_k 1 differs from the oracle's greedy codes at frame {first_divergence(got, orc)}"
