"""``make_logits_processors`` inside the frame on the GPU (csm_set_c0_processors): the launch path's
c0_process_kernel and the persistent frame decoder's head_publish, against the oracle, against the paused
host path (the same descriptors wrapped in plain callables, which ``device_processors`` turns down) and
against each other.

The designed input makes the processors' effect analytic: logit_bias {A: 50, B: 40} with repetition
penalty 4.  The synthetic c0 logits are small (|raw| < 4, asserted below from the taps), so c0 is A
unless A is in the repetition window and B is not (50 + r > 40 + r', 12.5 + r/4 > 10 + r'/4, but
12.5 + r/4 < 40 + r').  With a window of 4: A B A A A A B ..., frame 3 = A shows a duplicate in the
window penalised once (twice: 3.1 < 10), frame 6 = B that B has left the window; with a window of 1: A B A B."""
import numpy as np
import pytest

from helpers import first_divergence, oracle_for, prompt_ids, tiny_prompt_ids
from rigs import ab, build_model, codes_per_utterance, frame_taps, handoffs, synchronize

pytestmark = pytest.mark.gpu

A, B_ = 5, 9
RAW_BOUND = 4.0


def procs_ab(context=4):
    from csm_mlx.sampling import make_logits_processors
    return make_logits_processors(logit_bias={A: 50.0, B_: 40.0}, repetition_penalty=4.0, repetition_context_size=context)


def expected_c0(frames, context):
    out = []
    for f in range(frames):
        win = out[max(0, f - context):] if f else []
        out.append(B_ if (A in win and B_ not in win) else A)
    return out


def wrapped(procs, raw=None):
    """The same processors as plain callables (the paused host path); ``raw`` collects the logits the
    first one receives: the engine's unprocessed c0 logits of every frame."""
    def wrap(i, p):
        def fn(tokens, logits):
            if raw is not None and i == 0:
                raw.append(np.array(logits, np.float32, copy=True))
            return p(tokens, logits)
        return fn
    return [wrap(i, p) for i, p in enumerate(procs)]


def run_frames(model, prompts, frames, sampler, seeds, procs):
    """Frame by frame (one graph replay or one paused frame per call): codes (F, B, K) and the c0_logits
    tap (B, V) after every frame."""
    from csm_mlx.generation import device_processors
    dev = device_processors(procs, sampler)
    c0_hist = []
    paused = None if dev is not None or not procs else lambda cache, f: cache.run_processed(procs, c0_hist)
    hist, _, taps = frame_taps(model, prompts, frames, sampler, seeds, ("c0_logits",), step=paused, processors=dev)
    return hist, taps["c0_logits"]


@pytest.fixture(scope="module")
def tiny():
    args, w, m = build_model("tiny", "float32", max_batch=4)
    return m, oracle_for(args, w), args


def tiny_prompts(args, seeds):
    from csm_mlx.tokenizers import tokenize_text_segment
    return [tokenize_text_segment(tiny_prompt_ids(s), 0, args.n_audio_codebooks) for s in seeds]


@pytest.mark.parametrize("context,frames", [(4, 10), (1, 4)])
def test_launch_path_greedy_bias_and_penalty(tiny, context, frames):
    from csm_mlx.generation import device_processors
    from csm_mlx.sampling import Sampler
    from oracle.csm_oracle import text_frame
    model, o, args = tiny
    K, seeds, smp = args.n_audio_codebooks, (21, 22, 23), Sampler(0.0, 0)
    prompts, procs = tiny_prompts(args, seeds), procs_ab(context)
    assert device_processors(procs, smp) is not None
    got = codes_per_utterance(model, prompts, frames, smp, None, procs)
    raw = []
    host = wrapped(procs, raw)
    assert device_processors(host, smp) is None
    paused = codes_per_utterance(model, prompts, frames, smp, None, host)
    print("max |raw c0 logit|", max(float(np.abs(r).max()) for r in raw))
    assert len(raw) == frames and all(np.abs(r).max() < RAW_BOUND for r in raw)
    for b, s in enumerate(seeds):
        ref = o.generate_codes(*text_frame(tiny_prompt_ids(s), K), frames, processors=procs)
        assert first_divergence(got[b], ref) is None, (b, got[b][:, 0], ref[:, 0])
        assert first_divergence(got[b], paused[b]) is None, (b, got[b][:, 0], paused[b][:, 0])
        assert list(got[b][:, 0]) == expected_c0(frames, context)
    if context == 4:
        assert got[0][3, 0] == A and got[0][6, 0] == B_
    # frame by frame: the tap holds the processed logits, the same bits on both paths
    h_dev, t_dev = run_frames(model, prompts, frames, smp, None, procs)
    h_host, t_host = run_frames(model, prompts, frames, smp, None, host)
    assert np.array_equal(h_dev, h_host) and np.array_equal(h_dev[:, 0], got[0])
    for f in range(frames):
        assert np.array_equal(t_dev[f], t_host[f]), f"frame {f}: processed c0 logits differ from the paused path"


@pytest.mark.parametrize("sampler_kw,seeds", [(dict(temp=0.8, top_k=5), (31, 32, 33)),
                                              (dict(temp=0.8, top_p=0.9), (35, 41, 51))])
def test_launch_path_sampled_penalty(tiny, sampler_kw, seeds):
    """Penalty 1.3 over a window of 20, no bias, 12 frames; the prompt seeds are ones where the oracle's
    codes change under the penalty and a penalised logit is negative (the multiply branch)."""
    from csm_mlx.sampling import Sampler, make_logits_processors
    from oracle.csm_oracle import text_frame
    model, o, args = tiny
    K, frames = args.n_audio_codebooks, 12
    smp = Sampler(sampler_kw["temp"], sampler_kw.get("top_k", 0), sampler_kw.get("top_p", 0.0))
    prompts = tiny_prompts(args, seeds)
    rng = [1000 + s for s in seeds]
    procs = make_logits_processors(repetition_penalty=1.3, repetition_context_size=20)
    got = codes_per_utterance(model, prompts, frames, smp, rng, procs)
    raw = []
    paused = codes_per_utterance(model, prompts, frames, smp, rng, wrapped(procs, raw))
    plain = codes_per_utterance(model, prompts, frames, smp, rng, None)
    negative = 0
    for b, s in enumerate(seeds):
        ref = o.generate_codes(*text_frame(tiny_prompt_ids(s), K), frames, temperature=smp.temp, top_k=smp.top_k,
                               top_p=smp.top_p, seed=rng[b], processors=procs)
        assert first_divergence(got[b], ref) is None, (b, got[b][:, 0], ref[:, 0])
        assert first_divergence(got[b], paused[b]) is None, (b, got[b][:, 0], paused[b][:, 0])
        assert first_divergence(got[b], plain[b]) is not None, f"utterance {b}: the penalty changed nothing"
        for f in range(1, len(got[b])):
            negative += int((raw[f][b, np.unique(got[b][:f, 0])] < 0).sum())
    assert negative > 0, "no penalised logit was negative: the multiply branch did not run"


@pytest.fixture(scope="module", params=["bf16", "q4"])
def model_1b(request):
    args, w, m = build_model("1b", request.param, max_batch=8)
    yield m, args, w, request.param
    del m


def test_persistent_decoder_greedy(model_1b):
    """csm_1b, B = 1: the persistent frame decoder applies the processors to its own head rows."""
    from csm_mlx.sampling import Sampler
    from csm_mlx.tokenizers import tokenize_text_segment
    model, args, w, dtype = model_1b
    frames, smp, procs = 8, Sampler(0.0, 0), procs_ab(4)
    prompt = tokenize_text_segment(prompt_ids(41), 0, 32)
    (ref, ref_taps), (got, got_taps) = ab(model, "dec_frame", lambda: run_frames(model, [prompt], frames, smp, [0], procs),
                                          frames * handoffs("dec_frame", args.n_audio_codebooks))
    raw = []
    paused, _ = run_frames(model, [prompt], frames, smp, [0], wrapped(procs, raw))
    print("max |raw c0 logit|", max(float(np.abs(r).max()) for r in raw))
    assert all(np.abs(r).max() < RAW_BOUND for r in raw)
    assert first_divergence(got[:, 0], ref[:, 0]) is None, f"codes differ from the launch path at {first_divergence(got[:, 0], ref[:, 0])}"
    assert first_divergence(got[:, 0], paused[:, 0]) is None
    assert list(got[:, 0, 0]) == expected_c0(frames, 4)
    for f in range(frames):
        a, b = got_taps[f][0], ref_taps[f][0]
        assert np.abs(a - b).max() <= 2e-3 * np.abs(b).max(), f"frame {f}: processed c0 logits differ"
    orc = oracle_for(args, w, bf16=(dtype == "bf16"), q4=(dtype == "q4")).generate_codes(*prompt, frames, processors=procs)
    assert first_divergence(got[:, 0], orc) is None


@pytest.mark.parametrize("top_k", [0, 50])
def test_persistent_decoder_sampled(model_1b, top_k):
    """The Gumbel-key (top_k 0) and every-logit (top_k 50) publications of the processed c0 rows."""
    from csm_mlx.sampling import Sampler
    from csm_mlx.tokenizers import tokenize_text_segment
    model, args, w, dtype = model_1b
    frames, smp, procs = 6, Sampler(0.8, top_k), procs_ab(4)
    prompt = tokenize_text_segment(prompt_ids(41), 0, 32)
    ref, got = ab(model, "dec_frame", lambda: codes_per_utterance(model, [prompt], frames, smp, [4242], procs)[0],
                  frames * handoffs("dec_frame", args.n_audio_codebooks))
    assert len(got) == frames and first_divergence(got, ref) is None, \
        f"sampled codes differ from the launch path at frame {first_divergence(got, ref)}: {got[:, 0]} vs {ref[:, 0]}"
    assert set(got[:, 0]) <= {A, B_}


@pytest.mark.parametrize("model_1b", ["bf16"], indirect=True)
def test_batched_1b_matches_paused_path(model_1b):
    """B = 8: the one-partial c0 hand-over into the batched step-1 projection and the persistent step."""
    from csm_mlx.sampling import Sampler
    from csm_mlx.tokenizers import tokenize_text_segment
    model, args, w, dtype = model_1b
    frames, smp, procs = 6, Sampler(0.0, 0), procs_ab(4)
    prompts = [tokenize_text_segment(prompt_ids(50 + b), 0, 32) for b in range(8)]
    got = codes_per_utterance(model, prompts, frames, smp, None, procs)
    paused = codes_per_utterance(model, prompts, frames, smp, None, wrapped(procs))
    for b in range(8):
        assert first_divergence(got[b], paused[b]) is None, (b, got[b][:, 0], paused[b][:, 0])
        assert list(got[b][:, 0]) == expected_c0(frames, 4)
    synchronize(model)                                                            # no hand-off timeout flag left


def test_stream_generate_and_graph_replay(tiny):
    from csm_mlx import stream_generate
    from csm_mlx.config import MIMI_CONFIGURATION
    from csm_mlx.mimi import MimiCodec
    from csm_mlx.sampling import Sampler
    from csm_mlx.tokenizers import set_audio_tokenizer
    from csm_mlx.weights import synthetic_mimi_weights
    model, _, args = tiny
    mm = MIMI_CONFIGURATION["tiny"]
    codec = MimiCodec(mm, max_batch=4, max_frames=300)
    codec.load_weights(synthetic_mimi_weights(mm))
    set_audio_tokenizer(codec, args.n_audio_codebooks)
    ids, procs = tiny_prompt_ids(21), procs_ab(4)
    dev = list(stream_generate(model, ids, 0, [], max_audio_length_ms=6 * 80, temperature=0.0, logits_processors=procs))
    host = list(stream_generate(model, ids, 0, [], max_audio_length_ms=6 * 80, temperature=0.0,
                                logits_processors=wrapped(procs)))
    assert len(dev) == len(host) == 6
    for a, b in zip(dev, host):
        assert float(np.sqrt(np.mean((a - b) ** 2))) <= 1e-4
    prompts = tiny_prompts(args, (21, 22, 23))
    one = codes_per_utterance(model, prompts, 40, Sampler(0.0, 0), None, procs)
    two = codes_per_utterance(model, prompts, 40, Sampler(0.0, 0), None, procs)
    for a, b in zip(one, two):
        assert len(a) == 40 and np.array_equal(a, b)
        assert list(a[:, 0]) == expected_c0(40, 4)


def test_set_c0_processors_validation_and_reset(tiny):
    from csm_mlx import _lib
    from csm_mlx.generation import FrameCache
    from csm_mlx.sampling import LogitBias, RepetitionPenalty, Sampler
    model, _, args = tiny
    V, L, smp = args.n_audio_vocab, _lib.lib(), Sampler(0.0, 0)
    prompts = tiny_prompts(args, (21,))
    plain = codes_per_utterance(model, prompts, 6, smp, None, None)[0]
    for bad in ((LogitBias((V,), (1.0,)), None), (LogitBias((-1,), (1.0,)), None), (None, RepetitionPenalty(-1.0, 4)),
                (None, RepetitionPenalty(1.1, 257))):
        with pytest.raises(ValueError):
            FrameCache(model, 1, smp, None, bad)
    FrameCache(model, 1, smp, None)
    idx, val = np.array([V], np.int32), np.array([1.0], np.float32)
    for call in ((1, _lib.ptr(idx), _lib.ptr(val), 0.0, 0), (0, None, None, -1.0, 4), (0, None, None, 1.1, 257),
                 (0, None, None, 1.1, -1)):
        assert L.csm_set_c0_processors(model.engine, *call) == _lib.CSM_ERR_ARG
    changed = codes_per_utterance(model, prompts, 6, smp, None, procs_ab(4))[0]
    assert first_divergence(changed, plain) is not None
    again = codes_per_utterance(model, prompts, 6, smp, None, None)[0]                   # a new csm_begin: processors off
    assert first_divergence(again, plain) is None
