/*
 * csm_hip.h -- C ABI of libcsm_hip.so, the MI355X (gfx950) engine behind the
 * csm_mlx drop-in API.  Plain pointers and sizes only; no torch types.
 *
 * Every entry point returns 0 on success or a negative csm_status; the message
 * of the last failure on the calling thread is available from csm_last_error().
 * The Python layer (csm-mlx_amd/csm_mlx/_lib.py) binds these with ctypes and
 * maps failures to the reference's exceptions.
 *
 * Reference interfaces replaced (all /root/reference/csm_mlx/...):
 *   csm_engine_create / csm_load_tensor    CSM(args) + Module.load_weights
 *                                          (models.py:31-77; README.md:38-40)
 *   csm_set_rope_table                     Llama3ScaledRoPE.rope_init cache (attention.py:57-92)
 *   csm_begin / csm_prefill                generate(): prompt assembly + first generate_frame
 *                                          backbone pass (generation.py:108-140)
 *   csm_run_frames                         the frame loop: generate_frame (generation.py:21-92)
 *                                          + EOS test (:151) + feedback row (:156-161)
 *   csm_read_codes                         the stacked samples (generation.py:154, :167-170)
 *   mimi_*                                 moshi_mlx Mimi encode / decode / decode_step /
 *                                          reset_state (tokenizers.py:14-21, 61-85, 148-150;
 *                                          generation.py:224-258)
 */
#ifndef CSM_HIP_H
#define CSM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum csm_status {
  CSM_OK = 0,
  CSM_ERR_ARG = -1,       /* bad argument / shape (ValueError) */
  CSM_ERR_HIP = -2,       /* HIP runtime failure (RuntimeError) */
  CSM_ERR_STATE = -3,     /* call out of order, e.g. weights missing */
  CSM_ERR_TOO_LONG = -4   /* prompt + frames exceed the 2048-position window (generation.py:132-137) */
};

/* CSM_Q4: MLX affine int4, group 64 (nn.quantize(model, 64, 4)); as a host source dtype, CSM_U32 marks
 * MLX-packed int4 weights (8 nibbles per uint32, element j at bits 4*(j%8)). */
enum csm_dtype { CSM_F32 = 0, CSM_BF16 = 1, CSM_Q4 = 2, CSM_U32 = 3 };

typedef struct csm_llama_dims {
  int n_layers, hidden, n_heads, n_kv_heads, head_dim, intermediate;
  float eps;
} csm_llama_dims;

typedef struct csm_dims {
  csm_llama_dims backbone, decoder;
  int n_text_vocab, n_audio_vocab, n_audio_codebooks;
  int max_seq_len; /* RoPE / KV window: 2048 (generation.py:132, attention.py:38) */
} csm_dims;

typedef struct csm_engine csm_engine;

const char* csm_last_error(void);
int csm_device_count(int* n);

/* weight_dtype: storage of every Linear/Embedding weight (CSM_F32 parity mode, CSM_BF16 perf, CSM_Q4 int4
 * g64: float weights loaded into it are quantized on the device; MLX-quantized checkpoints load as
 * <name>.weight (CSM_U32 [n][K/8]) + <name>.scales + <name>.biases ([n][K/64] f32 or bf16)).
 * audio_head is never quantized (bf16 in a CSM_Q4 engine). */
int csm_engine_create(const csm_dims* dims, int device, int weight_dtype, int max_batch, int max_frames,
                      csm_engine** out);
int csm_engine_destroy(csm_engine* e);
/* name: MLX parameter key; host: src_dtype data, C-contiguous, shape as in the checkpoint */
int csm_load_tensor(csm_engine* e, const char* name, const void* host, int src_dtype, const int64_t* shape,
                    int ndim);
/* which: 0 backbone, 1 decoder; table [max_seq_len][head_dim/2][2] = (cos, sin) float32 */
int csm_set_rope_table(csm_engine* e, int which, const float* table, int n_pos, int head_dim);
/* returns CSM_ERR_STATE and names the first missing tensor when weights are incomplete */
int csm_weights_ready(csm_engine* e);
/* Multi-GPU weight distribution (no reference counterpart: the reference is single-device).  The
 * engine's resident weight buffers -- every Linear / Embedding / norm / head matrix in kernel layout
 * and storage dtype, in a fixed order -- so one rank's loaded buffers can be broadcast device to
 * device (RCCL) into identically created engines.  *n = buffer count; up to cap (ptr, bytes) pairs
 * are written.  csm_weights_received then marks a receiving engine's weights as loaded (derived
 * tables and tiled copies rebuild at the next csm_begin). */
int csm_weight_buffers(csm_engine* e, void** ptrs, uint64_t* bytes, int cap, int* n);
int csm_weights_received(csm_engine* e);
/* nn.quantize(model, group_size, bits) (run_streaming_csm_mlx.py:811-818; README.md:108-111): convert every
 * loaded Linear / Embedding weight to int4 in place (MLX affine rule, oracle/quant_oracle.py).  Only
 * group_size 64, bits 4.  audio_head and the norms keep their dtype. */
int csm_quantize(csm_engine* e, int group_size, int bits);

/* Start a batch of B utterances.  temperature 0 = greedy (generation.py:51); top_k 0 = off.
 * seeds[B]: per-utterance sampling seeds (build's counter-based Gumbel sampler). */
int csm_begin(csm_engine* e, int B, const uint64_t* seeds, float temperature, int top_k);
/* mlx_lm make_sampler's filters beyond top_k (README.md:49, cli/generate.py:168-174: temp, top_p, min_p,
 * min_tokens_to_keep, top_k), applied in its order top_k -> top_p -> min_p to the log-probabilities
 * before the Gumbel-max draw (oracle/csm_oracle.py filter_keep).  top_p in (0, 1) and min_p != 0 are
 * active; call after csm_begin, before the first frame (csm_begin resets them to off). */
int csm_set_sampler_filters(csm_engine* e, double top_p, double min_p, int min_tokens_to_keep);
/* mlx_lm make_logits_processors on the c0 logits (generation.py:44-49), run inside the frame: first
 * logits[bias_idx[i]] += bias_val[i] (n_bias 0: no bias), then for every code t among the utterance's last
 * repetition_context_size c0 codes of this generation, once per distinct t, logits[t] * penalty when
 * negative, else logits[t] / penalty (penalty 0: none); all float32.  CSM_ERR_ARG for an index outside
 * [0, n_audio_vocab), a penalty < 0 or a context < 0 or above the device cap of 256.
 * Call after csm_begin, before the first frame (csm_begin resets to off). */
int csm_set_c0_processors(csm_engine* e, int n_bias, const int32_t* bias_idx, const float* bias_val,
                          float repetition_penalty, int repetition_context_size);
/* Prompt rows of utterance b: tokens/mask [T][K+1] (text id in the last column), appended after the rows the
 * utterance already holds.  Rows past position max_seq_len - 1: CSM_ERR_TOO_LONG, checked before anything is
 * launched (csm_prefill_batch alike: one utterance too long refuses the whole call). */
int csm_prefill(csm_engine* e, int b, int T, const int32_t* tokens, const uint8_t* mask);
/* csm_prefill for several utterances at once (the rows of generate_batch's prompts): utts[i] gets
 * Ts[i] rows, rows of all of them concatenated in tokens / masks.  Up to max_seq_len rows per pass
 * run as ONE pass of every backbone projection (the weights stream once for all of them; each row
 * keeps its own utterance's KV cache and positions), so the results are those of csm_prefill per
 * utterance up to summation order.  No reference counterpart (the reference is batch-1). */
int csm_prefill_batch(csm_engine* e, int n, const int32_t* utts, const int32_t* Ts, const int32_t* tokens,
                      const uint8_t* masks);
/* Generate up to nframes frames for the whole batch (one HIP graph replay per frame).
 * *all_done (optional) = 1 when every utterance hit EOS. */
int csm_run_frames(csm_engine* e, int nframes, int* all_done);
/* csm_run_frames without waiting on this chunk: enqueues nframes frames, then waits for the PREVIOUS
 * chunk enqueued by this call (not for the frames just enqueued) and sets *prev_all_done = 1 when every
 * utterance had hit EOS by its end, 0 when not, -1 when there was no previous chunk.  The generation loop
 * (generation.py:139-161) thus tests EOS one chunk behind while the next chunk already runs, so the GPU
 * never idles on the host's poll; frames enqueued past an all-EOS chunk change no returned code or frame
 * count.  CSM_ERR_HIP if a persistent kernel's hand-off timed out in the polled chunk. */
int csm_run_frames_ahead(csm_engine* e, int nframes, int* prev_all_done);
/* One frame (generation.py:21-92 + the EOS test :151) with its result handed back: out_codes [B][K]
 * int32 = the frame's codes (the `sample` generate_frame returns), done [B] = utterances past EOS.
 * Either pointer may be NULL.  Equivalent to csm_run_frames(e, 1, NULL) followed by a read of the
 * frame's codes; CSM_ERR_STATE when the engine's frame capacity is exhausted. */
int csm_frame_step(csm_engine* e, int32_t* out_codes, uint8_t* done);
/* One frame split around a host hook on the c0 logits (logits_processors, generation.py:42-49):
 * csm_frame_c0_logits runs the backbone step + codebook0_head and copies logits [B][V] out;
 * csm_frame_finish takes the (processed) logits [B][V] back, picks c0 (arg-max when greedy, else the
 * engine's sampler) and runs the 31 decoder steps.  Replaces generate_frame's processor loop
 * (generation.py:44-49) -- called once per frame instead of csm_run_frames.  mlx_lm's two standard
 * processors (logit_bias, repetition_penalty) no longer need it: csm_set_c0_processors runs them inside
 * the frame; this pair remains for arbitrary host callables. */
int csm_frame_c0_logits(csm_engine* e, float* logits);
int csm_frame_finish(csm_engine* e, const float* logits, int* all_done);
/* A frame sampled on the host by an arbitrary sampler callable (the sampler= keyword the reference CLI
 * passes, cli/generate.py:168-174, :197-199; upstream csm-mlx applied it to every codebook's logits):
 * after csm_frame_c0_logits, call csm_frame_host_step K times; call i (1..K) hands the host's codes[B]
 * of codebook i-1 to the engine, which feeds them forward (as csm_frame_forced does) and runs decoder
 * step i + its head: logits [B][V] receive codebook i's logits for calls 1..K-1; call K finishes the
 * frame (history, EOS) and sets *all_done.  Replaces csm_frame_finish for that frame. */
int csm_frame_host_step(csm_engine* e, const int32_t* codes, float* logits, int* all_done);
/* Teacher-forced frame (the scoring form of trainer.py:203-318 compute_loss): the backbone step
 * consumes the previous frame, then every head stores its logits while the code fed forward is
 * codes[B][K] (the target frame).  c0_logits [B][V] and ci_logits [K-1][B][V] (optional, may be
 * NULL) receive the logits that predict codes[b][0] and codes[b][1..K-1]; ce [B][K] (optional)
 * their cross entropies logsumexp(logits) - logits[code], reduced on the device. */
int csm_frame_forced(csm_engine* e, const int32_t* codes, float* c0_logits, float* ci_logits, float* ce);
/* hist [F][B][K] int32 of the frames generated so far, n_frames[B] emitted frames (EOS excluded),
 * done[B].  Any pointer may be NULL. */
int csm_read_codes(csm_engine* e, int32_t* hist, int32_t* n_frames, uint8_t* done, int* frames_run);
/* Continuous batching (no reference counterpart: the reference runs one utterance per call).  The B rows of
 * the batch csm_begin started are slots: each holds at most one utterance, and at any frame boundary (between
 * two csm_run_frames calls) a slot can start a new utterance or be parked while the others go on.  An
 * utterance's codes depend only on its prompt, its seed, the sampler and the processors -- not on the slot,
 * on when it joined, on the other slots or on what ran in the slot before.  The first slot call after
 * csm_begin puts the engine in slot mode; csm_begin leaves it.  In slot mode the code history is a ring of
 * max_frames frames, so a session may run any number of frames while no single utterance exceeds max_frames.
 *   csm_slot_restart  slot b starts a new utterance: the pending backbone row of the batch runs first (the
 *                     other slots' last frame reaches their KV caches), then slot b's position, frame
 *                     counters, done flag and codes are cleared and its seed set.  Follow with csm_prefill(b)
 *                     or one csm_prefill_batch for all the slots restarted at this boundary.
 *   csm_slot_release  slot b holds no utterance: it is parked (position 0, done set); its rows still run in
 *                     every frame but touch nothing outside the slot.
 *   csm_slot_read     codes [n][K] of slot b's utterance (EOS excluded; cap_frames = rows the buffer holds,
 *                     CSM_ERR_ARG when it is too small), *n_frames and *done; any pointer may be NULL.
 *   csm_slot_set_sampling  slot b's utterance has a sampler and processors of its own (below); every
 *                     csm_slot_restart and csm_slot_release puts the slot back on the batch's.
 * CSM_ERR_STATE: b >= B; a restart between csm_frame_c0_logits and csm_frame_finish; running frames while a
 * restarted slot has no prompt; frames that would take an utterance past max_frames;
 * csm_read_codes(hist != NULL), csm_frame_c0_logits and csm_frame_forced in slot mode (csm_read_codes still
 * polls n_frames and done). */
int csm_slot_restart(csm_engine* e, int b, uint64_t seed);
int csm_slot_release(csm_engine* e, int b);
int csm_slot_read(csm_engine* e, int b, int32_t* codes, int cap_frames, int* n_frames, uint8_t* done);
/* The sampler and the c0 processors of one utterance: csm_begin's temperature and top_k, csm_set_sampler_filters'
 * top_p, min_p and min_tokens_to_keep, csm_set_c0_processors' bias, penalty and context, with their meanings
 * (temperature 0: greedy, and then no filter; n_bias 0: no bias; repetition_penalty 0: none). */
typedef struct csm_sampling {
  float temperature; int top_k; double top_p, min_p; int min_tokens_to_keep;
  int n_bias; const int32_t* bias_idx; const float* bias_val;
  float repetition_penalty; int repetition_context_size;
} csm_sampling;
/* Slot b's utterance samples with *s instead of the batch's sampler and processors (s NULL: the batch's
 * again).  After csm_slot_restart(b), before the first frame of that utterance.  The values live in device
 * memory, written on the engine stream: frames already enqueued do not see them, and a join captures no
 * graph -- only a change of what the slots holding an utterance need between them does (all greedy / some
 * sampled / some with top_p or min_p / some with a bias or penalty: one frame graph each).  A greedy utterance
 * beside sampled ones gets the codes it gets in a greedy batch.  CSM_ERR_ARG as csm_set_sampler_filters and
 * csm_set_c0_processors (a bias index outside [0, n_audio_vocab), a penalty < 0, a context above 256, ...);
 * CSM_ERR_STATE for b >= B, outside slot mode, for a parked slot, or once the utterance has run a frame. */
int csm_slot_set_sampling(csm_engine* e, int b, const csm_sampling* s);
/* Shared context prefixes (no reference counterpart: the reference's generate() pushes every context segment
 * through the backbone again for each sentence, generation.py:108-125).  Attention is causal, so the backbone
 * K / V of a prompt's first P rows depend on those rows alone: they are saved once and loaded into any
 * utterance or slot that begins with the same rows, which then prefills only what follows (csm_prefill* append
 * after the rows an utterance holds).  A prefix is a compact device buffer [layer][k|v][Hkv][rows][hd] fp32
 * owned by the engine until csm_prefix_free or csm_engine_destroy; a growing batch does not lose it.
 *   csm_prefix_save  positions 0 .. rows-1 of utterance b's backbone caches, every layer -> *id (a small
 *                    handle).  Right after a prefill or in the middle of an utterance; the batch goes on as
 *                    if it had not been called.  Only rows that have reached the cache count (the row of the
 *                    last frame's codes has not until the next frame runs): CSM_ERR_ARG unless
 *                    1 <= rows <= rows held; CSM_ERR_STATE when b holds none (fresh, restarted or parked).
 *   csm_prefix_load  for n distinct utterances at once: prefix ids[i] -> utterance utts[i], positions
 *                    0 .. rows-1, and its position becomes rows - 1; one launch on the engine stream for all n,
 *                    not waited for.  The utterance still has no prompt: frames stay CSM_ERR_STATE
 *                    ("csm_prefill not called") until at least one more row is prefilled.  Several utterances
 *                    may load the same prefix.  Works after csm_begin and after csm_slot_restart.  Refused
 *                    before anything is launched, every utterance left as it was: CSM_ERR_STATE when an
 *                    utterance already holds rows, between csm_frame_c0_logits and csm_frame_finish, or for
 *                    a stale prefix; CSM_ERR_ARG for an unknown handle or an utterance out of range or
 *                    repeated; CSM_ERR_TOO_LONG when rows >= max_seq_len.
 *   csm_prefix_free  waits for the engine stream (a load in flight still reads the buffer), then releases it.
 *   csm_prefix_info  *rows and *bytes of a prefix (either may be NULL).
 * A prefix is valid for the weights and the RoPE table it was computed with: after csm_load_tensor (adapters
 * included), csm_quantize, csm_set_rope_table or csm_weights_received every older prefix is stale -- it cannot
 * be loaded, csm_prefix_info still answers for it and csm_prefix_free still frees it. */
int csm_prefix_save(csm_engine* e, int b, int rows, int* id);
int csm_prefix_load(csm_engine* e, int n, const int32_t* utts, const int32_t* ids);
int csm_prefix_free(csm_engine* e, int id);
int csm_prefix_info(csm_engine* e, int id, int* rows, int64_t* bytes);
/* Debug / parity taps: "h_last" [B][D], "c0_logits" [B][Vpad], "ci_logits" [K-1][B][Vpad], "codes" [B][K],
 * "audio_head" [K-1][Vpad][Dd] (f32 or bf16 bits),
 * "weight:<MLX name>" a whole (unfused) Linear / Embedding matrix in its device layout (int4: nibbles
 * [N][K/2] then {scale, bias} bf16 pairs [N][K/64]). */
int csm_debug_read(csm_engine* e, const char* what, void* host, int64_t nbytes, int64_t* needed);
/* The module views of CSM (models.py:53-92): rows[n] of a stored Linear / Embedding weight (MLX key,
 * e.g. "audio_embeddings.weight") as fp32 [n][in] (int4: the dequantized values the kernels use) --
 * CSM.embed_tokens / embed_audio / <module>.weight -- and a Linear applied on the GPU: y [M][out] =
 * x [M][in] . W^T (the GEMV's arithmetic) for a Linear key, or x [M][Dd] . audio_head[i] for
 * "audio_head.<i>" (generation.py:79). */
int csm_read_rows(csm_engine* e, const char* name, int n, const int32_t* rows, float* out);
int csm_linear(csm_engine* e, const char* name, int M, const float* x, float* y);
/* Device pointer of the code history [F][B][K] (for on-device Mimi decode) */
int csm_codes_device_ptr(csm_engine* e, void** dev_ptr);
int csm_synchronize(csm_engine* e);
/* ------------------------------------------------------------------ Mimi codec */
typedef struct mimi_dims {
  int channels, dimension, n_filters, n_ratios, ratios[8];
  int kernel_size, residual_kernel_size, last_kernel_size, compress;
  int num_heads, num_layers, dim_feedforward, context;
  int n_q, bins, codebook_dim, downsample_stride;
  float norm_eps;
  int gelu_erf;   /* 0: tanh approximation (mlx gelu_approx), 1: exact */
  int attn_mode;  /* 0: moshi_mlx (no mask inside a call), 1: causal sliding window */
} mimi_dims;

typedef struct mimi_codec mimi_codec;

int mimi_create(const mimi_dims* dims, int device, int max_batch, int max_frames, mimi_codec** out);
int mimi_destroy(mimi_codec* m);
int mimi_load_tensor(mimi_codec* m, const char* name, const void* host, int src_dtype, const int64_t* shape,
                     int ndim);
/* RoPE table for the codec transformer: [n_pos][head_dim/2][2] */
int mimi_set_rope_table(mimi_codec* m, const float* table, int n_pos, int head_dim);
int mimi_weights_ready(mimi_codec* m);
/* pcm [B][N] float32 host -> codes [B][n_q][Tf] int32 host; *n_frames_out = Tf */
int mimi_encode(mimi_codec* m, int B, int N, const float* pcm, int32_t* codes, int* n_frames_out);
/* as mimi_encode with utterance b's N samples at rows[b] (pcm NULL): the batched context encode of
   tokenize_segments_batch (reference tokenizers.py:61-85 per segment) without a host-side stacking copy */
int mimi_encode_rows(mimi_codec* m, int B, int N, const float* pcm, const float* const* rows, int32_t* codes,
                     int* n_frames_out);
/* codes [B][n_q][F] -> pcm [B][F*frame_size].  codes_on_device / pcm_on_device select device pointers;
 * codes_layout 0 = [B][n_q][F], 1 = engine history [F][B][n_q] */
int mimi_decode(mimi_codec* m, int B, int F, const int32_t* codes, int codes_on_device, int codes_layout,
                float* pcm, int pcm_on_device);
/* streaming: reset per-utterance state, then one frame at a time: codes [B][n_q] -> pcm [B][frame_size] */
int mimi_reset_state(mimi_codec* m, int B);
int mimi_decode_step(mimi_codec* m, int B, const int32_t* codes, float* pcm);
/* Slot streaming (the codec's side of csm_slot_*): every row of the streaming decoder state is a slot with its
 * own stream and its own latent position, so one slot starts a new utterance while its neighbours go on.
 *   mimi_slot_reset    row b starts a new stream: its slice of every conv / upsample history is zeroed and
 *                      its position set to 0 by one small launch on the codec stream (no wait).  The KV
 *                      caches are not cleared: from position 0 on the slot reads only keys it has written
 *                      since.  The first call after mimi_create or mimi_reset_state puts the codec in slot
 *                      mode and clears every row once; mimi_reset_state and mimi_decode leave slot mode.
 *                      CSM_ERR_ARG: b outside [0, max_batch), or a codec of more than 256 rows.
 *   mimi_decode_slots  n consecutive frames of rows 0..B-1 in one pass, each slot continuing its own stream:
 *                      codes from a ring history [F_cap][B][n_q] (csm_codes_device_ptr's layout with
 *                      codes_on_device, the same layout in host memory without) at rows
 *                      (first_row + f) % F_cap, f < n; pcm [B][n * frame_size] float32 host.  active[B]
 *                      (host): an inactive row still runs (its pcm is not audio) but its position does not
 *                      advance, and it must be reset before it carries a stream again.  Waits for the
 *                      codec stream.  A slot's frames equal mimi_decode_step's on that stream alone,
 *                      however the frames are split over calls.
 *                      CSM_ERR_STATE: not in slot mode.  CSM_ERR_ARG: B > max_batch, n < 1, n > F_cap, or an
 *                      active slot would pass the codec's capacity (refused before anything is launched).
 * mimi_decode_step in slot mode is CSM_ERR_STATE. */
int mimi_slot_reset(mimi_codec* m, int b);
int mimi_decode_slots(mimi_codec* m, int B, int n, const int32_t* hist, int codes_on_device, int F_cap,
                      int first_row, const uint8_t* active, float* pcm);
/* Streaming encode, the other half of the moshi Mimi streaming interface: every row of the codec is a slot with
 * an encode stream of its own (conv histories, encoder-transformer KV, latent position), so audio arriving in
 * blocks is encoded in one pass per tick for all callers.  The state is allocated by the first
 * mimi_encode_slot_reset, is separate from the decoder's streaming state and from the one-shot encode's KV:
 * mimi_reset_state, mimi_decode, mimi_decode_slots, mimi_decode_step, mimi_encode and mimi_encode_rows neither
 * read nor change it, and these two calls leave the decoder's slot mode alone.
 *   mimi_encode_slot_reset  row b starts a new stream: its histories zeroed and its position set to 0 by one
 *                      small launch on the codec stream (enqueued, not waited for).  The first call allocates
 *                      the state, every row an idle slot at position 0.
 *                      CSM_ERR_ARG: b outside [0, max_batch), or a codec of more than 256 rows.
 *   mimi_encode_slots  n whole frames of rows 0..B-1 in one pass: pcm [B][n * frame_size] float32 host ->
 *                      codes [B][n_q][n] int32 host; waits for the codec stream.  A slot's codes equal the
 *                      frame-by-frame encode of its stream alone however the frames are split over calls: in
 *                      the causal attention mode the one-shot encode of the same audio, in the moshi_mlx mode
 *                      each frame sees its own frame's keys and the past (a call per frame).  No end-of-clip
 *                      padding exists in a stream: a trailing partial frame cannot be encoded.  active[B]
 *                      (host): an inactive row flows through the pass (its codes mean nothing), but neither its
 *                      histories nor its position change and its keys land where its next active call
 *                      overwrites them, so its stream goes on at its next active call without a reset.
 *                      Afterwards mimi_debug_read "rows" holds the pre-RVQ latent [B * n][dimension], row
 *                      b * n + f.
 *                      CSM_ERR_STATE: no mimi_encode_slot_reset yet.  CSM_ERR_ARG: a null pointer, B outside
 *                      [1, max_batch], n < 1, a codec of more than 256 rows, or an active slot whose position
 *                      + n * downsample_stride + 4 exceeds the codec's latent capacity (as n *
 *                      downsample_stride + 4 alone does for any slot): refused before anything is launched,
 *                      no stream changes. */
int mimi_encode_slot_reset(mimi_codec* m, int b);
int mimi_encode_slots(mimi_codec* m, int B, int n, const float* pcm, const uint8_t* active, int32_t* codes);

#ifdef __cplusplus
}
#endif
#endif /* CSM_HIP_H */
