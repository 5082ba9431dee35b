// CSM engine, continuous batching: the B rows of a batch as slots whose utterances start and leave at frame
// boundaries while the others go on (csm_slot_restart / csm_slot_release / csm_slot_read).
//
// Everything a slot owns sits behind pointers the captured frame graphs already hold -- its position, done
// flag, frame count, own frame index (the samplers' counter), seed, feedback codes and parked mark -- so a
// restart rewrites that state with one small kernel on the engine stream and no graph is captured again.
// The code history stays [F_cap][B][K] but is written as a ring over the global frame index; slot b's
// utterance occupies the rows from slot_first[b] on.
//
// Per-utterance sampling (csm_slot_set_sampling): the sampler's and the c0 processors' parameters of slot b are
// row b of a device table the sample kernels, the persistent step's sampler and c0_process_kernel read at run
// time, written on the engine stream like the rest of a slot's state, so frames already enqueued never see a
// later write and a join captures nothing; csm_engine.hip frame_plan picks the frame's plan class from the rows.
// The batch's values are the same record (csm_engine::batch); the value checks and the rounding into a record
// that csm_begin, csm_set_sampler_filters, csm_set_c0_processors and csm_slot_set_sampling share are here
// (sampling_set_*, upload_dense_bias).
#include "csm_engine.h"

namespace {

struct SlotResetParams {
  uint8_t* done;
  int* n_frames;
  int* slot_frame;
  int* codes;  // [B][K]
  uint8_t* parked;
  int* pos;
  uint64_t* seeds;
  float* h_last;  // [B][D]
  int b, K, D;
  uint64_t seed;
  int park;  // 1: the slot holds no utterance from here on
  SlotSampling* sampling;  // per-slot operation: the table, whose row b goes back to the batch's values (null: no table in use)
  SlotSampling batch;
};

// Slot b starts afresh (park 0) or is parked (park 1).  A parked slot's rows still run in every launch: its
// position stays 0 (embed skips the increment), its done flag is set so the EOS poll never waits for it, and its
// backbone output is zeroed so its first frame's head reads finite rows whatever ran in the slot before.
__global__ __launch_bounds__(256) void slot_reset_kernel(SlotResetParams p) {
  const int t = threadIdx.x, b = p.b;
  if (t == 0) {
    p.done[b] = p.park ? 1 : 0;
    p.n_frames[b] = 0;
    p.slot_frame[b] = 0;
    p.parked[b] = p.park ? 1 : 0;
    p.pos[b] = 0;
    p.seeds[b] = p.seed;
    if (p.sampling) p.sampling[b] = p.batch;
  }
  for (int k = t; k < p.K; k += 256) p.codes[(size_t)b * p.K + k] = 0;
  if (p.park)
    for (int d = t; d < p.D; d += 256) p.h_last[(size_t)b * p.D + d] = 0.f;
}

// The checks and bookkeeping csm_slot_restart and csm_slot_release share
void slot_reset(csm_engine* e, int b, uint64_t seed, bool park) {
  if (!e) throw CsmError(CSM_ERR_ARG, "null engine");
  if (e->B <= 0) throw CsmError(CSM_ERR_STATE, "csm_begin not called");
  if (b < 0) throw CsmError(CSM_ERR_ARG, "slot index out of range");
  if (b >= e->B) throw CsmError(CSM_ERR_STATE, "slot " + std::to_string(b) + " beyond the batch of " + std::to_string(e->B));
  if (e->c0_pending) throw CsmError(CSM_ERR_STATE, "csm_frame_finish pending");
  HIPCHK(hipSetDevice(e->dev));
  if (e->ahead_pending) {  // a chunk enqueued by csm_run_frames_ahead: its pinned copies land first
    HIPCHK(hipStreamSynchronize(e->st));
    e->ahead_pending = false;
  }
  if (!e->slot_mode) {
    e->slot_mode = true;
    ++e->filters_id;  // the batch-1 frame decoder leaves the frame graph: capture again
  }
  const bool body = !park && e->need_body;
  if (body)
    for (int u = 0; u < e->B; ++u)
      if (!e->parked_host[u] && u != b && e->pos_host[u] + 1 >= e->dims.max_seq_len)
        throw CsmError(CSM_ERR_TOO_LONG, "rows exceed the 2048-position window");
  SlotResetParams p{};
  p.done = e->done; p.n_frames = e->n_frames; p.slot_frame = e->slot_frame; p.codes = e->codes; p.parked = e->parked;
  p.pos = e->pos; p.seeds = e->seeds; p.h_last = e->h_last; p.b = b; p.K = e->K; p.D = e->D; p.seed = seed; p.park = park ? 1 : 0;
  // the slot forgets its utterance's own sampling: the next one starts from the batch's
  p.sampling = e->per_slot ? e->slot_sampling : nullptr; p.batch = e->batch;
  e->samp_own[b] = 0;
  hipLaunchKernelGGL(slot_reset_kernel, dim3(1), dim3(256), 0, e->st, p);
  HIPCHK(hipGetLastError());
  if (body) {
    // the other slots' previous frame reaches their KV before this slot's prompt rows are prefilled (prefill
    // clears need_body): the pending backbone row of the whole batch, eagerly.  It follows the reset, so the
    // leaving utterance's row lands at position 1 of its slot, inside the cache wherever that utterance
    // stopped; the prompt the caller prefills next overwrites it and sets the position.
    body_if_needed(e);
    e->need_body = false;
  }
  e->parked_host[b] = park ? 1 : 0;
  e->pos_host[b] = park ? 0 : -1;  // a restarted slot's prompt rows start at position 0
  e->prompt_len[b] = -1;
  e->slot_first[b] = e->frames_run;
}

// One row of the table, by value: ordered on the engine stream behind the frames already enqueued
__global__ void slot_sampling_set_kernel(SlotSampling* table, int b, SlotSampling row) {
  if (threadIdx.x == 0) table[b] = row;
}

// The whole table from the host's view of it: the rows of the slots with an override, the batch's for the rest
void upload_slot_sampling(csm_engine* e) {
  std::vector<SlotSampling> rows(e->B);
  for (int b = 0; b < e->B; ++b) rows[b] = e->samp_own[b] ? e->samp_host[b] : e->batch;
  HIPCHK(hipMemcpyAsync(e->slot_sampling, rows.data(), rows.size() * sizeof(SlotSampling), hipMemcpyHostToDevice, e->st));
  HIPCHK(hipStreamSynchronize(e->st));  // (the host rows are released on return)
}

// csm_sampling -> a table row.  A greedy utterance has no filter chain, whatever top_p and min_p say (the
// batch's csm_set_sampler_filters keeps them: frame_plan ignores the filters of a greedy record).
SlotSampling checked_row(csm_engine* e, const csm_sampling& s) {
  SlotSampling r{};
  sampling_set_sampler(r, s.temperature, s.top_k);
  sampling_set_filters(r, s.top_p, s.min_p, s.min_tokens_to_keep);
  sampling_set_processors(e, r, 2, s.n_bias, s.bias_idx, s.bias_val, s.repetition_penalty, s.repetition_context_size);
  if (!(r.temperature > 0.f)) {
    r.use_top_p = r.use_min_p = 0;
    r.log_min_p = 0.f;
  }
  return r;
}

}  // namespace

void sampling_set_sampler(SlotSampling& r, float temperature, int top_k) {
  if (!(temperature >= 0.f)) throw CsmError(CSM_ERR_ARG, "temperature must be >= 0");  // (refuses NaN too)
  r.temperature = temperature;
  r.top_k = top_k;
}

void sampling_set_filters(SlotSampling& r, double top_p, double min_p, int min_tokens_to_keep) {
  if (!(top_p >= 0.0 && top_p <= 1.0) || !(min_p >= 0.0 && min_p <= 1.0) || min_tokens_to_keep < 1)
    throw CsmError(CSM_ERR_ARG, "top_p and min_p must lie in [0, 1], min_tokens_to_keep >= 1");
  // mlx_lm make_sampler: top_p active in (0, 1), min_p when != 0; the cuts are the float32 values
  // its comparisons use: 1 - top_p and log(min_p) evaluated in double, then rounded
  r.use_top_p = top_p > 0.0 && top_p < 1.0;
  r.use_min_p = min_p != 0.0;
  r.top_p_cut = (float)(1.0 - top_p);
  r.log_min_p = r.use_min_p ? (float)std::log(min_p) : 0.f;
  r.min_keep = min_tokens_to_keep;
}

void sampling_set_processors(const csm_engine* e, SlotSampling& r, int bias_mode, int n_bias, const int32_t* bias_idx,
                             const float* bias_val, float repetition_penalty, int repetition_context_size) {
  if (n_bias < 0 || (n_bias > 0 && (!bias_idx || !bias_val))) throw CsmError(CSM_ERR_ARG, "bad logit_bias arguments");
  for (int i = 0; i < n_bias; ++i)
    if (bias_idx[i] < 0 || bias_idx[i] >= e->V)
      throw CsmError(CSM_ERR_ARG, "logit_bias index " + std::to_string(bias_idx[i]) + " outside [0, " + std::to_string(e->V) + ")");
  if (!(repetition_penalty >= 0.f)) throw CsmError(CSM_ERR_ARG, "repetition_penalty must be >= 0");
  if (repetition_context_size < 0 || repetition_context_size > C0_WINDOW_MAX)
    throw CsmError(CSM_ERR_ARG, "repetition_context_size must lie in [0, " + std::to_string(C0_WINDOW_MAX) + "]");
  r.penalty = repetition_penalty;
  r.context = repetition_penalty > 0.f ? repetition_context_size : 0;
  r.bias = n_bias > 0 ? bias_mode : 0;
}

void upload_dense_bias(csm_engine* e, float* dst, int n_bias, const int32_t* bias_idx, const float* bias_val) {
  if (n_bias <= 0) return;
  std::vector<float> dense(e->Vpad, 0.f);
  for (int i = 0; i < n_bias; ++i) dense[bias_idx[i]] = bias_val[i];
  HIPCHK(hipMemcpyAsync(dst, dense.data(), dense.size() * 4, hipMemcpyHostToDevice, e->st));
  HIPCHK(hipStreamSynchronize(e->st));  // (the host vector is released on return)
}

void refresh_slot_sampling(csm_engine* e) {
  if (!e->per_slot) return;
  HIPCHK(hipSetDevice(e->dev));
  upload_slot_sampling(e);
}

extern "C" {

int csm_slot_restart(csm_engine* e, int b, uint64_t seed) {
  CSM_TRY { slot_reset(e, b, seed, false); }
  CSM_CATCH
}

int csm_slot_release(csm_engine* e, int b) {
  CSM_TRY { slot_reset(e, b, 0, true); }
  CSM_CATCH
}

int csm_slot_set_sampling(csm_engine* e, int b, const csm_sampling* s) {
  CSM_TRY {
    if (!e) throw CsmError(CSM_ERR_ARG, "null engine");
    if (e->B <= 0 || !e->slot_mode) throw CsmError(CSM_ERR_STATE, "csm_slot_set_sampling outside slot mode: csm_slot_restart first");
    if (b < 0) throw CsmError(CSM_ERR_ARG, "slot index out of range");
    if (b >= e->B) throw CsmError(CSM_ERR_STATE, "slot " + std::to_string(b) + " beyond the batch of " + std::to_string(e->B));
    if (e->c0_pending) throw CsmError(CSM_ERR_STATE, "csm_frame_finish pending");
    if (e->parked_host[b]) throw CsmError(CSM_ERR_STATE, "slot " + std::to_string(b) + " holds no utterance: csm_slot_restart first");
    if (e->frames_run > e->slot_first[b])
      throw CsmError(CSM_ERR_STATE, "slot " + std::to_string(b) + ": its utterance has already run a frame");
    const SlotSampling row = s ? checked_row(e, *s) : e->batch;
    HIPCHK(hipSetDevice(e->dev));
    if (s) upload_dense_bias(e, e->slot_bias + (size_t)b * e->Vpad, s->n_bias, s->bias_idx, s->bias_val);  // the slot's own row
    e->samp_own[b] = s ? 1 : 0;
    e->samp_host[b] = row;
    if (s && !e->per_slot) {  // the first override of this batch: every slot's row, the batch's for the others
      e->per_slot = true;
      upload_slot_sampling(e);
    } else if (e->per_slot) {
      hipLaunchKernelGGL(slot_sampling_set_kernel, dim3(1), dim3(64), 0, e->st, e->slot_sampling, b, row);
      HIPCHK(hipGetLastError());
    }
  }
  CSM_CATCH
}

int csm_slot_read(csm_engine* e, int b, int32_t* codes, int cap_frames, int* n_frames, uint8_t* done) {
  CSM_TRY {
    if (!e) throw CsmError(CSM_ERR_ARG, "null engine");
    if (b < 0) throw CsmError(CSM_ERR_ARG, "slot index out of range");
    if (b >= e->B) throw CsmError(CSM_ERR_STATE, "slot " + std::to_string(b) + " beyond the batch of " + std::to_string(e->B));
    if (codes && cap_frames < 0) throw CsmError(CSM_ERR_ARG, "negative frame capacity");
    HIPCHK(hipSetDevice(e->dev));
    HIPCHK(hipStreamSynchronize(e->st));
    check_handoffs(e);
    int n = 0;
    uint8_t d = 0;
    HIPCHK(hipMemcpy(&n, e->n_frames + b, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&d, e->done + b, 1, hipMemcpyDeviceToHost));
    if (codes) {
      const int first = e->slot_first[b];
      if (n < 0 || n > e->frames_run - first || e->frames_run - first > e->F_cap)
        throw CsmError(CSM_ERR_STATE, "slot " + std::to_string(b) + ": its frames are no longer in the history");
      if (n > cap_frames) throw CsmError(CSM_ERR_ARG, "csm_slot_read: " + std::to_string(n) + " frames do not fit the buffer");
      const size_t K = e->K, pitch = (size_t)e->B * K * 4;
      for (int i = 0; i < n;) {  // at most two runs of consecutive ring rows
        const int row = (first + i) % e->F_cap, run = std::min(n - i, e->F_cap - row);
        HIPCHK(hipMemcpy2D(codes + (size_t)i * K, K * 4, e->hist + ((size_t)row * e->B + b) * K, pitch, K * 4, run,
                           hipMemcpyDeviceToHost));
        i += run;
      }
    }
    if (n_frames) *n_frames = n;
    if (done) *done = d;
  }
  CSM_CATCH
}

}  // extern "C"
