// CSM engine, frame ABI: csm_begin, prompt prefill and the calls that run frames and read their codes.
#include "csm_engine.h"

namespace {

// The checks every call that starts a frame makes (each caller keeps its own order among its other checks)
void require_prefilled(csm_engine* e) {  // (a parked slot has no prompt and needs none)
  for (int b = 0; b < e->B; ++b)
    if (e->prompt_len[b] < 0 && !e->parked_host[b]) throw CsmError(CSM_ERR_STATE, "csm_prefill not called for every utterance");
}
void require_window(csm_engine* e, int nframes) {
  int maxpos = 0;
  for (int b = 0; b < e->B; ++b)
    if (!e->parked_host[b]) maxpos = std::max(maxpos, e->pos_host[b]);
  if (maxpos + nframes + (e->need_body ? 1 : 0) > e->dims.max_seq_len)
    throw CsmError(CSM_ERR_TOO_LONG, "frames exceed the 2048-position window");
}

// Slot mode: no utterance may run past the F_cap frames of history that csm_slot_read can still reach
void require_ring(csm_engine* e, int nframes) {
  for (int b = 0; b < e->B; ++b)
    if (!e->parked_host[b] && e->frames_run + nframes - e->slot_first[b] > e->F_cap)
      throw CsmError(CSM_ERR_STATE, "slot " + std::to_string(b) + ": an utterance longer than the " + std::to_string(e->F_cap) +
                                        "-frame history (csm_engine_create's max_frames)");
}

// Waits for the stream; 1 when every utterance of the batch has reached EOS
int wait_all_done(csm_engine* e) {
  std::vector<uint8_t> d(e->B);
  HIPCHK(hipMemcpyAsync(d.data(), e->done, e->B, hipMemcpyDeviceToHost, e->st));
  HIPCHK(hipStreamSynchronize(e->st));
  int all = 1;
  for (auto v : d) all &= (v != 0);
  return all;
}

}  // namespace

// The backbone row of the previous frame's codes, when one is due: the captured graph or eager launches
// (a parked slot's position stays where the device keeps it: 0)
void body_if_needed(csm_engine* e, bool graph) {
  if (!e->need_body) return;
  if (graph) HIPCHK(hipGraphLaunch(e->g_body, e->st));
  else enqueue_body(e, e->st);
  for (int b = 0; b < e->B; ++b)
    if (!e->parked_host[b]) e->pos_host[b] += 1;
}

extern "C" {

int csm_begin(csm_engine* e, int B, const uint64_t* seeds, float temperature, int top_k) {
  CSM_TRY {
    e->c0_pending = false;
    if (e->ahead_pending) {  // the last chunk's pinned copies land before the slots are reused
      HIPCHK(hipStreamSynchronize(e->st));
      e->ahead_pending = false;
    }
    if (B <= 0) throw CsmError(CSM_ERR_ARG, "batch size out of range");
    SlotSampling batch{};  // the sampler given here, no filter chain, no c0 processors
    batch.min_keep = 1;
    sampling_set_sampler(batch, temperature, top_k);
    HIPCHK(hipSetDevice(e->dev));
    ensure_batch(e, B);
    if (e->tiled_dirty) build_tiled(e);
    if (e->proj_tab_dirty) build_proj_table(e);
    e->batch_epoch = e->weights_epoch;
    e->pos_host.assign(B, -1);
    e->B = B;
    e->batch = batch;
    ++e->filters_id;
    e->frames_run = 0;
    e->need_body = false;
    e->prompt_len.assign(B, -1);
    e->slot_mode = false;
    e->parked_host.assign(B, 0);
    e->slot_first.assign(B, 0);
    e->per_slot = false;
    e->samp_own.assign(B, 0);
    e->samp_host.assign(B, SlotSampling{});
    std::vector<uint64_t> s(B, 0);
    if (seeds) memcpy(s.data(), seeds, B * 8);
    HIPCHK(hipMemcpyAsync(e->seeds, s.data(), B * 8, hipMemcpyHostToDevice, e->st));
    HIPCHK(hipMemsetAsync(e->done, 0, B, e->st));
    HIPCHK(hipMemsetAsync(e->n_frames, 0, B * 4, e->st));
    HIPCHK(hipMemsetAsync(e->slot_frame, 0, B * 4, e->st));
    HIPCHK(hipMemsetAsync(e->parked, 0, B, e->st));
    HIPCHK(hipMemsetAsync(e->frame_ctr, 0, 16, e->st));
    HIPCHK(hipMemsetAsync(e->codes, 0, (size_t)B * e->K * 4, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
  }
  CSM_CATCH
}

int csm_set_sampler_filters(csm_engine* e, double top_p, double min_p, int min_tokens_to_keep) {
  CSM_TRY {
    if (!e) throw CsmError(CSM_ERR_ARG, "null engine");
    if (e->frames_run > 0 || e->c0_pending) throw CsmError(CSM_ERR_STATE, "set the sampler filters before the first frame");
    sampling_set_filters(e->batch, top_p, min_p, min_tokens_to_keep);
    ++e->filters_id;
    refresh_slot_sampling(e);
  }
  CSM_CATCH
}

int csm_set_c0_processors(csm_engine* e, int n_bias, const int32_t* bias_idx, const float* bias_val, float repetition_penalty,
                          int repetition_context_size) {
  CSM_TRY {
    if (!e) throw CsmError(CSM_ERR_ARG, "null engine");
    if (e->frames_run > 0 || e->c0_pending) throw CsmError(CSM_ERR_STATE, "set the c0 processors before the first frame");
    SlotSampling batch = e->batch;
    sampling_set_processors(e, batch, 1, n_bias, bias_idx, bias_val, repetition_penalty, repetition_context_size);
    HIPCHK(hipSetDevice(e->dev));
    if (n_bias > 0 && !e->c0_bias) e->c0_bias = (float*)e->alloc((size_t)e->Vpad * 4);
    upload_dense_bias(e, e->c0_bias, n_bias, bias_idx, bias_val);
    e->batch = batch;
    ++e->filters_id;  // the frame graphs hold these by value: re-capture
    refresh_slot_sampling(e);
  }
  CSM_CATCH
}

int csm_prefill(csm_engine* e, int b, int T, const int32_t* tokens, const uint8_t* mask) {
  CSM_TRY {
    if (b < 0 || b >= e->B) throw CsmError(CSM_ERR_ARG, "utterance index out of range");
    if (T <= 0) throw CsmError(CSM_ERR_ARG, "prompt length out of range");
    const int start = e->pos_host[b] + 1;  // rows append after what the backbone already holds
    if (start + T > e->dims.max_seq_len)  // (before the staging cap: M_cap >= max_seq_len, so a prompt one row over is this)
      throw CsmError(CSM_ERR_TOO_LONG, "rows exceed the 2048-position window");
    if (T > e->M_cap) throw CsmError(CSM_ERR_ARG, "prompt length out of range");
    HIPCHK(hipSetDevice(e->dev));
    const int K = e->K;
    HIPCHK(hipMemcpyAsync(e->tok, tokens, (size_t)T * (K + 1) * 4, hipMemcpyHostToDevice, e->st));
    HIPCHK(hipMemcpyAsync(e->msk, mask, (size_t)T * (K + 1), hipMemcpyHostToDevice, e->st));
    EmbedParams ep{};
    ep.tok = e->tok; ep.mask = e->msk; ep.text_emb = e->text_emb; ep.audio_emb = e->audio_emb; ep.V = e->V;
    ep.K = K; ep.D = e->D; ep.out = e->x;
    embed(e, ep, T, e->st);
    RowMap rm{T, b, nullptr, start};
    if (e->attn_tiles_on && T >= 16) {  // attention tiles: <= 64 consecutive rows (launch_attn's >= 16-row bar)
      // staged in pinned memory: the copy stays asynchronous (this call's closing synchronize is what
      // makes the staging reusable by the next csm_prefill; not so when this call throws first: ADVICE.md)
      const int nt = (T + 63) / 64;
      if (!e->ptiles_pin) HIPCHK(hipHostMalloc((void**)&e->ptiles_pin, (e->M_cap / 64 + 1) * sizeof(int2), hipHostMallocDefault));
      for (int t = 0; t < nt; ++t) e->ptiles_pin[t] = make_int2(64 * t, std::min(64, T - 64 * t));
      HIPCHK(hipMemcpyAsync(e->ptiles, e->ptiles_pin, nt * sizeof(int2), hipMemcpyHostToDevice, e->st));
      rm.tiles = e->ptiles;
      rm.ntiles = nt;
    }
    run_stack(e, e->bb, e->x, T, e->q, e->att, e->mlp, rm, e->st);
    launch_rmsnorm_rows(e->x + (size_t)(T - 1) * e->D, e->D, e->bb.norm, e->bb.d.eps, e->D,
                        e->h_last + (size_t)b * e->D, e->D, 1, e->st);
    e->pos_host[b] = start + T - 1;  // position of the last processed backbone row
    HIPCHK(hipMemcpyAsync(e->pos + b, &e->pos_host[b], 4, hipMemcpyHostToDevice, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    HIPCHK(hipGetLastError());
    e->prompt_len[b] = std::max(e->prompt_len[b], 0) + T;
    e->need_body = false;
  }
  CSM_CATCH
}

int csm_prefill_batch(csm_engine* e, int n, const int32_t* utts, const int32_t* Ts, const int32_t* tokens,
                      const uint8_t* masks) {
  CSM_TRY {
    if (n <= 0 || !utts || !Ts || !tokens || !masks) throw CsmError(CSM_ERR_ARG, "bad csm_prefill_batch arguments");
    const int K = e->K;
    std::vector<int> start(n);
    std::vector<size_t> row0(n + 1, 0);
    std::vector<char> seen(e->B, 0);
    for (int i = 0; i < n; ++i) {
      const int b = utts[i], T = Ts[i];
      if (b < 0 || b >= e->B || seen[b]) throw CsmError(CSM_ERR_ARG, "utterance index out of range or repeated");
      seen[b] = 1;
      if (T <= 0) throw CsmError(CSM_ERR_ARG, "prompt length out of range");
      start[i] = e->pos_host[b] + 1;
      if (start[i] + T > e->dims.max_seq_len) throw CsmError(CSM_ERR_TOO_LONG, "rows exceed the 2048-position window");
      if (T > e->M_cap) throw CsmError(CSM_ERR_ARG, "prompt length out of range");
      row0[i + 1] = row0[i] + T;
    }
    HIPCHK(hipSetDevice(e->dev));
    const size_t cap = e->prefill_rows > 0 ? std::min(e->prefill_rows, e->M_cap) : e->M_cap;
    // utterances in groups of at most M_cap rows: one pass of every projection per group (the
    // weights stream once for all of the group's rows), rows mapped to (utterance, position)
    std::vector<int> rb, rp;
    std::vector<int2> tl;
    for (int i0 = 0; i0 < n;) {
      int i1 = i0;
      while (i1 < n && row0[i1 + 1] - row0[i0] <= cap) ++i1;
      if (i1 == i0) i1 = i0 + 1;  // one utterance longer than a lowered cap: a group of its own (T <= M_cap)
      const int R = (int)(row0[i1] - row0[i0]);
      rb.assign(R, 0);
      rp.assign(R, 0);
      for (int i = i0; i < i1; ++i)
        for (int t = 0; t < Ts[i]; ++t) {
          rb[row0[i] - row0[i0] + t] = utts[i];
          rp[row0[i] - row0[i0] + t] = start[i] + t;
        }
      HIPCHK(hipMemcpyAsync(e->tok, tokens + row0[i0] * (K + 1), (size_t)R * (K + 1) * 4, hipMemcpyHostToDevice, e->st));
      HIPCHK(hipMemcpyAsync(e->msk, masks + row0[i0] * (K + 1), (size_t)R * (K + 1), hipMemcpyHostToDevice, e->st));
      HIPCHK(hipMemcpyAsync(e->row_b, rb.data(), (size_t)R * 4, hipMemcpyHostToDevice, e->st));
      HIPCHK(hipMemcpyAsync(e->row_pos, rp.data(), (size_t)R * 4, hipMemcpyHostToDevice, e->st));
      tl.clear();  // attention tiles: <= 64 consecutive rows of one utterance
      for (int i = i0; i < i1; ++i)
        for (int t0 = 0; t0 < Ts[i]; t0 += 64) tl.push_back(make_int2((int)(row0[i] - row0[i0]) + t0, std::min(64, Ts[i] - t0)));
      HIPCHK(hipMemcpyAsync(e->ptiles, tl.data(), tl.size() * sizeof(int2), hipMemcpyHostToDevice, e->st));
      EmbedParams ep{};
      ep.tok = e->tok; ep.mask = e->msk; ep.text_emb = e->text_emb; ep.audio_emb = e->audio_emb; ep.V = e->V;
      ep.K = K; ep.D = e->D; ep.out = e->x;
      embed(e, ep, R, e->st);
      RowMap rm{1, 0, nullptr, 0};
      rm.row_b = e->row_b;
      rm.row_pos = e->row_pos;
      if (e->attn_tiles_on) {
        rm.tiles = e->ptiles;
        rm.ntiles = (int)tl.size();
      }
      run_stack(e, e->bb, e->x, R, e->q, e->att, e->mlp, rm, e->st);
      for (int i = i0; i < i1; ++i) {  // h_last = norm(last row) of each utterance
        const size_t last = row0[i + 1] - 1 - row0[i0];
        launch_rmsnorm_rows(e->x + last * e->D, e->D, e->bb.norm, e->bb.d.eps, e->D, e->h_last + (size_t)utts[i] * e->D,
                            e->D, 1, e->st);
      }
      HIPCHK(hipStreamSynchronize(e->st));  // the host row tables are reused by the next group
      HIPCHK(hipGetLastError());
      i0 = i1;
    }
    for (int i = 0; i < n; ++i) {
      const int b = utts[i];
      e->pos_host[b] = start[i] + Ts[i] - 1;
      HIPCHK(hipMemcpyAsync(e->pos + b, &e->pos_host[b], 4, hipMemcpyHostToDevice, e->st));
      e->prompt_len[b] = std::max(e->prompt_len[b], 0) + Ts[i];
    }
    HIPCHK(hipStreamSynchronize(e->st));
    e->need_body = false;
  }
  CSM_CATCH
}

int csm_run_frames(csm_engine* e, int nframes, int* all_done) {
  CSM_TRY {
    if (e->c0_pending) throw CsmError(CSM_ERR_STATE, "csm_frame_finish pending");
    require_prefilled(e);
    HIPCHK(hipSetDevice(e->dev));
    // the history is [F_cap] frames: a plain batch stops there; in slot mode it is a ring and only each
    // utterance's own length is bounded by it
    if (e->slot_mode) require_ring(e, nframes);
    else if (e->frames_run + nframes > e->F_cap) nframes = e->F_cap - e->frames_run;
    require_window(e, nframes);
    if (nframes <= 0) { if (all_done) *all_done = 0; return CSM_OK; }
    // CSM_GRAPH=0: eager launches of the same kernels (rocprofv3 kernel tracing of graph
    // replays crashes on ROCm 7.2, so profiling runs use this mode).
    static const bool use_graph = env_on("CSM_GRAPH");
    if (!use_graph) {
      for (int f = 0; f < nframes; ++f) {
        body_if_needed(e);
        enqueue_head(e, e->st);
        e->need_body = true;
        e->frames_run++;
      }
      HIPCHK(hipGetLastError());
      nframes = 0;
    }
    // The graphs hold the batch's record by value: every call that writes it (csm_begin, csm_set_*) counts
    // filters_id up.  (Per-slot sampling: the slots' values are read from device memory, so a join captures
    // nothing; a change of the plan class does.)
    const int plan = frame_plan(e).key();
    if (use_graph && (e->g_B != e->B || e->g_filters != e->filters_id || e->g_plan != plan || !e->g_head)) {
      if (e->frames_run > 0) HIPCHK(hipStreamSynchronize(e->st));  // frames enqueued without a wait still replay the old graphs
      if (e->g_body) (void)hipGraphExecDestroy(e->g_body);
      if (e->g_head) (void)hipGraphExecDestroy(e->g_head);
      e->g_body = capture(e, enqueue_body);
      e->g_head = capture(e, enqueue_head);
      e->g_B = e->B;
      e->g_filters = e->filters_id;
      e->g_plan = plan;
    }
    for (int f = 0; f < nframes; ++f) {
      body_if_needed(e, true);
      HIPCHK(hipGraphLaunch(e->g_head, e->st));
      e->need_body = true;
      e->frames_run++;
    }
    if (all_done) {
      const int all = wait_all_done(e);
      check_handoffs(e);
      *all_done = all;
    }
  }
  CSM_CATCH
}

int csm_run_frames_ahead(csm_engine* e, int nframes, int* prev_all_done) {
  if (!e || !prev_all_done) { csm_set_error("null engine or result pointer"); return CSM_ERR_ARG; }
  const int rc = csm_run_frames(e, nframes, nullptr);  // enqueued, no wait
  if (rc != CSM_OK) return rc;
  CSM_TRY {
    if (!e->ahead_pin) {
      HIPCHK(hipHostMalloc((void**)&e->ahead_pin, 2 * e->ahead_bytes(), hipHostMallocDefault));
      for (hipEvent_t& ev : e->ahead_ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    const int s = e->ahead_slot;
    uint8_t* pin = e->ahead_pin + s * e->ahead_bytes();
    int* perr = reinterpret_cast<int*>(pin + e->ahead_bytes() - 8);
    perr[0] = perr[1] = 0;  // (slot s was last read two chunks ago, after its event)
    HIPCHK(hipMemcpyAsync(pin, e->done, e->B, hipMemcpyDeviceToHost, e->st));
    // (the persistent batched decoder step's flag is not polled here: ADVICE.md, the csm_run_frames_ahead item)
    if (e->h_df.err) HIPCHK(hipMemcpyAsync(perr, e->h_df.err, 4, hipMemcpyDeviceToHost, e->st));
    if (e->h_bb.err) HIPCHK(hipMemcpyAsync(perr + 1, e->h_bb.err, 4, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipEventRecord(e->ahead_ev[s], e->st));
    int res = -1;
    if (e->ahead_pending) {
      const int q = s ^ 1;
      HIPCHK(hipEventSynchronize(e->ahead_ev[q]));
      const uint8_t* pq = e->ahead_pin + q * e->ahead_bytes();
      const int* qerr = reinterpret_cast<const int*>(pq + e->ahead_bytes() - 8);
      if (qerr[0] || qerr[1]) {
        // the chunk just enqueued has written slot s behind its event: drain the stream and forget both
        // slots, so a later call (with or without csm_begin) never polls a stale done state
        HIPCHK(hipStreamSynchronize(e->st));
        e->ahead_pending = false;
        e->ahead_slot = 0;
        check_handoffs(e);  // resets the device flags and raises
      }
      res = 1;
      for (int b = 0; b < e->B; ++b) res &= pq[b] != 0;
    }
    e->ahead_slot = s ^ 1;
    e->ahead_pending = true;
    *prev_all_done = res;
  }
  CSM_CATCH
}

int csm_frame_step(csm_engine* e, int32_t* out_codes, uint8_t* done) {
  if (!e) { csm_set_error("null engine"); return CSM_ERR_ARG; }
  if (!e->slot_mode && e->frames_run >= e->F_cap) { csm_set_error("frame capacity reached"); return CSM_ERR_STATE; }
  const int rc = csm_run_frames(e, 1, nullptr);
  if (rc != CSM_OK) return rc;
  CSM_TRY {
    if (out_codes)
      HIPCHK(hipMemcpyAsync(out_codes, e->codes, (size_t)e->B * e->K * 4, hipMemcpyDeviceToHost, e->st));
    if (done) HIPCHK(hipMemcpyAsync(done, e->done, e->B, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    check_handoffs(e);
  }
  CSM_CATCH
}

// One frame in two halves around a host hook on the c0 logits (generation.py:42-49): eager launches
// of the same kernels the frame graph holds.
int csm_frame_c0_logits(csm_engine* e, float* logits) {
  CSM_TRY {
    require_prefilled(e);
    if (e->slot_mode) throw CsmError(CSM_ERR_STATE, "host-paused frames are not available in slot mode");
    if (e->c0_pending) throw CsmError(CSM_ERR_STATE, "csm_frame_c0_logits called again before csm_frame_finish");
    if (!logits) throw CsmError(CSM_ERR_ARG, "null logits buffer");
    HIPCHK(hipSetDevice(e->dev));
    if (e->frames_run + 1 > e->F_cap) throw CsmError(CSM_ERR_STATE, "frame capacity reached");
    require_window(e, 1);
    body_if_needed(e);
    e->need_body = false;
    enqueue_head_phase(e, e->st, HeadPhase::C0Logits);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy2DAsync(logits, (size_t)e->V * 4, e->c0_logits, (size_t)e->Vpad * 4, (size_t)e->V * 4, e->B,
                            hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    check_handoffs(e);  // the backbone row may have run on the persistent step
    e->c0_pending = true;
    e->host_piece = 1;
  }
  CSM_CATCH
}

int csm_frame_finish(csm_engine* e, const float* logits, int* all_done) {
  CSM_TRY {
    if (!e->c0_pending) throw CsmError(CSM_ERR_STATE, "csm_frame_finish without csm_frame_c0_logits");
    if (!logits) throw CsmError(CSM_ERR_ARG, "null logits buffer");
    HIPCHK(hipSetDevice(e->dev));
    HIPCHK(hipMemcpy2DAsync(e->c0_logits, (size_t)e->Vpad * 4, logits, (size_t)e->V * 4, (size_t)e->V * 4, e->B,
                            hipMemcpyHostToDevice, e->st));
    enqueue_head_phase(e, e->st, HeadPhase::FromHostC0);
    HIPCHK(hipGetLastError());
    e->c0_pending = false;
    e->need_body = true;
    e->frames_run++;
    if (all_done) {
      *all_done = wait_all_done(e);
    } else {
      HIPCHK(hipStreamSynchronize(e->st));  // the host logits buffer may be released on return
    }
    check_handoffs(e);
  }
  CSM_CATCH
}

int csm_frame_host_step(csm_engine* e, const int32_t* codes, float* logits, int* all_done) {
  CSM_TRY {
    if (!e->c0_pending) throw CsmError(CSM_ERR_STATE, "csm_frame_host_step without csm_frame_c0_logits");
    if (!codes) throw CsmError(CSM_ERR_ARG, "null codes");
    const int piece = e->host_piece;  // codes are those of codebook piece - 1
    if (piece < e->K && !logits) throw CsmError(CSM_ERR_ARG, "null logits buffer");
    for (int b = 0; b < e->B; ++b)
      if (codes[b] < 0 || codes[b] >= e->V) throw CsmError(CSM_ERR_ARG, "host-sampled code out of range");
    HIPCHK(hipSetDevice(e->dev));
    HIPCHK(hipMemcpy2DAsync(e->force + (piece - 1), (size_t)e->K * 4, codes, 4, 4, e->B, hipMemcpyHostToDevice, e->st));
    enqueue_head_phase(e, e->st, HeadPhase::HostPiece, piece);
    HIPCHK(hipGetLastError());
    if (piece < e->K) {
      HIPCHK(hipMemcpy2DAsync(logits, (size_t)e->V * 4, e->ci_logits + (size_t)(piece - 1) * e->B * e->Vpad,
                              (size_t)e->Vpad * 4, (size_t)e->V * 4, e->B, hipMemcpyDeviceToHost, e->st));
      HIPCHK(hipStreamSynchronize(e->st));
      e->host_piece = piece + 1;
      if (all_done) *all_done = 0;
    } else {
      e->c0_pending = false;
      e->host_piece = 1;
      e->need_body = true;
      e->frames_run++;
      const int all = wait_all_done(e);
      if (all_done) *all_done = all;
    }
    check_handoffs(e);
  }
  CSM_CATCH
}

int csm_frame_forced(csm_engine* e, const int32_t* codes, float* c0_logits, float* ci_logits, float* ce) {
  CSM_TRY {
    require_prefilled(e);
    if (e->slot_mode) throw CsmError(CSM_ERR_STATE, "teacher-forced frames are not available in slot mode");
    if (e->c0_pending) throw CsmError(CSM_ERR_STATE, "csm_frame_finish pending");
    if (!codes) throw CsmError(CSM_ERR_ARG, "null codes");
    HIPCHK(hipSetDevice(e->dev));
    if (e->frames_run + 1 > e->F_cap) throw CsmError(CSM_ERR_STATE, "frame capacity reached");
    require_window(e, 1);
    for (int i = 0; i < e->B * e->K; ++i)
      if (codes[i] < 0 || codes[i] >= e->V) throw CsmError(CSM_ERR_ARG, "forced code out of range");
    HIPCHK(hipMemcpyAsync(e->force, codes, (size_t)e->B * e->K * 4, hipMemcpyHostToDevice, e->st));
    body_if_needed(e);
    enqueue_head_phase(e, e->st, HeadPhase::Forced);
    if (ce) launch_forced_ce(e->c0_logits, e->ci_logits, e->force, e->force_ce, e->B, e->K, e->V, e->Vpad, e->st);
    HIPCHK(hipGetLastError());
    e->need_body = true;
    e->frames_run++;
    const size_t V = e->V, Vp = e->Vpad, B = e->B;
    if (c0_logits)
      HIPCHK(hipMemcpy2DAsync(c0_logits, V * 4, e->c0_logits, Vp * 4, V * 4, B, hipMemcpyDeviceToHost, e->st));
    if (ci_logits)
      HIPCHK(hipMemcpy2DAsync(ci_logits, V * 4, e->ci_logits, Vp * 4, V * 4, (size_t)(e->K - 1) * B,
                              hipMemcpyDeviceToHost, e->st));
    if (ce) HIPCHK(hipMemcpyAsync(ce, e->force_ce, B * e->K * 4, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    check_handoffs(e);  // the backbone row may have run on the persistent step
  }
  CSM_CATCH
}

int csm_read_codes(csm_engine* e, int32_t* hist, int32_t* n_frames, uint8_t* done, int* frames_run) {
  CSM_TRY {
    HIPCHK(hipSetDevice(e->dev));
    HIPCHK(hipStreamSynchronize(e->st));
    check_handoffs(e);
    if (hist && e->slot_mode)
      throw CsmError(CSM_ERR_STATE, "the history is a ring in slot mode: read a slot's codes with csm_slot_read");
    if (hist)
      HIPCHK(hipMemcpy(hist, e->hist, (size_t)e->frames_run * e->B * e->K * 4, hipMemcpyDeviceToHost));
    if (n_frames) HIPCHK(hipMemcpy(n_frames, e->n_frames, e->B * 4, hipMemcpyDeviceToHost));
    if (done) HIPCHK(hipMemcpy(done, e->done, e->B, hipMemcpyDeviceToHost));
    if (frames_run) *frames_run = e->frames_run;
  }
  CSM_CATCH
}

int csm_codes_device_ptr(csm_engine* e, void** p) {
  CSM_TRY { *p = e->hist; }
  CSM_CATCH
}

int csm_synchronize(csm_engine* e) {
  CSM_TRY {
    HIPCHK(hipSetDevice(e->dev));
    HIPCHK(hipStreamSynchronize(e->st));
    check_handoffs(e);
    HIPCHK(hipGetLastError());
  }
  CSM_CATCH
}

}  // extern "C"
