// CSM engine, lab and inspection: debug taps, row / Linear probes, the microbenchmarks and the option
// switchboard.
#include "csm_engine.h"

namespace {

// The microbenchmarks' timing loop: `warm` warm-up launches, then `iters` timed ones between two events.
// launch(i) enqueues the i-th launch on st; returns the average microseconds per timed launch.
template <class Launch, class AfterWarm>
float time_launches(hipStream_t st, int warm, int iters, Launch&& launch, AfterWarm&& after_warm) {
  for (int i = 0; i < warm; ++i) launch(i);
  hipEvent_t a, b;
  HIPCHK(hipEventCreate(&a));
  HIPCHK(hipEventCreate(&b));
  after_warm();
  HIPCHK(hipEventRecord(a, st));
  for (int i = 0; i < iters; ++i) launch(i);
  HIPCHK(hipEventRecord(b, st));
  HIPCHK(hipEventSynchronize(b));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return ms * 1000.f / iters;
}
template <class Launch>
float time_launches(hipStream_t st, int warm, int iters, Launch&& launch) {
  return time_launches(st, warm, iters, launch, [] {});
}

}  // namespace

extern "C" {

int csm_debug_read(csm_engine* e, const char* what, void* host, int64_t nbytes, int64_t* needed) {
  CSM_TRY {
    HIPCHK(hipSetDevice(e->dev));
    HIPCHK(hipStreamSynchronize(e->st));
    const std::string w(what);
    const void* src = nullptr;
    size_t n = 0;
    const size_t B = e->B, Vp = e->Vpad;
    if (w == "h_last") { src = e->h_last; n = B * e->D * 4; }
    else if (w == "c0_logits") { src = e->c0_logits; n = B * Vp * 4; }
    else if (w == "ci_logits") { src = e->ci_logits; n = (e->K - 1) * B * Vp * 4; }
    else if (w == "codes") { src = e->codes; n = B * e->K * 4; }
    else if (w == "pos") { src = e->pos; n = B * 4; }
    else if (w == "dec_frame_epoch") { src = e->h_df.epoch; n = 4; }
    else if (w == "dec_xsd_epoch") { src = e->h_xsd.epoch; n = 4; }
    else if (w == "dec_xsd_stamps" && e->h_xsd.stamps) { src = e->h_xsd.stamps; n = e->h_xsd.stamps_bytes; }
    else if (w == "bb_step_epoch" && e->h_bb.epoch) { src = e->h_bb.epoch; n = 4; }  // advances by 80 per row it ran
    else if (w == "bb_step_stamps" && e->h_bb.stamps) { src = e->h_bb.stamps; n = e->h_bb.stamps_bytes; }  // advances by the hand-offs of every frame it ran
    else if (w == "dec_frame_stamps" && e->h_df.stamps) { src = e->h_df.stamps; n = e->h_df.stamps_bytes; }
    else if (w == "audio_head") {  // device layout [K-1][Vpad][Dd], f32 or bf16 bits
      src = e->audio_head; n = (size_t)(e->K - 1) * Vp * e->Dd * (e->head_wdt == WDT_F32 ? 4 : 2);
    }
    else if (w.rfind("weight:", 0) == 0) {  // a whole stored matrix in its device layout (not fused ones)
      Place pl;
      if (!weight_place(e, w.substr(7), pl) || pl.n != pl.Ntot) throw CsmError(CSM_ERR_ARG, "no whole matrix " + w);
      src = pl.base;
      n = e->wbytes(pl.Ntot, pl.K);
    }
    else throw CsmError(CSM_ERR_ARG, "unknown debug tap " + w);
    if (needed) *needed = (int64_t)n;
    if (host) {
      if ((size_t)nbytes < n) throw CsmError(CSM_ERR_ARG, "debug buffer too small");
      HIPCHK(hipMemcpy(host, src, n, hipMemcpyDeviceToHost));
    }
  }
  CSM_CATCH
}

int csm_kv_read(csm_engine* e, int b, int layer, int first, int rows, float* k, float* v) {
  CSM_TRY {
    if (!e) throw CsmError(CSM_ERR_ARG, "null engine");
    const Stack& s = e->bb;
    if (b < 0 || b >= e->B || layer < 0 || layer >= s.d.n_layers || first < 0 || rows < 1 || first + rows > s.S_cap)
      throw CsmError(CSM_ERR_ARG, "csm_kv_read: utterance, layer or positions out of range");
    HIPCHK(hipSetDevice(e->dev));
    HIPCHK(hipStreamSynchronize(e->st));
    const size_t hd = s.d.head_dim, Hkv = s.d.n_kv_heads, run = (size_t)rows * hd * 4, pitch = (size_t)s.S_cap * hd * 4;
    const size_t off = ((size_t)b * Hkv * s.S_cap + first) * hd;
    if (k) HIPCHK(hipMemcpy2D(k, run, s.L[layer].kc + off, pitch, run, Hkv, hipMemcpyDeviceToHost));
    if (v) HIPCHK(hipMemcpy2D(v, run, s.L[layer].vc + off, pitch, run, Hkv, hipMemcpyDeviceToHost));
  }
  CSM_CATCH
}

int csm_read_rows(csm_engine* e, const char* name, int n, const int32_t* rows, float* out) {
  CSM_TRY {
    if (!name || n < 0 || (n > 0 && (!rows || !out))) throw CsmError(CSM_ERR_ARG, "bad csm_read_rows arguments");
    Place pl;
    if (!weight_place(e, name, pl)) throw CsmError(CSM_ERR_ARG, std::string("not a Linear / Embedding weight: ") + name);
    if (!e->loaded.count(name)) throw CsmError(CSM_ERR_STATE, std::string("weight not loaded: ") + name);
    std::vector<int> idx(n);
    for (int i = 0; i < n; ++i) {
      if (rows[i] < 0 || rows[i] >= pl.n) throw CsmError(CSM_ERR_ARG, "row index out of range");
      idx[i] = pl.row0 + rows[i] * pl.rstep;
    }
    if (n == 0) return CSM_OK;
    HIPCHK(hipSetDevice(e->dev));
    DevBuf di((size_t)n * 4), dout((size_t)n * pl.K * 4);
    HIPCHK(hipMemcpyAsync(di.p, idx.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->st));
    launch_table_rows(pl.base, e->wdt, pl.Ntot, pl.K, (const int*)di.p, n, (float*)dout.p, e->st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)n * pl.K * 4, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
  }
  CSM_CATCH
}

int csm_linear(csm_engine* e, const char* name, int M, const float* x, float* y) {
  CSM_TRY {
    if (!name || M <= 0 || !x || !y) throw CsmError(CSM_ERR_ARG, "bad csm_linear arguments");
    const std::string nm(name);
    const void* W = nullptr;
    int wdt = e->wdt, N = 0, K = 0, row0 = 0, rstep = 1, n_out = 0;
    if (nm.rfind("audio_head.", 0) == 0) {  // audio_head[i] (in, out): x @ audio_head[i] (generation.py:79)
      char* end = nullptr;
      const long i = strtol(nm.c_str() + 11, &end, 10);
      if (!end || *end || i < 0 || i >= e->K - 1) throw CsmError(CSM_ERR_ARG, "audio_head index out of range");
      if (!e->loaded.count("audio_head")) throw CsmError(CSM_ERR_STATE, "weight not loaded: audio_head");
      wdt = e->head_wdt;
      W = (const char*)e->audio_head + (size_t)i * e->Vpad * e->Dd * (wdt == WDT_F32 ? 4 : 2);
      N = e->Vpad; K = e->Dd; n_out = e->V;
    } else {
      Place pl;
      if (!weight_place(e, nm, pl) || nm.find("embeddings") != std::string::npos)
        throw CsmError(CSM_ERR_ARG, "not a Linear weight: " + nm);
      if (!e->loaded.count(nm)) throw CsmError(CSM_ERR_STATE, "weight not loaded: " + nm);
      W = pl.base; N = pl.Ntot; K = pl.K; row0 = pl.row0; rstep = pl.rstep; n_out = pl.n;
    }
    HIPCHK(hipSetDevice(e->dev));
    DevBuf dx((size_t)M * K * 4), dy((size_t)M * N * 4);
    HIPCHK(hipMemcpyAsync(dx.p, x, (size_t)M * K * 4, hipMemcpyHostToDevice, e->st));
    GemvParams g = gp(e);
    g.W = W; g.N = N; g.K = K; g.x = (const float*)dx.p; g.xs = K; g.M = M; g.out = (float*)dy.p; g.os = N;
    // default: the GEMV's fp32 arithmetic at any row count; option "linear_mfma": the batched
    // frame's MFMA GEMM where eligible (its split-K scratch reserved here: captured graphs re-capture)
    g.no_mfma = !(e->linear_mfma && gemm_mfma_eligible(N, K, M, wdt));
    if (!g.no_mfma) {
      if (e->tiled_dirty) build_tiled(e);
      if (gemm_reserve(e->ws, N, K, M)) e->g_B = -1;
    }
    launch_gemv(g, wdt, EPI_STORE, 0, e->st, 2);
    HIPCHK(hipGetLastError());
    std::vector<float> full((size_t)M * N);
    HIPCHK(hipMemcpyAsync(full.data(), dy.p, full.size() * 4, hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    for (int m = 0; m < M; ++m)
      for (int j = 0; j < n_out; ++j) y[(size_t)m * n_out + j] = full[(size_t)m * N + row0 + (size_t)j * rstep];
  }
  CSM_CATCH
}

int csm_bench_gemv(csm_engine* e, int which, int M, int iters, float* avg_us, double* bytes) {
  CSM_TRY {
    if (M <= 0 || M > 2 * e->B_max || iters <= 0) throw CsmError(CSM_ERR_ARG, "bad bench arguments");
    HIPCHK(hipSetDevice(e->dev));
    if (e->tiled_dirty) build_tiled(e);
    const int stack = (which & 7) / 4;
    Stack& s = stack == 0 ? e->bb : e->dec;
    const int tag = stack == 0 ? 0 : 1;
    float* x = stack == 0 ? e->x : e->dx;
    float* mlp = stack == 0 ? e->mlp : e->dmlp;
    const int D = s.d.hidden, F = s.d.intermediate;
    const int kind = which % 4;
    // one launch per layer in turn, as the frame does, so the weight working set (and hence
    // L2 / Infinity-Cache residency) matches the real frame: backbone 16 x 67 MB streams from
    // HBM, decoder 4 x 33.5 MB stays within the 256 MiB Infinity Cache.
    auto params = [&](int layer, int& epi, int& norm) {
      const LayerW& l = s.L[layer];
      GemvParams g = gp(e);
      if (kind == 0) {  // norm + gate/up + SiLU
        g.W = l.wgu; g.N = 2 * F; g.K = D; g.x = x; g.xs = D; g.M = M; g.nw = l.n2; g.eps = s.d.eps;
        g.out = mlp; g.os = F; epi = EPI_SILU_MUL; norm = 1;
      } else if (kind == 1) {  // down + residual
        g.W = l.wd; g.N = D; g.K = F; g.x = mlp; g.xs = F; g.M = M; g.out = x; g.os = D; epi = EPI_ADD; norm = 0;
      } else if (kind == 2) {  // norm + QKV + RoPE + KV append (position 0)
        g.W = l.wqkv; g.N = s.qkv_rows(); g.K = D; g.x = x; g.xs = D; g.M = M; g.nw = l.n1; g.eps = s.d.eps;
        g.out = stack == 0 ? e->q : e->dq; g.os = s.q_dim(); g.Hq = s.d.n_heads; g.Hkv = s.d.n_kv_heads;
        g.hd = s.d.head_dim; g.S_cap = s.S_cap; g.rope = s.rope; g.kc = l.kc; g.vc = l.vc; g.rm = RowMap{1, 0, nullptr, 0};
        epi = EPI_QKV; norm = 1;
      } else {  // o_proj + residual
        g.W = l.wo; g.N = D; g.K = s.q_dim(); g.x = stack == 0 ? e->att : e->datt; g.xs = s.q_dim(); g.M = M;
        g.out = x; g.os = D; epi = EPI_ADD; norm = 0;
      }
      return g;
    };
    // which & 8: the streaming matrix-core GEMM (gemm_xs) of the same projection at M rows, with the
    // decoder path's operands and producer outputs (split rows in, split rows + sums out; lab timing)
    const bool xsb = (which & 8) != 0;
    auto xs_params = [&](GemvParams g, int epi) {
      const int Dm = s.d.hidden;
      g.x = nullptr;
      g.xs_in = (epi == EPI_ADD && g.K == F) ? e->xs_F : (epi == EPI_ADD ? e->xs_A : e->xs_D);
      g.ss_in = e->xs_ss; g.ss_n = gemm_xs_tiles(Dm, F, M); g.ss_stride = GEMM_XS_MAX_M;
      const bool noprod = (which & 16) != 0;  // lab: without the producer outputs (their cost)
      if (epi == EPI_SILU_MUL) { g.out = noprod ? mlp : nullptr; if (!noprod) { g.xs_out = e->xs_F; g.xs_K = F; } }
      if (epi == EPI_ADD && !noprod) { g.xs_out = e->xs_D; g.xs_nw = s.L[0].n1; g.ss_out = e->xs_ss; g.xs_K = Dm; }
      if (e->wdt == WDT_Q4) { g.hs_in = e->hs_D; g.hs_out = (epi == EPI_SILU_MUL) ? e->hs_F : e->hs_A; }
      return g;
    };
    int epi = 0, norm = 0;
    GemvParams g = params(0, epi, norm);
    size_t nbytes = e->wbytes(g.N, g.K);
    nbytes += (size_t)M * g.K * 4 + (size_t)M * (epi == EPI_SILU_MUL ? F : D) * 4 * (epi == EPI_ADD ? 2 : 1);
    const char* lenv = getenv("CSM_BENCH_LAYERS");  // lab: rotate over fewer layers (cache residency)
    const int nl = lenv ? std::max(1, std::min(atoi(lenv), s.d.n_layers)) : s.d.n_layers;
    auto run1 = [&](int i) {
      GemvParams gi = params(i % nl, epi, norm);
      if (xsb) {
        if (!norm) gi.nw = nullptr;
        launch_gemm_xs(xs_params(gi, epi), epi, e->st, tag == 0 && gemv_nt(0), e->wdt);
      } else {
        launch_gemv(gi, e->wdt, epi, norm, e->st, tag);
      }
    };
    const float us = time_launches(e->st, nl, iters, run1, [&] {
      if (xsb) gemm_xs_stamps_report("warm");  // lab builds: clears the stamps of the warm-up launches
    });
    if (xsb) gemm_xs_stamps_report((std::string(stack ? "dec" : "bb") + " kind " + std::to_string(kind) + " M " + std::to_string(M)).c_str());
    if (avg_us) *avg_us = us;
    if (bytes) *bytes = (double)nbytes;
  }
  CSM_CATCH
}

int csm_bench_dec_frame(csm_engine* e, int iters, float* avg_us, double* bytes) {
  CSM_TRY {
    if (!e || iters <= 0) throw CsmError(CSM_ERR_ARG, "bad bench arguments");
    if (!dec_frame_eligible(e)) throw CsmError(CSM_ERR_STATE, "the persistent frame decoder is not active on this engine");
    if (e->prompt_len.empty() || e->prompt_len[0] < 0) throw CsmError(CSM_ERR_STATE, "csm_prefill first (the replay needs h_last)");
    HIPCHK(hipSetDevice(e->dev));
    // The replay recomputes the last frame's head from the same h_last: the same codes, logits and
    // decoder K/V rows are written again (the advance launch is not replayed).
    const size_t D = e->Dd, DB = e->D, V = e->V, F = e->dec.d.intermediate, QKV = e->dec.qkv_rows();
    const size_t HKV = e->dec.d.n_kv_heads, HD = e->dec.d.head_dim;
    // every weight in its storage format (bf16, or int4 nibbles + affine words); audio_head stays bf16
    auto wb = [&](size_t n, size_t k) { return (double)e->wbytes(n, k); };
    double nb = wb(V, DB) + DB * 4 + wb(D, DB);                       // codebook0_head, h_last, projection
    for (int step = 1; step < e->K; ++step) {
      const int rows = step == 1 ? 2 : 1, pos = step == 1 ? 1 : step;
      for (int l = 0; l < DEC_FRAME_LAYERS; ++l) {
        nb += (l == 0 && step > 1) ? (double)QKV * 4 : wb(QKV, D);          // folded qkv0 table row / QKV
        nb += wb(D, D) + wb(2 * F, D) + wb(D, F);                           // o, gate/up, down
        nb += 2.0 * HKV * (pos + 1) * HD * 4 + 2.0 * HKV * rows * HD * 4;    // K/V history read + append
      }
      nb += (double)V * D * 2 + D * 4;                                      // audio_head[step-1], next x row
    }
    const float us = time_launches(e->st, 2, iters, [&](int) { enqueue_dec_frame_only(e, e->st); });
    check_handoffs(e);
    if (avg_us) *avg_us = us;
    if (bytes) *bytes = nb;
  }
  CSM_CATCH
}

int csm_bench_dec_xsd(csm_engine* e, int iters, float* avg_us, double* bytes) {
  CSM_TRY {
    if (!e || iters <= 0) throw CsmError(CSM_ERR_ARG, "bad bench arguments");
    const int M = e->B, K = e->K;
    // (a weaker predicate than the live path's plan_step: ADVICE.md, the csm_bench_dec_xsd item)
    if (e->frames_run < 1 || !xsd_eligible(e, M)) throw CsmError(CSM_ERR_STATE, "the persistent batched decoder step is not active on this engine");
    HIPCHK(hipSetDevice(e->dev));
    // The replay recomputes the last frame's last codebook step (i = K - 1) from the same partials of
    // step K - 2: the same K/V rows, codes, logits and partials are written again.
    const int Vp = e->Vpad, i = K - 1;
    const bool greedy = !frame_plan(e).sampled;
    auto part = [&](int cb) { return e->part + (size_t)cb * e->B_max * e->part_stride; };
    const int pn = greedy ? head_blocks(Vp, e->Dd, M, e->head_wdt) : 1;
    const size_t D = e->Dd, F = e->dec.d.intermediate, QKV = e->dec.qkv_rows(), HKV = e->dec.d.n_kv_heads, HD = e->dec.d.head_dim;
    auto wb = [&](size_t n, size_t k) { return (double)e->wbytes(n, k); };
    double nb = (double)M * (QKV + D) * 4;                                  // layer 0: folded table rows
    for (int l = 0; l < DEC_FRAME_LAYERS; ++l) {
      if (l > 0) nb += wb(QKV, D);
      nb += wb(D, D) + wb(2 * F, D) + wb(D, F);                             // weights in their storage format
      nb += 2.0 * M * HKV * (i + 1) * HD * 4;                               // K/V history read + append
    }
    nb += (double)Vp * D * 2;                                               // audio_head[i - 1] (bf16)
    const float us = time_launches(e->st, 2, iters, [&](int) {
      launch_xsd(e, M, i, part(i - 1), pn, part(i), e->st, xsd_head_tiled(e, M, i), false);
    });
    check_handoffs(e);
    if (avg_us) *avg_us = us;
    if (bytes) *bytes = nb;
  }
  CSM_CATCH
}

int csm_bench_bb_step(csm_engine* e, int iters, float* avg_us, double* bytes) {
  CSM_TRY {
    if (!e || iters <= 0) throw CsmError(CSM_ERR_ARG, "bad bench arguments");
    if (!bb_step_eligible(e)) throw CsmError(CSM_ERR_STATE, "the persistent backbone step is not active on this engine");
    if (e->frames_run < 2) throw CsmError(CSM_ERR_STATE, "run two frames first (the replay needs an embedded decode row)");
    HIPCHK(hipSetDevice(e->dev));
    // The replay recomputes the last backbone row from the same embedded x at the same position: the
    // same K/V rows and h_last are written again.
    int pos = 0;
    HIPCHK(hipMemcpy(&pos, e->pos, 4, hipMemcpyDeviceToHost));
    const csm_llama_dims& d = e->bb.d;
    const double D = d.hidden, F = d.intermediate, QKV = e->bb.qkv_rows(), HKV = d.n_kv_heads, HD = d.head_dim;
    double nb = D * 4 * 2;                                                     // x in, h_last out
    for (int l = 0; l < d.n_layers; ++l) {
      nb += (double)e->wbytes((size_t)QKV, (size_t)D) + (double)e->wbytes((size_t)D, (size_t)D) +   // weights in
            (double)e->wbytes(2 * (size_t)F, (size_t)D) + (double)e->wbytes((size_t)D, (size_t)F) +     // their storage
            2 * D * 4;                                                          // format; norm weights
      nb += 2 * HKV * (double)pos * HD * 4 + 2 * HKV * HD * 4;                  // K/V history read + append
    }
    const float us = time_launches(e->st, 2, iters, [&](int) { enqueue_bb_step(e, e->st); });
    check_handoffs(e);
    if (avg_us) *avg_us = us;
    if (bytes) *bytes = nb;
  }
  CSM_CATCH
}

int csm_set_option(csm_engine* e, const char* key, int value) {
  // switches that only set one flag (inverted: the flag is the option's negation)
  static const struct { const char* key; bool csm_engine::*flag; bool inverted; } flags[] = {
      {"linear_mfma", &csm_engine::linear_mfma, false},     {"fold_proj", &csm_engine::fold_proj, false},
      {"qkv0_tab", &csm_engine::use_qkv0_tab, false},       {"gemm_xs", &csm_engine::xs_on, false},
      {"bb_xs", &csm_engine::bb_xs_on, false},              {"qkv0_tab_batched", &csm_engine::no_tab_batched, true},
      {"attn_prefill", &csm_engine::attn_tiles_on, false},  {"dec_xsd_head", &csm_engine::xsd_head, false},
      {"dec_xsd_sample", &csm_engine::xsd_sample, false},
  };
  CSM_TRY {
    const std::string k(key ? key : "");
    auto need_engine = [&] { if (!e) throw CsmError(CSM_ERR_ARG, k + " needs an engine"); };
    const auto* f = std::find_if(std::begin(flags), std::end(flags), [&](const auto& o) { return k == o.key; });
    int hi = 0;  // the persistent kernel whose switch "<key>" or clock stamps buffer "<key>_stamps" k names
    while (hi < 3 && k != HANDOFF_KEYS[hi] && k != std::string(HANDOFF_KEYS[hi]) + "_stamps") ++hi;
    if (f != std::end(flags)) {
      need_engine();
      e->*f->flag = (value != 0) != f->inverted;
      if (k == "qkv0_tab" && e->use_qkv0_tab && !e->qkv0_built) e->proj_tab_dirty = true;  // built at the next csm_begin
    } else if (hi < 3) {
      need_engine();
      Handoff& h = *e->handoffs()[hi];
      if (k == HANDOFF_KEYS[hi]) h.on = value != 0;
      else if (value && !h.stamps) h.stamps = (unsigned long long*)e->alloc(h.stamps_bytes);
      else if (!value && h.stamps) { e->release(h.stamps); h.stamps = nullptr; }
    } else if (k == "prefill_rows") {
      if (!e || value < 0) throw CsmError(CSM_ERR_ARG, "prefill_rows needs an engine and a row count >= 0");
      e->prefill_rows = value;
    } else if (k == "inject_handoff_error") {  // test hook: raise the persistent kernels' timeout flags
      need_engine();
      const int one = 1;
      for (Handoff* h : e->handoffs())
        if (h->err && value) HIPCHK(hipMemcpy(h->err, &one, 4, hipMemcpyHostToDevice));
    } else {
      throw CsmError(CSM_ERR_ARG, "unknown option " + k);
    }
    if (e) e->g_B = -1;  // re-capture the frame graphs with the new setting
  }
  CSM_CATCH
}

}  // extern "C"
