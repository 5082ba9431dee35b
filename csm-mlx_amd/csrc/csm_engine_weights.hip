// CSM engine, lifecycle and weights: engine creation, batch-sized buffers, the weight loader and
// quantizer, and the tables derived from the weights (fragment-tiled copies, folded decoder inputs).
#include "csm_engine.h"

namespace {

void alloc_stack(csm_engine* e, Stack& s, const csm_llama_dims& d, int S_cap, const char* prefix) {
  s.d = d;
  s.S_cap = S_cap;
  s.L.resize(d.n_layers);
  const size_t D = d.hidden, F = d.intermediate, hd = d.head_dim;
  for (int i = 0; i < d.n_layers; ++i) {
    LayerW& l = s.L[i];
    l.wqkv = e->alloc(e->wbytes(s.qkv_rows(), D));
    l.wo = e->alloc(e->wbytes(D, s.q_dim()));
    l.wgu = e->alloc(e->wbytes(2 * F, D));
    l.wd = e->alloc(e->wbytes(D, F));
    if (e->wdt == WDT_BF16 && wdc_chunk((int)D) && F % wdc_chunk((int)D) == 0) l.wdc = e->alloc(D * F * 2);
    l.n1 = (float*)e->alloc(D * 4);
    l.n2 = (float*)e->alloc(D * 4);
    const std::string p = std::string(prefix) + ".layers." + std::to_string(i);
    for (const char* n : {".self_attn.q_proj.weight", ".self_attn.k_proj.weight", ".self_attn.v_proj.weight",
                          ".self_attn.o_proj.weight", ".mlp.gate_proj.weight", ".mlp.up_proj.weight",
                          ".mlp.down_proj.weight", ".input_layernorm.weight", ".post_attention_layernorm.weight"})
      e->required.push_back(p + n);
  }
  s.norm = (float*)e->alloc(D * 4);
  s.rope = (float*)e->alloc((size_t)S_cap * hd * 4);
  e->required.push_back(std::string(prefix) + ".norm.weight");
}

}  // namespace

// (Re)allocate everything sized by the batch: KV caches, decoder activations, code history.
void ensure_batch(csm_engine* e, int B) {
  if (B <= e->B_max && !e->batch_allocs.empty()) return;
  HIPCHK(hipDeviceSynchronize());
  for (void* p : e->batch_allocs) (void)hipFree(p);
  e->batch_allocs.clear();
  if (e->g_body) { (void)hipGraphExecDestroy(e->g_body); e->g_body = nullptr; }
  if (e->g_head) { (void)hipGraphExecDestroy(e->g_head); e->g_head = nullptr; }
  e->g_B = -1;
  e->B_max = std::max(B, e->B_max);
  const size_t Bm = e->B_max, D = e->D, Dd = e->Dd, K = e->K, Vp = e->Vpad;
  for (Stack* s : {&e->bb, &e->dec}) {
    const size_t kv = Bm * s->d.n_kv_heads * (size_t)s->S_cap * s->d.head_dim * 4;
    for (LayerW& l : s->L) {
      l.kc = (float*)e->balloc(kv);
      l.vc = (float*)e->balloc(kv);
    }
  }
  {  // the prefix copy kernel's table of the backbone caches (csm_engine_prefix.hip)
    std::vector<float*> tab;
    for (LayerW& l : e->bb.L) { tab.push_back(l.kc); tab.push_back(l.vc); }
    if (!e->kv_tab) e->kv_tab = (float**)e->alloc(tab.size() * sizeof(float*));
    HIPCHK(hipMemcpy(e->kv_tab, tab.data(), tab.size() * sizeof(float*), hipMemcpyHostToDevice));
  }
  e->h_last = (float*)e->balloc(Bm * D * 4);
  e->c0_logits = (float*)e->balloc(Bm * Vp * 4);
  e->force = (int*)e->balloc(Bm * K * 4);
  e->force_ce = (float*)e->balloc(Bm * K * 4);
  e->ci_logits = (float*)e->balloc((K - 1) * Bm * Vp * 4);
  e->dx = (float*)e->balloc(2 * Bm * Dd * 4);
  e->din = (float*)e->balloc(2 * Bm * D * 4);
  e->dq = (float*)e->balloc(2 * Bm * e->dec.q_dim() * 4);
  e->datt = (float*)e->balloc(2 * Bm * e->dec.q_dim() * 4);
  e->dmlp = (float*)e->balloc(2 * Bm * (size_t)e->dec.d.intermediate * 4);
  e->codes = (int*)e->balloc(Bm * K * 4);
  e->hist = (int*)e->balloc((size_t)e->F_cap * Bm * K * 4);
  e->pos = (int*)e->balloc(Bm * 4);
  e->n_frames = (int*)e->balloc(Bm * 4);
  e->slot_frame = (int*)e->balloc(Bm * 4);
  e->parked = (uint8_t*)e->balloc(Bm);
  e->slot_sampling = (SlotSampling*)e->balloc(Bm * sizeof(SlotSampling));
  e->slot_bias = (float*)e->balloc(Bm * Vp * 4);
  e->done = (uint8_t*)e->balloc(Bm);
  e->seeds = (uint64_t*)e->balloc(Bm * 8);
  // partial slots per row: enough for any head tiling (c0 / ci heads, dense or q4; >= Vp/2 blocks never occur)
  e->part_stride = (int)(Vp / 2);
  e->part = (unsigned long long*)e->balloc(K * Bm * (size_t)e->part_stride * 8);
  // split-K scratch of the MFMA path for every projection shape at its largest row count
  for (Stack* s : {&e->bb, &e->dec}) {
    const int Dm = s->d.hidden, F = s->d.intermediate, rows = (s == &e->bb) ? std::max(e->M_cap, (int)Bm) : 2 * (int)Bm;
    gemm_reserve(e->ws, s->qkv_rows(), Dm, rows);
    gemm_reserve(e->ws, Dm, s->q_dim(), rows);
    gemm_reserve(e->ws, 2 * F, Dm, rows);
    gemm_reserve(e->ws, Dm, F, rows);
  }
  gemm_reserve(e->ws, (int)Dd, (int)D, 2 * (int)Bm);
  gemm_reserve(e->ws, (int)Vp, (int)D, (int)Bm);   // c0 head
  gemm_reserve(e->ws, (int)Vp, (int)Dd, (int)Bm);  // ci heads
  // the streaming decoder path (gemm_xs): split-row buffers for up to GEMM_XS_MAX_M rows + its scratch
  {
    // (shared by the backbone and the decoder: their launches never overlap)
    // (2 Bm: the depth decoder's step 1 carries two rows per utterance)
    const int xm = GEMM_XS_MAX_M, rows = std::min(2 * (int)Bm, xm);
    size_t bD = 0, bA = 0, bF = 0;
    for (Stack* s : {&e->bb, &e->dec}) {
      const int Dm = s->d.hidden, F = s->d.intermediate;
      bD = std::max(bD, xs::bytes(xm, Dm));
      bA = std::max(bA, xs::bytes(xm, s->q_dim()));
      bF = std::max(bF, xs::bytes(xm, F));
      gemm_xs_reserve(e->ws, s->qkv_rows(), Dm, rows);
      gemm_xs_reserve(e->ws, Dm, s->q_dim(), rows);
      gemm_xs_reserve(e->ws, 2 * F, Dm, rows);
      gemm_xs_reserve(e->ws, Dm, F, rows);
    }
    gemm_xs_reserve(e->ws, (int)Vp, (int)Dd, rows);
    e->xs_D = e->balloc(bD);
    e->xs_A = e->balloc(bA);
    e->xs_F = e->balloc(bF);
    e->xs_ss = (float*)e->balloc((size_t)64 * xm * 4);
    for (float** h : {&e->hs_D, &e->hs_A, &e->hs_F}) *h = (float*)e->balloc(bF / xs::XS_EB / xm / 32 * xs::HS_ROWS * 4 + 4096);
  }
  // the persistent batched decoder step's scratch (csm_1b decoder shapes only; control words once per engine)
  {
    if (csm1b_decoder(e->dec.d)) {
      const size_t R = DEC_XSD_MAX_M_Q4;
      DecStepXsArgs& x = e->xsd;
      x.qkv = (float*)e->balloc(R * e->dec.qkv_rows() * 4);
      x.qkvp = (float*)e->balloc((2 * R * e->dec.qkv_rows() + (size_t)e->dec.qkv_rows() / 32 * R) * 4);  // + row scales [48][R]
      x.xs_att = e->balloc(xs::bytes(R, 1024));
      x.xs_x = e->balloc(xs::bytes(R, 1024));
      x.xs_h = e->balloc(xs::bytes(R, 8192));
      x.x_o = (float*)e->balloc(R * 1024 * 4);
      x.x_d = (float*)e->balloc(R * 1024 * 4);
      x.ss_o = (float*)e->balloc(32 * R * 4);
      x.dpart = (float*)e->balloc(8 * R * 1024 * 4);
      x.code_buf = (int*)e->balloc(R * 4);
      x.hs_att = (float*)e->balloc(1024 / 32 * R * 4);
      x.hs_x = (float*)e->balloc(1024 / 32 * R * 4);
      x.hs_h = (float*)e->balloc(8192 / 32 * R * 4);
      if (!e->h_xsd.buf) {
        e->h_xsd.buf = e->alloc(dec_step_xs_ctrl_bytes());
        e->h_xsd.epoch = (unsigned*)e->alloc(16);
        e->h_xsd.err = (int*)e->alloc(16);
      }
    }
  }
}

// Fragment-tiled copies (launch_gemm_retile) of every matrix the batched MFMA path reads -- stack
// projections, projection, codebook0_head, the bf16 audio_head slices -- rebuilt in place after any
// weight change (csm_load_tensor, csm_quantize), at csm_begin, before graphs capture them.
void build_tiled(csm_engine* e) {
  // pass 0 allocates (alloc's zero fill runs on the null stream: drained before pass 1 writes the
  // copies on the engine stream), pass 1 re-lays every matrix
  for (int pass = 0; pass < 2; ++pass) {
  size_t idx = 0;
  auto one = [&](const void* W, int N, int K, int wdt) {
    if (wdt != WDT_BF16 && wdt != WDT_Q4) return;
    if (pass == 0) {
      if (idx++ == e->tiled_bufs.size()) e->tiled_bufs.push_back(e->alloc(gemm_tiled_bytes(N, K, wdt)));
      return;
    }
    void* T = e->tiled_bufs[idx++];
    launch_gemm_retile(W, T, N, K, wdt, e->st);
    e->ws.tiled[W] = T;
  };
  for (Stack* s : {&e->bb, &e->dec})
    for (LayerW& l : s->L) {
      const int D = s->d.hidden, F = s->d.intermediate;
      one(l.wqkv, s->qkv_rows(), D, e->wdt);
      one(l.wo, D, s->q_dim(), e->wdt);
      one(l.wgu, 2 * F, D, e->wdt);
      one(l.wd, D, F, e->wdt);
    }
  one(e->proj, e->Dd, e->D, e->wdt);
  one(e->c0_head, e->Vpad, e->D, e->wdt);
  if (e->wdt == WDT_Q4)  // the persistent kernels' chunk-major down copies (bb_step_q4 / dec_frame_q4)
    for (Stack* s : {&e->bb, &e->dec})
      for (LayerW& l : s->L) {
        const int D = s->d.hidden, F = s->d.intermediate;
        if (F % 64) continue;
        if (pass == 0) { if (!l.wdq) l.wdq = e->alloc(q4_bytes(D, F)); }
        else launch_q4_down_cm(l.wd, D, F, l.wdq, e->st);
      }
  if (e->head_wdt == WDT_BF16)
    for (int cb = 0; cb < e->K - 1; ++cb) one((const char*)e->audio_head + (size_t)cb * e->Vpad * e->Dd * 2, e->Vpad, e->Dd, WDT_BF16);
  HIPCHK(hipDeviceSynchronize());
  }
  HIPCHK(hipGetLastError());
  e->tiled_dirty = false;
}

// proj_tab[cb] = projection(E_a rows of codebook cb), computed by the projection GEMV itself
// (per-row arithmetic identical to the per-step launch it replaces).
void build_proj_table(csm_engine* e) {
  const int V = e->V, D = e->D, Dd = e->Dd;
  float* scratch = e->mlp;  // [M_cap][F] fp32: >= V*D floats (checked at create)
  for (int cb = 0; cb < e->K - 1; ++cb) {
    if (e->wdt == WDT_Q4) launch_q4_to_f32(e->audio_emb, V * e->K, D, cb * V, V, scratch, e->st);
    else launch_to_f32((const char*)e->audio_emb + (size_t)cb * V * D * e->wsz, e->wdt, scratch, (size_t)V * D, e->st);
    GemvParams g = gp(e);
    g.W = e->proj; g.N = Dd; g.K = D; g.x = scratch; g.xs = D; g.M = V;
    g.out = e->proj_tab + (size_t)cb * V * Dd; g.os = Dd;
    g.no_mfma = 1;  // the GEMV's per-row arithmetic (the step-1 launch's), never the matrix cores
    launch_gemv_table(g, e->wdt, EPI_STORE, 0, e->st, 1);
  }
  HIPCHK(hipStreamSynchronize(e->st));
  HIPCHK(hipGetLastError());
  e->proj_tab_dirty = false;
  // layer-0 QKV of every folded decoder input row, by the frame's own QKV GEMV (one launch per
  // codebook where the shape allows, else 4 rows per launch: per-row arithmetic of the 1-row launch)
  if (!e->use_qkv0_tab) return;  // built at the next csm_begin after csm_set_option("qkv0_tab", 1)
  const Stack& s = e->dec;
  const LayerW& l0 = s.L[0];
  for (int cb = 1; cb < e->K - 1; ++cb) {
    GemvParams g = gp(e);
    g.W = l0.wqkv; g.N = s.qkv_rows(); g.K = Dd; g.x = e->proj_tab + (size_t)cb * V * Dd; g.xs = Dd;
    g.M = V; g.nw = l0.n1; g.eps = s.d.eps; g.Hq = s.d.n_heads; g.Hkv = s.d.n_kv_heads;
    g.hd = s.d.head_dim; g.S_cap = s.S_cap; g.rope = s.rope; g.rm = RowMap{1, 0, nullptr, cb + 1};
    g.qkv_tab = e->qkv0_tab + (size_t)cb * V * s.qkv_rows();
    launch_gemv_table(g, e->wdt, EPI_QKV, 1, e->st, 1);
  }
  HIPCHK(hipStreamSynchronize(e->st));
  HIPCHK(hipGetLastError());
  e->qkv0_built = true;
}

bool weight_place(csm_engine* e, const std::string& name, Place& pl) {
  for (int which = 0; which < 2; ++which) {
    Stack& s = which == 0 ? e->bb : e->dec;
    const std::string pre = which == 0 ? "backbone.layers." : "decoder.layers.";
    if (name.rfind(pre, 0) != 0) continue;
    int li = -1;
    char tail[128] = {0};
    if (sscanf(name.c_str() + pre.size(), "%d.%127s", &li, tail) != 2 || li < 0 || li >= s.d.n_layers) return false;
    LayerW& l = s.L[li];
    const std::string t(tail);
    const int D = s.d.hidden, F = s.d.intermediate, qd = s.q_dim(), kvd = s.d.n_kv_heads * s.d.head_dim;
    const int qkv = s.qkv_rows();
    if (t == "self_attn.q_proj.weight") pl = Place{l.wqkv, qkv, D, 0, 1, qd};
    else if (t == "self_attn.k_proj.weight") pl = Place{l.wqkv, qkv, D, qd, 1, kvd};
    else if (t == "self_attn.v_proj.weight") pl = Place{l.wqkv, qkv, D, qd + kvd, 1, kvd};
    else if (t == "self_attn.o_proj.weight") pl = Place{l.wo, D, qd, 0, 1, D};
    else if (t == "mlp.gate_proj.weight") pl = Place{l.wgu, 2 * F, D, 0, 2, F};
    else if (t == "mlp.up_proj.weight") pl = Place{l.wgu, 2 * F, D, 1, 2, F};
    else if (t == "mlp.down_proj.weight") pl = Place{l.wd, D, F, 0, 1, D};
    else return false;
    return true;
  }
  const int D = e->D, Dd = e->Dd, V = e->V, K = e->K, Vp = e->Vpad;
  if (name == "text_embeddings.weight") pl = Place{e->text_emb, e->dims.n_text_vocab, D, 0, 1, e->dims.n_text_vocab};
  else if (name == "audio_embeddings.weight") pl = Place{e->audio_emb, V * K, D, 0, 1, V * K};
  else if (name == "projection.weight") pl = Place{e->proj, Dd, D, 0, 1, Dd};
  else if (name == "codebook0_head.weight") pl = Place{e->c0_head, Vp, D, 0, 1, V};
  else return false;
  return true;
}

namespace {

// int4 engine: an MLX float weight is quantized on the device; a pre-quantized one (uint32
// .weight + .scales + .biases, MLX QuantizedLinear / QuantizedEmbedding keys) is placed once all
// three parts have arrived.  Returns false for names that are not quantized parameters.
bool load_q4(csm_engine* e, const std::string& name, const void* host, int src_dtype, const std::vector<int64_t>& shp) {
  std::string base = name, part = "weight";
  for (const char* suf : {".scales", ".biases"})
    if (name.size() > strlen(suf) && name.compare(name.size() - strlen(suf), strlen(suf), suf) == 0) {
      base = name.substr(0, name.size() - strlen(suf)) + ".weight";
      part = suf + 1;
    }
  Place pl;
  if (!weight_place(e, base, pl)) return false;
  size_t numel = 1;
  for (auto v : shp) numel *= (size_t)v;
  if (part == "weight" && src_dtype != CSM_U32) {  // float weight -> quantize (nn.quantize)
    if (shp != std::vector<int64_t>{pl.n, pl.K}) throw CsmError(CSM_ERR_ARG, "shape mismatch for " + name);
    auto h = convert_to(host, src_dtype, numel, WDT_F32);
    DevBuf tmp(h.size());
    HIPCHK(hipMemcpy(tmp.p, h.data(), h.size(), hipMemcpyHostToDevice));
    launch_q4_quantize(tmp.p, WDT_F32, pl.n, pl.K, pl.base, pl.Ntot, pl.row0, pl.rstep, e->st);
    HIPCHK(hipStreamSynchronize(e->st));
    HIPCHK(hipGetLastError());
    e->loaded.insert(base);
    if (base == "audio_embeddings.weight" || base == "projection.weight") e->proj_tab_dirty = true;
    return true;
  }
  auto& pq = e->pending_q4[base];
  const size_t es = src_dtype == CSM_F32 || src_dtype == CSM_U32 ? 4 : 2;
  if (part == "weight") {
    if (shp != std::vector<int64_t>{pl.n, pl.K / 8}) throw CsmError(CSM_ERR_ARG, "packed shape mismatch for " + name);
    pq.packed.assign((const uint8_t*)host, (const uint8_t*)host + numel * 4);
  } else {
    if (src_dtype != CSM_F32 && src_dtype != CSM_BF16) throw CsmError(CSM_ERR_ARG, name + " must be f32 or bf16");
    if (shp != std::vector<int64_t>{pl.n, pl.K / Q4_GROUP}) throw CsmError(CSM_ERR_ARG, "shape mismatch for " + name);
    if (!pq.scales.empty() || !pq.biases.empty())
      if (pq.sdt != src_dtype) throw CsmError(CSM_ERR_ARG, "scales / biases dtypes differ for " + base);
    pq.sdt = src_dtype;
    (part == "scales" ? pq.scales : pq.biases).assign((const uint8_t*)host, (const uint8_t*)host + numel * es);
  }
  if (pq.packed.empty() || pq.scales.empty() || pq.biases.empty()) return true;
  // all three parts present: nibble rows (strided for interleaved gate/up) + sb words
  const size_t rowb = (size_t)pl.K / 2;
  HIPCHK(hipMemcpy2D((uint8_t*)pl.base + (size_t)pl.row0 * rowb, rowb * pl.rstep, pq.packed.data(), rowb, rowb, pl.n,
                     hipMemcpyHostToDevice));
  DevBuf sc(pq.scales.size()), bi(pq.biases.size());
  HIPCHK(hipMemcpy(sc.p, pq.scales.data(), pq.scales.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(bi.p, pq.biases.data(), pq.biases.size(), hipMemcpyHostToDevice));
  launch_q4_set_sb(sc.p, bi.p, pq.sdt == CSM_BF16 ? WDT_BF16 : WDT_F32, pl.n, pl.K, pl.base, pl.Ntot, pl.row0,
                   pl.rstep, e->st);
  HIPCHK(hipStreamSynchronize(e->st));
  HIPCHK(hipGetLastError());
  e->pending_q4.erase(base);
  e->loaded.insert(base);
  if (base == "audio_embeddings.weight" || base == "projection.weight") e->proj_tab_dirty = true;
  return true;
}

}  // namespace

// =============================================================================== C ABI
extern "C" {

int csm_device_count(int* n) {
  CSM_TRY {
    int c = 0;
    HIPCHK(hipGetDeviceCount(&c));
    if (n) *n = c;
  }
  CSM_CATCH
}

int csm_engine_create(const csm_dims* dims, int device, int weight_dtype, int max_batch, int max_frames,
                      csm_engine** out) {
  CSM_TRY {
    if (!dims || !out || max_batch <= 0 || max_frames <= 0) throw CsmError(CSM_ERR_ARG, "bad engine arguments");
    const csm_llama_dims& b = dims->backbone;
    const csm_llama_dims& d = dims->decoder;
    for (const csm_llama_dims* x : {&b, &d}) {
      if (x->head_dim != 64 && x->head_dim != 128) throw CsmError(CSM_ERR_ARG, "head_dim must be 64 or 128");
      if (x->hidden % 256 || x->intermediate % 256 || (x->n_heads * x->head_dim) % 256)
        throw CsmError(CSM_ERR_ARG, "hidden/intermediate widths must be multiples of 256");
      if (x->n_heads % x->n_kv_heads) throw CsmError(CSM_ERR_ARG, "n_heads % n_kv_heads != 0");
    }
    if (b.n_heads * b.head_dim != b.hidden) throw CsmError(CSM_ERR_ARG, "backbone hidden != heads*head_dim");
    for (const csm_llama_dims* x : {&b, &d})
      if (x->n_heads / x->n_kv_heads > 4) throw CsmError(CSM_ERR_ARG, "GQA group > 4 unsupported");
    if (weight_dtype != CSM_F32 && weight_dtype != CSM_BF16 && weight_dtype != CSM_Q4)
      throw CsmError(CSM_ERR_ARG, "weight_dtype must be CSM_F32, CSM_BF16 or CSM_Q4");
    {  // every GEMV shape must tile into whole blocks (q4: any even N whose K the q4 tiling covers)
      const int Vp = (dims->n_audio_vocab + 7) / 8 * 8;
      std::vector<std::pair<int, int>> shapes = {{Vp, b.hidden}, {Vp, d.hidden}, {d.hidden, b.hidden}};
      for (const csm_llama_dims* x : {&b, &d}) {
        shapes.push_back({(x->n_heads + 2 * x->n_kv_heads) * x->head_dim, x->hidden});
        shapes.push_back({x->hidden, x->n_heads * x->head_dim});
        shapes.push_back({2 * x->intermediate, x->hidden});
        shapes.push_back({x->hidden, x->intermediate});
      }
      for (auto [N, Kd] : shapes) {
        for (int M : {1, 4})
          if (N % gemv_rows_per_block(N, Kd, M)) throw CsmError(CSM_ERR_ARG, "GEMV shape does not tile");
        if (!gemv_q4_supported(N, Kd) && weight_dtype == CSM_Q4)
          throw CsmError(CSM_ERR_ARG, "int4 GEMV does not support this shape");
      }
    }
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<csm_engine> e(new csm_engine());
    e->dims = *dims;
    e->dev = device;
    e->wdt = weight_dtype == CSM_F32 ? WDT_F32 : (weight_dtype == CSM_Q4 ? WDT_Q4 : WDT_BF16);
    e->head_wdt = e->wdt == WDT_F32 ? WDT_F32 : WDT_BF16;
    e->wsz = e->wdt == WDT_F32 ? 4 : 2;
    e->B_max = max_batch;
    e->F_cap = max_frames;
    e->K = dims->n_audio_codebooks;
    e->V = dims->n_audio_vocab;
    e->Vpad = (e->V + 7) / 8 * 8;
    e->D = b.hidden;
    e->Dd = d.hidden;
    const int S = dims->max_seq_len;
    e->M_cap = std::max(S, 2 * max_batch);
    int least = 0, greatest = 0;  // the engine's stream first (mimi_create)
    HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIPCHK(hipStreamCreateWithPriority(&e->st, hipStreamNonBlocking, greatest));
    alloc_stack(e.get(), e->bb, b, S, "backbone");
    alloc_stack(e.get(), e->dec, d, e->K, "decoder");
    const size_t D = e->D, Dd = e->Dd, K = e->K, Vp = e->Vpad;
    e->text_emb = e->alloc(e->wbytes(dims->n_text_vocab, D));
    e->audio_emb = e->alloc(e->wbytes((size_t)e->V * K, D));
    e->proj = e->alloc(e->wbytes(Dd, D));
    e->c0_head = e->alloc(e->wbytes(Vp, D));
    e->audio_head = e->alloc((K - 1) * Vp * Dd * (e->head_wdt == WDT_F32 ? 4 : 2));
    e->proj_tab = (float*)e->alloc((K - 1) * (size_t)e->V * Dd * 4);
    e->qkv0_tab = (float*)e->alloc((K - 1) * (size_t)e->V * e->dec.qkv_rows() * 4);
    for (const char* n : {"text_embeddings.weight", "audio_embeddings.weight", "projection.weight",
                          "codebook0_head.weight", "audio_head"})
      e->required.push_back(n);
    const size_t M = e->M_cap;
    e->x = (float*)e->alloc(M * D * 4);
    e->q = (float*)e->alloc(M * e->bb.q_dim() * 4);
    e->att = (float*)e->alloc(M * e->bb.q_dim() * 4);
    e->mlp = (float*)e->alloc(M * b.intermediate * 4);
    if (M * (size_t)b.intermediate < (size_t)e->V * e->D)
      throw CsmError(CSM_ERR_ARG, "activation scratch too small for the projection table build");
    e->tok = (int32_t*)e->alloc(M * (K + 1) * 4);
    e->msk = (uint8_t*)e->alloc(M * (K + 1));
    e->row_b = (int*)e->alloc(M * 4);
    e->row_pos = (int*)e->alloc(M * 4);
    e->ptiles = (int2*)e->alloc((M / 64 + (size_t)max_batch + 2) * sizeof(int2));
    e->frame_ctr = (int*)e->alloc(16);
    e->h_df.buf = e->alloc(dec_frame_gbuf_bytes());
    e->h_df.epoch = (unsigned*)e->alloc(16);
    e->h_df.err = (int*)e->alloc(16);
    if ((e->wdt == WDT_BF16 || e->wdt == WDT_Q4) && b.hidden == 2048 && b.n_layers == BB_STEP_LAYERS) {
      e->h_bb.buf = e->alloc(bb_step_gbuf_bytes());
      e->h_bb.epoch = (unsigned*)e->alloc(16);
      e->h_bb.err = (int*)e->alloc(16);
    }
    ensure_batch(e.get(), max_batch);
    HIPCHK(hipDeviceSynchronize());
    *out = e.release();
  }
  CSM_CATCH
}

int csm_engine_destroy(csm_engine* e) {
  CSM_TRY { delete e; }
  CSM_CATCH
}

int csm_set_rope_table(csm_engine* e, int which, const float* table, int n_pos, int head_dim) {
  CSM_TRY {
    Stack& s = which == 0 ? e->bb : e->dec;
    if (head_dim != s.d.head_dim || n_pos < s.S_cap) throw CsmError(CSM_ERR_ARG, "rope table shape mismatch");
    HIPCHK(hipSetDevice(e->dev));
    HIPCHK(hipMemcpy(s.rope, table, (size_t)s.S_cap * head_dim * 4, hipMemcpyHostToDevice));
    ++e->weights_epoch;  // saved prefixes hold keys rotated by the old table
  }
  CSM_CATCH
}

int csm_load_tensor(csm_engine* e, const char* cname, const void* host, int src_dtype, const int64_t* shape,
                    int ndim) {
  CSM_TRY {
    HIPCHK(hipSetDevice(e->dev));
    const std::string name(cname);
    std::vector<int64_t> shp(shape, shape + ndim);
    auto numel = [&]() { int64_t n = 1; for (auto s : shp) n *= s; return (size_t)n; };
    auto expect = [&](std::initializer_list<int64_t> want) {
      if (shp != std::vector<int64_t>(want)) throw CsmError(CSM_ERR_ARG, "shape mismatch for " + name);
    };
    if (name.rfind("decoder.layers.0.", 0) == 0) e->proj_tab_dirty = true;  // feeds the folded layer-0 QKV table
    e->tiled_dirty = true;
    ++e->weights_epoch;  // saved prefixes are stale from here on
    if (e->wdt == WDT_Q4 && load_q4(e, name, host, src_dtype, shp)) return CSM_OK;
    if (src_dtype == CSM_U32) throw CsmError(CSM_ERR_ARG, "packed int4 tensor " + name + " needs a CSM_Q4 engine");
    const size_t es = e->wsz;
    auto conv = [&](size_t n) { return convert_to(host, src_dtype, n, e->wdt); };
    auto conv_f32 = [&](size_t n) { return convert_to(host, src_dtype, n, WDT_F32); };

    // --- stack parameters
    for (int which = 0; which < 2; ++which) {
      Stack& s = which == 0 ? e->bb : e->dec;
      const std::string pre = which == 0 ? "backbone." : "decoder.";
      if (name.rfind(pre, 0) != 0) continue;
      const int D = s.d.hidden, F = s.d.intermediate, hd = s.d.head_dim;
      const int qd = s.q_dim(), kvd = s.d.n_kv_heads * hd;
      if (name == pre + "norm.weight") {
        expect({D});
        auto h = conv_f32(D);
        HIPCHK(hipMemcpy(s.norm, h.data(), D * 4, hipMemcpyHostToDevice));
        e->loaded.insert(name);
        return CSM_OK;
      }
      int li = -1;
      char tail[128] = {0};
      if (sscanf(name.c_str() + pre.size(), "layers.%d.%127s", &li, tail) != 2 || li < 0 || li >= s.d.n_layers)
        throw CsmError(CSM_ERR_ARG, "unknown tensor " + name);
      LayerW& l = s.L[li];
      const std::string t(tail);
      if (t == "self_attn.q_proj.weight") {
        expect({qd, D});
        auto h = conv(numel());
        HIPCHK(hipMemcpy(l.wqkv, h.data(), h.size(), hipMemcpyHostToDevice));
      } else if (t == "self_attn.k_proj.weight" || t == "self_attn.v_proj.weight") {
        expect({kvd, D});
        auto h = conv(numel());
        const size_t row0 = qd + (t[10] == 'k' ? 0 : kvd);
        HIPCHK(hipMemcpy((char*)l.wqkv + row0 * D * es, h.data(), h.size(), hipMemcpyHostToDevice));
      } else if (t == "self_attn.o_proj.weight") {
        expect({D, qd});
        auto h = conv(numel());
        HIPCHK(hipMemcpy(l.wo, h.data(), h.size(), hipMemcpyHostToDevice));
      } else if (t == "mlp.gate_proj.weight" || t == "mlp.up_proj.weight") {
        expect({F, D});
        auto h = conv(numel());
        const size_t off = (t[4] == 'g') ? 0 : 1;  // interleave: row 2j gate, 2j+1 up
        HIPCHK(hipMemcpy2D((char*)l.wgu + off * D * es, 2 * D * es, h.data(), D * es, D * es, F,
                           hipMemcpyHostToDevice));
      } else if (t == "mlp.down_proj.weight") {
        expect({D, F});
        auto h = conv(numel());
        HIPCHK(hipMemcpy(l.wd, h.data(), h.size(), hipMemcpyHostToDevice));
        if (l.wdc) {  // persistent kernels: columns chunk-major [F/R][D][R] (bf16)
          const int R = wdc_chunk(D);
          const uint16_t* src = reinterpret_cast<const uint16_t*>(h.data());
          std::vector<uint16_t> t2((size_t)D * F);
          for (int c = 0; c < F / R; ++c)
            for (int n = 0; n < D; ++n)
              memcpy(&t2[((size_t)c * D + n) * R], src + (size_t)n * F + (size_t)c * R, R * 2);
          HIPCHK(hipMemcpy(l.wdc, t2.data(), t2.size() * 2, hipMemcpyHostToDevice));
        }
      } else if (t == "input_layernorm.weight" || t == "post_attention_layernorm.weight") {
        expect({D});
        auto h = conv_f32(D);
        HIPCHK(hipMemcpy(t[0] == 'i' ? l.n1 : l.n2, h.data(), D * 4, hipMemcpyHostToDevice));
      } else {
        throw CsmError(CSM_ERR_ARG, "unknown tensor " + name);
      }
      e->loaded.insert(name);
      return CSM_OK;
    }
    const int64_t D = e->D, Dd = e->Dd, V = e->V, K = e->K, Vp = e->Vpad;
    if (name == "text_embeddings.weight") {
      expect({e->dims.n_text_vocab, D});
      auto h = conv(numel());
      HIPCHK(hipMemcpy(e->text_emb, h.data(), h.size(), hipMemcpyHostToDevice));
    } else if (name == "audio_embeddings.weight") {
      e->proj_tab_dirty = true;
      expect({V * K, D});
      auto h = conv(numel());
      HIPCHK(hipMemcpy(e->audio_emb, h.data(), h.size(), hipMemcpyHostToDevice));
    } else if (name == "projection.weight") {
      e->proj_tab_dirty = true;
      expect({Dd, D});
      auto h = conv(numel());
      HIPCHK(hipMemcpy(e->proj, h.data(), h.size(), hipMemcpyHostToDevice));
    } else if (name == "codebook0_head.weight") {
      expect({V, D});
      auto h = conv(numel());  // rows V..Vpad stay zero (padding)
      HIPCHK(hipMemcpy(e->c0_head, h.data(), h.size(), hipMemcpyHostToDevice));
    } else if (name == "audio_head") {
      expect({K - 1, Dd, V});
      // (in,out) layout -> per-codebook (out,in) GEMV rows: [K-1][Vpad][Dd]
      auto f = conv_f32(numel());
      const float* src = reinterpret_cast<const float*>(f.data());
      std::vector<float> t((size_t)(K - 1) * Vp * Dd, 0.f);
      for (int64_t c = 0; c < K - 1; ++c)
        for (int64_t i = 0; i < Dd; ++i)
          for (int64_t v = 0; v < V; ++v) t[((size_t)c * Vp + v) * Dd + i] = src[((size_t)c * Dd + i) * V + v];
      auto h = convert_to(t.data(), CSM_F32, t.size(), e->head_wdt);
      HIPCHK(hipMemcpy(e->audio_head, h.data(), h.size(), hipMemcpyHostToDevice));
    } else {
      throw CsmError(CSM_ERR_ARG, "unknown tensor " + name);
    }
    e->loaded.insert(name);
  }
  CSM_CATCH
}

int csm_weights_ready(csm_engine* e) {
  CSM_TRY {
    for (const auto& n : e->required)
      if (!e->loaded.count(n)) throw CsmError(CSM_ERR_STATE, "missing weight " + n);
  }
  CSM_CATCH
}

// resident weight buffers in a fixed order (identical across engines of the same dims / dtype)
static std::vector<std::pair<void*, size_t>> weight_buffers(csm_engine* e) {
  std::vector<std::pair<void*, size_t>> b;
  for (Stack* s : {&e->bb, &e->dec}) {
    const size_t D = s->d.hidden, F = s->d.intermediate;
    b.emplace_back(s->norm, D * 4);
    for (LayerW& l : s->L) {
      b.emplace_back(l.wqkv, e->wbytes(s->qkv_rows(), D));
      b.emplace_back(l.wo, e->wbytes(D, s->q_dim()));
      b.emplace_back(l.wgu, e->wbytes(2 * F, D));
      b.emplace_back(l.wd, e->wbytes(D, F));
      if (l.wdc) b.emplace_back(l.wdc, D * F * 2);
      b.emplace_back(l.n1, D * 4);
      b.emplace_back(l.n2, D * 4);
    }
  }
  const size_t D = e->D, Dd = e->Dd, V = e->V, K = e->K, Vp = e->Vpad;
  b.emplace_back(e->text_emb, e->wbytes(e->dims.n_text_vocab, D));
  b.emplace_back(e->audio_emb, e->wbytes(V * K, D));
  b.emplace_back(e->proj, e->wbytes(Dd, D));
  b.emplace_back(e->c0_head, e->wbytes(Vp, D));
  b.emplace_back(e->audio_head, (K - 1) * Vp * Dd * (e->head_wdt == WDT_F32 ? 4 : 2));
  return b;
}

int csm_weight_buffers(csm_engine* e, void** ptrs, uint64_t* bytes, int cap, int* n) {
  CSM_TRY {
    if (!e || !n || cap < 0) throw CsmError(CSM_ERR_ARG, "bad csm_weight_buffers arguments");
    const auto b = weight_buffers(e);
    *n = (int)b.size();
    for (int i = 0; i < cap && i < (int)b.size(); ++i) {
      if (ptrs) ptrs[i] = b[i].first;
      if (bytes) bytes[i] = b[i].second;
    }
  }
  CSM_CATCH
}

int csm_weights_received(csm_engine* e) {
  CSM_TRY {
    HIPCHK(hipSetDevice(e->dev));
    HIPCHK(hipDeviceSynchronize());
    for (const auto& nm : e->required) e->loaded.insert(nm);
    e->tiled_dirty = true;
    e->proj_tab_dirty = true;
    ++e->weights_epoch;
    e->g_B = -1;
  }
  CSM_CATCH
}

int csm_quantize(csm_engine* e, int group_size, int bits) {
  CSM_TRY {
    if (group_size != Q4_GROUP || bits != 4) throw CsmError(CSM_ERR_ARG, "only group_size=64, bits=4 is supported");
    if (e->wdt == WDT_Q4) return CSM_OK;  // already quantized (nn.quantize on a quantized model is a no-op here)
    HIPCHK(hipSetDevice(e->dev));
    HIPCHK(hipDeviceSynchronize());
    const int old = e->wdt;
    // every Linear / Embedding matrix, whole (all rows of fused / interleaved layouts): row order kept
    std::vector<std::tuple<void**, int, int>> mats;
    for (Stack* s : {&e->bb, &e->dec})
      for (LayerW& l : s->L) {
        const int D = s->d.hidden, F = s->d.intermediate;
        mats.emplace_back(&l.wqkv, s->qkv_rows(), D);
        mats.emplace_back(&l.wo, D, s->q_dim());
        mats.emplace_back(&l.wgu, 2 * F, D);
        mats.emplace_back(&l.wd, D, F);
      }
    mats.emplace_back(&e->text_emb, e->dims.n_text_vocab, e->D);
    mats.emplace_back(&e->audio_emb, e->V * e->K, e->D);
    mats.emplace_back(&e->proj, e->Dd, e->D);
    mats.emplace_back(&e->c0_head, e->Vpad, e->D);
    for (auto& [pp, N, Kd] : mats)
      if (!gemv_q4_supported(N, Kd)) throw CsmError(CSM_ERR_ARG, "int4 GEMV does not support this shape");
    // the bf16 chunk-major down_proj copies serve only the bf16 persistent kernels: freed, so an
    // nn.quantize'd engine lists the same weight buffers as one created as CSM_Q4 (csm_weight_buffers)
    for (Stack* s : {&e->bb, &e->dec})
      for (LayerW& l : s->L)
        if (l.wdc) { e->release(l.wdc); l.wdc = nullptr; }
    for (auto& [pp, N, Kd] : mats) {
      void* q = e->alloc(q4_bytes(N, Kd));
      launch_q4_quantize(*pp, old, N, Kd, q, N, 0, 1, e->st);
      HIPCHK(hipStreamSynchronize(e->st));
      HIPCHK(hipGetLastError());
      e->release(*pp);
      *pp = q;
    }
    e->head_wdt = old;
    e->wdt = WDT_Q4;
    e->proj_tab_dirty = true;
    for (void* t : e->tiled_bufs) e->release(t);  // re-sized for int4 at the next csm_begin
    e->tiled_bufs.clear();
    e->ws.tiled.clear();
    e->tiled_dirty = true;
    ++e->weights_epoch;
    e->g_B = -1;
  }
  CSM_CATCH
}

}  // extern "C"
