// CSM engine: device-resident weights, KV caches and the graph-captured frame loop behind
// the C ABI of include/csm_hip.h.
//
// One frame (generation.py:21-92) is two captured HIP graphs replayed back to back:
//   body : embed(previous codes) -> 16 backbone layers (M = B rows) -> final RMSNorm -> h_last
//   head : c0 head -> sample c0 (+ gather decoder rows) -> 31 x [projection -> 4 decoder layers
//          -> ci head -> sample ci (+ gather next row)] -> advance (history, EOS, frame counter)
// All per-frame state (positions, codes, frame counter) lives in device memory so the same
// graphs replay every frame without host involvement; the host only polls EOS flags.
//
// This file holds the frame paths: the block stacks, the predicates that select among the execution
// paths (the *_eligible functions and plan_step), the body / head enqueue and graph capture.  The other
// engine sources are listed in csm_engine.h.
#include "csm_engine.h"

// One Llama block stack over M rows of the residual stream x (in place).
// gather0: x-gather fields for layer 0's QKV GEMV (its input rows come from a table; the GEMV also
// writes them to x as the residual stream).
void run_stack(csm_engine* e, Stack& s, float* x, int M, float* q, float* att, float* mlp, const RowMap& rm,
               hipStream_t st, const GemvParams* gather0, const AttnParams* attn0) {
  const csm_llama_dims& d = s.d;
  const int tag = (&s == &e->dec) ? 1 : 0;
  const int D = d.hidden, F = d.intermediate, hd = d.head_dim, Hq = d.n_heads, Hkv = d.n_kv_heads;
  for (int i = 0; i < d.n_layers; ++i) {
    LayerW& l = s.L[i];
    GemvParams g = gp(e);
    // norm1 + QKV + RoPE + KV append
    g.W = l.wqkv; g.N = s.qkv_rows(); g.K = D; g.x = x; g.xs = D; g.M = M; g.nw = l.n1; g.eps = d.eps;
    g.out = q; g.os = s.q_dim(); g.Hq = Hq; g.Hkv = Hkv; g.hd = hd; g.S_cap = s.S_cap; g.rope = s.rope;
    g.kc = l.kc; g.vc = l.vc; g.rm = rm;
    if (i == 0 && gather0) {
      g.xpart = gather0->xpart; g.xpart_stride = gather0->xpart_stride; g.xpart_n = gather0->xpart_n;
      g.xtab = gather0->xtab; g.xtab_f32 = gather0->xtab_f32; g.xV = gather0->xV; g.xcb = gather0->xcb;
      g.x_codes = gather0->x_codes; g.x_codes_K = gather0->x_codes_K; g.x_copy = x;
    }
    const bool gathered = (i == 0 && attn0);  // layer 0 QKV from the folded table (attention gathers it)
    if (!gathered) launch_gemv(g, e->wdt, EPI_QKV, 1, st, tag);
    // attention, then o_proj + residual
    AttnParams a = gathered ? *attn0 : AttnParams{};
    a.q = q; a.qs = s.q_dim(); a.M = M; a.kc = l.kc; a.vc = l.vc; a.Hq = Hq; a.Hkv = Hkv; a.S_cap = s.S_cap;
    a.scale = 1.0f / sqrtf((float)hd); a.mode = ATTN_CAUSAL; a.window = 0; a.rm = rm; a.out = att;
    a.os = s.q_dim();
    g = gp(e);
    g.W = l.wo; g.N = D; g.K = s.q_dim(); g.x = att; g.xs = s.q_dim(); g.M = M; g.out = x; g.os = D;
    launch_attn(a, hd, st);
    launch_gemv(g, e->wdt, EPI_ADD, 0, st, tag);
    // norm2 + gate/up + SiLU*up
    g = gp(e);
    g.W = l.wgu; g.N = 2 * F; g.K = D; g.x = x; g.xs = D; g.M = M; g.nw = l.n2; g.eps = d.eps; g.out = mlp;
    g.os = F;
    launch_gemv(g, e->wdt, EPI_SILU_MUL, 1, st, tag);
    // down + residual
    g = gp(e);
    g.W = l.wd; g.N = D; g.K = F; g.x = mlp; g.xs = F; g.M = M; g.out = x; g.os = D;
    launch_gemv(g, e->wdt, EPI_ADD, 0, st, tag);
  }
}

namespace {

// The conditions the streaming matrix-core GEMM (gemm_xs.hip) puts on a block stack of M rows
bool stack_xs_eligible(csm_engine* e, const Stack& s, int M) {
  const int D = s.d.hidden, F = s.d.intermediate;
  return e->xs_on && e->xs_D && M >= GEMM_MFMA_MIN_M && M <= GEMM_XS_MAX_M && (e->wdt == WDT_BF16 || e->wdt == WDT_Q4) &&
         gemm_xs_eligible(s.qkv_rows(), D, M, e->wdt) && gemm_xs_eligible(D, s.q_dim(), M, e->wdt) &&
         gemm_xs_eligible(2 * F, D, M, e->wdt) && gemm_xs_eligible(D, F, M, e->wdt) && gemm_xs_tiles(D, F, M) <= 64 &&
         gemm_xs_tiles(D, s.q_dim(), M) <= 64;
}

// The batched depth decoder at codebook steps >= 2 (generation.py:72-89 at batch M) on the streaming
// stack, its head included.
bool dec_xs_eligible(csm_engine* e, int M) {
  const Stack& s = e->dec;
  const int Dd = s.d.hidden;
  return stack_xs_eligible(e, s, M) && e->head_wdt == WDT_BF16 && s.d.head_dim == 128 && s.S_cap <= 32 &&
         gemm_xs_eligible(e->Vpad, Dd, M, e->head_wdt) &&
         // the next step's row gather reads head_blocks() arg-max partials per row: the streaming head
         // must write exactly that many (one per 64-row tile)
         gemm_xs_tiles(e->Vpad, Dd, M, true) == head_blocks(e->Vpad, Dd, M, e->head_wdt);
}

// The batched backbone step (generation.py:39 at batch M, one decode row per utterance) on the streaming
// stack: the embedding gather writes split rows (x * n1[0]) + per-512-column sums of squares.
bool bb_xs_eligible(csm_engine* e, int M) {
  const int D = e->bb.d.hidden;
  return stack_xs_eligible(e, e->bb, M) && D % 512 == 0 && D / 512 <= 64;
}

// A block stack on the streaming matrix-core GEMM (gemm_xs.hip): every projection's epilogue (and the
// attention) writes the split activations of the next one (xs.h) -- o_proj: the new residual x * n2 (+
// per-row sums of squares), gate/up: SiLU*up, down: the new residual x * next layer's n1 -- so no launch
// re-normalises or re-splits rows.  Layer 0 reads the split rows its caller wrote (xs_D, ss_n0 sums of
// squares per row), or with l0_qkv false gathers q | k | v and its input row from the folded tables (attn0).
struct XsStack {
  Stack& s;
  float *x, *q, *att;  // fp32 residual stream, q rows, attention output
  bool nt;             // non-temporal weight loads
  bool l0_qkv;         // layer 0 projects its q | k | v
  int ss_n0;           // sums-of-squares slots per row of layer 0's input
  bool head_rows;      // the last down writes split rows x * final norm for a streaming head
};
void run_stack_xs(csm_engine* e, const XsStack& v, int M, const RowMap& rm, hipStream_t st, const AttnParams& attn0) {
  Stack& s = v.s;
  const csm_llama_dims& d = s.d;
  const int D = d.hidden, F = d.intermediate;
  const int ss_o = gemm_xs_tiles(D, s.q_dim(), M), ss_d = gemm_xs_tiles(D, F, M);
  const bool q4 = e->wdt == WDT_Q4;  // int4 consumers also read the half-group sums of their operand
  float* hsD = q4 ? e->hs_D : nullptr;
  float* hsA = q4 ? e->hs_A : nullptr;
  float* hsF = q4 ? e->hs_F : nullptr;
  for (int i = 0; i < d.n_layers; ++i) {
    LayerW& l = s.L[i];
    if (i > 0 || v.l0_qkv) {  // norm1 + QKV + RoPE + KV append from the split rows the previous down wrote
      GemvParams g = gp(e);
      g.W = l.wqkv; g.N = s.qkv_rows(); g.K = D; g.M = M; g.nw = l.n1; g.eps = d.eps;
      g.out = v.q; g.os = s.q_dim(); g.Hq = d.n_heads; g.Hkv = d.n_kv_heads; g.hd = d.head_dim;
      g.S_cap = s.S_cap; g.rope = s.rope; g.kc = l.kc; g.vc = l.vc; g.rm = rm;
      g.xs_in = e->xs_D; g.ss_in = e->xs_ss; g.ss_n = i == 0 ? v.ss_n0 : ss_d; g.ss_stride = GEMM_XS_MAX_M; g.hs_in = hsD;
      launch_gemm_xs(g, EPI_QKV, st, v.nt, e->wdt);
    }
    AttnParams a = i == 0 ? attn0 : AttnParams{};
    a.q = v.q; a.qs = s.q_dim(); a.M = M; a.kc = l.kc; a.vc = l.vc; a.Hq = d.n_heads; a.Hkv = d.n_kv_heads;
    a.S_cap = s.S_cap; a.scale = 1.0f / sqrtf((float)d.head_dim); a.mode = ATTN_CAUSAL; a.window = 0; a.rm = rm;
    a.out = v.att; a.os = s.q_dim(); a.xs_out = e->xs_A; a.xs_K = s.q_dim(); a.hs_out = hsA;
    launch_attn(a, d.head_dim, st);
    {  // o_proj + residual -> x; split (x * n2) + sums of squares for gate/up
      GemvParams g = gp(e);
      g.W = l.wo; g.N = D; g.K = s.q_dim(); g.M = M; g.out = v.x; g.os = D; g.xs_in = e->xs_A;
      g.xs_out = e->xs_D; g.xs_nw = l.n2; g.ss_out = e->xs_ss; g.ss_stride = GEMM_XS_MAX_M; g.xs_K = D;
      g.hs_in = hsA; g.hs_out = hsD;
      launch_gemm_xs(g, EPI_ADD, st, v.nt, e->wdt);
    }
    {  // norm2 + gate/up + SiLU*up -> split h
      GemvParams g = gp(e);
      g.W = l.wgu; g.N = 2 * F; g.K = D; g.M = M; g.nw = l.n2; g.eps = d.eps; g.out = nullptr; g.os = F;
      g.xs_in = e->xs_D; g.ss_in = e->xs_ss; g.ss_n = ss_o; g.ss_stride = GEMM_XS_MAX_M;
      g.xs_out = e->xs_F; g.xs_K = F; g.hs_in = hsD; g.hs_out = hsF;
      launch_gemm_xs(g, EPI_SILU_MUL, st, v.nt, e->wdt);
    }
    {  // down + residual -> x; split (x * next norm) + sums of squares (without head_rows the last layer's
       // rows go to the final norm in fp32 only)
      GemvParams g = gp(e);
      g.W = l.wd; g.N = D; g.K = F; g.M = M; g.out = v.x; g.os = D; g.xs_in = e->xs_F; g.hs_in = hsF;
      if (i + 1 < d.n_layers || v.head_rows) {
        g.xs_out = e->xs_D; g.xs_nw = i + 1 < d.n_layers ? s.L[i + 1].n1 : s.norm; g.ss_out = e->xs_ss;
        g.ss_stride = GEMM_XS_MAX_M; g.xs_K = D; g.hs_out = hsD;
      }
      launch_gemm_xs(g, EPI_ADD, st, v.nt, e->wdt);
    }
  }
}

// l0_qkv: step 1, whose rows launch_xs_rows split after the projection
void run_dec_xs(csm_engine* e, int M, const RowMap& rm, hipStream_t st, const AttnParams& attn0, bool l0_qkv = false) {
  run_stack_xs(e, XsStack{e->dec, e->dx, e->dq, e->datt, false, l0_qkv, (e->Dd + 511) / 512, true}, M, rm, st, attn0);
}

void run_bb_xs(csm_engine* e, int M, const RowMap& rm, hipStream_t st) {
  run_stack_xs(e, XsStack{e->bb, e->x, e->q, e->att, gemv_nt(0), true, e->D / 512, false}, M, rm, st, AttnParams{});
}

// Layer weights, norms, caches and hand-off state of a persistent kernel's argument block (BbStepArgs and
// DecFrameArgs share these fields)
template <class Args>
void fill_persistent(Args& a, csm_engine* e, const Stack& s, int n_layers, const Handoff& h) {
  for (int l = 0; l < n_layers; ++l) {
    const LayerW& w = s.L[l];
    a.wqkv[l] = (const bf16_t*)w.wqkv; a.wo[l] = (const bf16_t*)w.wo; a.wgu[l] = (const bf16_t*)w.wgu;
    a.wdc[l] = (const bf16_t*)(e->wdt == WDT_Q4 ? w.wdq : w.wdc); a.n1[l] = w.n1; a.n2[l] = w.n2; a.kc[l] = w.kc; a.vc[l] = w.vc;
  }
  a.norm = s.norm; a.rope = s.rope; a.S_cap = s.S_cap; a.eps = s.d.eps;
  a.gbuf = (unsigned long long*)h.buf; a.epoch = h.epoch; a.err = h.err; a.stamps = h.stamps;
}

// The chunk-major down copies the batch-1 persistent kernels read (the int4 ones are rebuilt at csm_begin)
bool has_down_copies(csm_engine* e, const Stack& s) {
  const bool q4 = e->wdt == WDT_Q4;
  for (const LayerW& l : s.L)
    if (!(q4 ? l.wdq : l.wdc)) return false;
  return !(q4 && e->tiled_dirty);
}

// codes are final: EOS test, history, frame counter
AdvanceParams advance_params(csm_engine* e) {
  AdvanceParams ap{};
  ap.codes = e->codes; ap.hist = e->hist; ap.F_cap = e->F_cap; ap.B = e->B; ap.K = e->K; ap.V = e->V; ap.done = e->done;
  ap.n_frames = e->n_frames; ap.frame_ctr = e->frame_ctr; ap.slot_frame = e->slot_frame;
  return ap;
}

}  // namespace

void embed(csm_engine* e, const EmbedParams& ep, int M, hipStream_t st) {
  if (e->wdt == WDT_Q4) launch_embed_q4(ep, e->dims.n_text_vocab, M, st);
  else launch_embed(ep, e->wdt, M, st);
}

// The persistent backbone step runs the 16 blocks + final norm of a batch-1 decode row when the
// engine has csm_1b's backbone shapes in bf16 or int4 (with the chunk-major down copies) and the device
// has the 256 CUs its one-workgroup-per-CU grid assumes.
bool bb_step_eligible(csm_engine* e) {
  Handoff& h = e->h_bb;
  if (!h.on || !h.buf || e->B != 1 || (e->wdt != WDT_BF16 && e->wdt != WDT_Q4)) return false;
  const csm_llama_dims& d = e->bb.d;
  if (d.hidden != 2048 || d.intermediate != 8192 || d.n_heads != 32 || d.n_kv_heads != 8 || d.head_dim != 64 ||
      d.n_layers != BB_STEP_LAYERS)
    return false;
  if (!has_down_copies(e, e->bb)) return false;
  return h.resident(e->dev, e->wdt == WDT_Q4, bb_step_kernel_ptr, BB_STEP_WGS, BB_STEP_THREADS);
}

void enqueue_bb_step(csm_engine* e, hipStream_t st) {
  BbStepArgs a{};
  fill_persistent(a, e, e->bb, BB_STEP_LAYERS, e->h_bb);
  a.x = e->x; a.pos = e->pos; a.h_last = e->h_last;
  launch_bb_step(a, st, e->wdt == WDT_Q4);
}

void enqueue_body(csm_engine* e, hipStream_t st) {
  const int B = e->B;
  EmbedParams ep{};
  ep.codes = e->codes; ep.text_emb = e->text_emb; ep.audio_emb = e->audio_emb; ep.V = e->V; ep.K = e->K;
  ep.D = e->D; ep.out = e->x; ep.pos_inc = e->pos; ep.parked = e->parked;
  // batched backbone rows on the streaming GEMM (round 4 default; option bb_xs / CSM_BB_XS=0: gemm_wide)
  const bool bb_xs = e->bb_xs_on && !bb_step_eligible(e) && bb_xs_eligible(e, B);
  if (bb_xs) {
    ep.xs_out = e->xs_D; ep.xs_nw = e->bb.L[0].n1; ep.ss_out = e->xs_ss; ep.ss_stride = GEMM_XS_MAX_M;
    ep.hs_out = e->wdt == WDT_Q4 ? e->hs_D : nullptr;
  }
  embed(e, ep, B, st);
  if (bb_step_eligible(e)) {
    enqueue_bb_step(e, st);
    return;
  }
  RowMap rm{1, 0, e->pos, 0};
  if (bb_xs) run_bb_xs(e, B, rm, st);
  else run_stack(e, e->bb, e->x, B, e->q, e->att, e->mlp, rm, st);
  launch_rmsnorm_rows(e->x, e->D, e->bb.norm, e->bb.d.eps, e->D, e->h_last, e->D, B, st);
}

// The persistent frame decoder runs the whole head of a batch-1 frame (greedy, or sampled: its heads
// then hand every logit to every workgroup, which runs the sampler's top-k + Gumbel-max) when the engine has
// csm_1b's decoder shapes in bf16 or int4 and the folded tables, and the device has the 256 CUs its grid of
// one workgroup per CU assumes.
bool dec_frame_eligible(csm_engine* e) {
  Handoff& h = e->h_df;
  if (e->slot_mode) return false;  // its sampler counter and c0 window read the global frame index
  if (!h.on || e->B != 1 || (e->wdt != WDT_BF16 && e->wdt != WDT_Q4) || e->head_wdt != WDT_BF16) return false;
  if (frame_plan(e).filtered) return false;  // filters: sample_filtered_kernel
  if (!csm1b_decoder(e->dec.d) || e->dec.d.n_layers != DEC_FRAME_LAYERS || e->bb.d.hidden != 2048 || e->V <= 2048 ||
      e->V > 2051 || e->K > 32 || e->dec.S_cap != e->K)
    return false;
  if (!has_down_copies(e, e->dec)) return false;
  if (!e->proj_tab || !e->fold_proj || !e->use_qkv0_tab || !e->qkv0_built || e->proj_tab_dirty) return false;
  return h.resident(e->dev, e->wdt == WDT_Q4, dec_frame_kernel_ptr, DEC_FRAME_WGS, DEC_FRAME_THREADS);
}

void enqueue_dec_frame_only(csm_engine* e, hipStream_t st) {
  DecFrameArgs a{};
  fill_persistent(a, e, e->dec, DEC_FRAME_LAYERS, e->h_df);
  a.c0_head = (const bf16_t*)e->c0_head; a.proj = (const bf16_t*)e->proj; a.audio_head = (const bf16_t*)e->audio_head;
  a.proj_tab = e->proj_tab; a.qkv0_tab = e->qkv0_tab; a.h_last = e->h_last;
  a.V = e->V; a.VP = e->Vpad; a.K = e->K; a.codes = e->codes; a.c0_logits = e->c0_logits; a.ci_logits = e->ci_logits;
  // (wnt / hnt stay zero: no kernel reads them any more)
  const SlotSampling& s = e->batch;
  a.temperature = s.temperature; a.top_k = s.top_k; a.seeds = e->seeds; a.frame_ctr = e->frame_ctr;
  a.c0_bias = s.bias ? e->c0_bias : nullptr; a.hist = e->hist; a.c0_penalty = s.penalty; a.c0_context = s.context;
  launch_dec_frame(a, st, e->wdt == WDT_Q4);
}

// The persistent batched decoder step (dec_step_xs.hip) runs a codebook step >= 2 of the streaming
// matrix-core path when the decoder has csm_1b's shapes in bf16 or int4, the rows fit one 32-row tile (int4:
// 64 rows) and the device holds one 512-thread workgroup on each of its 256 CUs.
bool xsd_eligible(csm_engine* e, int M) {
  Handoff& h = e->h_xsd;
  const bool q4 = e->wdt == WDT_Q4;
  if (!h.on || !h.buf || M < 1 || M > (q4 ? DEC_XSD_MAX_M_Q4 : DEC_XSD_MAX_M) || (e->wdt != WDT_BF16 && !q4) ||
      e->head_wdt != WDT_BF16 || e->tiled_dirty || GEMM_XS_MAX_M != 64)
    return false;
  if (!csm1b_decoder(e->dec.d) || e->dec.d.n_layers != DEC_FRAME_LAYERS || e->dec.S_cap > 32) return false;
  return h.resident(e->dev, q4, dec_step_xs_kernel_ptr, DEC_XSD_WGS, DEC_XSD_THREADS);
}

// The fragment-tiled copy of step i's head when the persistent step can run it in its own launch (option
// dec_xsd_head): 64-row tiles, one arg-max partial each -- the launch path's partial count.  Null otherwise.
const void* xsd_head_tiled(csm_engine* e, int M, int i) {
  const int Vp = e->Vpad, ht = (Vp + 63) / 64;
  auto it = e->ws.tiled.find((const char*)e->audio_head + (size_t)(i - 1) * Vp * e->Dd * 2);
  // (int4: the head's (tile, row tile) pairs on the 64 attention + 32 plain workgroups: <= 48 tiles)
  const bool fits = e->xsd_head && it != e->ws.tiled.end() && ht == head_blocks(Vp, e->Dd, M, e->head_wdt) &&
                    ht <= (e->wdt == WDT_Q4 ? 48 : 64);
  return fits ? it->second : nullptr;
}

// step i >= 2 of the batched decoder: M rows (utterances 0..M-1) at position i; the codes of codebook
// i - 1 come from the head partials part_prev (part_n per row).  head_tiled (xsd_head_tiled): the step's
// head runs in the same launch (its logits, and arg-max partials in part_out, are written); sample: and the
// sampler.
void launch_xsd(csm_engine* e, int M, int i, const unsigned long long* part_prev, int part_n, unsigned long long* part_out,
                hipStream_t st, const void* head_tiled, bool sample) {
  DecStepXsArgs a = e->xsd;
  const Stack& s = e->dec;
  for (int l = 0; l < DEC_FRAME_LAYERS; ++l) {
    const LayerW& w = s.L[l];
    a.wqkv[l] = (const uint8_t*)e->ws.tiled.at(w.wqkv); a.wo[l] = (const uint8_t*)e->ws.tiled.at(w.wo);
    a.wgu[l] = (const uint8_t*)e->ws.tiled.at(w.wgu); a.wd[l] = (const uint8_t*)e->ws.tiled.at(w.wd);
    a.n1[l] = w.n1; a.n2[l] = w.n2; a.kc[l] = w.kc; a.vc[l] = w.vc;
  }
  a.norm = s.norm; a.rope = s.rope; a.S_cap = s.S_cap; a.eps = s.d.eps;
  a.M = M; a.step = i;
  a.part = part_prev; a.part_stride = e->part_stride; a.part_n = part_n; a.V = e->V;
  a.qkv0_tab = e->qkv0_tab + (size_t)(i - 1) * e->V * s.qkv_rows();
  a.proj_tab = e->proj_tab + (size_t)(i - 1) * e->V * e->Dd;
  a.codes = e->codes; a.codes_K = e->K;
  a.xs_out = e->xs_D; a.ss_out = e->xs_ss; a.ss_stride = GEMM_XS_MAX_M;
  a.hs_out = e->hs_D;  // (int4: the half-group sums of xs_out)
  const Handoff& h = e->h_xsd;
  a.ctrl = (unsigned*)h.buf; a.epoch = h.epoch; a.err = h.err; a.stamps = h.stamps;
  if (head_tiled) {
    const int Vp = e->Vpad;
    a.head_w = (const uint8_t*)head_tiled; a.head_nt32 = (Vp + 31) / 32; a.head_tiles = (Vp + 63) / 64; a.Vp = Vp; a.n_valid = e->V;
    a.head_out = e->ci_logits + (size_t)(i - 1) * e->B * Vp; a.head_part = part_out;
    if (sample) {
      a.sample = 1; a.s_top_k = e->batch.top_k; a.s_K = e->K; a.s_cb = i; a.s_temperature = e->batch.temperature;
      a.s_seeds = e->seeds; a.s_slot_frame = e->slot_frame;
      a.s_slots = e->per_slot ? e->slot_sampling : nullptr;
    }
  }
  launch_dec_step_xs(a, st, e->wdt == WDT_Q4);
}

// A hand-off wait of a persistent kernel that timed out leaves its flag raised: report it.
// Every raised flag is cleared and named in the one error.
void check_handoffs(csm_engine* e) {
  std::string who;
  for (Handoff* h : e->handoffs()) {
    if (!h->err) continue;
    int v = 0;
    HIPCHK(hipMemcpy(&v, h->err, 4, hipMemcpyDeviceToHost));
    if (v) {
      HIPCHK(hipMemset(h->err, 0, 4));
      if (h == &e->h_xsd) {  // counters and flags are out of step with the epoch: start both afresh
        // (no synchronise follows these null-stream fills: ADVICE.md, the xsd reset item)
        HIPCHK(hipMemset(h->buf, 0, dec_step_xs_ctrl_bytes()));
        HIPCHK(hipMemset(h->epoch, 0, 4));
      }
      who += std::string(who.empty() ? "" : " and ") + h->name;
    }
  }
  if (!who.empty()) throw CsmError(CSM_ERR_HIP, who + ": a hand-off wait timed out (results of this batch are invalid)");
}

namespace {

// How codebook step i of the head runs: decided once per step from the engine's state, then
// enqueue_head_phase only dispatches on it.  This and the *_eligible predicates above are the one place
// where the execution path is selected.
struct StepPlan {
  int M;        // rows: two per utterance at step 1, one after
  bool folded;  // steps >= 2 read projection(E_a[c]) from the folded table instead of projecting
  enum Rows {
    ROWS_GEMV,    // layer 0's QKV GEMV gathers its input rows itself (after the projection GEMV when not folded)
    ROWS_DENSE,   // batched: the gathered rows are materialised densely, every projection runs on the matrix cores
    ROWS_TABLES,  // layer 0's q | k | v and input row are gathered from the folded tables by the attention
  } rows;
  enum Blocks {
    BLOCKS_STACK,       // run_stack: one GEMV / GEMM launch per projection
    BLOCKS_STREAMING,   // run_dec_xs: the streaming matrix-core stack
    BLOCKS_PERSISTENT,  // launch_xsd: the four layers in one persistent launch
  } blocks;
  enum Head {
    HEAD_GEMV,       // launch_gemv on the fp32 rows
    HEAD_STREAMING,  // launch_gemm_xs on the split rows the last down wrote
    HEAD_IN_STEP,    // written by the persistent step's launch
  } head;
  const void* head_tiled;  // HEAD_IN_STEP: the head's fragment-tiled copy
  bool sample_in_step;     // the persistent step's launch samples too (no sample kernel follows)
};

StepPlan plan_step(csm_engine* e, int i, bool fuse_sample) {
  StepPlan p{};
  const int D = e->D, Dd = e->Dd;
  p.M = (i == 1) ? 2 * e->B : e->B;
  p.folded = i >= 2 && e->proj_tab && e->fold_proj;
  const bool use_tab = p.folded && e->use_qkv0_tab && e->qkv0_built && !e->no_tab_batched;
  if (!use_tab && (gemm_mfma_eligible(Dd, D, p.M, e->wdt) || gemm_mfma_eligible(e->dec.qkv_rows(), Dd, p.M, e->wdt))) {
    p.rows = StepPlan::ROWS_DENSE;
    // step 1 (two rows per utterance) on the streaming GEMM too: the projected rows split once, layer 0's
    // QKV projected from them; the head stays on the dense path (it reads one row of each pair)
    const bool xs_s1 = i == 1 && !p.folded && e->xs_step1 && dec_xs_eligible(e, p.M) && Dd % 512 == 0;
    p.blocks = xs_s1 ? StepPlan::BLOCKS_STREAMING : StepPlan::BLOCKS_STACK;
  } else if (use_tab) {
    p.rows = StepPlan::ROWS_TABLES;
    if (dec_xs_eligible(e, p.M)) {  // streaming matrix-core decoder + head
      p.blocks = xsd_eligible(e, p.M) ? StepPlan::BLOCKS_PERSISTENT : StepPlan::BLOCKS_STREAMING;
      p.head = StepPlan::HEAD_STREAMING;
    }
    if (p.blocks == StepPlan::BLOCKS_PERSISTENT && (p.head_tiled = xsd_head_tiled(e, p.M, i))) {
      p.head = StepPlan::HEAD_IN_STEP;
      // the sampled step's sampler in the same launch (option dec_xsd_sample; V within the sampler's reach)
      p.sample_in_step = fuse_sample && e->xsd_sample && e->V <= DEC_XSD_THREADS * DEC_XSD_SAMPLE_NPT;
    }
  }
  return p;
}

}  // namespace

FramePlan frame_plan(const csm_engine* e) {
  FramePlan f{};
  f.per_slot = e->per_slot;
  auto need = [&f](const SlotSampling& s) {
    f.sampled |= s.temperature > 0.f;
    f.filtered |= s.temperature > 0.f && (s.use_top_p || s.use_min_p);
    f.processors |= s.bias != 0 || s.penalty > 0.f;
  };
  if (!e->per_slot) {
    need(e->batch);
    return f;
  }
  for (int b = 0; b < e->B; ++b)
    if (!e->parked_host[b]) need(e->samp_own[b] ? e->samp_host[b] : e->batch);
  return f;
}

void enqueue_head_phase(csm_engine* e, hipStream_t st, HeadPhase phase, int piece) {
  if (phase == HeadPhase::Frame && dec_frame_eligible(e)) {
    enqueue_dec_frame_only(e, st);
    launch_advance(advance_params(e), st);
    return;
  }
  const int B = e->B, K = e->K, D = e->D, Dd = e->Dd, V = e->V, Vp = e->Vpad;
  const FramePlan fp = frame_plan(e);
  const SlotSampling* slots = fp.per_slot ? e->slot_sampling : nullptr;  // the kernels read row b's values from it
  const bool host_codes = phase == HeadPhase::Forced || phase == HeadPhase::HostPiece;  // fed forward from e->force
  const bool greedy = !fp.sampled && !host_codes;
  // the frame's own logits processors (csm_set_c0_processors) transform the stored c0 logits before c0 is picked
  const bool c0_proc = phase == HeadPhase::Frame && fp.processors;
  const bool c0_sampled = !greedy || phase == HeadPhase::FromHostC0 || c0_proc;  // c0 published by sample_kernel as a single partial
  // sampled frames (top-k only): the persistent step's launch can run the sampler too
  const bool fuse_sample = !greedy && (phase == HeadPhase::Frame || phase == HeadPhase::FromHostC0) && !fp.filtered;
  const int n0 = head_blocks(Vp, D, B, e->wdt);        // c0-head blocks (partials per row)
  const int ni = head_blocks(Vp, Dd, B, e->head_wdt);  // ci-head blocks
  auto part = [&](int cb) { return e->part + (size_t)cb * e->B_max * e->part_stride; };
  SampleParams sp{};
  sp.ls = Vp; sp.V = V; sp.seeds = e->seeds; sp.slot_frame = e->slot_frame; sp.K = K; sp.codes = e->codes;
  sp.part_stride = e->part_stride; sp.slots = slots;
  {  // (the batch's values as scalars: csm_kernels.h SampleParams)
    const SlotSampling& s = e->batch;
    sp.temperature = s.temperature; sp.top_k = s.top_k; sp.use_top_p = s.use_top_p; sp.use_min_p = s.use_min_p;
    sp.min_keep = s.min_keep; sp.top_p_cut = s.top_p_cut; sp.log_min_p = s.log_min_p;
  }
  sp.forced = host_codes ? e->force : nullptr;
  // c0 = codebook0_head(h_last) (generation.py:42); greedy arg-max fused into the GEMV epilogue
  GemvParams g = gp(e);
  g.W = e->c0_head; g.N = Vp; g.K = D; g.x = e->h_last; g.xs = D; g.M = B; g.out = e->c0_logits; g.os = Vp;
  g.part = part(0); g.part_stride = e->part_stride; g.n_valid = V;
  if (phase != HeadPhase::FromHostC0 && phase != HeadPhase::HostPiece)
    launch_gemv(g, e->wdt, (greedy && phase == HeadPhase::Frame && !c0_proc) ? EPI_ARGMAX : EPI_STORE, 0, st);
  if (phase == HeadPhase::C0Logits) return;
  if (c0_proc) {
    C0ProcessParams cp{};
    cp.logits = e->c0_logits; cp.ls = Vp; cp.V = V; cp.hist = e->hist; cp.B = B; cp.K = K; cp.F_cap = e->F_cap;
    cp.frame_ctr = e->frame_ctr; cp.slot_frame = e->slot_frame;
    cp.batch = e->batch; cp.slots = slots; cp.bias = e->c0_bias; cp.slot_bias = e->slot_bias;
    launch_c0_process(cp, st);
  }
  const bool pieces = phase == HeadPhase::HostPiece;
  const int cb_first = pieces ? piece - 1 : 0;  // the code fed forward before the first step below
  if (c0_sampled) {
    sp.logits = e->c0_logits; sp.cb = cb_first; sp.part = part(cb_first);
    launch_sample(sp, B, fp.filtered, st);
  }
  const int i_lo = pieces ? piece : 1, i_hi = pieces ? std::min(piece + 1, K) : K;
  for (int i = i_lo; i < i_hi; ++i) {
    const StepPlan plan = plan_step(e, i, fuse_sample);
    const int M = plan.M;
    // decoder(projection(decoder_inputs)) (generation.py:74-77): the projection gathers its input
    // rows itself -- [h_last, E_a[c0]] at step 1 (:62-64), E_a[c_{i-1} + V*(i-1)] after (:87-89)
    g = gp(e);
    g.W = e->proj; g.N = Dd; g.K = D; g.x = e->h_last; g.xs = D; g.M = M; g.out = e->dx; g.os = Dd;
    g.xpart = part(i - 1); g.xpart_stride = e->part_stride; g.xpart_n = i == 1 ? (c0_sampled ? 1 : n0) : (greedy ? ni : 1);
    g.xtab = e->audio_emb; g.xV = V; g.xcb = i - 1; g.x_step1 = (i == 1); g.x_codes = e->codes; g.x_codes_K = K;
    g.xtab_q4_rows = e->wdt == WDT_Q4 ? V * K : 0;
    GemvParams g0 = g;  // steps >= 2: layer 0 gathers projection(E_a[c]) from the folded table
    g0.xtab = e->proj_tab; g0.xtab_f32 = 1; g0.xtab_q4_rows = 0;
    RowMap rm = (i == 1) ? RowMap{2, 0, nullptr, 0} : RowMap{1, 0, nullptr, i};
    if (plan.rows == StepPlan::ROWS_DENSE) {
      if (!plan.folded) {
        GemvParams gr = g;
        gr.K = D; gr.out = e->din; gr.os = D;
        launch_gather_rows(gr, e->wdt, st);
        GemvParams gj = gp(e);
        gj.W = e->proj; gj.N = Dd; gj.K = D; gj.x = e->din; gj.xs = D; gj.M = M; gj.out = e->dx; gj.os = Dd;
        launch_gemv(gj, e->wdt, EPI_STORE, 0, st);
      } else {
        GemvParams gr = g0;
        gr.K = Dd; gr.out = e->dx; gr.os = Dd;
        launch_gather_rows(gr, e->wdt, st);
      }
      if (plan.blocks == StepPlan::BLOCKS_STREAMING) {
        launch_xs_rows(e->dx, (int)Dd, M, (int)Dd, e->dec.L[0].n1, e->xs_D, e->xs_ss, GEMM_XS_MAX_M,
                       e->wdt == WDT_Q4 ? e->hs_D : nullptr, st);
        run_dec_xs(e, M, rm, st, AttnParams{}, true);
      } else {
        run_stack(e, e->dec, e->dx, M, e->dq, e->datt, e->dmlp, rm, st, nullptr);
      }
    } else if (plan.rows == StepPlan::ROWS_TABLES) {
      // (no layer-0 QKV projection; at >= 8 rows the other projections run on the matrix cores)
      AttnParams a0{};
      a0.g_tab = e->qkv0_tab + (size_t)(i - 1) * V * e->dec.qkv_rows(); a0.g_row = e->dec.qkv_rows();
      a0.g_part = g.xpart; a0.g_part_stride = g.xpart_stride; a0.g_part_n = g.xpart_n; a0.g_V = V;
      a0.g_codes = e->codes; a0.g_codes_K = K; a0.g_cb = i - 1;
      a0.g_xtab = e->proj_tab + (size_t)(i - 1) * V * Dd; a0.g_xout = e->dx; a0.g_D = Dd;
      if (plan.blocks == StepPlan::BLOCKS_PERSISTENT)
        launch_xsd(e, M, i, g.xpart, g.xpart_n, part(i), st, plan.head_tiled, plan.sample_in_step);
      else if (plan.blocks == StepPlan::BLOCKS_STREAMING) run_dec_xs(e, M, rm, st, a0);
      else run_stack(e, e->dec, e->dx, M, e->dq, e->datt, e->dmlp, rm, st, nullptr, &a0);
    } else {
      if (!plan.folded) launch_gemv(g, e->wdt, EPI_STORE, 0, st);
      run_stack(e, e->dec, e->dx, M, e->dq, e->datt, e->dmlp, rm, st, plan.folded ? &g0 : nullptr);
    }
    // ci_logits = norm(hidden[:, -1]) @ audio_head[i-1]  (generation.py:79)
    g = gp(e);
    g.W = (const char*)e->audio_head + (size_t)(i - 1) * Vp * Dd * (e->head_wdt == WDT_F32 ? 4 : 2); g.N = Vp; g.K = Dd;
    g.x = e->dx + (i == 1 ? Dd : 0); g.xs = (i == 1 ? 2 * Dd : Dd); g.M = B; g.nw = e->dec.norm;
    g.eps = e->dec.d.eps; g.out = e->ci_logits + (size_t)(i - 1) * B * Vp; g.os = Vp;
    g.part = part(i); g.part_stride = e->part_stride; g.n_valid = V;
    if (plan.head == StepPlan::HEAD_STREAMING) {  // the head reads the split rows (x * final norm) the last down wrote
      // (the persistent step's combines write 32 sum-of-squares tiles)
      g.xs_in = e->xs_D; g.ss_in = e->xs_ss;
      g.ss_n = plan.blocks == StepPlan::BLOCKS_PERSISTENT ? 32 : gemm_xs_tiles(Dd, e->dec.d.intermediate, M);
      g.ss_stride = GEMM_XS_MAX_M;
      launch_gemm_xs(g, greedy ? EPI_ARGMAX : EPI_STORE, st, gemv_nt(2), e->head_wdt);
    } else if (plan.head == StepPlan::HEAD_GEMV) {
      launch_gemv(g, e->head_wdt, greedy ? EPI_ARGMAX : EPI_STORE, 1, st);
    }
    if (!greedy && !pieces && !plan.sample_in_step) {
      sp.logits = e->ci_logits + (size_t)(i - 1) * B * Vp; sp.cb = i; sp.part = part(i);
      launch_sample(sp, B, fp.filtered, st);
    }
  }
  if (pieces && piece < K) return;  // the frame continues with the host's next code
  AdvanceParams ap = advance_params(e);
  if (greedy) {
    ap.last_part = part(K - 1); ap.last_stride = e->part_stride; ap.last_n = ni;
  }
  launch_advance(ap, st);
}

void enqueue_head(csm_engine* e, hipStream_t st) { enqueue_head_phase(e, st, HeadPhase::Frame); }

hipGraphExec_t capture(csm_engine* e, void (*fn)(csm_engine*, hipStream_t)) {
  hipGraph_t graph;
  HIPCHK(hipStreamBeginCapture(e->st, hipStreamCaptureModeThreadLocal));
  fn(e, e->st);
  HIPCHK(hipStreamEndCapture(e->st, &graph));
  hipGraphExec_t exec;
  HIPCHK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
  (void)hipGraphDestroy(graph);
  return exec;
}
