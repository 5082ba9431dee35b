// Mimi codec engine behind the mimi_* C ABI (include/csm_hip.h).
//
// Reference: moshi_mlx Mimi(mimi_202407(n_q)) as used by /root/reference/csm_mlx/tokenizers.py:14-21,
// 61-85, 148-150 and generation.py:224-258; restated in oracle/mimi_oracle.py.
//
// Layout: SEANet activations are [B][C][T] fp32, transformer rows [B*T][C].  The decoder SEANet
// has only stride-1 causal convs and k = 2s transposed convs, so every op is evaluated on an
// input *window* = [history (pad samples) | new samples]; one-shot decode is one window with a
// zero history, decode_step is the same code with n = 2 new latent steps per frame and the
// history carried between calls (per-utterance state, unlike the reference's process-global Mimi).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "../../include/csm_hip_prof.h"
#include "engine_util.h"
#include "mimi_kernels.h"

namespace {

struct MConv {
  int cin, cout, k, stride, dil, elu;
  float* w = nullptr;
  float* b = nullptr;
};
struct MConvTr {
  int cin, cout, k, s, elu;
  float* wt = nullptr;  // [s][cout][cin][2]
  float* b = nullptr;
};
struct MRes {
  int ch, hid, k, dil;
  MConv c1, c2;
};
struct MOp {
  int kind;  // 0 conv, 1 convtr, 2 res
  int idx;
};
struct MTLayer {
  float *in_w, *out_w, *n1w, *n1b, *n2w, *n2b, *l1, *l2, *ls1, *ls2;
};
struct Dest {
  float* ptr;
  size_t numel;
  int kind;  // 0 plain, 1 convtr rearrange, 2 codebook sum, 3 codebook usage
  int a, b, c;  // convtr: cin, cout, k ; codebook: flat index
  std::vector<int64_t> shape;
};

}  // namespace

struct mimi_codec {
  mimi_dims d;
  int dev = 0;
  hipStream_t st = nullptr;
  int B_max = 0, F_max = 0, S_cap = 0, hd = 0;
  std::vector<MConv> convs;
  std::vector<MConvTr> convtrs;
  std::vector<MRes> res;
  std::vector<MOp> enc_ops, dec_ops;
  std::vector<MTLayer> etr, dtr;
  float *down_w = nullptr, *up_w = nullptr;
  float* rvq_in[2] = {nullptr, nullptr};
  float* rvq_out[2] = {nullptr, nullptr};
  float *cb = nullptr, *c2half = nullptr;  // [n_q][bins][cd], [n_q][bins]
  float* cbT = nullptr;                    // [n_q][cd][bins]: codebooks dims-major (RVQ encode distance GEMM)
  float* rvq_r = nullptr;                  // RVQ encode scratch: 2 x [M][cd] residuals, 2 x [M][bins / 256] partials
  size_t rvq_r_n = 0;
  unsigned long long* rvq_p = nullptr;
  size_t rvq_p_n = 0;
  float* rope = nullptr;
  std::map<std::string, Dest> dest;
  std::set<std::string> loaded;
  std::vector<std::vector<float>> cb_sum, cb_usage;
  std::vector<void*> allocs;
  // workspace (grown on demand)
  size_t ws_big = 0, ws_rows = 0;
  float *W0 = nullptr, *W1 = nullptr, *H = nullptr, *E = nullptr;  // E: ELU of the encoder's current buffer
  float* ks_ws = nullptr;  // split-K scratch of the codec GEMMs (MIMI_KS_WS_FLOATS, mimi_kernels.h)
  float *R = nullptr, *Rh = nullptr, *Rqkv = nullptr, *Rq = nullptr, *Ratt = nullptr, *Rf = nullptr;
  size_t r_rows = 0;  // rows of R the last call left (mimi_debug_read "rows")
  int* dcodes = nullptr;
  size_t dcodes_n = 0;
  // transformer KV (encoder one-shot; decoder one-shot + streaming)
  std::vector<float*> ekc, evc, dkc, dvc;
  // streaming state
  int s_B = 0, s_off = 0;
  std::vector<float*> hist;  // per decoder op input history [B_max][cin][pad]
  float* up_hist = nullptr;  // [B_max][dim][1]
  std::vector<int> hist_pad;
  // slot mode (mimi_slot_reset / mimi_decode_slots): every row of the streaming state is a slot with its own
  // latent position (device; the host mirror serves the capacity check only)
  bool slot_mode = false;
  int* slot_pos = nullptr;  // [B_max]
  std::vector<int> slot_pos_host;
  // streaming encoder (mimi_encode_slot_reset / mimi_encode_slots), allocated by the first reset: every row a
  // slot with its own encode stream, whatever the decoder's streaming mode is
  bool enc_ready = false;
  std::vector<float*> enc_hist;   // per encoder op input history [B_max][cin][op_pad]
  float* enc_down_hist = nullptr;  // the downsample conv's [B_max][D][s]
  // encoder-transformer KV of the streams (not ekc / evc, which every one-shot encode overwrites), with one
  // spare row B_max: where an inactive slot's keys go when they would not fit behind its position
  std::vector<float*> enc_kc, enc_vc;
  int* enc_pos = nullptr;  // [B_max] latent position (device; the host mirror serves the capacity check only)
  std::vector<int> enc_pos_host;
  int* enc_rowtab = nullptr;  // the spare-row pass's per-row {slot, position} tables, 2 x [rows]
  size_t enc_rowtab_n = 0;

  void* alloc(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) throw CsmError(CSM_ERR_HIP, "hipMalloc(" + std::to_string(bytes) + ") failed");
    (void)hipMemset(p, 0, bytes);
    (void)hipDeviceSynchronize();  // the null-stream fill is not ordered with the engine's non-blocking stream
    allocs.push_back(p);
    return p;
  }
  ~mimi_codec() {
    for (void* p : allocs) (void)hipFree(p);
    for (float* p : {W0, W1, H, E, R, Rh, Rqkv, Rq, Ratt, Rf}) if (p) (void)hipFree(p);
    if (dcodes) (void)hipFree(dcodes);
    if (rvq_r) (void)hipFree(rvq_r);
    if (rvq_p) (void)hipFree(rvq_p);
    if (enc_rowtab) (void)hipFree(enc_rowtab);
    if (st) (void)hipStreamDestroy(st);
  }
  int op_cin(const MOp& o) const {
    return o.kind == 0 ? convs[o.idx].cin : (o.kind == 1 ? convtrs[o.idx].cin : res[o.idx].ch);
  }
  int op_cout(const MOp& o) const {
    return o.kind == 0 ? convs[o.idx].cout : (o.kind == 1 ? convtrs[o.idx].cout : res[o.idx].ch);
  }
  // history samples an op needs in front of its new input (stride-1 conv: k_eff - 1; convtr: 1; res: k_eff - 1)
  int op_pad(const MOp& o) const {
    if (o.kind == 0) return (convs[o.idx].k - 1) * convs[o.idx].dil + 1 - convs[o.idx].stride;
    if (o.kind == 1) return 1;
    return (res[o.idx].k - 1) * res[o.idx].dil;
  }
};

namespace {

void add_dest(mimi_codec* m, const std::string& name, float* ptr, std::vector<int64_t> shape, int kind = 0, int a = 0,
              int b = 0, int c = 0) {
  size_t n = 1;
  for (auto s : shape) n *= (size_t)s;
  m->dest[name] = Dest{ptr, n, kind, a, b, c, shape};
}

void build_layout(mimi_codec* m) {
  const mimi_dims& d = m->d;
  auto conv = [&](const std::string& key, int cin, int cout, int k, int stride, int dil, int elu) {
    MConv c{cin, cout, k, stride, dil, elu};
    c.w = (float*)m->alloc((size_t)cout * cin * k * 4);
    c.b = (float*)m->alloc((size_t)cout * 4);
    add_dest(m, key + ".conv.conv.weight", c.w, {cout, cin, k});
    add_dest(m, key + ".conv.conv.bias", c.b, {cout});
    return c;
  };
  auto add_res = [&](const std::string& key, int ch) {
    MRes r{ch, ch / d.compress, d.residual_kernel_size, 1};
    r.c1 = conv(key + ".block.1", ch, r.hid, r.k, 1, r.dil, 1);
    r.c2 = conv(key + ".block.3", r.hid, ch, 1, 1, 1, 1);
    m->res.push_back(r);
    return MOp{2, (int)m->res.size() - 1};
  };
  auto add_conv = [&](const std::string& key, int cin, int cout, int k, int stride, int elu) {
    m->convs.push_back(conv(key, cin, cout, k, stride, 1, elu));
    return MOp{0, (int)m->convs.size() - 1};
  };
  auto add_convtr = [&](const std::string& key, int cin, int cout, int s) {
    MConvTr t{cin, cout, 2 * s, s, 1};
    t.wt = (float*)m->alloc((size_t)s * cout * cin * 2 * 4);
    t.b = (float*)m->alloc((size_t)cout * 4);
    add_dest(m, key + ".convtr.convtr.weight", t.wt, {cin, cout, 2 * s}, 1, cin, cout, 2 * s);
    add_dest(m, key + ".convtr.convtr.bias", t.b, {cout});
    m->convtrs.push_back(t);
    return MOp{1, (int)m->convtrs.size() - 1};
  };
  const int nf = d.n_filters;
  // encoder (moshi SEANetEncoder indices; ELU modules occupy indices)
  int idx = 0, mult = 1;
  m->enc_ops.push_back(add_conv("encoder.model.0", d.channels, nf, d.kernel_size, 1, 0));
  idx = 1;
  for (int r = d.n_ratios - 1; r >= 0; --r) {
    const int ratio = d.ratios[r], ch = mult * nf;
    m->enc_ops.push_back(add_res("encoder.model." + std::to_string(idx), ch));
    idx += 2;
    m->enc_ops.push_back(add_conv("encoder.model." + std::to_string(idx), ch, 2 * ch, 2 * ratio, ratio, 1));
    idx += 1;
    mult *= 2;
  }
  idx += 1;
  m->enc_ops.push_back(add_conv("encoder.model." + std::to_string(idx), mult * nf, d.dimension, d.last_kernel_size, 1, 1));
  // decoder
  mult = 1 << d.n_ratios;
  m->dec_ops.push_back(add_conv("decoder.model.0", d.dimension, mult * nf, d.kernel_size, 1, 0));
  idx = 1;
  for (int r = 0; r < d.n_ratios; ++r) {
    const int ratio = d.ratios[r], ch = mult * nf;
    idx += 1;
    m->dec_ops.push_back(add_convtr("decoder.model." + std::to_string(idx), ch, ch / 2, ratio));
    idx += 1;
    m->dec_ops.push_back(add_res("decoder.model." + std::to_string(idx), ch / 2));
    idx += 1;
    mult /= 2;
  }
  idx += 1;
  m->dec_ops.push_back(add_conv("decoder.model." + std::to_string(idx), nf, d.channels, d.last_kernel_size, 1, 1));
  // transformers
  const int D = d.dimension, F = d.dim_feedforward;
  for (int which = 0; which < 2; ++which) {
    auto& T = which == 0 ? m->etr : m->dtr;
    const std::string pre = which == 0 ? "encoder_transformer" : "decoder_transformer";
    T.resize(d.num_layers);
    for (int l = 0; l < d.num_layers; ++l) {
      MTLayer& L = T[l];
      const std::string p = pre + ".transformer.layers." + std::to_string(l);
      L.in_w = (float*)m->alloc((size_t)3 * D * D * 4);
      L.out_w = (float*)m->alloc((size_t)D * D * 4);
      L.l1 = (float*)m->alloc((size_t)F * D * 4);
      L.l2 = (float*)m->alloc((size_t)D * F * 4);
      for (float** v : {&L.n1w, &L.n1b, &L.n2w, &L.n2b, &L.ls1, &L.ls2}) *v = (float*)m->alloc((size_t)D * 4);
      add_dest(m, p + ".self_attn.in_proj_weight", L.in_w, {3 * D, D});
      add_dest(m, p + ".self_attn.out_proj.weight", L.out_w, {D, D});
      add_dest(m, p + ".linear1.weight", L.l1, {F, D});
      add_dest(m, p + ".linear2.weight", L.l2, {D, F});
      add_dest(m, p + ".norm1.weight", L.n1w, {D});
      add_dest(m, p + ".norm1.bias", L.n1b, {D});
      add_dest(m, p + ".norm2.weight", L.n2w, {D});
      add_dest(m, p + ".norm2.bias", L.n2b, {D});
      add_dest(m, p + ".layer_scale_1.scale", L.ls1, {D});
      add_dest(m, p + ".layer_scale_2.scale", L.ls2, {D});
    }
  }
  const int s = d.downsample_stride;
  m->down_w = (float*)m->alloc((size_t)D * D * 2 * s * 4);
  m->up_w = (float*)m->alloc((size_t)D * 2 * s * 4);
  add_dest(m, "downsample.conv.conv.conv.weight", m->down_w, {D, D, 2 * s});
  add_dest(m, "upsample.convtr.convtr.convtr.weight", m->up_w, {D, 1, 2 * s});
  const int cd = d.codebook_dim;
  const char* qn[2] = {"rvq_first", "rvq_rest"};
  for (int q = 0; q < 2; ++q) {
    m->rvq_in[q] = (float*)m->alloc((size_t)cd * D * 4);
    m->rvq_out[q] = (float*)m->alloc((size_t)D * cd * 4);
    add_dest(m, std::string("quantizer.") + qn[q] + ".input_proj.weight", m->rvq_in[q], {cd, D, 1});
    add_dest(m, std::string("quantizer.") + qn[q] + ".output_proj.weight", m->rvq_out[q], {D, cd, 1});
  }
  m->cb = (float*)m->alloc((size_t)d.n_q * d.bins * cd * 4);
  m->c2half = (float*)m->alloc((size_t)d.n_q * d.bins * 4);
  m->cbT = (float*)m->alloc((size_t)d.n_q * d.bins * cd * 4);
  m->cb_sum.assign(d.n_q, {});
  m->cb_usage.assign(d.n_q, {});
  for (int k = 0; k < d.n_q; ++k) {
    const std::string p = k == 0 ? std::string("quantizer.rvq_first.vq.layers.0._codebook")
                                 : "quantizer.rvq_rest.vq.layers." + std::to_string(k - 1) + "._codebook";
    add_dest(m, p + ".embedding_sum", nullptr, {d.bins, cd}, 2, k);
    add_dest(m, p + ".cluster_usage", nullptr, {d.bins}, 3, k);
  }
}

void finish_codebook(mimi_codec* m, int k) {
  const int bins = m->d.bins, cd = m->d.codebook_dim;
  auto& s = m->cb_sum[k];
  auto& u = m->cb_usage[k];
  if (s.empty() || u.empty()) return;
  std::vector<float> e((size_t)bins * cd), c2(bins);
  for (int i = 0; i < bins; ++i) {
    const float us = std::max(u[i], 1e-5f);  // embedding_sum / clamp(cluster_usage, eps)
    double acc = 0.0;
    for (int j = 0; j < cd; ++j) {
      const float v = s[(size_t)i * cd + j] / us;
      e[(size_t)i * cd + j] = v;
      acc += (double)v * (double)v;
    }
    c2[i] = (float)(acc / 2.0);
  }
  HIPCHK(hipMemcpy(m->cb + (size_t)k * bins * cd, e.data(), e.size() * 4, hipMemcpyHostToDevice));
  std::vector<float> et((size_t)bins * cd);
  for (int i = 0; i < bins; ++i)
    for (int j = 0; j < cd; ++j) et[(size_t)j * bins + i] = e[(size_t)i * cd + j];
  HIPCHK(hipMemcpy(m->cbT + (size_t)k * bins * cd, et.data(), et.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(m->c2half + (size_t)k * bins, c2.data(), c2.size() * 4, hipMemcpyHostToDevice));
}

template <typename T>
void grow(T*& p, size_t& cap, size_t n) {
  if (n <= cap) return;
  if (p) (void)hipFree(p);
  p = nullptr;
  if (hipMalloc((void**)&p, n * sizeof(T)) != hipSuccess) throw CsmError(CSM_ERR_HIP, "workspace allocation failed");
  cap = n;
}

void ensure_ws(mimi_codec* m, size_t big, size_t rows_M) {
  // (the buffers of a group grow together, on the group's one capacity: each from a capacity of 0)
  auto regrow = [](float*& p, size_t n) {
    size_t none = 0;
    grow(p, none, n);
  };
  if (big > m->ws_big) {
    for (float** p : {&m->W0, &m->W1, &m->H, &m->E}) regrow(*p, big);
    m->ws_big = big;
  }
  if (rows_M > m->ws_rows) {
    const size_t D = m->d.dimension, F = m->d.dim_feedforward;
    const std::pair<float**, size_t> rows[] = {{&m->R, D},  {&m->Rh, std::max(D, (size_t)m->d.codebook_dim)},
                                               {&m->Rqkv, 3 * D}, {&m->Rq, D}, {&m->Ratt, D}, {&m->Rf, F}};
    for (const auto& r : rows) regrow(*r.first, rows_M * r.second);
    m->ws_rows = rows_M;
  }
}

// An activation tensor in conv layout: channel rows cs floats apart, sample 0 at off of each row, len
// samples; utterances are (channels of the op that reads or writes it) * cs apart.
struct Act {
  float* p;
  int cs, off, len;
};

// The causal conv c from `in` to the out.len steps of `out`, left-padded by pad_l (zeros, or the edge sample)
ConvParams conv_params(mimi_codec* m, const MConv& c, Act in, Act out, int B, int pad_l, bool replicate = false) {
  ConvParams p{};
  p.ks_ws = m->ks_ws;
  p.x = in.p; p.Cin = c.cin; p.Tin = in.len; p.x_bstride = c.cin * in.cs; p.x_cstride = in.cs; p.x_off = in.off;
  p.w = c.w; p.bias = c.b; p.Cout = c.cout; p.k = c.k; p.stride = c.stride; p.dil = c.dil; p.pad_l = pad_l;
  p.replicate = replicate; p.elu_in = c.elu;
  p.y = out.p; p.Tout = out.len; p.y_bstride = c.cout * out.cs; p.y_cstride = out.cs; p.y_off = out.off; p.B = B;
  return p;
}

// out = epi(x [M][K] . W [N][K]^T), both row-major and dense
LinParams lin_params(mimi_codec* m, const float* x, int M, int K, const float* W, int N, float* out,
                     int epi = EPI_STORE, const float* scale = nullptr) {
  LinParams lp{};
  lp.ks_ws = m->ks_ws;
  lp.x = x; lp.M = M; lp.K = K; lp.xs = K; lp.W = W; lp.N = N; lp.out = out; lp.os = N; lp.epi = epi; lp.scale = scale;
  return lp;
}

// x rows [M = B*T][D] in place through the codec transformer; positions offset..offset+T-1, or with slot_pos
// (device, [B]) utterance b's at slot_pos[b]..slot_pos[b]+T-1: the T rows are then T / downsample_stride frames
// of one call, and in the moshi_mlx mode each sees the keys a decode_step call of its own would (ATTN_FRAMES).
// row_b / row_pos (device, [M]): every row's cache row and position from these tables instead.
void run_transformer(mimi_codec* m, std::vector<MTLayer>& T, std::vector<float*>& kc, std::vector<float*>& vc, int B,
                     int Tn, int offset, const int* slot_pos = nullptr, const int* row_b = nullptr,
                     const int* row_pos = nullptr) {
  const mimi_dims& d = m->d;
  const int D = d.dimension, M = B * Tn, H = d.num_heads, hd = m->hd, F = d.dim_feedforward;
  hipStream_t st = m->st;
  RowMap rm{Tn, 0, slot_pos, offset};
  rm.row_b = row_b;
  rm.row_pos = row_pos;
  for (size_t l = 0; l < T.size(); ++l) {
    MTLayer& L = T[l];
    launch_layernorm_rows(m->R, D, L.n1w, L.n1b, d.norm_eps, m->Rh, M, st);
    launch_linear(lin_params(m, m->Rh, M, D, L.in_w, 3 * D, m->Rqkv), st);
    launch_rope_append(m->Rqkv, M, D, H, hd, m->rope, rm, m->Rq, kc[l], vc[l], m->S_cap, st);
    AttnParams a{};
    a.q = m->Rq; a.qs = D; a.M = M; a.kc = kc[l]; a.vc = vc[l]; a.Hq = H; a.Hkv = H; a.S_cap = m->S_cap;
    a.scale = 1.0f / sqrtf((float)hd); a.window = d.context; a.rm = rm; a.out = m->Ratt; a.os = D;
    a.mode = d.attn_mode != 0 ? ATTN_WINDOW : (slot_pos ? ATTN_FRAMES : ATTN_BLOCK);
    a.blk = d.downsample_stride;
    launch_attn(a, hd, st);
    mimi_count_launch();
    launch_linear(lin_params(m, m->Ratt, M, D, L.out_w, D, m->R, EPI_ADD, L.ls1), st);
    launch_layernorm_rows(m->R, D, L.n2w, L.n2b, d.norm_eps, m->Rh, M, st);
    LinParams up = lin_params(m, m->Rh, M, D, L.l1, F, m->Rf, EPI_GELU);
    up.gelu_erf = d.gelu_erf;
    launch_linear(up, st);
    launch_linear(lin_params(m, m->Rf, M, F, L.l2, D, m->R, EPI_ADD, L.ls2), st);
  }
}

int64_t conv_out_len(int64_t T, int k_eff, int stride) {  // causal conv with right "extra" padding
  const int pad = k_eff - stride;
  const double n_frames = (double)(T - k_eff + pad) / stride + 1.0;
  const int64_t ideal = ((int64_t)std::ceil(n_frames) - 1) * stride + (k_eff - pad);
  const int64_t extra = ideal - T;
  return (T + pad + extra - k_eff) / stride + 1;
}

// CSM_MIMI_ELU_PRE=0: ELU in every consumer's staging loads (A/B); else once, by the producer
bool mimi_elu_pre() {
  static const bool v = [] { const char* e = getenv("CSM_MIMI_ELU_PRE"); return !(e && e[0] == '0'); }();
  return v;
}

// How an op stores its output for the ELU of the op after it: ELU(y) in place of y, or ELU(y) to y2 beside y
struct EluOut {
  int elu_out = 0;
  float* y2 = nullptr;
};

// A residual block: ELU -> conv(k, ch -> hid) into m->H -> ELU -> conv(1, hid -> ch) + identity skip
// (true_skip).  x1 is what block.1 reads, left-padded by pad_l (x1_elu: it already holds ELU(x)); skip is the
// block's input at the output steps.  H feeds only block.3's ELU, so it holds ELU(h) unless CSM_MIMI_ELU_PRE=0.
void run_res(mimi_codec* m, const MRes& r, Act x1, bool x1_elu, int pad_l, Act skip, Act out, int B, EluOut eo) {
  const Act h{m->H, out.len, 0, out.len};
  ConvParams p = conv_params(m, r.c1, x1, h, B, pad_l);
  p.elu_in = !x1_elu;
  p.elu_out = mimi_elu_pre();
  launch_conv1d(p, m->st);
  ConvParams q = conv_params(m, r.c2, h, out, B, 0);
  q.elu_in = !mimi_elu_pre();
  q.resid = skip.p; q.r_bstride = r.ch * skip.cs; q.r_cstride = skip.cs; q.r_off = skip.off;
  q.elu_out = eo.elu_out; q.y2 = eo.y2;
  launch_conv1d(q, m->st);
}

// One decoder-SEANet op on a window buffer: input window `in` = [P history | n new] samples per channel,
// output written behind the next op's history (out.off) of `out`.
// in_elu: the window holds ELU(x) (its producer stored it so); out_elu: store ELU(y) for an ELU-input
// next op (histories copy whichever the window holds, so the two stay consistent from call to call)
void run_window_op(mimi_codec* m, const MOp& o, Act in, int P, Act out, int B, bool in_elu, bool out_elu) {
  if (o.kind == 0) {
    const MConv& c = m->convs[o.idx];
    ConvParams p = conv_params(m, c, in, out, B, 0);
    p.elu_in = c.elu && !in_elu;
    p.elu_out = out_elu;
    launch_conv1d(p, m->st);
  } else if (o.kind == 1) {
    const MConvTr& t = m->convtrs[o.idx];
    ConvTrParams p{};
    p.ks_ws = m->ks_ws;
    p.x = in.p; p.Cin = t.cin; p.Tin = in.len; p.x_bstride = t.cin * in.cs; p.x_cstride = in.cs; p.x_off = in.off;
    p.wt = t.wt; p.bias = t.b; p.Cout = t.cout; p.s = t.s; p.elu_in = t.elu && !in_elu; p.t_in0 = P; p.n_in = in.len - P;
    p.y = out.p; p.y_bstride = t.cout * out.cs; p.y_cstride = out.cs; p.y_off = out.off; p.B = B;
    launch_convtr(p, m->st);
  } else {
    // block.1 reads the whole window; the skip is the window behind its history
    run_res(m, m->res[o.idx], in, false, 0, Act{in.p, in.cs, in.off + P, out.len}, out, B, EluOut{out_elu, nullptr});
  }
}

// Decoder from latent rows (already through the transformer): conv layout x [B][dim][n] in m->W0
// at offset P0 (history slot).  Returns pcm in the final window (device).  `stream` = keep histories.
const float* run_decoder_seanet(mimi_codec* m, int B, int n_lat, bool use_hist) {
  const auto& ops = m->dec_ops;
  float* bufs[2] = {m->W0, m->W1};
  int n = n_lat;
  int cur = 0;
  bool in_elu = false;
  auto elu_input = [&](const MOp& o) {
    return (o.kind == 0 && m->convs[o.idx].elu) || (o.kind == 1 && m->convtrs[o.idx].elu);
  };
  for (size_t i = 0; i < ops.size(); ++i) {
    const MOp& o = ops[i];
    const int P = m->op_pad(o);
    const int cin = m->op_cin(o);
    const int cs_in = P + n;
    float* in = bufs[cur];
    // history -> window head (zeros for one-shot)
    if (P > 0) {
      if (use_hist) {
        launch_copy_window(m->hist[i], B, cin, cin * P, P, 0, in, cin * cs_in, cs_in, 0, P, m->st);
      } else {
        // the B utterances' cin rows are B * cin rows of pitch cs_in: one 2-D fill for all (not one per utterance)
        HIPCHK(hipMemset2DAsync(in, (size_t)cs_in * 4, 0, (size_t)P * 4, (size_t)cin * B, m->st));
      }
    }
    const int n_out = o.kind == 1 ? n * m->convtrs[o.idx].s : n;
    const bool last = i + 1 == ops.size();
    const int P_next = last ? 0 : m->op_pad(ops[i + 1]);
    const int cs_out = P_next + n_out;
    // an output that only an ELU-input op reads is stored as ELU(y) (a transposed conv's output feeds a
    // residual block, whose skip needs y itself)
    const bool out_elu = mimi_elu_pre() && !last && o.kind != 1 && elu_input(ops[i + 1]);
    run_window_op(m, o, Act{in, cs_in, 0, cs_in}, P, Act{bufs[cur ^ 1], cs_out, P_next, n_out}, B, in_elu, out_elu);
    in_elu = out_elu;
    // window tail -> history for the next call
    if (use_hist && P > 0) launch_copy_window(in, B, cin, cin * cs_in, cs_in, n, m->hist[i], cin * P, P, 0, P, m->st);
    n = n_out;
    cur ^= 1;
  }
  return bufs[cur];
}

size_t decoder_ws(mimi_codec* m, int n_lat) {  // max window elements per utterance
  size_t best = (size_t)m->d.dimension * (n_lat + 8);
  int n = n_lat;
  for (const MOp& o : m->dec_ops) {
    const int P = m->op_pad(o);
    best = std::max(best, (size_t)m->op_cin(o) * (P + n));
    if (o.kind == 1) n *= m->convtrs[o.idx].s;
    best = std::max(best, (size_t)m->op_cout(o) * (n + 8));
  }
  return best;
}

// The PCM of n_lat latent steps after run_decoder_seanet: [B][1][n] in the ping-pong buffer it ended in
struct Pcm {
  const float* p;
  int n;
};
Pcm decoder_pcm(const mimi_codec* m, int n_lat) {
  int n = n_lat;
  for (const MOp& o : m->dec_ops)
    if (o.kind == 1) n *= m->convtrs[o.idx].s;
  return Pcm{m->dec_ops.size() % 2 == 0 ? m->W0 : m->W1, n};
}

// The streaming encoder SEANet: n new samples per slot (whole frames, so every strided conv divides its input)
// behind conv0's history in m->W0, every op on its window [history | new] as run_decoder_seanet runs the
// decoder's, the histories rolled by one launch per op for the active slots only.  Returns the buffer holding
// the dense output [B][dimension][*n_out].
float* run_encoder_stream(mimi_codec* m, int B, int n, const MimiSlotMask& active, int* n_out_lat) {
  const auto& ops = m->enc_ops;
  float* bufs[2] = {m->W0, m->W1};
  int cur = 0;
  bool in_elu = false;
  for (size_t i = 0; i < ops.size(); ++i) {
    const MOp& o = ops[i];
    const int P = m->op_pad(o), cin = m->op_cin(o), cs_in = P + n;
    float* in = bufs[cur];
    launch_mimi_window_roll(m->enc_hist[i], in, B, cin, P, n, active, nullptr, m->st);
    const int n_out = o.kind == 0 ? n / m->convs[o.idx].stride : n;
    const bool last = i + 1 == ops.size();
    const int P_next = last ? 0 : m->op_pad(ops[i + 1]);
    // as in the decoder: an output that only an ELU-input conv reads is stored as ELU(y), and so is its history
    const bool out_elu = mimi_elu_pre() && !last && ops[i + 1].kind == 0 && m->convs[ops[i + 1].idx].elu;
    run_window_op(m, o, Act{in, cs_in, 0, cs_in}, P, Act{bufs[cur ^ 1], P_next + n_out, P_next, n_out}, B, in_elu,
                  out_elu);
    in_elu = out_elu;
    n = n_out;
    cur ^= 1;
  }
  *n_out_lat = n;
  return bufs[cur];
}

size_t encoder_stream_ws(mimi_codec* m, int n) {  // max window elements per slot
  size_t best = 0;
  for (size_t i = 0; i < m->enc_ops.size(); ++i) {
    const MOp& o = m->enc_ops[i];
    best = std::max(best, (size_t)m->op_cin(o) * (m->op_pad(o) + n));
    if (o.kind == 0) n /= m->convs[o.idx].stride;
    best = std::max(best, (size_t)m->op_cout(o) * (n + 8));
  }
  return std::max(best, (size_t)m->d.dimension * (m->d.downsample_stride + n + 8));
}

int mimi_frame_size(const mimi_codec* m) {
  int fs = m->d.downsample_stride;
  for (int r = 0; r < m->d.n_ratios; ++r) fs *= m->d.ratios[r];
  return fs;
}

// Slot b's encoder histories zeroed and its position set to 0 (b < 0: every slot's): one launch, no wait
void enc_slot_reset_launch(mimi_codec* m, int b) {
  MimiSlotResetParams p{};
  for (size_t i = 0; i < m->enc_hist.size(); ++i) {
    if (!m->enc_hist[i]) continue;
    if (p.n >= MIMI_SLOT_BUFS - 1) throw CsmError(CSM_ERR_ARG, "codec with more streaming buffers than the slot reset table");
    p.buf[p.n] = m->enc_hist[i];
    p.per[p.n++] = m->op_cin(m->enc_ops[i]) * m->op_pad(m->enc_ops[i]);
  }
  p.buf[p.n] = m->enc_down_hist;
  p.per[p.n++] = m->d.dimension * m->d.downsample_stride;
  p.slot_pos = m->enc_pos; p.b = b; p.B = m->B_max;
  launch_mimi_slot_reset(p, m->st);
  HIPCHK(hipGetLastError());
  if (b < 0) std::fill(m->enc_pos_host.begin(), m->enc_pos_host.end(), 0);
  else m->enc_pos_host[b] = 0;
}

}  // namespace

// =============================================================================== C ABI
bool mimi_kv_view(mimi_codec* m, int side, int layer, MimiKvView* out) {
  if (!m || !out || layer < 0 || layer >= m->d.num_layers || (side != 0 && side != 1)) return false;
  if (side == 1 && !m->enc_ready) return false;
  const std::vector<float*>& kc = side ? m->enc_kc : m->dkc;
  const std::vector<float*>& vc = side ? m->enc_vc : m->dvc;
  if ((size_t)layer >= kc.size() || (size_t)layer >= vc.size()) return false;
  *out = MimiKvView{kc[layer], vc[layer], m->B_max + side, m->d.num_heads, m->S_cap, m->hd, m->dev, m->st};
  return true;
}

extern "C" {

int mimi_create(const mimi_dims* dims, int device, int max_batch, int max_frames, mimi_codec** out) {
  CSM_TRY {
    if (!dims || !out || max_batch <= 0 || max_frames <= 0) throw CsmError(CSM_ERR_ARG, "bad codec arguments");
    if (dims->dimension % dims->num_heads) throw CsmError(CSM_ERR_ARG, "dimension % heads");
    const int hd = dims->dimension / dims->num_heads;
    if (hd != 64 && hd != 128) throw CsmError(CSM_ERR_ARG, "codec head_dim must be 64 or 128");
    if (dims->codebook_dim % 4 || dims->codebook_dim > 1024) throw CsmError(CSM_ERR_ARG, "codebook_dim");
    if (dims->n_ratios <= 0 || dims->n_ratios > 8) throw CsmError(CSM_ERR_ARG, "ratios");
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<mimi_codec> m(new mimi_codec());
    m->d = *dims;
    m->dev = device;
    m->hd = hd;
    m->B_max = max_batch;
    m->F_max = max_frames;
    m->S_cap = 2 * max_frames * dims->downsample_stride / 2 + 16;  // latent (25 Hz) positions
    m->S_cap = std::max(m->S_cap, 2 * max_frames + 16);
    // the codec's stream at the lowest priority (the engine's at the highest), so a streaming decode_step
    // overlapping the frame engine yields the CUs to the engine's dependent launches: config 3 +0.4-0.5 %
    // in two alternating pairs against default priorities (profiles/r06_ab_stream_prio.txt)
    int least = 0, greatest = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIPCHK(hipStreamCreateWithPriority(&m->st, hipStreamNonBlocking, least));
    build_layout(m.get());
    m->rope = (float*)m->alloc((size_t)m->S_cap * hd * 4);
    const size_t kv = (size_t)max_batch * dims->num_heads * m->S_cap * hd * 4;
    for (int l = 0; l < dims->num_layers; ++l) {
      m->ekc.push_back((float*)m->alloc(kv));
      m->evc.push_back((float*)m->alloc(kv));
      m->dkc.push_back((float*)m->alloc(kv));
      m->dvc.push_back((float*)m->alloc(kv));
    }
    for (const MOp& o : m->dec_ops) {
      const int P = m->op_pad(o);
      m->hist_pad.push_back(P);
      m->hist.push_back(P > 0 ? (float*)m->alloc((size_t)max_batch * m->op_cin(o) * P * 4) : nullptr);
    }
    m->up_hist = (float*)m->alloc((size_t)max_batch * dims->dimension * 4);
    m->slot_pos = (int*)m->alloc((size_t)max_batch * 4);
    m->slot_pos_host.assign(max_batch, 0);
    m->ks_ws = (float*)m->alloc(MIMI_KS_WS_FLOATS * 4);
    HIPCHK(hipDeviceSynchronize());
    *out = m.release();
  }
  CSM_CATCH
}

int mimi_destroy(mimi_codec* m) {
  CSM_TRY { delete m; }
  CSM_CATCH
}

int mimi_set_rope_table(mimi_codec* m, const float* table, int n_pos, int head_dim) {
  CSM_TRY {
    if (head_dim != m->hd || n_pos < m->S_cap) throw CsmError(CSM_ERR_ARG, "codec rope table shape mismatch");
    HIPCHK(hipSetDevice(m->dev));
    HIPCHK(hipMemcpy(m->rope, table, (size_t)m->S_cap * head_dim * 4, hipMemcpyHostToDevice));
    m->loaded.insert("__rope__");
  }
  CSM_CATCH
}

int mimi_load_tensor(mimi_codec* m, const char* cname, const void* host, int src_dtype, const int64_t* shape,
                     int ndim) {
  CSM_TRY {
    HIPCHK(hipSetDevice(m->dev));
    const std::string name(cname);
    auto it = m->dest.find(name);
    if (it == m->dest.end()) throw CsmError(CSM_ERR_ARG, "unknown tensor " + name);
    const Dest& d = it->second;
    if (std::vector<int64_t>(shape, shape + ndim) != d.shape) throw CsmError(CSM_ERR_ARG, "shape mismatch for " + name);
    auto h = convert_to(host, src_dtype, d.numel, 0);
    const float* f = reinterpret_cast<const float*>(h.data());
    if (d.kind == 0) {
      HIPCHK(hipMemcpy(d.ptr, f, d.numel * 4, hipMemcpyHostToDevice));
    } else if (d.kind == 1) {  // ConvTranspose (cin, cout, k=2s) -> [s][cout][cin][2]
      const int cin = d.a, cout = d.b, k = d.c, s = k / 2;
      std::vector<float> t((size_t)s * cout * cin * 2);
      for (int ci = 0; ci < cin; ++ci)
        for (int co = 0; co < cout; ++co)
          for (int j = 0; j < k; ++j) {
            const int r = j % s, e = j / s;
            t[(((size_t)r * cout + co) * cin + ci) * 2 + e] = f[((size_t)ci * cout + co) * k + j];
          }
      HIPCHK(hipMemcpy(d.ptr, t.data(), t.size() * 4, hipMemcpyHostToDevice));
    } else if (d.kind == 2) {
      m->cb_sum[d.a].assign(f, f + d.numel);
      finish_codebook(m, d.a);
    } else {
      m->cb_usage[d.a].assign(f, f + d.numel);
      finish_codebook(m, d.a);
    }
    m->loaded.insert(name);
  }
  CSM_CATCH
}

int mimi_weights_ready(mimi_codec* m) {
  CSM_TRY {
    for (const auto& kv : m->dest)
      if (!m->loaded.count(kv.first)) throw CsmError(CSM_ERR_STATE, "missing codec weight " + kv.first);
    if (!m->loaded.count("__rope__")) throw CsmError(CSM_ERR_STATE, "codec rope table not set");
  }
  CSM_CATCH
}

int mimi_encode(mimi_codec* m, int B, int N, const float* pcm, int32_t* codes, int* n_frames_out) {
  return mimi_encode_rows(m, B, N, pcm, nullptr, codes, n_frames_out);
}

int mimi_encode_rows(mimi_codec* m, int B, int N, const float* pcm, const float* const* rows, int32_t* codes,
                     int* n_frames_out) {
  CSM_TRY {
    if (B <= 0 || B > m->B_max || N <= 0) throw CsmError(CSM_ERR_ARG, "bad encode shape");
    if (!pcm && !rows) throw CsmError(CSM_ERR_ARG, "encode: no audio");
    HIPCHK(hipSetDevice(m->dev));
    const mimi_dims& d = m->d;
    hipStream_t st = m->st;
    // lengths through the encoder
    std::vector<int64_t> lens{N};
    size_t big = (size_t)N * std::max(d.n_filters, d.channels) + 64;
    int64_t T = N;
    for (const MOp& o : m->enc_ops) {
      if (o.kind == 0) {
        const MConv& c = m->convs[o.idx];
        T = conv_out_len(T, (c.k - 1) * c.dil + 1, c.stride);
      }
      big = std::max(big, (size_t)m->op_cout(o) * (T + 8));
      lens.push_back(T);
    }
    const int64_t T25 = T;
    if (T25 + 4 > m->S_cap) throw CsmError(CSM_ERR_ARG, "audio longer than the codec capacity");
    const int s = d.downsample_stride;
    const int64_t Tf = conv_out_len(T25, 2 * s, s);
    big = std::max(big, (size_t)d.dimension * (T25 + 8));
    ensure_ws(m, big * B, (size_t)B * std::max<int64_t>(T25, Tf) + 8);
    if (pcm) {
      HIPCHK(hipMemcpyAsync(m->W0, pcm, (size_t)B * N * 4, hipMemcpyHostToDevice, st));
    } else {  // one host row per utterance, straight into its slot (no host-side stacking copy)
      for (int b = 0; b < B; ++b)
        HIPCHK(hipMemcpyAsync(m->W0 + (size_t)b * N, rows[b], (size_t)N * 4, hipMemcpyHostToDevice, st));
    }
    float* bufs[2] = {m->W0, m->W1};
    int cur = 0;
    int64_t Tin = N;
    // ELU once per element (CSM_MIMI_ELU_PRE=0: in every consumer's staging loads, A/B): an op whose
    // next op is an ELU-input conv stores ELU(y) in place of y; one whose next op is a residual block
    // (ELU for its first conv, y itself for the skip) also writes ELU(y) to m->E.  in_elu: bufs[cur]
    // holds ELU(x); have_e: m->E holds ELU(bufs[cur]).
    const bool elu_pre = mimi_elu_pre();
    bool in_elu = false, have_e = false;
    auto out_elu = [&](size_t i) {
      EluOut eo;
      const MOp* nx = i + 1 < m->enc_ops.size() ? &m->enc_ops[i + 1] : nullptr;
      if (!elu_pre || !nx) return eo;
      if (nx->kind == 0 && m->convs[nx->idx].elu) eo.elu_out = 1;
      else if (nx->kind != 0) eo.y2 = m->E;
      return eo;
    };
    auto full = [](float* p, int64_t T) { return Act{p, (int)T, 0, (int)T}; };  // a whole sequence, dense
    for (size_t i = 0; i < m->enc_ops.size(); ++i) {
      const MOp& o = m->enc_ops[i];
      float* in = bufs[cur];
      float* out = bufs[cur ^ 1];
      const EluOut eo = out_elu(i);
      if (o.kind == 0) {
        const MConv& c = m->convs[o.idx];
        const int k_eff = (c.k - 1) * c.dil + 1;
        const int64_t Tout = lens[i + 1];
        ConvParams p = conv_params(m, c, full(in, Tin), full(out, Tout), B, k_eff - c.stride);
        if (in_elu && !c.elu) throw CsmError(CSM_ERR_HIP, "mimi encoder: ELU bookkeeping");
        if (in_elu) p.elu_in = 0;
        p.elu_out = eo.elu_out; p.y2 = eo.y2;
        launch_conv1d(p, st);
        Tin = Tout;
      } else {  // resblock on the full sequence (causal, zero left pad); block.1 reads m->E when it holds ELU(in)
        const MRes& r = m->res[o.idx];
        if (in_elu) throw CsmError(CSM_ERR_HIP, "mimi encoder: ELU bookkeeping");
        run_res(m, r, full(have_e ? m->E : in, Tin), have_e, (r.k - 1) * r.dil, full(in, Tin), full(out, Tin), B, eo);
      }
      in_elu = eo.elu_out != 0;
      have_e = eo.y2 != nullptr;
      cur ^= 1;
    }
    // transformer on [B][dim][T25]
    const int D = d.dimension;
    launch_conv_to_rows(bufs[cur], B, D, (int)T25, D * (int)T25, (int)T25, 0, m->R, st);
    run_transformer(m, m->etr, m->ekc, m->evc, B, (int)T25, 0);
    launch_rows_to_conv(m->R, B, D, (int)T25, bufs[cur ^ 1], D * (int)T25, (int)T25, 0, st);
    cur ^= 1;
    // downsample: k = 2s, stride s, replicate pad, no bias
    const MConv down{D, D, 2 * s, s, 1, 0, m->down_w, nullptr};
    launch_conv1d(conv_params(m, down, full(bufs[cur], T25), full(bufs[cur ^ 1], Tf), B, s, true), st);
    cur ^= 1;
    // split RVQ: semantic and acoustic both quantize the same latent
    launch_conv_to_rows(bufs[cur], B, D, (int)Tf, D * (int)Tf, (int)Tf, 0, m->R, st);
    const int M = B * (int)Tf, cd = d.codebook_dim;
    m->r_rows = (size_t)M;  // R: the pre-RVQ latent, read only from here on
    grow(m->dcodes, m->dcodes_n, (size_t)B * d.n_q * Tf);
    for (int q = 0; q < 2; ++q) {
      launch_linear(lin_params(m, m->R, M, D, m->rvq_in[q], cd, m->Rh), st);
      const int k0 = q == 0 ? 0 : 1, k1 = q == 0 ? 1 : d.n_q;
      if (k1 <= k0) continue;
      // many rows: one distance GEMM launch per codebook (profiles/r04_ab_rvq_gemm.txt), else a block per row
      if (M >= 256 && rvq_gemm_eligible(cd, d.bins)) {
        grow(m->rvq_r, m->rvq_r_n, (size_t)2 * M * cd);
        grow(m->rvq_p, m->rvq_p_n, 2 * rvq_gemm_parts(M, d.bins));
        launch_rvq_encode_gemm(m->Rh, M, (int)Tf, cd, m->cb, m->cbT, m->c2half, d.bins, k0, k1, d.n_q, m->dcodes,
                               m->rvq_r, m->rvq_p, st);
      } else {
        launch_rvq_encode(m->Rh, M, (int)Tf, cd, m->cb, m->c2half, d.bins, k0, k1, d.n_q, m->dcodes, st);
      }
    }
    HIPCHK(hipMemcpyAsync(codes, m->dcodes, (size_t)B * d.n_q * Tf * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    if (n_frames_out) *n_frames_out = (int)Tf;
  }
  CSM_CATCH
}

// slots: the rows are slots at their own positions (m->slot_pos), the codes layout 2's ring
static void decode_frames(mimi_codec* m, int B, int F, const int32_t* dcodes, int layout, bool stream,
                          bool slots = false, int first_row = 0, int F_cap = 0) {
  const mimi_dims& d = m->d;
  hipStream_t st = m->st;
  const int D = d.dimension, cd = d.codebook_dim, s = d.downsample_stride;
  const int n_lat = F * s;
  const int M = B * F;
  // RVQ decode: semantic + acoustic gathers, output projections summed into conv layout [B][D][F]
  launch_rvq_gather(dcodes, layout, B, F, d.n_q, 0, 1, m->cb, d.bins, cd, m->Rh, st, first_row, F_cap);
  LinParams lp = lin_params(m, m->Rh, M, cd, m->rvq_out[0], D, m->W1);
  lp.conv_T = F; lp.conv_bstride = D * F;
  launch_linear(lp, st);
  if (d.n_q > 1) {
    launch_rvq_gather(dcodes, layout, B, F, d.n_q, 1, d.n_q, m->cb, d.bins, cd, m->Rh, st, first_row, F_cap);
    lp.W = m->rvq_out[1];
    lp.accumulate = 1;
    launch_linear(lp, st);
  }
  // upsample (depthwise ConvTranspose k=2s): window [1 history | F new] in H
  const int cs = F + 1;
  if (stream) {
    launch_copy_window(m->up_hist, B, D, D, 1, 0, m->H, D * cs, cs, 0, 1, st);
  } else {
    HIPCHK(hipMemset2DAsync(m->H, (size_t)cs * 4, 0, 4, (size_t)D * B, st));  // B * D rows of pitch cs
  }
  launch_copy_window(m->W1, B, D, D * F, F, 0, m->H, D * cs, cs, 1, F, st);
  if (stream) launch_copy_window(m->H, B, D, D * cs, cs, F, m->up_hist, D, 1, 0, 1, st);
  launch_upsample_dw(m->H, B, D, D * cs, cs, 0, m->up_w, s, 1, F, m->W1, D * n_lat, n_lat, 0, st);
  // transformer on the latent steps
  launch_conv_to_rows(m->W1, B, D, n_lat, D * n_lat, n_lat, 0, m->R, st);
  if (slots) {
    run_transformer(m, m->dtr, m->dkc, m->dvc, B, n_lat, 0, m->slot_pos);
  } else {
    run_transformer(m, m->dtr, m->dkc, m->dvc, B, n_lat, m->s_off);
    m->s_off += n_lat;
  }
  m->r_rows = (size_t)B * n_lat;  // R: the decoder transformer's output, read only from here on
  const int P0 = m->op_pad(m->dec_ops[0]);
  launch_rows_to_conv(m->R, B, D, n_lat, m->W0, D * (P0 + n_lat), P0 + n_lat, P0, st);
  run_decoder_seanet(m, B, n_lat, stream);
}

int mimi_decode(mimi_codec* m, int B, int F, const int32_t* codes, int codes_on_device, int codes_layout, float* pcm,
                int pcm_on_device) {
  CSM_TRY {
    if (B <= 0 || B > m->B_max || F <= 0) throw CsmError(CSM_ERR_ARG, "bad decode shape");
    if (2 * F + 4 > m->S_cap) throw CsmError(CSM_ERR_ARG, "more frames than the codec capacity");
    HIPCHK(hipSetDevice(m->dev));
    const mimi_dims& d = m->d;
    const int s = d.downsample_stride;
    const size_t per = decoder_ws(m, F * s);
    ensure_ws(m, per * B + 64, (size_t)B * F * s + 8);
    // Mimi.decode resets the decoder state first (moshi_mlx), so a one-shot decode starts at position 0
    // (and writes the decoder KV of rows 0..B-1 from there: the slots' streams end here)
    m->s_off = 0;
    m->slot_mode = false;
    const int32_t* dc = codes;
    if (!codes_on_device) {
      grow(m->dcodes, m->dcodes_n, (size_t)B * d.n_q * F);
      HIPCHK(hipMemcpyAsync(m->dcodes, codes, (size_t)B * d.n_q * F * 4, hipMemcpyHostToDevice, m->st));
      dc = m->dcodes;
    }
    decode_frames(m, B, F, dc, codes_layout, false);
    m->s_off = 0;
    const Pcm out = decoder_pcm(m, F * s);
    HIPCHK(hipMemcpyAsync(pcm, out.p, (size_t)B * out.n * 4,
                          pcm_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    HIPCHK(hipGetLastError());
  }
  CSM_CATCH
}

int mimi_reset_state(mimi_codec* m, int B) {
  CSM_TRY {
    if (B <= 0 || B > m->B_max) throw CsmError(CSM_ERR_ARG, "bad batch");
    HIPCHK(hipSetDevice(m->dev));
    m->s_B = B;
    m->s_off = 0;
    m->slot_mode = false;
    for (size_t i = 0; i < m->hist.size(); ++i)
      if (m->hist[i])
        HIPCHK(hipMemsetAsync(m->hist[i], 0, (size_t)B * m->op_cin(m->dec_ops[i]) * m->hist_pad[i] * 4, m->st));
    HIPCHK(hipMemsetAsync(m->up_hist, 0, (size_t)B * m->d.dimension * 4, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
  }
  CSM_CATCH
}

int mimi_decode_step(mimi_codec* m, int B, const int32_t* codes, float* pcm) {
  CSM_TRY {
    if (m->slot_mode)
      throw CsmError(CSM_ERR_STATE, "the codec is in slot mode (mimi_slot_reset): mimi_reset_state(B) leaves it");
    if (B != m->s_B) throw CsmError(CSM_ERR_STATE, "mimi_reset_state(B) must precede decode_step");
    const int s = m->d.downsample_stride;
    if (m->s_off + s + 4 > m->S_cap) throw CsmError(CSM_ERR_ARG, "stream longer than the codec capacity");
    HIPCHK(hipSetDevice(m->dev));
    const size_t per = decoder_ws(m, s);
    ensure_ws(m, per * B + 64, (size_t)B * s + 8);
    grow(m->dcodes, m->dcodes_n, (size_t)B * m->d.n_q);
    HIPCHK(hipMemcpyAsync(m->dcodes, codes, (size_t)B * m->d.n_q * 4, hipMemcpyHostToDevice, m->st));
    decode_frames(m, B, 1, m->dcodes, 0, true);
    const Pcm out = decoder_pcm(m, s);
    HIPCHK(hipMemcpyAsync(pcm, out.p, (size_t)B * out.n * 4, hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    HIPCHK(hipGetLastError());
  }
  CSM_CATCH
}

// Slot b's streaming state zeroed and its position set to 0 (b < 0: every slot's): one launch, no wait
static void slot_reset_launch(mimi_codec* m, int b) {
  MimiSlotResetParams p{};
  for (size_t i = 0; i < m->hist.size(); ++i) {
    if (!m->hist[i]) continue;
    if (p.n >= MIMI_SLOT_BUFS - 1) throw CsmError(CSM_ERR_ARG, "codec with more streaming buffers than the slot reset table");
    p.buf[p.n] = m->hist[i];
    p.per[p.n++] = m->op_cin(m->dec_ops[i]) * m->hist_pad[i];
  }
  p.buf[p.n] = m->up_hist;
  p.per[p.n++] = m->d.dimension;
  p.slot_pos = m->slot_pos; p.b = b; p.B = m->B_max;
  launch_mimi_slot_reset(p, m->st);
  HIPCHK(hipGetLastError());
  if (b < 0) std::fill(m->slot_pos_host.begin(), m->slot_pos_host.end(), 0);
  else m->slot_pos_host[b] = 0;
}

int mimi_slot_reset(mimi_codec* m, int b) {
  CSM_TRY {
    if (!m) throw CsmError(CSM_ERR_ARG, "null codec");
    if (b < 0 || b >= m->B_max) throw CsmError(CSM_ERR_ARG, "codec slot index out of range");
    if (m->B_max > MIMI_SLOTS_MAX) throw CsmError(CSM_ERR_ARG, "a slot-mode codec serves at most 256 slots");
    HIPCHK(hipSetDevice(m->dev));
    if (!m->slot_mode) {  // the first reset since mimi_reset_state / creation: every row starts as an idle slot
      m->slot_mode = true;
      m->s_B = 0;
      slot_reset_launch(m, -1);
    } else {
      slot_reset_launch(m, b);
    }
  }
  CSM_CATCH
}

int mimi_decode_slots(mimi_codec* m, int B, int n, const int32_t* hist, int codes_on_device, int F_cap, int first_row,
                      const uint8_t* active, float* pcm) {
  CSM_TRY {
    if (!m || !hist || !active || !pcm) throw CsmError(CSM_ERR_ARG, "null codec, history, active mask or pcm");
    if (!m->slot_mode) throw CsmError(CSM_ERR_STATE, "mimi_slot_reset must precede mimi_decode_slots");
    if (B <= 0 || B > m->B_max) throw CsmError(CSM_ERR_ARG, "bad slot count");
    if (F_cap < 1 || n < 1 || n > F_cap) throw CsmError(CSM_ERR_ARG, "bad frame count for the ring history");
    if (first_row < 0 || first_row >= F_cap) throw CsmError(CSM_ERR_ARG, "first ring row out of range");
    const mimi_dims& d = m->d;
    const int s = d.downsample_stride, steps = n * s;
    if (steps + 4 > m->S_cap) throw CsmError(CSM_ERR_ARG, "more frames than the codec capacity");
    for (int b = 0; b < B; ++b)
      if (active[b] && m->slot_pos_host[b] + steps + 4 > m->S_cap)
        throw CsmError(CSM_ERR_ARG, "slot " + std::to_string(b) + ": stream longer than the codec capacity");
    HIPCHK(hipSetDevice(m->dev));
    // an idle row still flows through the pass at its own position: one whose last stream stopped near the
    // end of the cache goes back to 0 first (it starts its next stream with a reset anyway)
    for (int b = 0; b < B; ++b)
      if (!active[b] && m->slot_pos_host[b] + steps + 4 > m->S_cap) slot_reset_launch(m, b);
    const size_t per = decoder_ws(m, steps);
    ensure_ws(m, per * B + 64, (size_t)B * steps + 8);
    const int32_t* dc = hist;
    if (!codes_on_device) {
      const size_t ring = (size_t)F_cap * B * d.n_q;
      grow(m->dcodes, m->dcodes_n, ring);
      HIPCHK(hipMemcpyAsync(m->dcodes, hist, ring * 4, hipMemcpyHostToDevice, m->st));
      dc = m->dcodes;
    }
    decode_frames(m, B, n, dc, 2, true, true, first_row, F_cap);
    MimiSlotMask mask{};
    for (int b = 0; b < B; ++b) {
      mask.v[b] = active[b] ? 1 : 0;
      if (active[b]) m->slot_pos_host[b] += steps;
    }
    launch_mimi_slot_advance(m->slot_pos, mask, B, steps, m->st);
    const Pcm out = decoder_pcm(m, steps);
    HIPCHK(hipMemcpyAsync(pcm, out.p, (size_t)B * out.n * 4, hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    HIPCHK(hipGetLastError());
  }
  CSM_CATCH
}

int mimi_encode_slot_reset(mimi_codec* m, int b) {
  CSM_TRY {
    if (!m) throw CsmError(CSM_ERR_ARG, "null codec");
    if (b < 0 || b >= m->B_max) throw CsmError(CSM_ERR_ARG, "codec slot index out of range");
    if (m->B_max > MIMI_SLOTS_MAX) throw CsmError(CSM_ERR_ARG, "a streaming encoder serves at most 256 slots");
    HIPCHK(hipSetDevice(m->dev));
    if (!m->enc_ready) {  // the first reset allocates the state (zeroed: every row an idle slot at position 0)
      const mimi_dims& d = m->d;
      for (const MOp& o : m->enc_ops) {
        const int P = m->op_pad(o);
        m->enc_hist.push_back(P > 0 ? (float*)m->alloc((size_t)m->B_max * m->op_cin(o) * P * 4) : nullptr);
      }
      m->enc_down_hist = (float*)m->alloc((size_t)m->B_max * d.dimension * d.downsample_stride * 4);
      const size_t kv = (size_t)(m->B_max + 1) * d.num_heads * m->S_cap * m->hd * 4;
      for (int l = 0; l < d.num_layers; ++l) {
        m->enc_kc.push_back((float*)m->alloc(kv));
        m->enc_vc.push_back((float*)m->alloc(kv));
      }
      m->enc_pos = (int*)m->alloc((size_t)m->B_max * 4);
      m->enc_pos_host.assign(m->B_max, 0);
      m->enc_ready = true;
    }
    enc_slot_reset_launch(m, b);
  }
  CSM_CATCH
}

int mimi_encode_slots(mimi_codec* m, int B, int n, const float* pcm, const uint8_t* active, int32_t* codes) {
  CSM_TRY {
    if (!m || !pcm || !active || !codes) throw CsmError(CSM_ERR_ARG, "null codec, pcm, active mask or codes");
    if (!m->enc_ready) throw CsmError(CSM_ERR_STATE, "mimi_encode_slot_reset must precede mimi_encode_slots");
    if (B <= 0 || B > m->B_max || B > MIMI_SLOTS_MAX) throw CsmError(CSM_ERR_ARG, "bad slot count");
    if (n < 1) throw CsmError(CSM_ERR_ARG, "bad frame count");
    const mimi_dims& d = m->d;
    const int s = d.downsample_stride, D = d.dimension, cd = d.codebook_dim;
    if ((int64_t)n * s + 4 > m->S_cap) throw CsmError(CSM_ERR_ARG, "more frames than the codec capacity");
    const int steps = n * s, N = n * mimi_frame_size(m);
    // refused before anything is launched: no stream changes
    for (int b = 0; b < B; ++b)
      if (active[b] && m->enc_pos_host[b] + steps + 4 > m->S_cap)
        throw CsmError(CSM_ERR_ARG, "slot " + std::to_string(b) + ": stream longer than the codec capacity");
    HIPCHK(hipSetDevice(m->dev));
    hipStream_t st = m->st;
    ensure_ws(m, encoder_stream_ws(m, N) * B + 64, (size_t)B * steps + 8);
    MimiSlotMask mask{};
    bool spare = false;  // an inactive slot too near the end of its cache for this pass's keys
    for (int b = 0; b < B; ++b) {
      mask.v[b] = active[b] ? 1 : 0;
      spare = spare || (!active[b] && m->enc_pos_host[b] + steps + 4 > m->S_cap);
    }
    // pcm rows behind conv0's history
    const int P0 = m->op_pad(m->enc_ops[0]);
    HIPCHK(hipMemcpy2DAsync(m->W0 + P0, (size_t)(P0 + N) * 4, pcm, (size_t)N * 4, (size_t)N * 4, (size_t)B,
                            hipMemcpyHostToDevice, st));
    int n25 = 0;
    float* lat = run_encoder_stream(m, B, N, mask, &n25);
    if (n25 != steps) throw CsmError(CSM_ERR_HIP, "mimi streaming encoder: frame bookkeeping");
    launch_conv_to_rows(lat, B, D, steps, D * steps, steps, 0, m->R, st);
    // an inactive slot's rows run at its own position, on keys it overwrites when it goes on; one that has no
    // room left there runs in the caches' spare row from position 0 (per-row tables from the host mirror)
    std::vector<int> tab;
    if (spare) {
      const size_t M = (size_t)B * steps;
      tab.resize(2 * M);
      for (int b = 0; b < B; ++b) {
        const bool sp = !active[b] && m->enc_pos_host[b] + steps + 4 > m->S_cap;
        for (int t = 0; t < steps; ++t) {
          tab[(size_t)b * steps + t] = sp ? m->B_max : b;
          tab[M + (size_t)b * steps + t] = (sp ? 0 : m->enc_pos_host[b]) + t;
        }
      }
      grow(m->enc_rowtab, m->enc_rowtab_n, 2 * M);
      HIPCHK(hipMemcpyAsync(m->enc_rowtab, tab.data(), 2 * M * 4, hipMemcpyHostToDevice, st));
      run_transformer(m, m->etr, m->enc_kc, m->enc_vc, B, steps, 0, m->enc_pos, m->enc_rowtab, m->enc_rowtab + M);
    } else {
      run_transformer(m, m->etr, m->enc_kc, m->enc_vc, B, steps, 0, m->enc_pos);
    }
    // downsample (k = 2s, stride s) on its window; a stream's first call pads with its first latent step
    float* win = lat == m->W0 ? m->W1 : m->W0;
    float* out = lat;
    launch_rows_to_conv(m->R, B, D, steps, win, D * (s + steps), s + steps, s, st);
    launch_mimi_window_roll(m->enc_down_hist, win, B, D, s, steps, mask, m->enc_pos, st);
    const MConv down{D, D, 2 * s, s, 1, 0, m->down_w, nullptr};
    launch_conv1d(conv_params(m, down, Act{win, s + steps, 0, s + steps}, Act{out, n, 0, n}, B, 0), st);
    launch_conv_to_rows(out, B, D, n, D * n, n, 0, m->R, st);
    const int M = B * n;
    m->r_rows = (size_t)M;  // R: the pre-RVQ latent, read only from here on
    grow(m->dcodes, m->dcodes_n, (size_t)B * d.n_q * n);
    for (int q = 0; q < 2; ++q) {
      launch_linear(lin_params(m, m->R, M, D, m->rvq_in[q], cd, m->Rh), st);
      const int k0 = q == 0 ? 0 : 1, k1 = q == 0 ? 1 : d.n_q;
      if (k1 <= k0) continue;
      if (M >= 256 && rvq_gemm_eligible(cd, d.bins)) {  // the rule of mimi_encode_rows
        grow(m->rvq_r, m->rvq_r_n, (size_t)2 * M * cd);
        grow(m->rvq_p, m->rvq_p_n, 2 * rvq_gemm_parts(M, d.bins));
        launch_rvq_encode_gemm(m->Rh, M, n, cd, m->cb, m->cbT, m->c2half, d.bins, k0, k1, d.n_q, m->dcodes, m->rvq_r,
                               m->rvq_p, st);
      } else {
        launch_rvq_encode(m->Rh, M, n, cd, m->cb, m->c2half, d.bins, k0, k1, d.n_q, m->dcodes, st);
      }
    }
    for (int b = 0; b < B; ++b)
      if (active[b]) m->enc_pos_host[b] += steps;
    launch_mimi_slot_advance(m->enc_pos, mask, B, steps, st);
    HIPCHK(hipMemcpyAsync(codes, m->dcodes, (size_t)B * d.n_q * n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
  }
  CSM_CATCH
}

int mimi_debug_read(mimi_codec* m, const char* what, void* host, int64_t nbytes, int64_t* needed) {
  CSM_TRY {
    if (!m || !what) throw CsmError(CSM_ERR_ARG, "bad mimi_debug_read arguments");
    const std::string w(what);
    if (w == "launches") {  // the process-wide host counter of codec kernel launches, one int64
      if (needed) *needed = 8;
      if (host) {
        if (nbytes < 8) throw CsmError(CSM_ERR_ARG, "debug buffer too small");
        const long long v = mimi_kernel_launches();
        memcpy(host, &v, 8);
      }
      return CSM_OK;
    }
    if (w != "rows") throw CsmError(CSM_ERR_ARG, "unknown codec debug tap " + w);
    if (!m->R || !m->r_rows) throw CsmError(CSM_ERR_STATE, "no encode / decode call has run yet");
    HIPCHK(hipSetDevice(m->dev));
    HIPCHK(hipStreamSynchronize(m->st));
    const size_t n = m->r_rows * (size_t)m->d.dimension * 4;
    if (needed) *needed = (int64_t)n;
    if (host) {
      if (nbytes < 0 || (size_t)nbytes < n) throw CsmError(CSM_ERR_ARG, "debug buffer too small");
      HIPCHK(hipMemcpy(host, m->R, n, hipMemcpyDeviceToHost));
    }
  }
  CSM_CATCH
}

}  // extern "C"
