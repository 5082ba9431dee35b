// Mimi codec, lab door: one codec kernel launch on caller-supplied host arrays, and the launchers' own
// plan for a geometry (include/csm_hip_prof.h).  No codec handle (but mimi_kv_read, the inspection door of a
// codec's KV caches, at the end): every entry allocates on the current
// device, uploads, launches on a stream of its own with its own split-K scratch, downloads and frees.
// Output buffers arrive with the caller's initial content (a sentinel, or the values an accumulating
// store adds onto) and are returned whole, so a store outside the addressed region shows.
// Every entry checks its geometry against the array sizes before anything is launched: CSM_ERR_ARG.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/csm_hip_prof.h"
#include "engine_util.h"
#include "mimi_kernels.h"

namespace {

constexpr int64_t LAB_MAX = (int64_t)1 << 28;  // elements of any one array / columns of any one launch

struct LabBuf {
  void* p = nullptr;
  LabBuf() = default;
  LabBuf(const void* host, size_t bytes) { upload(host, bytes); }
  void upload(const void* host, size_t bytes) {
    HIPCHK(hipMalloc(&p, bytes ? bytes : 4));
    if (host && bytes) HIPCHK(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
  }
  ~LabBuf() { if (p) (void)hipFree(p); }
  LabBuf(const LabBuf&) = delete;
  LabBuf& operator=(const LabBuf&) = delete;
  float* f() const { return (float*)p; }
};

struct LabStream {
  hipStream_t st = nullptr;
  LabStream() { HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); }
  ~LabStream() { if (st) (void)hipStreamDestroy(st); }
};

void need(bool ok, const char* what) {
  if (!ok) throw CsmError(CSM_ERR_ARG, std::string("mimi lab: ") + what);
}

// last element + 1 of a [B][C][len] region at (bstride, cstride, off); -1 when a field is out of range
int64_t region_end(int64_t B, int64_t bstride, int64_t C, int64_t cstride, int64_t off, int64_t len) {
  if (B <= 0 || C <= 0 || len <= 0 || bstride < 0 || cstride < 0 || off < 0) return -1;
  if (bstride > LAB_MAX || cstride > LAB_MAX || off > LAB_MAX) return -1;
  return (B - 1) * bstride + (C - 1) * cstride + off + len;
}

enum { CV_CIN, CV_TIN, CV_XB, CV_XOFF, CV_XC, CV_COUT, CV_K, CV_STRIDE, CV_DIL, CV_PADL, CV_REPL, CV_ELU_IN, CV_TOUT,
       CV_YB, CV_YC, CV_YOFF, CV_RB, CV_RC, CV_ROFF, CV_B, CV_ELU_OUT, CV_N };
enum { CT_CIN, CT_TIN, CT_XB, CT_XC, CT_XOFF, CT_COUT, CT_S, CT_ELU_IN, CT_TIN0, CT_NIN, CT_YB, CT_YC, CT_YOFF, CT_B,
       CT_N };
enum { LN_M, LN_K, LN_XS, LN_N, LN_OS, LN_EPI, LN_GELU_ERF, LN_CONV_T, LN_CONV_B, LN_ACC, LN_N_FIELDS };

// The parameter blocks from the geometry arrays (pointers left null), every field range-checked; the
// sizes the arrays must have come back in *_need.
ConvParams conv_params(const int* g, int n, bool resid, int64_t& x_need, int64_t& w_need, int64_t& y_need,
                       int64_t& r_need) {
  need(g && n == CV_N, "conv1d geometry: 21 fields");
  ConvParams p{};
  p.Cin = g[CV_CIN]; p.Tin = g[CV_TIN]; p.x_bstride = g[CV_XB]; p.x_off = g[CV_XOFF]; p.x_cstride = g[CV_XC];
  p.Cout = g[CV_COUT]; p.k = g[CV_K]; p.stride = g[CV_STRIDE]; p.dil = g[CV_DIL]; p.pad_l = g[CV_PADL];
  p.replicate = g[CV_REPL] != 0; p.elu_in = g[CV_ELU_IN] != 0; p.Tout = g[CV_TOUT]; p.y_bstride = g[CV_YB];
  p.y_cstride = g[CV_YC]; p.y_off = g[CV_YOFF]; p.r_bstride = g[CV_RB]; p.r_cstride = g[CV_RC]; p.r_off = g[CV_ROFF];
  p.B = g[CV_B]; p.elu_out = g[CV_ELU_OUT] != 0;
  need(p.Cin > 0 && p.Cout > 0 && p.k > 0 && p.k <= 1024 && p.stride > 0 && p.dil > 0 && p.pad_l >= 0, "conv1d shape");
  need(p.stride <= 1024 && p.dil <= 1024 && p.pad_l <= (1 << 20), "conv1d shape");
  need(p.B > 0 && p.B <= 1024 && p.Tin > 0 && p.Tout > 0, "conv1d batch / lengths");
  need((int64_t)p.Cin * p.k <= (1 << 24) && p.Cout <= (1 << 20), "conv1d K / Cout");
  need((int64_t)p.B * p.Tout <= LAB_MAX && (int64_t)p.Tout * p.stride <= LAB_MAX, "conv1d columns");
  x_need = region_end(p.B, p.x_bstride, p.Cin, p.x_cstride, p.x_off, p.Tin);
  y_need = region_end(p.B, p.y_bstride, p.Cout, p.y_cstride, p.y_off, p.Tout);
  r_need = resid ? region_end(p.B, p.r_bstride, p.Cout, p.r_cstride, p.r_off, p.Tout) : 0;
  w_need = (int64_t)p.Cout * p.Cin * p.k;
  need(x_need > 0 && y_need > 0 && r_need >= 0, "conv1d strides / offsets");
  need(x_need <= LAB_MAX && y_need <= LAB_MAX && r_need <= LAB_MAX && w_need <= LAB_MAX, "conv1d array sizes");
  return p;
}

ConvTrParams convtr_params(const int* g, int n, int64_t& x_need, int64_t& w_need, int64_t& y_need) {
  need(g && n == CT_N, "convtr geometry: 14 fields");
  ConvTrParams p{};
  p.Cin = g[CT_CIN]; p.Tin = g[CT_TIN]; p.x_bstride = g[CT_XB]; p.x_cstride = g[CT_XC]; p.x_off = g[CT_XOFF];
  p.Cout = g[CT_COUT]; p.s = g[CT_S]; p.elu_in = g[CT_ELU_IN] != 0; p.t_in0 = g[CT_TIN0]; p.n_in = g[CT_NIN];
  p.y_bstride = g[CT_YB]; p.y_cstride = g[CT_YC]; p.y_off = g[CT_YOFF]; p.B = g[CT_B];
  need(p.Cin > 0 && p.Cin <= (1 << 20) && p.Cout > 0 && p.Cout <= (1 << 20) && p.s > 0 && p.s <= 64, "convtr shape");
  need(p.B > 0 && p.B <= 512 && p.n_in > 0 && p.t_in0 >= 0 && p.Tin > 0, "convtr batch / lengths");
  need((int64_t)p.t_in0 + p.n_in <= p.Tin, "convtr: inputs [t_in0, t_in0 + n_in) inside Tin");
  need((int64_t)p.B * p.n_in * p.s <= LAB_MAX, "convtr columns");
  x_need = region_end(p.B, p.x_bstride, p.Cin, p.x_cstride, p.x_off, p.Tin);
  y_need = region_end(p.B, p.y_bstride, p.Cout, p.y_cstride, p.y_off, (int64_t)p.n_in * p.s);
  w_need = (int64_t)p.s * p.Cout * p.Cin * 2;
  need(x_need > 0 && y_need > 0, "convtr strides / offsets");
  need(x_need <= LAB_MAX && y_need <= LAB_MAX && w_need <= LAB_MAX, "convtr array sizes");
  return p;
}

LinParams lin_params(const int* g, int n, int64_t& x_need, int64_t& w_need, int64_t& o_need) {
  need(g && n == LN_N_FIELDS, "linear geometry: 10 fields");
  LinParams p{};
  p.M = g[LN_M]; p.K = g[LN_K]; p.xs = g[LN_XS]; p.N = g[LN_N]; p.os = g[LN_OS]; p.epi = g[LN_EPI];
  p.gelu_erf = g[LN_GELU_ERF] != 0; p.conv_T = g[LN_CONV_T]; p.conv_bstride = g[LN_CONV_B]; p.accumulate = g[LN_ACC] != 0;
  need(p.M > 0 && p.M <= (1 << 20) && p.K > 0 && p.K <= (1 << 20) && p.N > 0 && p.N <= (1 << 20), "linear shape");
  need(p.xs >= p.K && p.xs <= (1 << 24), "linear: xs >= K");
  need(p.epi == EPI_STORE || p.epi == EPI_ADD || p.epi == EPI_GELU, "linear epilogue");
  x_need = (int64_t)(p.M - 1) * p.xs + p.K;
  w_need = (int64_t)p.N * p.K;
  if (p.conv_T) {
    need(p.conv_T > 0 && p.M % p.conv_T == 0, "linear conv store: M a multiple of T");
    need(p.conv_bstride >= 0 && p.conv_bstride <= LAB_MAX, "linear conv store: batch stride");
    o_need = (int64_t)(p.M / p.conv_T - 1) * p.conv_bstride + (int64_t)p.N * p.conv_T;
  } else {
    need(p.os >= p.N && p.os <= (1 << 24), "linear: os >= N");
    o_need = (int64_t)(p.M - 1) * p.os + p.N;
  }
  need(x_need <= LAB_MAX && w_need <= LAB_MAX && o_need <= LAB_MAX, "linear array sizes");
  return p;
}

void finish(hipStream_t st) {
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
}

}  // namespace

extern "C" {

int mimi_lab_plan(int op, const int* geo, int n_geo, int* out) {
  CSM_TRY {
    need(out != nullptr, "plan: no output");
    float ws_present = 0.f;  // the plan of a launch that has split-K scratch, as every codec launch does
    MimiPlan pl{};
    int64_t a, b, c, d;
    if (op == 0) {
      ConvParams p = conv_params(geo, n_geo, false, a, b, c, d);
      p.ks_ws = &ws_present;
      pl = mimi_plan_conv1d(p);
    } else if (op == 1) {
      ConvTrParams p = convtr_params(geo, n_geo, a, b, c);
      p.ks_ws = &ws_present;
      pl = mimi_plan_convtr(p);
    } else if (op == 2) {
      LinParams p = lin_params(geo, n_geo, a, b, c);
      p.ks_ws = &ws_present;
      pl = mimi_plan_linear(p);
    } else {
      need(false, "plan: op 0 conv1d, 1 convtr, 2 linear");
    }
    out[0] = pl.kernel; out[1] = pl.bm; out[2] = pl.ks; out[3] = pl.fold;
  }
  CSM_CATCH
}

int mimi_lab_conv1d(const int* geo, int n_geo, const float* x, int64_t x_n, const float* w, int64_t w_n, const float* bias,
                    const float* resid, int64_t r_n, float* y, float* y2, int64_t y_n) {
  CSM_TRY {
    int64_t xn, wn, yn, rn;
    ConvParams p = conv_params(geo, n_geo, resid != nullptr, xn, wn, yn, rn);
    need(x && w && y, "conv1d: x, w and y are required");
    need(x_n >= xn && w_n == wn && y_n >= yn && (!resid || r_n >= rn), "conv1d: an array is smaller than its geometry");
    need(x_n <= LAB_MAX && y_n <= LAB_MAX && r_n <= LAB_MAX, "conv1d array sizes");
    LabStream s;
    LabBuf dx(x, (size_t)x_n * 4), dw(w, (size_t)w_n * 4), dy(y, (size_t)y_n * 4), ws(nullptr, MIMI_KS_WS_FLOATS * 4);
    LabBuf db, dr, dy2;
    if (bias) db.upload(bias, (size_t)p.Cout * 4);
    if (resid) dr.upload(resid, (size_t)r_n * 4);
    if (y2) dy2.upload(y2, (size_t)y_n * 4);
    p.x = dx.f(); p.w = dw.f(); p.y = dy.f(); p.ks_ws = ws.f();
    p.bias = bias ? db.f() : nullptr; p.resid = resid ? dr.f() : nullptr; p.y2 = y2 ? dy2.f() : nullptr;
    launch_conv1d(p, s.st);
    finish(s.st);
    HIPCHK(hipMemcpy(y, dy.p, (size_t)y_n * 4, hipMemcpyDeviceToHost));
    if (y2) HIPCHK(hipMemcpy(y2, dy2.p, (size_t)y_n * 4, hipMemcpyDeviceToHost));
  }
  CSM_CATCH
}

int mimi_lab_convtr(const int* geo, int n_geo, const float* x, int64_t x_n, const float* wt, int64_t w_n, const float* bias,
                    float* y, int64_t y_n) {
  CSM_TRY {
    int64_t xn, wn, yn;
    ConvTrParams p = convtr_params(geo, n_geo, xn, wn, yn);
    need(x && wt && y, "convtr: x, wt and y are required");
    need(x_n >= xn && w_n == wn && y_n >= yn, "convtr: an array is smaller than its geometry");
    need(x_n <= LAB_MAX && y_n <= LAB_MAX, "convtr array sizes");
    LabStream s;
    LabBuf dx(x, (size_t)x_n * 4), dw(wt, (size_t)w_n * 4), dy(y, (size_t)y_n * 4), ws(nullptr, MIMI_KS_WS_FLOATS * 4);
    LabBuf db;
    if (bias) db.upload(bias, (size_t)p.Cout * 4);
    p.x = dx.f(); p.wt = dw.f(); p.y = dy.f(); p.ks_ws = ws.f(); p.bias = bias ? db.f() : nullptr;
    launch_convtr(p, s.st);
    finish(s.st);
    HIPCHK(hipMemcpy(y, dy.p, (size_t)y_n * 4, hipMemcpyDeviceToHost));
  }
  CSM_CATCH
}

int mimi_lab_linear(const int* geo, int n_geo, const float* x, int64_t x_n, const float* W, int64_t w_n, const float* scale,
                    float* out, int64_t out_n) {
  CSM_TRY {
    int64_t xn, wn, on;
    LinParams p = lin_params(geo, n_geo, xn, wn, on);
    need(x && W && out, "linear: x, W and out are required");
    need(x_n >= xn && w_n == wn && out_n >= on, "linear: an array is smaller than its geometry");
    need(x_n <= LAB_MAX && out_n <= LAB_MAX, "linear array sizes");
    LabStream s;
    LabBuf dx(x, (size_t)x_n * 4), dw(W, (size_t)w_n * 4), dout(out, (size_t)out_n * 4), ws(nullptr, MIMI_KS_WS_FLOATS * 4);
    LabBuf dsc;
    if (scale) dsc.upload(scale, (size_t)p.N * 4);
    p.x = dx.f(); p.W = dw.f(); p.out = dout.f(); p.ks_ws = ws.f(); p.scale = scale ? dsc.f() : nullptr;
    // the decode GEMV reads its rows eight floats at a time: the lab hands it only rows laid out so
    if (mimi_plan_linear(p).kernel == MIMI_KERNEL_GEMV) need(p.xs % 8 == 0 && p.os % 8 == 0, "linear (GEMV): xs, os % 8");
    launch_linear(p, s.st);
    finish(s.st);
    HIPCHK(hipMemcpy(out, dout.p, (size_t)out_n * 4, hipMemcpyDeviceToHost));
  }
  CSM_CATCH
}

int mimi_lab_layernorm(int M, int D, const float* x, const float* w, const float* b, float eps, float* out, int64_t out_n) {
  CSM_TRY {
    need(x && w && b && out, "layernorm: x, w, b and out are required");
    need(M > 0 && M <= (1 << 20) && D > 0 && D <= (1 << 20) && (int64_t)M * D <= LAB_MAX, "layernorm shape");
    need(out_n >= (int64_t)M * D && out_n <= LAB_MAX, "layernorm: out is smaller than M x D");
    LabStream s;
    LabBuf dx(x, (size_t)M * D * 4), dw(w, (size_t)D * 4), db(b, (size_t)D * 4), dout(out, (size_t)out_n * 4);
    launch_layernorm_rows(dx.f(), D, dw.f(), db.f(), eps, dout.f(), M, s.st);
    finish(s.st);
    HIPCHK(hipMemcpy(out, dout.p, (size_t)out_n * 4, hipMemcpyDeviceToHost));
  }
  CSM_CATCH
}

int mimi_lab_rvq_encode(int gemm, int M, int T, int cd, int bins, int n_q, int k0, int k1, const float* cb,
                        const float* c2half, float* r, int32_t* codes) {
  CSM_TRY {
    need(cb && c2half && r && codes, "rvq: cb, c2half, r and codes are required");
    need(M > 0 && M <= (1 << 16) && T > 0 && M % T == 0, "rvq rows: M a multiple of T");
    need(cd > 0 && cd % 4 == 0 && cd <= 1024 && bins > 0 && bins <= (1 << 16), "rvq: cd % 4, cd <= 1024");
    need(n_q > 0 && n_q <= 64 && k0 >= 0 && k0 < k1 && k1 <= n_q, "rvq codebook range");
    need(!gemm || rvq_gemm_eligible(cd, bins), "rvq distance GEMM: cd % 32, cd <= 256, bins % 256");
    const size_t cbn = (size_t)n_q * bins * cd, rn = (size_t)M * cd, cn = (size_t)M * n_q;
    LabStream s;
    LabBuf dcb(cb, cbn * 4), dc2(c2half, (size_t)n_q * bins * 4), dr(r, rn * 4), dcodes(codes, cn * 4);
    if (gemm) {
      std::vector<float> t(cbn);  // dims-major, as finish_codebook lays the engine's copy out
      for (int k = 0; k < n_q; ++k)
        for (int i = 0; i < bins; ++i)
          for (int j = 0; j < cd; ++j) t[((size_t)k * cd + j) * bins + i] = cb[((size_t)k * bins + i) * cd + j];
      LabBuf dcbT(t.data(), cbn * 4), rbuf(nullptr, 2 * rn * 4), pbuf(nullptr, 2 * rvq_gemm_parts(M, bins) * 8);
      launch_rvq_encode_gemm(dr.f(), M, T, cd, dcb.f(), dcbT.f(), dc2.f(), bins, k0, k1, n_q, (int*)dcodes.p, rbuf.f(),
                             (unsigned long long*)pbuf.p, s.st);
      finish(s.st);
    } else {
      launch_rvq_encode(dr.f(), M, T, cd, dcb.f(), dc2.f(), bins, k0, k1, n_q, (int*)dcodes.p, s.st);
      finish(s.st);
    }
    HIPCHK(hipMemcpy(r, dr.p, rn * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(codes, dcodes.p, cn * 4, hipMemcpyDeviceToHost));
  }
  CSM_CATCH
}

int mimi_kv_read(mimi_codec* m, int side, int b, int layer, int first, int rows, float* k, float* v) {
  CSM_TRY {
    MimiKvView c{};
    need(mimi_kv_view(m, side, layer, &c), "kv read: null codec, side (0 decoder, 1 streaming encoder) without a cache, or layer");
    need(b >= 0 && b < c.rows && first >= 0 && rows >= 1 && (int64_t)first + rows <= c.S_cap, "kv read: row or positions out of range");
    HIPCHK(hipSetDevice(c.dev));
    HIPCHK(hipStreamSynchronize(c.st));
    const size_t run = (size_t)rows * c.hd * 4, pitch = (size_t)c.S_cap * c.hd * 4;
    const size_t off = ((size_t)b * c.heads * c.S_cap + first) * c.hd;
    if (k) HIPCHK(hipMemcpy2D(k, run, c.k + off, pitch, run, c.heads, hipMemcpyDeviceToHost));
    if (v) HIPCHK(hipMemcpy2D(v, run, c.v + off, pitch, run, c.heads, hipMemcpyDeviceToHost));
  }
  CSM_CATCH
}

}  // extern "C"
