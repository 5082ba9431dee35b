// The blocks the projection kernels share -- y = norm(x) W^T as gemv_kernel / gemv_xl_kernel
// (csm_kernels.hip), gemv_q4_kernel (q4_kernels.hip), gemm_wide_kernel (gemm_kernels.hip) and
// gemm_xs_kernel (gemm_xs.hip), plus gather_rows_kernel -- each defined once:
//   argmax_code / resolve_code / gather_codes   the code of a gathered row from the producer's arg-max partials
//   PairMap / pair_sum / pair_key / wave_max_key   the parts of the GEMV tail: pair thread map, group sum, arg-max key
//   tiled_copy_or_abort / require_scratch / gemm_ws_grow   the host side of the two matrix-core launchers
//   the vector typedefs and buffer-resource constants of the two matrix-core sources
// Every kernel keeps its own K loop, LDS layout and n < N guards; nothing here changes a summation
// order or a cache policy.  Three blocks stay written in their kernels, because folded they moved
// registers or rescheduled a kernel: the row source of each GEMV and of
// gather_rows_kernel, the skeleton of each GEMV's tail around the parts, and the split-K hand-off and
// tile arg-max of gemm_wide_kernel and gemm_xs_kernel, whose device code is the same as before the fold.
#pragma once
#include <cstdio>
#include <cstdlib>

#include "csm_kernels.h"

namespace gp {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) unsigned int gu32;

constexpr int RSRC3 = 0x00020000;  // buffer descriptor word 3 (raw 32-bit format)
constexpr int SC1 = 16;            // cache policy: sc1 (agent-coherent, as __hip_atomic_load/store)
constexpr int NT = 2;              // cache policy: non-temporal
constexpr int MAX_SLICES = 16;     // split-K slices of a tile at most

// ---------------------------------------------------------------------------- gathered-row codes
// The code a producer's arg-max partials pp[0..n) name, clamped into the vocabulary (a row of NaN
// logits leaves no winner).  One wave; every lane returns it.
__device__ __forceinline__ int argmax_code(const unsigned long long* pp, int n, int lane, int V) {
  return min(max(unpack_argmax(wave_argmax_partials(pp, n, lane)), 0), V - 1);
}

// x gather mode (GemvParams::xpart): row m is a table row, except the even rows of decoder step 1
// (x_step1), which are the dense rows m >> 1
__device__ __forceinline__ bool gathered(const GemvParams& p, int m) { return p.xpart && !(p.x_step1 && !(m & 1)); }
__device__ __forceinline__ int dense_row(const GemvParams& p, int m) { return p.x_step1 ? (m >> 1) : m; }

// One wave resolves gathered row m's code; with `publish` its lane 0 also writes codes[b][xcb].
__device__ __forceinline__ int resolve_code(const GemvParams& p, int m, int lane, bool publish) {
  const int bb = dense_row(p, m);
  const int c = argmax_code(p.xpart + (size_t)bb * p.xpart_stride, p.xpart_n, lane, p.xV);
  if (publish && lane == 0) p.x_codes[(size_t)bb * p.x_codes_K + p.xcb] = c;
  return c;
}

// The gather prologue of a 256-thread block: codes of rows m0 .. m0 + mn - 1 into gcode[0..mn), a
// wave per row, then a barrier.
__device__ __forceinline__ void gather_codes(const GemvParams& p, int m0, int mn, int* gcode, bool publish) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = wave; i < mn; i += 4) {
    if (!gathered(p, m0 + i)) continue;
    const int c = resolve_code(p, m0 + i, lane, publish);
    if (lane == 0) gcode[i] = c;
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------- GEMV tail
// Packed arg-max key of the pair (n, n + 1): the entries below n_valid (the unpadded vocabulary)
__device__ __forceinline__ unsigned long long pair_key(const GemvParams& p, int n, float a, float b) {
  unsigned long long key = n < p.n_valid ? pack_argmax(a, n) : 0ull;
  if (n + 1 < p.n_valid) {
    const unsigned long long kb = pack_argmax(b, n + 1);
    key = kb > key ? kb : key;
  }
  return key;
}
__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}
// Thread tid < NPAIR of a block of NG groups x MT rows x RPT weight rows owns one pair: group g, row i,
// weight rows rp, rp + 1 of the group
template <int NG, int MT, int RPT>
struct PairMap {
  static constexpr int NPAIR = NG * MT * (RPT / 2);
  int g, i, rp;
  __device__ __forceinline__ explicit PairMap(int tid)
      : g(tid / (MT * (RPT / 2))), i(tid % (MT * (RPT / 2)) / (RPT / 2)), rp(tid % (RPT / 2) * 2) {}
};
// the pair's two dot products: the group's WPG wave partials from red, in wave order
template <int WPG, int MT, int RS>
__device__ __forceinline__ void pair_sum(const float (&red)[4][MT][RS], int g, int i, int rp, float& a, float& b) {
  a = 0.f;
  b = 0.f;
#pragma unroll
  for (int w = 0; w < WPG; ++w) {
    a += red[g * WPG + w][i][rp];
    b += red[g * WPG + w][i][rp + 1];
  }
}

// ---------------------------------------------------------------------------- host side
// The fragment-tiled copy of p.W (built by the engine, launch_gemm_retile, outside graph capture)
inline const void* tiled_copy_or_abort(const GemvParams& p) {
  if (p.ws) {
    const auto ti = p.ws->tiled.find(p.W);
    if (ti != p.ws->tiled.end()) return ti->second;
  }
  fprintf(stderr, "csm: no fragment-tiled copy of an N=%d K=%d weight for the MFMA path\n", p.N, p.K);
  abort();
}

// A split launch's slab and tickets from the engine's scratch (reserved outside graph capture); `what`
// prefixes the message ("" or "gemm_xs ")
inline void require_scratch(GemvParams& p, size_t need, size_t tk, const char* what) {
  if (!p.ws || need > p.ws->bytes || tk > p.ws->n) {
    fprintf(stderr, "csm: %ssplit-K scratch not reserved for N=%d K=%d M=%d\n", what, p.N, p.K, p.M);
    abort();
  }
  p.kpart = p.ws->kpart;
  p.kticket = p.ws->tickets;
}

// Grow ws to a slab of `slab` bytes and `tk` zeroed tickets.  True when a buffer was reallocated
// (graphs holding the old ones are stale).
inline bool gemm_ws_grow(GemmWs& ws, size_t slab, size_t tk) {
  bool moved = false;
  if (slab > ws.bytes) {
    if (ws.kpart) (void)hipFree(ws.kpart);
    ws.kpart = nullptr;
    ws.bytes = 0;
    if (hipMalloc(&ws.kpart, slab) == hipSuccess) ws.bytes = slab;
    moved = true;
  }
  if (tk > ws.n) {
    if (ws.tickets) (void)hipFree(ws.tickets);
    ws.tickets = nullptr;
    ws.n = 0;
    if (hipMalloc(&ws.tickets, tk * 4) == hipSuccess && hipMemset(ws.tickets, 0, tk * 4) == hipSuccess &&
        hipDeviceSynchronize() == hipSuccess)  // (null-stream fill, drained before engine-stream use)
      ws.n = tk;
    moved = true;
  }
  return moved;
}

}  // namespace gp
