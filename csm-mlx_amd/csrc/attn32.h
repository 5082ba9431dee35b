// The depth decoder's attention of one (row, query head) by one wave: at most 32 cached positions, head_dim
// 128, fp32 throughout -- the one definition of the arithmetic that attn_short_head (csm_kernels.hip, the
// launch path), phase_attn (dec_frame.hip) and role_a (dec_step_xs.hip) share, so every execution path
// returns the same bits.  Two lane maps over the wave (all 64 lanes active):
//   scores  lane = (key kj = lane & 31, half hh = lane >> 5 of the head dims)
//   P.V     lane = (key half kv = lane >> 5: keys 16 kv .. 16 kv + 15, dims 4 dq .. 4 dq + 3, dq = lane & 31)
// A kernel calls the pieces between its own loads and stores; what differs per kernel stays there: where a
// key / value row comes from, the query staging and its wave fence, the layer-0 table gather with its cache,
// code and residual writes, every store of the output, barriers, flags and stamps.  The pieces are typed on
// the callers' vector types (HIP's float4 or an ext-vector float4): none converts.
#pragma once
#include "common.h"

namespace attn32 {

constexpr int HD = 128, NMAX = 32;  // fixed: the lane maps above (16 keys a half, readlane 16 + u) are written for them
// 1 / sqrt(HD) of the persistent kernels; the same float32 (bits 0x3DB504F3) as the host's
// 1.0f / sqrtf(128.f) that the launch path carries in AttnParams::scale
constexpr float SCALE = 0.08838834764831845f;

// Key kj's score against the scaled query.  k, q: this lane's half (hh) of the key row and of the query, in
// registers or LDS.  Four fmaf chains, the halves added by one shuffle (half 0 + half 1 on both lanes).
template <typename KT, typename QT>
__device__ __forceinline__ float score(const KT* k, const QT* q, int hh) {
  float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
#pragma unroll
  for (int d4 = 0; d4 < HD / 8; ++d4) {
    const KT a = k[d4];
    const QT b = q[d4];
    d0 = fmaf(b.x, a.x, d0);
    d1 = fmaf(b.y, a.y, d1);
    d2 = fmaf(b.z, a.z, d2);
    d3 = fmaf(b.w, a.w, d3);
  }
  const float part = (d0 + d1) + (d2 + d3);
  const float other = __shfl_xor(part, 32, 64);
  return hh == 0 ? part + other : other + part;
}

// Max-subtracted softmax over the n live keys in one pass: the bits of this lane's unnormalised probability
// (pv reads them through readlane) and the sum over the keys
struct Probs { int pji; float l_run; };
__device__ __forceinline__ Probs softmax(float s, int kj, int hh, int n) {
  if (kj >= n) s = -INFINITY;
  const float mx = wave_max(s);
  const float pj = kj < n ? expf(s - mx) : 0.f;
  return {__float_as_int(pj), wave_sum(hh == 0 ? pj : 0.f)};
}

// acc += p[j] * V[j] over keys j = 16 kv + u0 + u < n, u ascending; vv[u]: dims 4 dq .. 4 dq + 3 of key j's
// value row (rows past the last key are read but not used)
template <int U, typename AT, typename VT>
__device__ __forceinline__ void pv(AT& acc, int pji, const VT (&vv)[U], int u0, int kv, int n) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const float pa = __int_as_float(__builtin_amdgcn_readlane(pji, u0 + u));
    const float pb = __int_as_float(__builtin_amdgcn_readlane(pji, 16 + u0 + u));
    const float pw = kv ? pb : pa;
    if (16 * kv + u0 + u < n) {
      acc.x = fmaf(pw, vv[u].x, acc.x);
      acc.y = fmaf(pw, vv[u].y, acc.y);
      acc.z = fmaf(pw, vv[u].z, acc.z);
      acc.w = fmaf(pw, vv[u].w, acc.w);
    }
  }
}

// The two key halves' sums added by one exchange (lanes < 32: keys 0-15 + keys 16-31) and normalised:
// dims 4 dq .. 4 dq + 3 of the output
template <typename AT>
__device__ __forceinline__ AT finish(const AT& acc, float l_run) {
  const float t0 = __shfl_xor(acc.x, 32, 64), t1 = __shfl_xor(acc.y, 32, 64), t2 = __shfl_xor(acc.z, 32, 64),
              t3 = __shfl_xor(acc.w, 32, 64);
  const float inv = 1.f / l_run;
  AT o;
  o.x = (acc.x + t0) * inv;
  o.y = (acc.y + t1) * inv;
  o.z = (acc.z + t2) * inv;
  o.w = (acc.w + t3) * inv;
  return o;
}

// Half-group sum for an int4 o_proj: 32 columns = lanes dq = 8j .. 8j + 7, each lane's 4 in order, a butterfly
template <typename AT>
__device__ __forceinline__ float half_group_sum(const AT& o) {
  float hs = (o.x + o.y) + (o.z + o.w);
  hs += __shfl_xor(hs, 1, 64);
  hs += __shfl_xor(hs, 2, 64);
  hs += __shfl_xor(hs, 4, 64);
  return hs;
}

}  // namespace attn32
