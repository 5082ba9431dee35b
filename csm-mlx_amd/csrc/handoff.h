// Inter-workgroup hand-off primitives of the persistent kernels (dec_frame.hip, bb_step.hip,
// dec_step_xs.hip).
// A value travels as one naturally aligned 8-byte granule {fp32 bits, tag} written by ONE agent-scope
// relaxed (sc1) store and read with agent-scope relaxed (sc1) loads until the tag matches
// (MI355X_MICROARCH.md, inter-workgroup visibility and the hand-off price list).
#pragma once
#include "common.h"

namespace handoff {

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

__device__ __forceinline__ u64 gload(const u64* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void gput(u64* p, float v, unsigned tag) {
  __hip_atomic_store(p, ((u64)tag << 32) | __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void gput_u(u64* p, unsigned v, unsigned tag) {
  __hip_atomic_store(p, ((u64)tag << 32) | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void sc1_store_f(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 16-B agent-coherent (sc1) load at byte offset `off` of a buffer of `bytes` bytes
__device__ __forceinline__ u32x4_t sc1_load16(const void* base, int off, int bytes) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
  return __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 16));
}

// 8 products of one 16-B bf16 weight chunk with 8 consecutive fp32 activations (fixed order)
__device__ __forceinline__ float dot8(const u32x4_t w, const float* x) {
  const float4 a = *reinterpret_cast<const float4*>(x), b = *reinterpret_cast<const float4*>(x + 4);
  float s = bf16_lo(w.x) * a.x;
  s = fmaf(bf16_hi(w.x), a.y, s);
  s = fmaf(bf16_lo(w.y), a.z, s);
  s = fmaf(bf16_hi(w.y), a.w, s);
  s = fmaf(bf16_lo(w.z), b.x, s);
  s = fmaf(bf16_hi(w.z), b.y, s);
  s = fmaf(bf16_lo(w.w), b.z, s);
  s = fmaf(bf16_hi(w.w), b.w, s);
  return s;
}

// 16-B weight load as a raw buffer load: the matrix base rides in the (uniform) descriptor, the
// lane-dependent part in ONE voffset register shared by every layer and row, the row / chunk step in
// the scalar offset -- so per-layer weight addresses are not VGPR pairs the compiler keeps live
// across the frame loop.
// AUX: cache policy (2 = nt), a compile-time constant so no load sits in a branch of its own.
template <int AUX = 0>
__device__ __forceinline__ u32x4_t bload(const void* base, int voff, int soff) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000);
  return __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, AUX));
}

// The bounded-spin test of every hand-off wait: true once `spin` reaches `limit`, or -- looked at
// every 256 spins -- once another workgroup has raised the error word; either way the word is raised
// and the caller stops waiting (results garbage, the host raises), so the grid always drains.
__device__ __forceinline__ bool spin_fail(int* err, unsigned limit, unsigned spin) {
  if (spin >= limit || ((spin & 255) == 255 && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
    __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
  }
  return false;
}
// ... bound to a kernel's context (its args carry the error word)
constexpr unsigned SPIN_LIMIT = 1u << 22;  // ~0.1 s of s_sleep per hand-off before declaring failure
template <typename C>
__device__ __forceinline__ bool spin_fail(const C& c, unsigned spin) { return spin_fail(c.p.err, SPIN_LIMIT, spin); }

// threadIdx.x through an opaque move: lane-dependent addresses derived from it inside the frame loop
// are recomputed per iteration instead of being hoisted out of the loop and held (spilled) for the
// whole frame.
__device__ __forceinline__ int opaque_tid() {
  int t;
  asm volatile("v_mov_b32 %0, %1" : "=v"(t) : "v"((int)threadIdx.x));
  return t;
}

// The hand-off context of the persistent single-row kernels (dec_frame.hip, bb_step.hip): workgroup w's
// view of the granule buffer p.gbuf at hand-off number e.  A region is double-buffered by hand-off parity.
// An all-gather region (every workgroup reads every granule) is written in REP replicas, each
// rs_of(per) granules apart -- 4 KB-aligned plus a 256-B skew, so the replicas fall on different
// channels -- and workgroup w polls replica w % REP (speed only, never correctness).
__host__ __device__ constexpr size_t rs_of(size_t per) { return (per + 511) / 512 * 512 + 32; }
template <typename Args, typename Lds, int REP>
struct HandoffCtx {
  const Args& p;
  Lds& L;
  int w, tid, lane, wave;
  unsigned tag0;
  int e;  // hand-off counter
  __device__ void refresh() {
    tid = opaque_tid();
    lane = tid & 63;
    wave = tid >> 6;
  }
  __device__ unsigned tag() const { return tag0 + (unsigned)e; }
  __device__ u64* buf(size_t region, size_t per) const { return p.gbuf + region + (size_t)(e & 1) * per; }
  // replicated regions: replica r, this workgroup's replica (reads), and a store to one replica r of
  // granule i -- the publishing lanes are spread over the replicas (lane-parallel stores, one per lane),
  // so a hand-off costs its producer one store instruction, not REP
  __device__ u64* rbuf(size_t region, size_t per, int r) const {
    return p.gbuf + region + ((size_t)(e & 1) * REP + (size_t)r) * rs_of(per);
  }
  __device__ u64* rbuf(size_t region, size_t per) const { return rbuf(region, per, w % REP); }
  __device__ void put(size_t region, size_t per, size_t i, float v, int r) const { gput(rbuf(region, per, r) + i, v, tag()); }
  __device__ void put_u(size_t region, size_t per, size_t i, unsigned v, int r) const {
    gput_u(rbuf(region, per, r) + i, v, tag());
  }
};

// Wait until this thread's granules base[off[u]] (u < GPT, val[u]) carry `tag`, then use(probe).
// One probe, its stale granules re-polled.  The first probe's loads are unconditional (an unused
// entry reads granule 0 and counts as current): no branch around a load, so the compiler's vmcnt
// waits stay exact.  A granule's tag only moves from stale to current during a wait (its buffer is
// rewritten only after every workgroup has published the next hand-off), so any all-current probe is
// the hand-off.  fail(spin): the bounded-spin / error-flag test.  DELAY: sleeps before the first probe
// (fewer wasted probes while the producers are still working); REPOLL: sleeps between re-polls.
// Two probes in flight, each re-issued whole as soon as it returned stale, cost the frame decoder
// +12 % (profiles/r03_ab_poll.txt): every re-issued probe adds sc1 traffic on the lines every
// workgroup polls.
template <int GPT, int DELAY, int REPOLL, typename Fail, typename F>
__device__ __forceinline__ void poll_granules(const u64* base, const int (&off)[GPT], const bool (&val)[GPT], unsigned tag,
                                              Fail&& fail, F&& use) {
  auto cur = [&](const u64 (&x)[GPT]) {
    bool ok = true;
#pragma unroll
    for (int u = 0; u < GPT; ++u) ok &= !val[u] || (unsigned)(x[u] >> 32) == tag;
    return ok;
  };
  if constexpr (DELAY > 0) __builtin_amdgcn_s_sleep(DELAY);
  u64 g[GPT];
#pragma unroll
  for (int u = 0; u < GPT; ++u) g[u] = gload(base + (val[u] ? off[u] : 0));
  for (unsigned spin = 0; !cur(g) && !fail(spin); ++spin) {
    __builtin_amdgcn_s_sleep(REPOLL);
#pragma unroll
    for (int u = 0; u < GPT; ++u)
      if (val[u] && (unsigned)(g[u] >> 32) != tag) g[u] = gload(base + off[u]);
  }
  use(g);
}

// poll_granules over granule PAIRS: one 16-B sc1 load per pair (granules 2i, 2i + 1: their tags in
// words 1 and 3), pair offsets in granules (even).  Same protocol and vmcnt discipline as
// poll_granules (one probe, stale pairs re-polled); use(x) gets the u32x4 of every pair.
// Tearing: correctness needs each naturally aligned 8-B half of a 16-B sc1 load (and of a producer's
// 16-B sc1 store of two granules) to be seen whole, never a fresh tag beside a stale value.  The HIP /
// HSA memory model promises that only for aligned atomics of <= 8 B; on gfx950 under ROCm 7.2 16-B
// sc1 accesses are observed untorn at 8-B halves, not as an architectural guarantee
// (MI355X_MICROARCH.md, inter-workgroup visibility: "R2's granule ... also for 16-B
// sc1 halves").  The guard is the data: the 125-frame bf16 fixtures (tests/test_long_gpu.py) and the
// determinism checks (tests/test_dec_frame_gpu.py) run every frame through these polls, and a torn
// read would put a stale partial into a sum and change codes or logits.
template <int GPP, int DELAY, int REPOLL, typename Fail, typename F>
__device__ __forceinline__ void poll_pairs(const u64* base, int bytes, const int (&off)[GPP], unsigned tag, Fail&& fail, F&& use) {
  auto cur1 = [&](const u32x4_t& x) { return x.y == tag && x.w == tag; };
  if constexpr (DELAY > 0) __builtin_amdgcn_s_sleep(DELAY);
  u32x4_t g[GPP];
#pragma unroll
  for (int u = 0; u < GPP; ++u) g[u] = sc1_load16(base, off[u] * 8, bytes);
  for (unsigned spin = 0;; ++spin) {
    bool ok = true;
#pragma unroll
    for (int u = 0; u < GPP; ++u) ok &= cur1(g[u]);
    if (ok || fail(spin)) break;
    __builtin_amdgcn_s_sleep(REPOLL);
#pragma unroll
    for (int u = 0; u < GPP; ++u)
      if (!cur1(g[u])) g[u] = sc1_load16(base, off[u] * 8, bytes);
  }
  use(g);
}

// ---- int4 (MLX affine, group 64; common.h layout) weight chunks for the persistent kernels
// 4-B raw buffer load (an int4 group's {scale, bias} word), descriptor as bload
template <int AUX = 0>
__device__ __forceinline__ unsigned bload4(const void* base, int voff, int soff) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000);
  return __builtin_amdgcn_raw_buffer_load_b32(rs, voff, soff, AUX);
}
// One 16-B chunk of 32 nibbles (a half group: word i holds elements 8i .. 8i + 7, byte b elements 8i + 2b
// (low nibble) and 8i + 2b + 1) against 32 consecutive fp32 activations x (LDS), with that half group's
// affine word sb and activation sum hs: scale * sum_j q_j x_j + bias * sum_j x_j (the int4 GEMV's
// per-half-group arithmetic, q4_kernels.hip gemv_q4_kernel).
__device__ __forceinline__ float q4dot32(const u32x4_t w, const float* x, unsigned sb, float hs) {
  float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned u = w[i], lo = u & 0x0F0F0F0Fu, hi = (u >> 4) & 0x0F0F0F0Fu;
    const float4 a = *reinterpret_cast<const float4*>(x + 8 * i), b = *reinterpret_cast<const float4*>(x + 8 * i + 4);
    d0 = fmaf((float)(lo & 0xFFu), a.x, d0);
    d1 = fmaf((float)(hi & 0xFFu), a.y, d1);
    d2 = fmaf((float)((lo >> 8) & 0xFFu), a.z, d2);
    d3 = fmaf((float)((hi >> 8) & 0xFFu), a.w, d3);
    d0 = fmaf((float)((lo >> 16) & 0xFFu), b.x, d0);
    d1 = fmaf((float)((hi >> 16) & 0xFFu), b.y, d1);
    d2 = fmaf((float)(lo >> 24), b.z, d2);
    d3 = fmaf((float)(hi >> 24), b.w, d3);
  }
  return fmaf(bf16_lo(sb), (d0 + d1) + (d2 + d3), bf16_hi(sb) * hs);
}
// 8 nibbles of one word (elements j < 8, low nibble of byte b = element 2b) against x[0..7]
__device__ __forceinline__ float q4dot8(unsigned u, const float* x) {
  const unsigned lo = u & 0x0F0F0F0Fu, hi = (u >> 4) & 0x0F0F0F0Fu;
  const float4 a = *reinterpret_cast<const float4*>(x), b = *reinterpret_cast<const float4*>(x + 4);
  float s = (float)(lo & 0xFFu) * a.x;
  s = fmaf((float)(hi & 0xFFu), a.y, s);
  s = fmaf((float)((lo >> 8) & 0xFFu), a.z, s);
  s = fmaf((float)((hi >> 8) & 0xFFu), a.w, s);
  s = fmaf((float)((lo >> 16) & 0xFFu), b.x, s);
  s = fmaf((float)((hi >> 16) & 0xFFu), b.y, s);
  s = fmaf((float)(lo >> 24), b.z, s);
  s = fmaf((float)(hi >> 24), b.w, s);
  return s;
}
// Padded LDS layout of an int4 kernel's activation row: each 32-element half group 36 floats apart, so
// the 64 lanes' 16-B reads of their own half groups fall on distinct banks (gemv_q4_kernel's layout)
__device__ __forceinline__ int q4p(int k) { return (k >> 5) * 36 + (k & 31); }
// sums of lanes 0-31 and of lanes 32-63 (wave_sum's DPP row reductions, rows combined per half)
__device__ __forceinline__ float2 half_sums(float v) {
  v += dpp_f<0x128>(v);
  v += dpp_f<0x124>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0xB1>(v);
  return make_float2(lane_f(v, 0) + lane_f(v, 16), lane_f(v, 32) + lane_f(v, 48));
}
// sum over each aligned group of 16 lanes, to all of them: a half group's 32 elements held as one pair
// (2t, 2t + 1) per thread, the 16 threads in a fixed (xor butterfly) order
__device__ __forceinline__ float sum16(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  return v;
}

}  // namespace handoff
