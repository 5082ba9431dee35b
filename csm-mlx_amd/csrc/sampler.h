// mlx_lm make_sampler(temp, top_k) on one row of logits (generation.py:51-52), per workgroup: the one
// definition of the building blocks that sample_kernel and sample_filtered_kernel (csm_kernels.hip, the
// launch path), the persistent frame decoder's sample_code (dec_frame.hip) and the batched depth
// step's role_s (dec_step_xs.hip) share, so all of them pick identical codes.  Restated in float64 by
// oracle/csm_oracle.py sample_one.  The rule:
//   - the top_k-th largest logit is the threshold, every logit >= it is kept (ties at the k-th value too);
//   - the pick is the max of logit * (1 / temperature) + Gumbel noise (csm_kernels.h gumbel_noise) over the
//     kept entries, the first max: the lowest index on ties, whatever the visiting order;
//   - a row that leaves no winner (NaN logits) is clamped into the vocabulary.
#pragma once
#include <hip/hip_runtime.h>

#include "csm_kernels.h"

namespace sampler {

// A block of NT threads holds a row in per-thread slots: slot i of thread tid is entry tid + NT * i,
// i < NPT, so a caller samples rows of V <= NT * NPT.  The callers' slot counts:
constexpr int SAMPLE_NPT = 16;           // sample_kernel, sample_filtered_kernel (256 threads): checked at launch
constexpr int DEC_FRAME_SAMPLE_NPT = 5;  // dec_frame.hip sample_code (512 threads): asserted against its VMAX
static_assert(DEC_XSD_SAMPLE_NPT == 5, "dec_step_xs.hip role_s (512 threads): the engine checks V <= 512 x 5");

// The LDS words the blocks below are handed, laid out for a caller of NWAVES waves that carves them out
// of one borrowed array (asserted large enough at the call site)
template <int NWAVES>
struct Scratch {
  uint32_t hist[256];     // topk_threshold: digit histogram of one radix pass
  uint32_t wsum[NWAVES];  //   per-wave totals of the suffix count
  uint32_t sh[2];         //   [prefix, remain]
  double bv[NWAVES];      // block_argmax<double>: (value, index) per wave
  int bi[NWAVES];
};

// The blocks below read slot i through a callable logit(i), wherever the caller keeps the row (dec_frame:
// LDS).  This is the callable of a row held in registers.
template <int NPT>
struct RegSlots {
  const float (&lv)[NPT];
  __device__ __forceinline__ float operator()(int i) const { return lv[i]; }
};

// The k-th largest of the row's V logits (logit(i): slot i of this thread, read only where its entry is
// < V): radix select of the order-preserving key, 8 bits per pass; the digit is found by a parallel
// suffix count over the 256 bins (thread t < 256 holds digit 255 - t), not a serial scan.  Every logit >=
// the result is in the top-k set.  Called by the whole block (barriers inside); LDS: hist 256 words, wsum
// one per wave, sh 2.
template <int NT, int NPT, typename Logit>
__device__ __forceinline__ float topk_threshold(int tid, int V, int k, uint32_t* hist, uint32_t* wsum, uint32_t* sh,
                                                Logit&& logit) {
  static_assert(NT == 256 || NT == 512, "one thread per bin, further waves only count");
  const int lane = tid & 63, wave = tid >> 6;  // (made uniform by readfirstlane: sample_kernel 72 -> 90 VGPRs)
  const bool bin = NT == 256 || tid < 256;
  uint32_t prefix = 0, maskbits = 0, rem = (uint32_t)k;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (bin) hist[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      if (tid + NT * i < V) {
        const uint32_t key = f2key(logit(i));
        if ((key & maskbits) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    uint32_t h = 0, cnt = 0;
    if (bin) {
      h = hist[255 - tid];
      cnt = h;  // inclusive prefix over t = count of keys with digit >= 255 - t
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(cnt, o, 64);
        if (lane >= o) cnt += u;
      }
      if (lane == 63) wsum[wave] = cnt;
    }
    __syncthreads();
    if (bin) {
      for (int w = 0; w < wave; ++w) cnt += wsum[w];
      const uint32_t above = cnt - h;
      if (h > 0 && above < rem && rem <= cnt) {  // exactly one digit
        sh[0] = prefix | ((uint32_t)(255 - tid) << shift);
        sh[1] = rem - above;
      }
    }
    __syncthreads();
    prefix = sh[0];
    rem = sh[1];
    maskbits |= 255u << shift;
    __syncthreads();  // hist / sh reused by the next pass
  }
  return key2f(prefix);
}

// (value, index) arg-max with the first-max tie rule of mx.argmax
template <typename T>
__device__ __forceinline__ void argmax_merge(T& v, int& i, T ov, int oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}
// The block's winner, to every thread.  sv / si: NWAVES words of LDS each (one barrier; free again after
// the caller's next)
template <typename T, int NWAVES>
__device__ __forceinline__ int block_argmax(int tid, T v, int i, T* sv, int* si) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    argmax_merge(v, i, ov, oi);
  }
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0) {
    sv[wave] = v;
    si[wave] = i;
  }
  __syncthreads();
  T bv = sv[0];
  int bi = si[0];
  for (int w = 1; w < NWAVES; ++w) argmax_merge(bv, bi, sv[w], si[w]);
  return bi;
}
// NaN logits leave no winner; clamped so a bad row can never index outside the embedding table
__device__ __forceinline__ int clamp_code(int code, int V) { return min(max(code, 0), V - 1); }

// This thread's Gumbel-max candidate over its slots: (double)(l * inv_t) + noise(i, v) of the entries v < V
// with l >= thr, the first max (v increases with i).  noise(i, v): gumbel_noise(key, v), drawn here or --
// the persistent kernels -- ahead of their hand-off wait.  -> block_argmax<double>.
template <int NT, int NPT, typename Logit, typename Noise>
__device__ __forceinline__ void gumbel_pass(int tid, int V, float thr, float inv_t, Logit&& logit, Noise&& noise,
                                            double& best, int& bi) {
  best = -INFINITY;
  bi = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < NPT; ++i) {
    const int v = tid + NT * i;
    if (v >= V) continue;
    const float l = logit(i);
    if (!(l >= thr)) continue;
    const double val = (double)(l * inv_t) + noise(i, v);
    if (val > best) {
      best = val;
      bi = v;
    }
  }
}

// A greedy row (temperature 0): this thread's candidate for the first max of the raw logits -- the Gumbel
// pass with no threshold, the scale 1 (l * 1.0f is l) and no noise drawn, so 1 / temperature is never taken.
// -> block_argmax<double>, which picks what sample_kernel's greedy branch picks.
template <int NT, int NPT, typename Logit>
__device__ __forceinline__ void greedy_pass(int tid, int V, Logit&& logit, double& best, int& bi) {
  gumbel_pass<NT, NPT>(tid, V, -INFINITY, 1.0f, logit, [](int, int) { return 0.0; }, best, bi);
}

// Row b's record (csm_kernels.h SlotSampling): its slot's in per-slot operation (slots non-null), else the
// batch's.  b is the workgroup's row, so the result is block-uniform: read once, ahead of the loops.
__device__ __forceinline__ SlotSampling row_sampling(const SlotSampling* slots, int b, const SlotSampling& batch) {
  return slots ? slots[b] : batch;
}
// The same for a launch block that carries the batch's temperature / top_k as scalars (SampleParams,
// DecStepXsArgs: csm_kernels.h says why)
__device__ __forceinline__ float row_temperature(const SlotSampling* slots, int b, float temperature) {
  return slots ? slots[b].temperature : temperature;
}
__device__ __forceinline__ int row_top_k(const SlotSampling* slots, int b, int top_k) { return slots ? slots[b].top_k : top_k; }

}  // namespace sampler
