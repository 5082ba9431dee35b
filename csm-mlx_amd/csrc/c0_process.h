// mlx_lm make_logits_processors on the c0 logits (generation.py:44-49), per logit: the one definition of
// the arithmetic that c0_process_kernel (csm_kernels.hip, the launch path) and the persistent frame
// decoder's head_publish (dec_frame.hip) share.  Restated in numpy by csm_mlx/sampling.py LogitBias /
// RepetitionPenalty, which the host paths and the oracle call.
#pragma once
#include <hip/hip_runtime.h>

#include "csm_kernels.h"

// Logit l of vocabulary entry v after the bias add (bias [Vpad] dense, zero where unset; null: none) and
// then the repetition penalty over the window win[0..n) of this utterance's last c0 codes (n 0: none): a
// code in the window is penalised once however often it occurs, l * penalty when negative, else the
// correctly rounded l / penalty.  All float32 (numpy float32's add, multiply and divide).
// bias_v: bias[v] when the caller fetched it ahead (read only with a non-null bias).
__device__ __forceinline__ float c0_processed(float l, int v, const float* bias, float bias_v, const int* win, int n,
                                              float penalty) {
  if (bias) l += bias_v;
  bool hit = false;
  for (int j = 0; j < n; ++j) hit |= win[j] == v;
  if (hit) l = l < 0.f ? l * penalty : __fdiv_rn(l, penalty);
  return l;
}
__device__ __forceinline__ float c0_processed(float l, int v, const float* bias, const int* win, int n, float penalty) {
  return c0_processed(l, v, bias, bias ? bias[v] : 0.f, win, n, penalty);
}

// Entries of the window at frame f: the c0 codes of the utterance's last min(f, context) frames (never more
// than the C0_WINDOW_MAX entries the kernels stage in LDS)
__device__ __forceinline__ int c0_window_n(int f, int context, float penalty) {
  return penalty > 0.f ? min(min(f, context), C0_WINDOW_MAX) : 0;
}
// Entry j (0 = the newest) of utterance b's window in the code history hist [F][B][K]
__device__ __forceinline__ int c0_window_code(const int* hist, int f, int j, int b, int B, int K) {
  return hist[((size_t)(f - 1 - j) * B + b) * K];
}
// The same entry when the history is a ring of F_cap rows over the global frame index f (j < the utterance's
// own frame count <= f, so f - 1 - j >= 0; the identity of c0_window_code while f <= F_cap)
__device__ __forceinline__ int c0_window_code_ring(const int* hist, int f, int j, int b, int B, int K, int F_cap) {
  return hist[((size_t)((f - 1 - j) % F_cap) * B + b) * K];
}
