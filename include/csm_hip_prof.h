/*
 * csm_hip_prof.h -- tuning and profiling hooks of libcsm_hip.so.
 *
 * NOT part of the reference-facing ABI (include/csm_hip.h): no reference interface corresponds to
 * these.  bench.py uses csm_bench_dec_frame / csm_bench_gemv for the live roofline of the dominant kernel; the parity
 * tests use csm_set_option to A/B the opt-in fused paths against the default launches.
 */
#ifndef CSM_HIP_PROF_H
#define CSM_HIP_PROF_H

#include "csm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Replay one projection of the frame `iters` times on the engine stream (one launch per layer in
 * turn, as the frame does), timed with HIP events on that stream.  which = stack*4 + kind, stack 0
 * backbone / 1 decoder, kind 0 = norm+gate/up+SiLU, 1 = down+residual, 2 = norm+QKV+RoPE,
 * 3 = o_proj+residual; M rows (M >= 8 on bf16 / int4 weights: the MFMA GEMM the batched frame runs).
 * *bytes = algorithmic bytes per launch (weights in their storage format + activations read and
 * written). */
int csm_bench_gemv(csm_engine* e, int which, int M, int iters, float* avg_us, double* bytes);

/* Replay the persistent frame decoder (dec_frame.hip: codebook0_head + 31 decoder steps of a batch-1
 * greedy frame, one launch) `iters` times on the engine stream from the current h_last, timed with HIP
 * events on that stream.  Needs an engine on which that kernel is active and a prefilled utterance.
 * *bytes = algorithmic bytes per launch: every head and decoder weight the frame reads once in bf16,
 * the folded-table rows, h_last, and the decoder K/V rows read and appended. */
int csm_bench_dec_frame(csm_engine* e, int iters, float* avg_us, double* bytes);
/* The persistent backbone step (bb_step.hip) replayed `iters` times for the last decoded row (same x,
 * same position; idempotent): average launch time (HIP events, engine stream) and the algorithmic
 * bytes one launch moves (every backbone weight in bf16 + the K/V rows).  CSM_ERR_STATE when the
 * engine does not run it (not batch-1 bf16 csm_1b shapes, or no frame run yet). */
int csm_bench_bb_step(csm_engine* e, int iters, float* avg_us, double* bytes);
/* The persistent batched decoder step (dec_step_xs.hip; batch 1..32 bf16 / 1..64 int4 on the streaming
 * path) replayed `iters` times for the last codebook step of the last frame (same partials, same
 * position; idempotent): average launch time and the algorithmic bytes one launch reads (decoder weights
 * in their storage format + the bf16 audio_head slice + folded table rows + K/V history).  CSM_ERR_STATE
 * when the step kernel is not active on this engine. */
int csm_bench_dec_xsd(csm_engine* e, int iters, float* avg_us, double* bytes);

/* csm_prefix_load of prefix `id` into the empty utterance b (its checks and its effect), then the same copy
 * launch replayed `iters` times (same bytes to the same place), timed with HIP events on the engine stream.
 * *bytes = the prefix's bytes read once + written once. */
int csm_bench_prefix_load(csm_engine* e, int b, int id, int iters, float* avg_us, double* bytes);

/* Inspection door of the backbone KV caches: positions first .. first+rows-1 of utterance b in layer `layer`,
 * as k / v [Hkv][rows][hd] float32 (either may be NULL).  Waits for the engine stream.  CSM_ERR_ARG for an
 * utterance, layer or position range outside the engine's.  The tests of the prefix calls read the caches
 * through it; the product does not call it. */
int csm_kv_read(csm_engine* e, int b, int layer, int first, int rows, float* k, float* v);

/* Tuning / debug switches (re-capture the frame graphs), per engine: "fold_proj" (decoder steps >= 2
 * gather projection(E_a[c]) from a table built at csm_begin, default 1), "qkv0_tab" (decoder layer 0's
 * q, k, v gathered from a table at steps >= 2, default 1), "qkv0_tab_batched" (0: batched frames run
 * layer 0's QKV projection instead, default 1), "dec_frame" (batch-1 greedy bf16 frames on the
 * persistent frame decoder, dec_frame.hip: codebook0_head + 31 decoder steps in one launch, default 1),
 * "bb_step" (batch-1 bf16 backbone rows on the persistent backbone step, bb_step.hip: 16 blocks + the
 * final norm in one launch, default 1), "dec_frame_stamps" / "bb_step_stamps" (per-hand-off clock
 * stamps of the persistent kernels, read back with csm_debug_read, default 0), "linear_mfma" (csm_linear
 * runs the batched frame's MFMA GEMM at >= 8 rows instead of the GEMV, default 0: the GEMM's kernel
 * tests), "gemm_xs" (the batched depth decoder on the streaming matrix-core GEMM, gemm_xs.hip,
 * default 1), "bb_xs" (the batched backbone on it too, default 1), "prefill_rows" (row cap of one
 * csm_prefill_batch group, 0 = the engine's capacity), "attn_prefill" (prompt attention on the fp32 matrix
 * cores, a block per 64-row prompt run and kv head, default 1; 0 = one block per row, tests), "dec_xsd"
 * (codebook steps >= 2 of the streaming path on the persistent batched decoder step, dec_step_xs.hip:
 * <= 32 bf16 / <= 64 int4 rows, default 1), "dec_xsd_head" (its head in the same launch, default 1),
 * "dec_xsd_sample" (sampled top-k steps: sample_kernel's sampler in the same launch too, default 1),
 * "dec_xsd_stamps" (its per-role clock marks, csm_debug_read "dec_xsd_stamps", default 0),
 * "inject_handoff_error" (test hook). */
int csm_set_option(csm_engine* e, const char* key, int value);

/* Launch geometry the streaming matrix-core GEMM (gemm_xs.hip) would use for an (N, K) projection at M
 * rows (head != 0: an arg-max / SiLU launch) with weights of dtype wdt (CSM_BF16 or CSM_Q4): out[4] =
 * {weight-row tiles of 32 per block, K slices, ring depth, waves per block}.  Returns 1 if the shape is
 * eligible for that dtype (every 64-deep K stage falls on exactly one wave of one slice; int4: at most
 * Q4_XG stages per slice), else 0.  Host-only (no device call). */
int csm_xs_shape(int N, int K, int M, int head, int wdt, int* out);

/* The int4 GEMV's tiling for an [N][K] matrix (q4_kernels.hip): out[3] = {threads per row group G, K
 * steps per thread, rows per 256-thread block}.  Returns 1 if the shape is supported, else 0.  Host-only. */
int csm_q4_gemv_shape(int N, int K, int* out);

/* The matrix-core GEMMs' int4 -> bf16 expansion (xs.h q4_word_bf16) of n uint32 words of MLX nibbles, on
 * the current device: out[4 n] = the bf16 pairs (low half first) of the nibbles in order.  Test hook
 * (tests/test_gemm_kernel_gpu.py checks every nibble value at every position).  Returns CSM_OK or an error. */
int csm_q4_expand(const uint32_t* words, int n, uint32_t* out);

/* ---- Mimi codec lab door (csrc/mimi_lab.hip): one codec kernel launch on host arrays, no codec handle.
 * Each entry allocates on the current device, uploads, launches on a stream of its own with its own
 * split-K scratch, downloads and frees.  Output arrays are in / out: their content is uploaded first (a
 * sentinel, or the values an accumulating store adds onto) and the whole array comes back, so a store
 * outside the addressed region shows.  A geometry that does not fit its arrays (sizes in elements) is
 * CSM_ERR_ARG and nothing is launched.  The geometry arrays hold the parameter blocks' fields
 * (csrc/mimi_kernels.h) in this order:
 *   conv1d (21): Cin, Tin, x_bstride, x_off, x_cstride, Cout, k, stride, dil, pad_l, replicate, elu_in,
 *                Tout, y_bstride, y_cstride, y_off, r_bstride, r_cstride, r_off, B, elu_out
 *   convtr (14): Cin, Tin, x_bstride, x_cstride, x_off, Cout, s, elu_in, t_in0, n_in, y_bstride,
 *                y_cstride, y_off, B
 *   linear (10): M, K, xs, N, os, epi (0 store, 1 add, 4 GELU), gelu_erf, conv_T, conv_bstride, accumulate */

/* What the launcher would run for a geometry (op 0 conv1d, 1 convtr, 2 linear), from the function the
 * launchers themselves call: out[4] = {kernel (0 decode GEMV, 1 64 x 64 tile, 2 wide BM x 128 tile), BM of
 * the wide tile (32 / 64 / 128, else 0), split-K slices, fold (columns per utterance of a batch-folded
 * launch, else 0)}.  Host-only. */
int mimi_lab_plan(int op, const int* geo, int n_geo, int* out);
/* bias [Cout], resid (layout r_*), y2 (layout of y) optional (NULL); w [Cout][Cin][k]. */
int mimi_lab_conv1d(const int* geo, int n_geo, const float* x, int64_t x_n, const float* w, int64_t w_n,
                    const float* bias, const float* resid, int64_t r_n, float* y, float* y2, int64_t y_n);
/* wt [s][Cout][Cin][2] (phase-major, tap e = 0 then 1); bias optional. */
int mimi_lab_convtr(const int* geo, int n_geo, const float* x, int64_t x_n, const float* wt, int64_t w_n,
                    const float* bias, float* y, int64_t y_n);
/* W [N][K]; scale [N] optional (epi add). */
int mimi_lab_linear(const int* geo, int n_geo, const float* x, int64_t x_n, const float* W, int64_t w_n,
                    const float* scale, float* out, int64_t out_n);
/* LayerNorm of rows x [M][D] with w [D], b [D] (layernorm_rows_kernel); out [>= M * D] in / out. */
int mimi_lab_layernorm(int M, int D, const float* x, const float* w, const float* b, float eps, float* out,
                       int64_t out_n);
/* RVQ encode of rows r [M][cd] (in / out: the final residual) over codebooks [k0, k1) of cb [n_q][bins][cd]
 * with c2half [n_q][bins]; codes [M / T][n_q][T] in / out.  gemm = 0: the block-per-row kernel, 1: the
 * distance GEMM (cd % 32 == 0, cd <= 256, bins % 256 == 0). */
int mimi_lab_rvq_encode(int gemm, int M, int T, int cd, int bins, int n_q, int k0, int k1, const float* cb,
                        const float* c2half, float* r, int32_t* codes);
/* Inspection tap of a codec: "rows" = the engine's row buffer [rows][dimension] as the last call left it:
 * after mimi_encode* the pre-RVQ latent [B * Tf][D], after mimi_decode / mimi_decode_step the decoder
 * transformer's output [B * n_lat][D].  *needed = its bytes; host NULL: size query only.
 * "launches" = one int64: the kernel launches the codec code has made in this process so far (a host
 * counter; tools/slots_bench.py --stream divides its growth by the chunks decoded). */
int mimi_debug_read(mimi_codec* m, const char* what, void* host, int64_t nbytes, int64_t* needed);
/* Inspection door of a codec's transformer KV caches (as csm_kv_read): positions first .. first+rows-1 of cache
 * row b in layer `layer`, as k / v [num_heads][rows][head_dim] float32 (either may be NULL).  side 0: the
 * decoder's cache (rows 0 .. max_batch-1: mimi_decode, mimi_decode_step and the slot streams share it); side 1:
 * the streaming encoder's (rows 0 .. max_batch-1 the slots, row max_batch its spare row; it exists from the first
 * mimi_encode_slot_reset on).  Positions run to max_frames * downsample_stride + 15.  Waits for the codec's stream.  CSM_ERR_ARG
 * for a side, row, layer or position range outside the codec's.  tests/test_mimi_window_gpu.py reads the caches
 * through it; the product does not call it. */
int mimi_kv_read(mimi_codec* m, int side, int b, int layer, int first, int rows, float* k, float* v);

#ifdef __cplusplus
}
#endif
#endif /* CSM_HIP_PROF_H */
