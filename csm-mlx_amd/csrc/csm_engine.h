// Internal header of the CSM engine: the engine's state and the few functions its sources share.
//   csm_engine.hip          frame paths: the block stacks, path selection, body / head enqueue, graph capture
//   csm_engine_weights.hip  lifecycle and weights: create / destroy, loader, quantizer, derived tables
//   csm_engine_abi.hip      frame ABI: csm_begin, prefill, csm_run_frames*, csm_frame_*, csm_read_codes
//   csm_engine_slots.hip    continuous batching: csm_slot_restart / csm_slot_release / csm_slot_read / csm_slot_set_sampling
//   csm_engine_prefix.hip   shared context prefixes: csm_prefix_save / csm_prefix_load / csm_prefix_free / csm_prefix_info
//   csm_engine_lab.hip      lab and inspection: csm_bench_*, debug taps, csm_linear, csm_kv_read, csm_set_option
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/csm_hip.h"
#include "../../include/csm_hip_prof.h"
#include "csm_kernels.h"
#include "engine_util.h"
#include "xs.h"

#pragma GCC visibility push(hidden)

struct LayerW {
  void* wqkv = nullptr;  // [(Hq+2Hkv)*hd][D]
  void* wo = nullptr;    // [D][Hq*hd]
  void* wgu = nullptr;   // [2F][D] rows interleaved gate_j, up_j
  void* wd = nullptr;    // [D][F]
  void* wdc = nullptr;   // bf16 engines: down_proj re-laid chunk-major [F/R][D][R] for the fused MLP
  void* wdq = nullptr;   // int4 engines: the persistent kernels' chunk-major down copy (q4_down_cm), derived:
                         // rebuilt by build_tiled after any weight change, not a weight buffer
  float* n1 = nullptr;
  float* n2 = nullptr;
  float* kc = nullptr;   // [B][Hkv][S][hd]
  float* vc = nullptr;
};

struct Stack {
  csm_llama_dims d;
  std::vector<LayerW> L;
  float* norm = nullptr;
  float* rope = nullptr;  // [S][hd/2][2]
  int S_cap = 0;
  int qkv_rows() const { return (d.n_heads + 2 * d.n_kv_heads) * d.head_dim; }
  int q_dim() const { return d.n_heads * d.head_dim; }
};

// csm_1b's depth-decoder block shapes, which the persistent decoder kernels are written for
inline bool csm1b_decoder(const csm_llama_dims& d) {
  return d.hidden == 1024 && d.intermediate == 8192 && d.n_heads == 8 && d.n_kv_heads == 2 && d.head_dim == 128;
}

// The host's side of one persistent kernel (dec_frame.hip, bb_step.hip, dec_step_xs.hip): its hand-off
// memory, tag epoch, timeout flag and optional clock stamps, the on / off switch and the cached probe of
// whether the device can hold one workgroup on every CU at once (every workgroup must be resident: the
// hand-offs spin).
struct Handoff {
  const char* name;                      // as the timeout error names it
  size_t stamps_bytes;                   // size of the stamps buffer the "<key>_stamps" option allocates
  bool on;                               // csm_set_option "<key>" / CSM_<KEY>=0 turn the kernel off
  void* buf = nullptr;                   // hand-off granules (dec_step_xs: control words)
  unsigned* epoch = nullptr;
  int* err = nullptr;
  unsigned long long* stamps = nullptr;  // per-hand-off clock stamps (profiling)
  int hw = -1, hw_q4 = -1;               // the probe's answer per weight dtype (-1: not asked yet)
  Handoff(const char* n, const char* env, size_t sb) : name(n), stamps_bytes(sb), on(env_on(env)) {}
  // one `threads`-wide workgroup of `kernel(q4)` fits on each of the device's CUs, and there are `wgs` of them
  bool resident(int dev, bool q4, const void* (*kernel)(bool), int wgs, int threads) {
    int& h = q4 ? hw_q4 : hw;
    if (h < 0) {
      hipDeviceProp_t prop;
      int per_cu = 0;
      h = hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount == wgs &&
                  hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel(q4), threads, 0) == hipSuccess && per_cu >= 1
              ? 1 : 0;
    }
    return h == 1;
  }
};
// csm_set_option / csm_debug_read keys of csm_engine::handoffs(), in its order
constexpr const char* HANDOFF_KEYS[3] = {"dec_frame", "bb_step", "dec_xsd"};

// One join of the prefix copy kernel (csm_engine_prefix.hip): `rows` positions of slot b's backbone caches
// against the compact store [layer][k|v][Hkv][rows][hd] at `store`
struct PrefixJoin {
  float* store;
  int b, rows;
};

#pragma GCC visibility pop

struct csm_engine {
  csm_dims dims;
  int dev = 0;
  int wdt = WDT_BF16;       // Linear / Embedding weights: WDT_F32, WDT_BF16 or WDT_Q4 (nn.quantize'd)
  int head_wdt = WDT_BF16;  // audio_head: never quantized (a raw array, models.py:65-67)
  size_t wsz = 2;           // bytes per element of the dense (non-q4) weight dtype
  // bytes of one [N][K] Linear/Embedding weight in the engine's storage dtype
  size_t wbytes(size_t N, size_t K) const { return wdt == WDT_Q4 ? q4_bytes(N, K) : N * K * wsz; }
  // pre-quantized MLX tensors wait here until .weight, .scales and .biases have all arrived
  struct PendingQ4 {
    std::vector<uint8_t> packed, scales, biases;
    int sdt = 0;
    int64_t n = 0, k = 0;
  };
  std::map<std::string, PendingQ4> pending_q4;
  int B_max = 0, F_cap = 0, M_cap = 0;
  hipStream_t st = nullptr;
  Stack bb, dec;
  int V = 0, Vpad = 0, K = 0, D = 0, Dd = 0;
  void* text_emb = nullptr;
  void* audio_emb = nullptr;
  void* proj = nullptr;      // [Dd][D]
  void* c0_head = nullptr;   // [Vpad][D]
  void* audio_head = nullptr;  // [K-1][Vpad][Dd]
  // projection folded into the decoder-input table: proj_tab[cb][code] = projection(E_a[code + V*cb])
  // (fp32, the exact output of the projection GEMV), cb < K-1.  Decoder steps >= 2 gather their
  // input row from it instead of running the projection GEMV.
  float* proj_tab = nullptr;
  bool proj_tab_dirty = true;
  bool c0_pending = false;  // csm_frame_c0_logits ran; csm_frame_finish (or csm_frame_host_step) must follow
  int host_piece = 1;       // csm_frame_host_step: the codebook whose code the next call feeds is host_piece - 1
  // decoder layer 0's QKV folded too: qkv0_tab[cb][code] = RoPE'd (q, k | v) of layer 0 for input row
  // proj_tab[cb][code] at position cb + 1 (fp32, built by the same QKV GEMV); codebook steps >= 2 then
  // skip layer 0's QKV launch and its attention gathers the row (AttnParams::g_tab).
  float* qkv0_tab = nullptr;
  bool use_qkv0_tab = env_on("CSM_QKV0_TAB");  // csm_set_option "qkv0_tab"
  bool qkv0_built = false;
  // fragment-tiled copies of the matrices the MFMA path reads (build_tiled; ws.tiled maps them)
  std::vector<void*> tiled_bufs;
  bool tiled_dirty = true;
  std::set<std::string> loaded;
  std::vector<std::string> required;
  // activations
  float *x = nullptr, *q = nullptr, *att = nullptr, *mlp = nullptr;
  float *h_last = nullptr, *c0_logits = nullptr, *ci_logits = nullptr;
  int* force = nullptr;  // [B_max][K] teacher-forced codes (csm_frame_forced)
  float* force_ce = nullptr;  // [B_max][K] their cross entropies
  float *dx = nullptr, *din = nullptr, *dq = nullptr, *datt = nullptr, *dmlp = nullptr;
  int32_t* tok = nullptr;
  uint8_t* msk = nullptr;
  int *row_b = nullptr, *row_pos = nullptr;  // [M_cap] batched-prefill row tables
  int2* ptiles = nullptr;  // [M_cap / 64 + B_max + 2] prompt-prefill attention tiles (RowMap::tiles)
  // csm_run_frames_ahead: each chunk's done flags and the persistent kernels' error flags are copied to
  // pinned host memory behind its frames, with an event; a call waits for the previous chunk's only
  uint8_t* ahead_pin = nullptr;  // [2][ahead_bytes()]
  int2* ptiles_pin = nullptr;     // pinned staging of a single prompt's attention tiles (csm_prefill)
  hipEvent_t ahead_ev[2] = {nullptr, nullptr};
  int ahead_slot = 0;
  bool ahead_pending = false;
  size_t ahead_bytes() const { return (size_t)(B_max + 7) / 8 * 8 + 8; }
  bool attn_tiles_on = true;  // csm_set_option "attn_prefill": 0 = attn_block per row (A/B, tests)
  // per-batch state
  int *codes = nullptr, *hist = nullptr, *pos = nullptr, *n_frames = nullptr, *frame_ctr = nullptr;
  unsigned long long* part = nullptr;  // [K][B_max][part_stride] arg-max partials of the heads
  int part_stride = 0;
  uint8_t* done = nullptr;
  uint64_t* seeds = nullptr;
  int B = 0;
  // What the batch samples with (csm_kernels.h SlotSampling): the sampler of csm_begin, which also resets the
  // rest, mlx_lm's filter chain beyond top-k (csm_set_sampler_filters) and make_logits_processors on the c0
  // logits, run inside the frame (csm_set_c0_processors): the repetition penalty over the last batch.context
  // c0 codes of each utterance's history and, with batch.bias 1, the dense bias vector c0_bias [Vpad] (zero
  // where unset).  csm_engine_slots.hip checks and rounds the callers' values (sampling_*).
  SlotSampling batch{};
  float* c0_bias = nullptr;
  // the frame graphs capture the record by value: every call that writes it counts filters_id up
  int filters_id = 0, g_filters = -1;
  int frames_run = 0;
  bool need_body = false;
  std::vector<int> prompt_len;
  // Continuous batching (csm_engine_slots.hip): the B rows are slots whose utterances start (csm_slot_restart)
  // and leave (csm_slot_release) at frame boundaries while the others go on.  slot_frame[b] is the utterance's
  // own frame index -- what the samplers' counters, the EOS test, n_frames and the c0 repetition window count
  // in; after a plain csm_begin it equals frame_ctr[0] for every row.  parked[b] marks a slot with no
  // utterance: its position stays 0 and its done flag set.  The code history is then a ring over the global
  // frame index and slot_first[b] is the global frame at which slot b's utterance started.
  int* slot_frame = nullptr;  // [B_max]
  uint8_t* parked = nullptr;  // [B_max]
  bool slot_mode = false;     // from the first slot call after csm_begin until the next csm_begin
  std::vector<char> parked_host;
  std::vector<int> slot_first;
  // Per-utterance sampling (csm_slot_set_sampling): slot_sampling[b] is what slot b's utterance samples with
  // and slot_bias[b] its dense logit bias.  The kernels read them (per_slot: their table pointers are set)
  // from the first override after csm_begin on; until then `batch` serves every row and the frame runs
  // exactly as without this.  A slot with no override holds a copy of `batch`; samp_own[b] marks one that has
  // its own, samp_host mirrors the device rows for the plan (frame_plan).
  SlotSampling* slot_sampling = nullptr;  // [B_max]
  float* slot_bias = nullptr;             // [B_max][Vpad]
  bool per_slot = false;
  std::vector<SlotSampling> samp_host;
  std::vector<char> samp_own;
  // Shared context prefixes (csm_engine_prefix.hip): saved backbone K / V rows of a prompt's first positions,
  // each in a hipMalloc of its own (not in batch_allocs: a growing batch keeps them), by handle.  A prefix is
  // valid for the weights and RoPE table it was computed with: weights_epoch counts every change of either
  // (csm_load_tensor, csm_quantize, csm_set_rope_table, csm_weights_received), batch_epoch is its value at the
  // last csm_begin -- what the rows in the caches were computed with -- and a prefix records the latter.
  struct Prefix {
    float* buf = nullptr;
    int rows = 0;
    unsigned long long epoch = 0;
  };
  std::map<int, Prefix> prefixes;
  int prefix_next = 1;
  unsigned long long weights_epoch = 0, batch_epoch = 0;
  float** kv_tab = nullptr;  // device [2 * backbone layers]: layer l's kc at 2 l, vc at 2 l + 1 (ensure_batch)
  PrefixJoin* prefix_desc = nullptr;  // device [prefix_cap] joins of one copy launch
  PrefixJoin* prefix_pin = nullptr;   // their pinned staging; prefix_ev: its last upload has been read
  int prefix_cap = 0;
  hipEvent_t prefix_ev = nullptr;
  // graphs
  hipGraphExec_t g_body = nullptr, g_head = nullptr;
  int g_B = -1;
  int g_plan = -1;  // FramePlan::key() the graphs were captured for
  std::vector<void*> allocs;
  std::vector<void*> batch_allocs;
  std::vector<int> pos_host;
  bool fold_proj = true;  // csm_set_option "fold_proj": decoder steps >= 2 read the folded table
  bool linear_mfma = false;  // csm_set_option "linear_mfma": csm_linear on the MFMA GEMM (kernel tests)
  // csm_set_option "prefill_rows": row cap of one csm_prefill_batch group (0 = M_cap); lowering it makes
  // small test batches take the multi-group path that config 5's 64 x 248-row contexts take
  int prefill_rows = 0;
  // csm_set_option "qkv0_tab_batched" 0: batched (matrix-core) frames run layer 0's QKV projection
  // instead of gathering it from the folded table (A/B and parity checks)
  bool no_tab_batched = false;
  // batched depth decoder (8..64 utterances, bf16 or int4, codebook steps >= 2) on the streaming
  // matrix-core GEMM over pre-split activations (gemm_xs.hip): split rows x * norm [64][Dd], attention
  // output, SiLU*up rows [64][F] (xs.h layout), per-row partial sums of squares [64 tiles][64 rows],
  // half-group sums for int4.  Config 4 3917 vs 3729 frames/s on gemm_wide (r03).
  // csm_set_option "gemm_xs" / CSM_GEMM_XS=0 turn it off.
  bool xs_on = env_on("CSM_GEMM_XS");
  // the depth decoder's step 1 (2 rows per utterance) on the streaming GEMM as well (CSM_XS_STEP1=0: on
  // gemm_wide, the A/B)
  bool xs_step1 = env_on("CSM_XS_STEP1");
  void *xs_D = nullptr, *xs_A = nullptr, *xs_F = nullptr;
  float* xs_ss = nullptr;
  // the batched backbone on the streaming GEMM too (option bb_xs / CSM_BB_XS=0 off): with 8-wave blocks it
  // beats gemm_wide on every backbone shape -- int4 at 64 rows gate/up 40.4 -> 22.7, down 28.2 -> 18.9,
  // QKV 24.8 -> 18.3, o 15.8 -> 11.4 us; bf16 at 32 rows 63 -> 58 us per layer (profiles/r04_ab_xs_waves8.txt)
  bool bb_xs_on = env_on("CSM_BB_XS");
  float *hs_D = nullptr, *hs_A = nullptr, *hs_F = nullptr;  // int4 engines: half-group sums of the split rows
  GemmWs ws;         // split-K slabs + tickets of this engine's MFMA launches (ensure_batch sizes them)
  // persistent frame decoder (dec_frame.hip) for batch-1 bf16 / int4 frames
  Handoff h_df{"persistent frame decoder", "CSM_DEC_FRAME", (size_t)DEC_FRAME_WGS * DEC_FRAME_STAMPS * 8};
  // persistent backbone step (bb_step.hip) for batch-1 csm_1b decode rows
  Handoff h_bb{"persistent backbone step", "CSM_BB_STEP", (size_t)BB_STEP_WGS * BB_STEP_STAMPS * 8};
  // persistent batched depth-decoder step (dec_step_xs.hip): codebook steps >= 2 of 1..32 bf16 (64 int4)
  // rows in one launch instead of the streaming stack's ~20
  Handoff h_xsd{"persistent batched decoder step", "CSM_DEC_XSD", (size_t)DEC_XSD_WGS * DEC_XSD_STAMPS * 8};
  std::array<Handoff*, 3> handoffs() { return {&h_df, &h_bb, &h_xsd}; }  // (HANDOFF_KEYS names them)
  DecStepXsArgs xsd{};    // dec_step_xs's scratch pointers (ensure_batch)
  bool xsd_head = env_on("CSM_DEC_XSD_HEAD");      // "dec_xsd_head": the step's head in the same launch
  bool xsd_sample = env_on("CSM_DEC_XSD_SAMPLE");  // "dec_xsd_sample": + the sampler

  // zero-filled device memory owned by the engine (alloc) or by the current batch size (balloc)
  void* alloc_in(std::vector<void*>& pool, size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) throw CsmError(CSM_ERR_HIP, "hipMalloc(" + std::to_string(bytes) + ") failed");
    (void)hipMemset(p, 0, bytes);
    (void)hipDeviceSynchronize();  // the null-stream fill is not ordered with the engine's non-blocking stream
    pool.push_back(p);
    return p;
  }
  void* balloc(size_t bytes) { return alloc_in(batch_allocs, bytes); }
  void* alloc(size_t bytes) { return alloc_in(allocs, bytes); }
  void release(void* p) {
    for (auto& a : allocs)
      if (a == p) {
        (void)hipFree(p);
        a = allocs.back();
        allocs.pop_back();
        return;
      }
  }
  ~csm_engine() {
    for (hipEvent_t ev : ahead_ev)
      if (ev) (void)hipEventDestroy(ev);
    if (ahead_pin) (void)hipHostFree(ahead_pin);
    if (ptiles_pin) (void)hipHostFree(ptiles_pin);
    if (prefix_pin) (void)hipHostFree(prefix_pin);
    if (prefix_ev) (void)hipEventDestroy(prefix_ev);
    for (auto& kv : prefixes) (void)hipFree(kv.second.buf);
    if (g_body) (void)hipGraphExecDestroy(g_body);
    if (g_head) (void)hipGraphExecDestroy(g_head);
    for (void* p : allocs) (void)hipFree(p);
    for (void* p : batch_allocs) (void)hipFree(p);
    gemm_ws_free(ws);
    if (st) (void)hipStreamDestroy(st);
  }
};

#pragma GCC visibility push(hidden)

// GEMV / GEMM parameters bound to this engine's split-K scratch
inline GemvParams gp(csm_engine* e) {
  GemvParams g{};
  g.ws = &e->ws;
  return g;
}

// arg-max partial slots per row of a head launch (GEMV or MFMA path, dense or int4)
inline int head_blocks(int N, int K, int M, int wdt) { return gemv_partials(N, K, M, wdt); }

// Where an MLX Linear/Embedding weight lives in the engine: rows row0 + r*rstep (r < n) of a
// [Ntot][K] matrix at base.  False for parameters nn.quantize leaves alone (norms, audio_head).
struct Place {
  void* base = nullptr;
  int Ntot = 0, K = 0, row0 = 0, rstep = 1, n = 0;
};
bool weight_place(csm_engine* e, const std::string& name, Place& pl);

// Device scratch of one call (load-time conversions, csm_linear, csm_read_rows)
struct DevBuf {
  void* p = nullptr;
  explicit DevBuf(size_t n) { HIPCHK(hipMalloc(&p, n)); }
  ~DevBuf() { if (p) (void)hipFree(p); }
};

// What enqueue_head_phase enqueues of a frame's head.
enum class HeadPhase {
  Frame,       // the whole head (what the frame graph captures)
  C0Logits,    // the c0 head only, logits stored for the host (logits processors, generation.py:44-49)
  FromHostC0,  // the rest of the frame from c0 logits the host wrote back: c0 is picked by the sample kernel
               // (arg-max when greedy, published as one partial), then steps 1..K-1 as in Frame
  Forced,      // teacher forcing: every head stores its logits and the code fed forward is the caller's
               // (e->force [B][K]), as compute_loss feeds the target frame (trainer.py:233-262)
  HostPiece,   // one piece of a host-sampled frame (a sampler callable on the host, csm_frame_host_step):
               // piece p feeds the host's code for codebook p - 1 forward (e->force) and runs decoder step
               // p + its head (logits stored); piece K feeds the last code and advances the frame.  The c0
               // head ran as C0Logits (csm_frame_c0_logits).
};

// The plan class of a frame: which of the head's paths the whole batch takes.  Without per-slot sampling it
// restates the batch's sampler and processors; with it, it is the union of what the slots holding an
// utterance need -- any non-greedy slot: a sampled plan; any with top-p / min-p: the filtered kernel for all
// rows; any with a bias or penalty: the processors pass.  The per-slot values themselves are read from the
// table at run time, so only a change of key() captures the frame graph again.  frame_plan is the one place
// that decides sampled / filtered / processors: the head enqueue, dec_frame_eligible and launch_sample's
// caller read its result.
struct FramePlan {
  bool sampled, filtered, processors, per_slot;
  int key() const { return (sampled ? 1 : 0) | (filtered ? 2 : 0) | (processors ? 4 : 0) | (per_slot ? 8 : 0); }
};
FramePlan frame_plan(const csm_engine* e);
// csm_engine_slots.hip: the value checks of a row's sampler, filter chain and c0 processors and their rounding
// into the record -- the one copy behind csm_begin, csm_set_sampler_filters, csm_set_c0_processors and
// csm_slot_set_sampling (each keeps its own state checks); nothing is written when a check throws
void sampling_set_sampler(SlotSampling& r, float temperature, int top_k);
void sampling_set_filters(SlotSampling& r, double top_p, double min_p, int min_tokens_to_keep);
// bias_mode: what r.bias becomes with n_bias > 0 (1: the batch's vector, 2: a slot's own row)
void sampling_set_processors(const csm_engine* e, SlotSampling& r, int bias_mode, int n_bias, const int32_t* bias_idx,
                             const float* bias_val, float repetition_penalty, int repetition_context_size);
// the dense bias vector [Vpad] at dst, zero where unset (a repeated index: the last value); n_bias 0: untouched
void upload_dense_bias(csm_engine* e, float* dst, int n_bias, const int32_t* bias_idx, const float* bias_val);
// per-slot operation, after the batch's values changed -- the rows of the slots without an override follow
// (no-op otherwise)
void refresh_slot_sampling(csm_engine* e);

// csm_engine_weights.hip
void ensure_batch(csm_engine* e, int B);
void build_tiled(csm_engine* e);
void build_proj_table(csm_engine* e);
// csm_engine.hip
void run_stack(csm_engine* e, Stack& s, float* x, int M, float* q, float* att, float* mlp, const RowMap& rm,
               hipStream_t st, const GemvParams* gather0 = nullptr, const AttnParams* attn0 = nullptr);
void embed(csm_engine* e, const EmbedParams& ep, int M, hipStream_t st);
bool bb_step_eligible(csm_engine* e);
bool dec_frame_eligible(csm_engine* e);
bool xsd_eligible(csm_engine* e, int M);
void enqueue_bb_step(csm_engine* e, hipStream_t st);
void enqueue_dec_frame_only(csm_engine* e, hipStream_t st);
const void* xsd_head_tiled(csm_engine* e, int M, int i);
void launch_xsd(csm_engine* e, int M, int i, const unsigned long long* part_prev, int part_n, unsigned long long* part_out,
                hipStream_t st, const void* head_tiled, bool sample);
void enqueue_body(csm_engine* e, hipStream_t st);
void enqueue_head_phase(csm_engine* e, hipStream_t st, HeadPhase phase, int piece = 0);
void enqueue_head(csm_engine* e, hipStream_t st);
hipGraphExec_t capture(csm_engine* e, void (*fn)(csm_engine*, hipStream_t));
void check_handoffs(csm_engine* e);
// csm_engine_abi.hip
void body_if_needed(csm_engine* e, bool graph = false);

#pragma GCC visibility pop
