// CSM engine, shared context prefixes: the backbone K / V rows of a prompt's first positions kept outside the
// batch and put back into any slot (csm_prefix_save / csm_prefix_load / csm_prefix_free / csm_prefix_info).
//
// Attention is causal, so the K / V of a prompt's first P rows depend on those rows alone: a conversation's
// context is prefilled once, saved, and every later utterance that begins with it loads the rows instead of
// running them through the backbone again, then prefills only its own suffix (csm_prefill* append after what
// a slot holds).  A prefix is one compact device buffer [layer][k|v][Hkv][rows][hd] fp32; a slot's share of a
// cache [B][Hkv][S][hd] is Hkv runs of rows * hd floats, so both directions are 2 * layers * Hkv contiguous
// run-to-run copies per join, done by one kernel.
#include "csm_engine.h"

namespace {

struct PrefixCopyParams {
  float* const* kv_tab;     // [2 * layers]: layer l's K cache at 2 l, V cache at 2 l + 1
  const PrefixJoin* joins;  // [gridDim.x / (2 * layers * Hkv)]
  int* pos;                 // [B] (LOAD: the slot's position becomes rows - 1)
  int layers, Hkv, S_cap, hd;
};

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Block (x, y): run x = ((join * layers + l) * 2 + k|v) * Hkv + h, and of that run the 256-element chunks
// y, y + gridDim.y, ...  LOAD: store -> cache, else cache -> store.  Elements are 16 bytes when head_dim is a
// multiple of 4 (every run then starts on a 16-byte boundary on both sides), else dwords.  The store is read
// once per load: non-temporal loads, as the streamed weights are read.  The cache side of a load is read by
// the suffix prefill's attention next, and a save's source may still sit in L2: plain stores and loads.
// No atomics, no waiting on another block: every block copies its chunks and ends.
template <bool LOAD>
__global__ __launch_bounds__(256) void prefix_copy_kernel(PrefixCopyParams p) {
  const int per = 2 * p.layers * p.Hkv;
  const int j = blockIdx.x / per, rem = blockIdx.x % per, lk = rem / p.Hkv, h = rem % p.Hkv;
  const PrefixJoin jn = p.joins[j];
  float* cache = p.kv_tab[lk] + ((size_t)jn.b * p.Hkv + h) * p.S_cap * p.hd;
  float* store = jn.store + ((size_t)lk * p.Hkv + h) * jn.rows * p.hd;
  const size_t n = (size_t)jn.rows * p.hd, step = (size_t)gridDim.y * 256;
  if (LOAD && rem == 0 && blockIdx.y == 0 && threadIdx.x == 0) p.pos[jn.b] = jn.rows - 1;
  if (p.hd % 4 == 0) {
    const f32x4* src = reinterpret_cast<const f32x4*>(LOAD ? store : cache);
    f32x4* dst = reinterpret_cast<f32x4*>(LOAD ? cache : store);
    for (size_t i = (size_t)blockIdx.y * 256 + threadIdx.x; i < n / 4; i += step)
      dst[i] = LOAD ? __builtin_nontemporal_load(src + i) : src[i];
  } else {
    const float* src = LOAD ? store : cache;
    float* dst = LOAD ? cache : store;
    for (size_t i = (size_t)blockIdx.y * 256 + threadIdx.x; i < n; i += step) dst[i] = src[i];
  }
}

size_t prefix_bytes(const csm_engine* e, int rows) {
  const csm_llama_dims& d = e->bb.d;
  return (size_t)2 * d.n_layers * d.n_kv_heads * rows * d.head_dim * 4;
}

// The copy launch for the n joins staged in prefix_desc, the longest of max_rows rows
void enqueue_prefix_copy(csm_engine* e, int n, int max_rows, bool load) {
  const csm_llama_dims& d = e->bb.d;
  PrefixCopyParams p{};
  p.kv_tab = e->kv_tab; p.joins = e->prefix_desc; p.pos = e->pos;
  p.layers = d.n_layers; p.Hkv = d.n_kv_heads; p.S_cap = e->bb.S_cap; p.hd = d.head_dim;
  // runs on x; on y as many chunk walkers per run as bring the grid to ~8 blocks per CU of a 256-CU device,
  // never more than the longest run has 256-element chunks: a 1-row prefix is one block per run, a
  // 2046-row csm_1b prefix 256 runs x 8 walkers of 16 chunks each
  const size_t elems = (size_t)max_rows * d.head_dim / (d.head_dim % 4 == 0 ? 4 : 1);
  const int runs = n * 2 * d.n_layers * d.n_kv_heads;
  const int chunks = (int)((elems + 255) / 256);
  const int gy = std::max(1, std::min({chunks, (2048 + runs - 1) / runs, 65535}));
  if (load) hipLaunchKernelGGL(prefix_copy_kernel<true>, dim3(runs, gy), dim3(256), 0, e->st, p);
  else hipLaunchKernelGGL(prefix_copy_kernel<false>, dim3(runs, gy), dim3(256), 0, e->st, p);
  HIPCHK(hipGetLastError());
}

// One launch for `joins` (all LOAD or all save) on the engine stream, nothing waited for.  The joins travel
// through pinned staging; before the host rewrites it, the upload of the previous launch has been read.
void launch_prefix_copy(csm_engine* e, const std::vector<PrefixJoin>& joins, bool load) {
  const int n = (int)joins.size();
  if (n > e->prefix_cap) {
    HIPCHK(hipStreamSynchronize(e->st));  // a launch in flight still reads the old table
    if (e->prefix_pin) (void)hipHostFree(e->prefix_pin);
    if (e->prefix_desc) e->release(e->prefix_desc);
    e->prefix_pin = nullptr;
    e->prefix_desc = nullptr;
    e->prefix_cap = 0;
    const int cap = std::max(n, e->B_max);
    HIPCHK(hipHostMalloc((void**)&e->prefix_pin, cap * sizeof(PrefixJoin), hipHostMallocDefault));
    e->prefix_desc = (PrefixJoin*)e->alloc(cap * sizeof(PrefixJoin));
    e->prefix_cap = cap;
  }
  if (!e->prefix_ev) HIPCHK(hipEventCreateWithFlags(&e->prefix_ev, hipEventDisableTiming));
  else HIPCHK(hipEventSynchronize(e->prefix_ev));
  int max_rows = 0;
  for (int i = 0; i < n; ++i) {
    e->prefix_pin[i] = joins[i];
    max_rows = std::max(max_rows, joins[i].rows);
  }
  HIPCHK(hipMemcpyAsync(e->prefix_desc, e->prefix_pin, n * sizeof(PrefixJoin), hipMemcpyHostToDevice, e->st));
  HIPCHK(hipEventRecord(e->prefix_ev, e->st));
  enqueue_prefix_copy(e, n, max_rows, load);
}

void require_batch(csm_engine* e) {
  if (!e) throw CsmError(CSM_ERR_ARG, "null engine");
  if (e->B <= 0) throw CsmError(CSM_ERR_STATE, "csm_begin not called");
}

}  // namespace

extern "C" {

int csm_prefix_save(csm_engine* e, int b, int rows, int* id) {
  CSM_TRY {
    require_batch(e);
    if (!id) throw CsmError(CSM_ERR_ARG, "null handle pointer");
    if (b < 0 || b >= e->B) throw CsmError(CSM_ERR_ARG, "utterance index out of range");
    if (e->parked_host[b] || e->pos_host[b] < 0)
      throw CsmError(CSM_ERR_STATE, "utterance " + std::to_string(b) + " holds no rows to save");
    if (rows < 1 || rows > e->pos_host[b] + 1)
      throw CsmError(CSM_ERR_ARG, "csm_prefix_save: " + std::to_string(rows) + " rows, the utterance's cache holds " +
                                      std::to_string(e->pos_host[b] + 1));
    HIPCHK(hipSetDevice(e->dev));
    csm_engine::Prefix px;
    px.rows = rows;
    px.epoch = e->batch_epoch;
    if (hipMalloc((void**)&px.buf, prefix_bytes(e, rows)) != hipSuccess)
      throw CsmError(CSM_ERR_HIP, "hipMalloc(" + std::to_string(prefix_bytes(e, rows)) + ") failed");
    try {
      launch_prefix_copy(e, {PrefixJoin{px.buf, b, rows}}, false);
      HIPCHK(hipStreamSynchronize(e->st));
    } catch (...) {
      (void)hipFree(px.buf);
      throw;
    }
    *id = e->prefix_next++;
    e->prefixes[*id] = px;
  }
  CSM_CATCH
}

int csm_prefix_load(csm_engine* e, int n, const int32_t* utts, const int32_t* ids) {
  CSM_TRY {
    require_batch(e);
    if (n <= 0 || n > e->B || !utts || !ids) throw CsmError(CSM_ERR_ARG, "bad csm_prefix_load arguments");
    if (e->c0_pending) throw CsmError(CSM_ERR_STATE, "csm_frame_finish pending");
    std::vector<PrefixJoin> joins(n);
    std::vector<char> seen(e->B, 0);
    for (int i = 0; i < n; ++i) {
      const int b = utts[i];
      if (b < 0 || b >= e->B || seen[b]) throw CsmError(CSM_ERR_ARG, "utterance index out of range or repeated");
      seen[b] = 1;
      const auto it = e->prefixes.find(ids[i]);
      if (it == e->prefixes.end()) throw CsmError(CSM_ERR_ARG, "unknown prefix handle " + std::to_string(ids[i]));
      const csm_engine::Prefix& px = it->second;
      if (px.epoch != e->weights_epoch || e->batch_epoch != e->weights_epoch)
        throw CsmError(CSM_ERR_STATE, "prefix " + std::to_string(ids[i]) + " is stale: the weights or the RoPE table changed "
                                          "since it was computed (or since csm_begin)");
      if (e->pos_host[b] != -1)
        throw CsmError(CSM_ERR_STATE, "utterance " + std::to_string(b) + " already holds rows: a prefix loads into an empty one "
                                          "(after csm_begin or csm_slot_restart)");
      if (px.rows >= e->dims.max_seq_len) throw CsmError(CSM_ERR_TOO_LONG, "rows exceed the 2048-position window");
      joins[i] = PrefixJoin{px.buf, b, px.rows};
    }
    HIPCHK(hipSetDevice(e->dev));
    launch_prefix_copy(e, joins, true);
    // prompt_len stays -1: the slot has no h_last until a suffix of at least one row is prefilled
    for (const PrefixJoin& jn : joins) e->pos_host[jn.b] = jn.rows - 1;
  }
  CSM_CATCH
}

int csm_prefix_free(csm_engine* e, int id) {
  CSM_TRY {
    if (!e) throw CsmError(CSM_ERR_ARG, "null engine");
    const auto it = e->prefixes.find(id);
    if (it == e->prefixes.end()) throw CsmError(CSM_ERR_ARG, "unknown prefix handle " + std::to_string(id));
    HIPCHK(hipSetDevice(e->dev));
    HIPCHK(hipStreamSynchronize(e->st));  // a load still in flight reads the buffer
    (void)hipFree(it->second.buf);
    e->prefixes.erase(it);
  }
  CSM_CATCH
}

int csm_prefix_info(csm_engine* e, int id, int* rows, int64_t* bytes) {
  CSM_TRY {
    if (!e) throw CsmError(CSM_ERR_ARG, "null engine");
    const auto it = e->prefixes.find(id);
    if (it == e->prefixes.end()) throw CsmError(CSM_ERR_ARG, "unknown prefix handle " + std::to_string(id));
    if (rows) *rows = it->second.rows;
    if (bytes) *bytes = (int64_t)prefix_bytes(e, it->second.rows);
  }
  CSM_CATCH
}

// (include/csm_hip_prof.h) csm_prefix_load of one prefix into the empty utterance b, then the same copy launch
// replayed `iters` times (idempotent), timed with HIP events on the engine stream
int csm_bench_prefix_load(csm_engine* e, int b, int id, int iters, float* avg_us, double* bytes) {
  if (iters <= 0) { csm_set_error("bad bench arguments"); return CSM_ERR_ARG; }
  const int32_t b32 = b, id32 = id;
  const int rc = csm_prefix_load(e, 1, &b32, &id32);
  if (rc != CSM_OK) return rc;
  CSM_TRY {
    const int rows = e->prefixes.at(id).rows;
    hipEvent_t t0, t1;
    HIPCHK(hipEventCreate(&t0));
    HIPCHK(hipEventCreate(&t1));
    enqueue_prefix_copy(e, 1, rows, true);
    HIPCHK(hipEventRecord(t0, e->st));
    for (int i = 0; i < iters; ++i) enqueue_prefix_copy(e, 1, rows, true);
    HIPCHK(hipEventRecord(t1, e->st));
    HIPCHK(hipEventSynchronize(t1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, t0, t1));
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    if (avg_us) *avg_us = ms * 1000.f / iters;
    if (bytes) *bytes = 2.0 * (double)prefix_bytes(e, rows);  // every byte read once and written once
  }
  CSM_CATCH
}

}  // extern "C"
