// Evaluation metrics on the device (include/vlfb.h, "Evaluation metrics"): top-k hit counters, the clip-merge score
// table, per-class average precision / ROC-AUC, EPIC action top-k, AVA frame-mAP and the AVA multi-crop merge.  Replaces
// the host meter of the reference's lib/utils/metrics.py and tools/evaluate_actions.py, which fetches `pred` and `labels`
// every iteration.
//
// Determinism: every count is an integer (exact, order-independent); the only floating-point sums (AP, AUC) are taken
// over a fixed partition of the sorted column (AP_THREADS chunks of npad / AP_THREADS elements, then a fixed tree), the
// same in the LDS and the global-workspace path.  Built with -ffp-contract=off (csrc/Makefile): the action score
// (verb * noun) * prior is two fp32 roundings, as numpy forms it.
#include "vlfb_common.h"

namespace vlfb {

constexpr int MAX_K = 4;
struct TopK { int nk; int k[MAX_K]; };

// rank contribution of element j (score s) against the label's score sl at index jl
__device__ __forceinline__ int outranks(float s, int j, float sl, int jl) { return (s > sl || (s == sl && j < jl)) ? 1 : 0; }

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---- top-k hits: ONE workgroup, a wave per row; the adds into `hits` are plain int64 adds of one thread ---------------
// KEEP (vlfb_topk_hits_keep): the wave also stores its row as fp32, with the label, at table row *cursor + r when that is
// inside the table; every thread reads the cursor before the barrier below and one thread advances it behind it.
constexpr int TOPK_WAVES = 4;
template <typename T, bool KEEP>
__global__ __launch_bounds__(TOPK_WAVES * 64) void topk_hits_kernel(const T* __restrict__ scores, const int32_t* __restrict__ labels,
                                                                    int rows, int cols, TopK ks, int64_t* __restrict__ hits,
                                                                    float* __restrict__ table, int32_t* __restrict__ tlab,
                                                                    long long total, long long* cursor) {
  __shared__ int part[TOPK_WAVES][MAX_K + 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long cur = KEEP ? *cursor : 0;
  int mine[MAX_K + 1] = {0, 0, 0, 0, 0};
  for (int r = wave; r < rows; r += TOPK_WAVES) {
    const int jl = labels[r];
    const T* row = scores + (size_t)r * cols;
    if (KEEP) {
      const long long pos = cur + r;
      if (pos >= 0 && pos < total) {                          // (wave-uniform) rows behind the end of the data set are dropped
        float* dst = table + (size_t)pos * cols;
        for (int j = lane; j < cols; j += 64) dst[j] = Elem<T>::ld(row + j);
        if (lane == 0) tlab[pos] = jl;
      }
    }
    if (jl < 0 || jl >= cols) continue;                       // (wave-uniform)
    const float sl = Elem<T>::ld(row + jl);
    int rank = 0;
    for (int j = lane; j < cols; j += 64) rank += outranks(Elem<T>::ld(row + j), j, sl, jl);
    rank = wave_sum(rank);
    const bool valid = sl == sl;                              // a NaN label score is a counted miss
#pragma unroll
    for (int i = 0; i < MAX_K; ++i) mine[i] += (i < ks.nk && valid && rank < ks.k[i]) ? 1 : 0;
    mine[MAX_K] += 1;
  }
  if (lane == 0)
    for (int i = 0; i <= MAX_K; ++i) part[wave][i] = mine[i];
  __syncthreads();
  if (threadIdx.x <= ks.nk) {
    const int i = threadIdx.x == ks.nk ? MAX_K : threadIdx.x;
    int s = 0;
    for (int w = 0; w < TOPK_WAVES; ++w) s += part[w][i];
    hits[threadIdx.x] += s;
  }
  if (KEEP && threadIdx.x == 0) *cursor = cur + rows;
}

// ---- EPIC action top-k: a workgroup per row over the V x Nn products; integer atomic adds into `hits` -----------------
constexpr int ACT_THREADS = 256;
__global__ __launch_bounds__(ACT_THREADS) void action_topk_kernel(const float* __restrict__ verb, const float* __restrict__ noun,
                                                                  const float* __restrict__ prior, const int32_t* __restrict__ vl,
                                                                  const int32_t* __restrict__ nl, int V, int Nn, TopK ks,
                                                                  unsigned long long* __restrict__ hits) {
  __shared__ int part[ACT_THREADS / 64];
  const int r = blockIdx.x;
  const int lv = vl[r], ln = nl[r];
  if (lv < 0 || lv >= V || ln < 0 || ln >= Nn) return;          // (block-uniform)
  const float* v = verb + (size_t)r * V;
  const float* n = noun + (size_t)r * Nn;
  const int jl = lv * Nn + ln;
  float sl = v[lv] * n[ln];
  if (prior) sl = sl * prior[jl];
  int rank = 0;
  for (int j = threadIdx.x; j < V * Nn; j += ACT_THREADS) {
    const int a = j / Nn, b = j - a * Nn;
    float s = v[a] * n[b];
    if (prior) s = s * prior[j];
    rank += outranks(s, j, sl, jl);
  }
  rank = wave_sum(rank);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = rank;
  __syncthreads();
  if (threadIdx.x == 0) {
    rank = 0;
    for (int w = 0; w < ACT_THREADS / 64; ++w) rank += part[w];
    const bool valid = sl == sl;
    for (int i = 0; i < ks.nk; ++i)
      if (valid && rank < ks.k[i]) atomicAdd(hits + i, 1ull);
    atomicAdd(hits + ks.nk, 1ull);
  }
}

// ---- clip merge: a thread owns a column and walks the rows of the call IN ORDER, so rows that land on one item see each
// other; the cursor is advanced by a second one-lane launch behind it (every workgroup of the first has read it by then) --
constexpr int MERGE_THREADS = 64;
template <typename T>
__global__ __launch_bounds__(MERGE_THREADS) void merge_max_kernel(const T* __restrict__ scores, const int32_t* __restrict__ labels,
                                                                  int rows, int cols, float* __restrict__ table,
                                                                  uint8_t* __restrict__ tlab, long long n_items, long long total,
                                                                  const long long* __restrict__ cursor, int* __restrict__ mismatches) {
  const int c = blockIdx.x * MERGE_THREADS + threadIdx.x;
  if (c >= cols) return;
  const long long cur = *cursor;
  int bad = 0;
  for (int r = 0; r < rows; ++r) {
    const long long pos = cur + r;
    if (total > 0 && pos >= total) break;                      // rows behind the end of the data set (padding of the last batch)
    const size_t at = (size_t)(pos % n_items) * cols + c;
    const float s = Elem<T>::ld(scores + (size_t)r * cols + c);
    const float t = table[at];
    table[at] = s > t ? s : t;
    const uint8_t l = labels[(size_t)r * cols + c] > 0 ? 1 : 0;
    const uint8_t have = tlab[at];
    if (have == 255) tlab[at] = l;
    else if (have != l) ++bad;
  }
  if (bad) atomicAdd(mismatches, bad);
}
__global__ void cursor_advance_kernel(long long* cursor, int rows) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *cursor = *cursor + rows;
}

// ---- per-class AP / AUC -------------------------------------------------------------------------------------------------
constexpr int AP_THREADS = 512;
constexpr int AP_LDS_MAX = 8192;       // elements of a column the LDS path holds: 4 B key + 1 B label each = 40 KiB

// fp32 -> uint32 whose unsigned order is the float order; -0 == +0; never 0 (0 is the padding, it sorts behind everything)
__device__ __forceinline__ uint32_t order_key(float f) {
  if (f == 0.f) f = 0.f;
  const uint32_t u = __float_as_uint(f);
  const uint32_t k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return k ? k : 1u;
}

// exclusive prefix over one int per thread (Hillis-Steele in LDS, AP_THREADS entries); OP = sum or max
template <bool MAX>
__device__ __forceinline__ int block_exclusive(int v, int identity, int* buf) {
  const int t = threadIdx.x;
  buf[t] = v;
  __syncthreads();
  for (int off = 1; off < AP_THREADS; off <<= 1) {
    const int o = t >= off ? buf[t - off] : identity;
    __syncthreads();
    buf[t] = MAX ? max(buf[t], o) : buf[t] + o;
    __syncthreads();
  }
  const int ex = t ? buf[t - 1] : identity;
  __syncthreads();
  return ex;
}

// keys / labs: npad entries of this class, in LDS or in the global workspace
__device__ __forceinline__ void class_ap_auc_body(const float* __restrict__ table, const uint8_t* __restrict__ tlab, int n, int cols,
                                                  int npad, uint32_t* keys, uint8_t* labs, int* ibuf, double* dbuf,
                                                  double* __restrict__ ap, double* __restrict__ auc, int* __restrict__ n_pos) {
  const int c = blockIdx.x, t = threadIdx.x;
  for (int i = t; i < npad; i += AP_THREADS) {
    keys[i] = i < n ? order_key(table[(size_t)i * cols + c]) : 0u;
    labs[i] = i < n ? (tlab[(size_t)i * cols + c] == 1 ? 1 : 0) : 0;
  }
  __syncthreads();
  // bitonic network, descending
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = t; p < (npad >> 1); p += AP_THREADS) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));       // the lower index of pair p
        const int l = i | j;
        const bool desc = (i & k) == 0;
        const uint32_t a = keys[i], b = keys[l];
        if (desc ? a < b : a > b) {
          keys[i] = b; keys[l] = a;
          const uint8_t la = labs[i], lb = labs[l];
          labs[i] = lb; labs[l] = la;
        }
      }
      __syncthreads();
    }
  // thread t owns the chunk [lo, hi) of the sorted column
  const int L = (npad + AP_THREADS - 1) / AP_THREADS;
  const int lo = min(t * L, n), hi = min(lo + L, n);
  int cnt = 0;
  for (int i = lo; i < hi; ++i) cnt += labs[i];
  const int before = block_exclusive<false>(cnt, 0, ibuf);         // positives in [0, lo)
  // tp and index of the last run end in the chunk (a run ends at i when i is the last element or the next score differs)
  int tp = before, end_tp = -1, end_i = -1;
  for (int i = lo; i < hi; ++i) {
    tp += labs[i];
    if (i == n - 1 || keys[i + 1] != keys[i]) { end_tp = tp; end_i = i; }
  }
  int prev_tp = block_exclusive<true>(end_tp, -1, ibuf);           // tp_{g-1} / e_{g-1} of the first run end of the chunk
  int prev_e = block_exclusive<true>(end_i, -1, ibuf);
  if (prev_tp < 0) prev_tp = 0;
  if (t == AP_THREADS - 1) ibuf[0] = tp;                           // (the last chunk's running count is P: empty chunks carry it)
  __syncthreads();
  const long long P = ibuf[0];
  __syncthreads();
  double s_ap = 0.0, s_auc = 0.0;
  tp = before;
  for (int i = lo; i < hi; ++i) {
    tp += labs[i];
    if (i == n - 1 || keys[i + 1] != keys[i]) {
      const long long dtp = tp - prev_tp;
      const long long fp = (long long)i + 1 - tp, fp_prev = (long long)prev_e + 1 - prev_tp;
      if (dtp) s_ap += (double)(dtp * tp) / (double)(P * ((long long)i + 1));
      if (fp != fp_prev) s_auc += (double)((fp - fp_prev) * ((long long)tp + prev_tp)) / (double)(2 * P * ((long long)n - P));
      prev_tp = tp; prev_e = i;
    }
  }
  dbuf[t] = s_ap;
  dbuf[AP_THREADS + t] = s_auc;
  __syncthreads();
  for (int off = AP_THREADS >> 1; off > 0; off >>= 1) {
    if (t < off) {
      dbuf[t] += dbuf[t + off];
      dbuf[AP_THREADS + t] += dbuf[AP_THREADS + t + off];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    n_pos[c] = (int)P;
    ap[c] = P == 0 ? nan : dbuf[0];
    auc[c] = (P == 0 || P == n) ? nan : dbuf[AP_THREADS];
  }
}

__global__ __launch_bounds__(AP_THREADS) void class_ap_auc_lds_kernel(const float* __restrict__ table, const uint8_t* __restrict__ tlab,
                                                                     int n, int cols, int npad, double* __restrict__ ap,
                                                                     double* __restrict__ auc, int* __restrict__ n_pos) {
  __shared__ uint32_t keys[AP_LDS_MAX];
  __shared__ uint8_t labs[AP_LDS_MAX];
  __shared__ int ibuf[AP_THREADS];
  __shared__ double dbuf[2 * AP_THREADS];
  class_ap_auc_body(table, tlab, n, cols, npad, keys, labs, ibuf, dbuf, ap, auc, n_pos);
}
__global__ __launch_bounds__(AP_THREADS) void class_ap_auc_global_kernel(const float* __restrict__ table, const uint8_t* __restrict__ tlab,
                                                                        int n, int cols, int npad, uint32_t* ws_keys, uint8_t* ws_labs,
                                                                        double* __restrict__ ap, double* __restrict__ auc,
                                                                        int* __restrict__ n_pos) {
  __shared__ int ibuf[AP_THREADS];
  __shared__ double dbuf[2 * AP_THREADS];
  class_ap_auc_body(table, tlab, n, cols, npad, ws_keys + (size_t)blockIdx.x * npad, ws_labs + (size_t)blockIdx.x * npad, ibuf,
                    dbuf, ap, auc, n_pos);
}

static int pad_pow2(long long n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

static int check_ks(const char* what, const int32_t* ks, int nk, long long cols, TopK* out) {
  VLFB_REQUIRE(ks != nullptr && nk >= 1 && nk <= MAX_K, "%s: 1 <= nk <= %d values of k expected, got nk = %d", what, MAX_K, nk);
  out->nk = nk;
  for (int i = 0; i < MAX_K; ++i) out->k[i] = 0;
  for (int i = 0; i < nk; ++i) {
    VLFB_REQUIRE(ks[i] >= 1 && ks[i] <= cols, "%s: k = %d outside 1..cols = %lld", what, ks[i], cols);
    out->k[i] = ks[i];
  }
  return VLFB_OK;
}

}  // namespace vlfb

using namespace vlfb;

// (vlfb_query_workspace, csrc/vlfb_gemm.hip) -1 = bad arguments
int64_t vlfb_class_ap_workspace_bytes_impl(int64_t n, int64_t cols) {
  if (n < 1 || cols < 1 || n > VLFB_CLASS_AP_MAX_N) return -1;
  return (int64_t)pad_pow2(n) * cols * 5;
}

extern "C" int vlfb_topk_hits(const void* scores, int dtype, const int32_t* labels, int64_t rows, int64_t cols, const int32_t* ks,
                              int nk, int64_t* hits, vlfb_stream_t stream) {
  VLFB_REQUIRE(dtype_ok(dtype), "topk_hits: unknown dtype %d", dtype);
  VLFB_REQUIRE(rows >= 0 && cols >= 1 && rows < (1ll << 31) && cols < (1ll << 31), "topk_hits: bad rows / cols %lld x %lld",
               (long long)rows, (long long)cols);
  TopK tk;
  if (int rc = check_ks("topk_hits", ks, nk, cols, &tk)) return rc;
  VLFB_REQUIRE(hits != nullptr, "topk_hits: hits is required");
  if (rows == 0) return VLFB_OK;
  VLFB_REQUIRE(scores != nullptr && labels != nullptr, "topk_hits: scores and labels are required");
  hipStream_t s = static_cast<hipStream_t>(stream);
  with_elem(dtype, [&](auto t) {
    using T = decltype(t);
    topk_hits_kernel<T, false><<<1, TOPK_WAVES * 64, 0, s>>>(static_cast<const T*>(scores), labels, (int)rows, (int)cols, tk, hits,
                                                             nullptr, nullptr, 0, nullptr);
  });
  return check_launch("topk_hits");
}

extern "C" int vlfb_topk_hits_keep(const void* scores, int dtype, const int32_t* labels, int64_t rows, int64_t cols, const int32_t* ks,
                                   int nk, int64_t* hits, float* table, int32_t* table_labels, int64_t total_rows, int64_t* cursor,
                                   vlfb_stream_t stream) {
  VLFB_REQUIRE(dtype_ok(dtype), "topk_hits_keep: unknown dtype %d", dtype);
  VLFB_REQUIRE(rows >= 0 && cols >= 1 && rows < (1ll << 31) && cols < (1ll << 31), "topk_hits_keep: bad rows / cols %lld x %lld",
               (long long)rows, (long long)cols);
  TopK tk;
  if (int rc = check_ks("topk_hits_keep", ks, nk, cols, &tk)) return rc;
  VLFB_REQUIRE(hits != nullptr, "topk_hits_keep: hits is required");
  VLFB_REQUIRE(table != nullptr && table_labels != nullptr, "topk_hits_keep: table and table_labels are required");
  VLFB_REQUIRE(cursor != nullptr, "topk_hits_keep: cursor is required");
  VLFB_REQUIRE(total_rows >= 1, "topk_hits_keep: total_rows must be positive, got %lld", (long long)total_rows);
  if (rows == 0) return VLFB_OK;
  VLFB_REQUIRE(scores != nullptr && labels != nullptr, "topk_hits_keep: scores and labels are required");
  hipStream_t s = static_cast<hipStream_t>(stream);
  with_elem(dtype, [&](auto t) {
    using T = decltype(t);
    topk_hits_kernel<T, true><<<1, TOPK_WAVES * 64, 0, s>>>(static_cast<const T*>(scores), labels, (int)rows, (int)cols, tk, hits, table,
                                                            table_labels, total_rows, reinterpret_cast<long long*>(cursor));
  });
  return check_launch("topk_hits_keep");
}

extern "C" int vlfb_action_topk_hits(const float* verb, const float* noun, const float* prior, const int32_t* verb_labels,
                                     const int32_t* noun_labels, int64_t rows, int64_t V, int64_t Nn, const int32_t* ks, int nk,
                                     int64_t* hits, vlfb_stream_t stream) {
  VLFB_REQUIRE(rows >= 0 && rows < (1ll << 31) && V >= 1 && Nn >= 1 && V * Nn < (1ll << 31),
               "action_topk_hits: bad rows / V / Nn %lld, %lld, %lld", (long long)rows, (long long)V, (long long)Nn);
  TopK tk;
  if (int rc = check_ks("action_topk_hits", ks, nk, V * Nn, &tk)) return rc;
  VLFB_REQUIRE(hits != nullptr, "action_topk_hits: hits is required");
  if (rows == 0) return VLFB_OK;
  VLFB_REQUIRE(verb && noun && verb_labels && noun_labels, "action_topk_hits: verb, noun and both label vectors are required");
  action_topk_kernel<<<(unsigned)rows, ACT_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      verb, noun, prior, verb_labels, noun_labels, (int)V, (int)Nn, tk, reinterpret_cast<unsigned long long*>(hits));
  return check_launch("action_topk_hits");
}

extern "C" int vlfb_scores_merge_max(const void* scores, int dtype, const int32_t* labels, int64_t rows, int64_t cols, float* table,
                                     uint8_t* table_labels, int64_t n_items, int64_t total_rows, int64_t* cursor,
                                     int32_t* mismatches, vlfb_stream_t stream) {
  VLFB_REQUIRE(dtype_ok(dtype), "scores_merge_max: unknown dtype %d", dtype);
  VLFB_REQUIRE(rows >= 0 && rows < (1ll << 31) && cols >= 1 && cols < (1ll << 31), "scores_merge_max: bad rows / cols %lld x %lld",
               (long long)rows, (long long)cols);
  VLFB_REQUIRE(n_items >= 1, "scores_merge_max: n_items must be positive, got %lld", (long long)n_items);
  VLFB_REQUIRE(table != nullptr && table_labels != nullptr, "scores_merge_max: null table");
  VLFB_REQUIRE(cursor != nullptr && mismatches != nullptr, "scores_merge_max: cursor and mismatches are required");
  if (rows == 0) return VLFB_OK;
  VLFB_REQUIRE(scores != nullptr && labels != nullptr, "scores_merge_max: scores and labels are required");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned grid = (unsigned)((cols + MERGE_THREADS - 1) / MERGE_THREADS);
  long long* cur = reinterpret_cast<long long*>(cursor);
  with_elem(dtype, [&](auto t) {
    using T = decltype(t);
    merge_max_kernel<T><<<grid, MERGE_THREADS, 0, s>>>(static_cast<const T*>(scores), labels, (int)rows, (int)cols, table, table_labels,
                                                      n_items, total_rows, cur, mismatches);
  });
  cursor_advance_kernel<<<1, 64, 0, s>>>(cur, (int)rows);
  return check_launch("scores_merge_max");
}

extern "C" int vlfb_class_ap_auc(const float* table, const uint8_t* table_labels, int64_t n, int64_t cols, double* ap, double* auc,
                                 int32_t* n_pos, void* workspace, int64_t workspace_bytes, int flags, vlfb_stream_t stream) {
  VLFB_REQUIRE(n >= 1 && n <= VLFB_CLASS_AP_MAX_N, "class_ap_auc: n = %lld outside 1..%d", (long long)n, VLFB_CLASS_AP_MAX_N);
  VLFB_REQUIRE(cols >= 1 && cols < (1ll << 31), "class_ap_auc: bad cols %lld", (long long)cols);
  VLFB_REQUIRE(table != nullptr && table_labels != nullptr, "class_ap_auc: null table");
  VLFB_REQUIRE(ap != nullptr && auc != nullptr && n_pos != nullptr, "class_ap_auc: ap, auc and n_pos are required");
  VLFB_REQUIRE((flags & ~VLFB_CLASS_AP_FORCE_GLOBAL) == 0, "class_ap_auc: unknown flags 0x%x", flags);
  const int npad = pad_pow2(n);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (npad <= AP_LDS_MAX && !(flags & VLFB_CLASS_AP_FORCE_GLOBAL)) {
    class_ap_auc_lds_kernel<<<(unsigned)cols, AP_THREADS, 0, s>>>(table, table_labels, (int)n, (int)cols, npad, ap, auc, n_pos);
    return check_launch("class_ap_auc");
  }
  const int64_t need = vlfb_class_ap_workspace_bytes_impl(n, cols);
  if (workspace == nullptr || workspace_bytes < need)
    return set_error(VLFB_ERR_WORKSPACE, "class_ap_auc: short workspace: %lld bytes given, %lld needed (n = %lld, cols = %lld)",
                     (long long)workspace_bytes, (long long)need, (long long)n, (long long)cols);
  uint32_t* wk = static_cast<uint32_t*>(workspace);
  uint8_t* wl = reinterpret_cast<uint8_t*>(wk + (size_t)npad * cols);
  class_ap_auc_global_kernel<<<(unsigned)cols, AP_THREADS, 0, s>>>(table, table_labels, (int)n, (int)cols, npad, wk, wl, ap, auc, n_pos);
  return check_launch("class_ap_auc");
}

// ---- AVA frame-mAP (include/vlfb.h, "AVA frame-mAP"): PASCAL-VOC matching at IoU 0.5 and the envelope AP -----------------
namespace vlfb {

constexpr int AVA_THREADS = 128;               // a lane owns a class (classes beyond 128 are walked in further rounds)
constexpr int AVA_DCHUNK = 32;                 // detections whose IoU row is staged at a time: 32 x 128 fp64 = 32 KiB
constexpr int AVA_NONE = 255;                  // "no ground-truth box at IoU >= 0.5" in the best-box table

__global__ void ava_fill_tp_kernel(uint8_t* __restrict__ tp, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) tp[i] = 255;
}

// ground-truth rows per whitelisted class: a workgroup per class, integer partial counts, one writer
__global__ __launch_bounds__(256) void ava_count_gt_kernel(const int32_t* __restrict__ gt_class, int n_gt_rows,
                                                           const uint8_t* __restrict__ class_mask, int32_t* __restrict__ n_gt) {
  __shared__ int part[4];
  const int c = blockIdx.x;
  int cnt = 0;
  if (class_mask[c])
    for (int i = threadIdx.x; i < n_gt_rows; i += 256) cnt += gt_class[i] == c + 1 ? 1 : 0;
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) n_gt[c] = part[0] + part[1] + part[2] + part[3];
}

__device__ __forceinline__ double box_area(const double* b) { return (b[2] - b[0]) * (b[3] - b[1]); }

// One workgroup per image.  Phase 1 (per chunk of detections): the IoU rows in LDS, then the lane of class c finds, for
// every detection of the chunk, the FIRST index of the maximum IoU over the image's class-c boxes and keeps it when that
// IoU reaches 0.5.  Phase 2: the lane walks the image's detections by (score of its class descending, table row ascending)
// with the taken boxes as a bitmask in registers.  A best box that is taken makes a false positive: no second choice.
__global__ __launch_bounds__(AVA_THREADS) void ava_match_kernel(
    const float* __restrict__ scores, const double* __restrict__ det_box, int n_rows, int cols,
    const int32_t* __restrict__ img_det_ptr, const int32_t* __restrict__ det_rows, int n_det,
    const int32_t* __restrict__ img_gt_ptr, const double* __restrict__ gt_box, const int32_t* __restrict__ gt_class, int n_gt_rows,
    const uint8_t* __restrict__ class_mask, uint8_t* __restrict__ tp) {
  __shared__ double s_db[VLFB_AVA_MAX_DET][4];
  __shared__ double s_gb[VLFB_AVA_MAX_GT][4];
  __shared__ double s_iou[AVA_DCHUNK][VLFB_AVA_MAX_GT];
  __shared__ int s_row[VLFB_AVA_MAX_DET];
  __shared__ int s_gc[VLFB_AVA_MAX_GT];
  __shared__ uint8_t s_best[VLFB_AVA_MAX_DET][AVA_THREADS];
  const int img = blockIdx.x, t = threadIdx.x;
  // The entry point has checked the HOST copy of both CSRs, which the device copy must equal (include/vlfb.h): with equal
  // copies no clamp below ever acts.  They only keep the reads and writes of a call that breaks that rule inside the arrays;
  // its results are undefined, not a truncated evaluation.
  const int d_lo = min(max(img_det_ptr[img], 0), n_det), g_lo = min(max(img_gt_ptr[img], 0), n_gt_rows);
  const int nd = min(max(min(img_det_ptr[img + 1], n_det) - d_lo, 0), VLFB_AVA_MAX_DET);
  const int ng = min(max(min(img_gt_ptr[img + 1], n_gt_rows) - g_lo, 0), VLFB_AVA_MAX_GT);
  if (nd == 0) return;                                          // (block-uniform) ground truth only: counted by ava_count_gt_kernel
  for (int i = t; i < nd; i += AVA_THREADS) {
    const int row = det_rows[d_lo + i];
    const bool ok = row >= 0 && row < n_rows;
    s_row[i] = ok ? row : -1;
    for (int k = 0; k < 4; ++k) s_db[i][k] = ok ? det_box[(size_t)row * 4 + k] : 0.0;
  }
  for (int i = t; i < ng; i += AVA_THREADS) {
    s_gc[i] = gt_class[g_lo + i];
    for (int k = 0; k < 4; ++k) s_gb[i][k] = gt_box[(size_t)(g_lo + i) * 4 + k];
  }
  for (int cb = 0; cb < cols; cb += AVA_THREADS) {              // one round when cols <= 128: the IoU rows are formed once per image
    const int c = cb + t;
    const bool active = c < cols && class_mask[c] != 0;
    for (int d0 = 0; d0 < nd; d0 += AVA_DCHUNK) {
      const int dn = min(AVA_DCHUNK, nd - d0);
      __syncthreads();                                          // boxes staged / the previous chunk's rows read
      for (int e = t; e < dn * ng; e += AVA_THREADS) {
        const int di = e / ng, g = e - di * ng;
        const double* a = s_db[d0 + di];
        const double* b = s_gb[g];
        const double iw = fmin(a[2], b[2]) - fmax(a[0], b[0]);
        const double ih = fmin(a[3], b[3]) - fmax(a[1], b[1]);
        const double inter = fmax(iw, 0.0) * fmax(ih, 0.0);
        s_iou[di][g] = inter / (box_area(a) + box_area(b) - inter);
      }
      __syncthreads();
      if (active)
        for (int di = 0; di < dn; ++di) {
          int best = -1;
          double bv = 0.0;
          for (int g = 0; g < ng; ++g)
            if (s_gc[g] == c + 1) {
              const double v = s_iou[di][g];
              if (best < 0 || v > bv) { best = g; bv = v; }     // strict: the first index of the maximum
            }
          s_best[d0 + di][t] = (best >= 0 && bv >= 0.5) ? (uint8_t)best : (uint8_t)AVA_NONE;
        }
    }
    if (active) {
      unsigned long long done0 = 0, done1 = 0, taken0 = 0, taken1 = 0;
      for (int i = 0; i < nd; ++i)
        if (s_row[i] < 0) { if (i < 64) done0 |= 1ull << i; else done1 |= 1ull << (i - 64); }
      for (int step = 0; step < nd; ++step) {
        int pick = -1, prow = 0;
        float ps = 0.f;
        for (int i = 0; i < nd; ++i) {
          if ((i < 64 ? done0 >> i : done1 >> (i - 64)) & 1ull) continue;
          const int row = s_row[i];
          const float s = scores[(size_t)row * cols + c];
          if (pick < 0 || s > ps || (s == ps && row < prow)) { pick = i; ps = s; prow = row; }
        }
        if (pick < 0) break;
        if (pick < 64) done0 |= 1ull << pick; else done1 |= 1ull << (pick - 64);
        const int b = s_best[pick][t];
        uint8_t hit = 0;
        if (b != AVA_NONE) {
          const bool was = (b < 64 ? taken0 >> b : taken1 >> (b - 64)) & 1ull;
          if (!was) {
            hit = 1;
            if (b < 64) taken0 |= 1ull << b; else taken1 |= 1ull << (b - 64);
          }
        }
        tp[(size_t)prow * cols + c] = hit;
      }
    }
  }
}

// PASCAL AP of one class.  key = order_key(score) << 32 | (0x7fffffff - row) << 1 | tp, 0 for rows without a verdict and
// for the padding: descending order of the key is (score descending, row ascending) with the dropped rows behind everything.
constexpr int VOC_LDS_MAX = 4096;              // 8 B per key: 32 KiB beside the scan and sum buffers

// a / b > c / d for non-negative numerators and positive denominators below 2^31: exact
__device__ __forceinline__ bool frac_gt(int a, int b, int c, int d) { return (long long)a * d > (long long)c * b; }

__device__ __forceinline__ void class_ap_voc_body(const float* __restrict__ scores, const uint8_t* __restrict__ tpv,
                                                  const int32_t* __restrict__ n_gt, int n, int cols, int npad,
                                                  unsigned long long* keys, int* ibuf, double* dbuf, double* __restrict__ ap) {
  const int c = blockIdx.x, t = threadIdx.x;
  for (int i = t; i < npad; i += AP_THREADS) {
    unsigned long long k = 0;
    if (i < n) {
      const uint8_t v = tpv[(size_t)i * cols + c];
      if (v <= 1)
        k = ((unsigned long long)order_key(scores[(size_t)i * cols + c]) << 32) | ((unsigned long long)(0x7fffffffu - (uint32_t)i) << 1) | v;
    }
    keys[i] = k;
  }
  __syncthreads();
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = t; p < (npad >> 1); p += AP_THREADS) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const int l = i | j;
        const bool desc = (i & k) == 0;
        const unsigned long long a = keys[i], b = keys[l];
        if (desc ? a < b : a > b) { keys[i] = b; keys[l] = a; }
      }
      __syncthreads();
    }
  // thread t owns the chunk [lo, hi) of the sorted column; rows with a verdict come first
  const int L = (npad + AP_THREADS - 1) / AP_THREADS;
  const int lo = min(t * L, npad), hi = min(lo + L, npad);
  int cnt = 0, last = lo - 1;                                    // true positives of the chunk; its last row with a verdict
  for (int i = lo; i < hi; ++i)
    if (keys[i] != 0) { cnt += (int)(keys[i] & 1ull); last = i; }
  const int before = block_exclusive<false>(cnt, 0, ibuf);       // true positives in [0, lo)
  // the chunk's largest precision ctp_i / (i + 1), as an exact fraction (0 / 1 when the chunk holds no row)
  int bn = 0, bd = 1, ctp = before;
  for (int i = lo; i <= last; ++i) {
    ctp += (int)(keys[i] & 1ull);
    if (frac_gt(ctp, i + 1, bn, bd)) { bn = ctp; bd = i + 1; }
  }
  ibuf[t] = bn;
  ibuf[AP_THREADS + t] = bd;
  __syncthreads();
  int sn = 0, sd = 1;                                            // suffix maximum over the chunks behind this one
  for (int u = t + 1; u < AP_THREADS; ++u)
    if (frac_gt(ibuf[u], ibuf[AP_THREADS + u], sn, sd)) { sn = ibuf[u]; sd = ibuf[AP_THREADS + u]; }
  const long long G = n_gt[c];
  double sum = 0.0;
  ctp = before + cnt;
  for (int i = last; i >= lo; --i) {                             // right to left: (sn, sd) = max_{j >= i} ctp_j / (j + 1)
    if (frac_gt(ctp, i + 1, sn, sd)) { sn = ctp; sd = i + 1; }
    if (keys[i] & 1ull) {
      if (G > 0) sum += (double)sn / (double)((long long)sd * G);
      --ctp;
    }
  }
  dbuf[t] = sum;
  __syncthreads();
  for (int off = AP_THREADS >> 1; off > 0; off >>= 1) {
    if (t < off) dbuf[t] += dbuf[t + off];
    __syncthreads();
  }
  if (t == 0) ap[c] = G > 0 ? dbuf[0] : __longlong_as_double(0x7ff8000000000000ll);
}

__global__ __launch_bounds__(AP_THREADS) void class_ap_voc_lds_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ tpv,
                                                                     const int32_t* __restrict__ n_gt, int n, int cols, int npad,
                                                                     double* __restrict__ ap) {
  __shared__ unsigned long long keys[VOC_LDS_MAX];
  __shared__ int ibuf[2 * AP_THREADS];
  __shared__ double dbuf[AP_THREADS];
  class_ap_voc_body(scores, tpv, n_gt, n, cols, npad, keys, ibuf, dbuf, ap);
}
__global__ __launch_bounds__(AP_THREADS) void class_ap_voc_global_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ tpv,
                                                                        const int32_t* __restrict__ n_gt, int n, int cols, int npad,
                                                                        unsigned long long* ws_keys, double* __restrict__ ap) {
  __shared__ int ibuf[2 * AP_THREADS];
  __shared__ double dbuf[AP_THREADS];
  class_ap_voc_body(scores, tpv, n_gt, n, cols, npad, ws_keys + (size_t)blockIdx.x * npad, ibuf, dbuf, ap);
}

// a host copy of a CSR: starts at 0, never decreases, no image above `limit` entries; *total = its last value
static int check_csr(const char* what, const int32_t* p, int64_t n_img, int limit, int64_t* total) {
  VLFB_REQUIRE(p != nullptr, "ava_match_tp: the host copy of the %s CSR is required", what);
  VLFB_REQUIRE(p[0] == 0, "ava_match_tp: the %s CSR starts at %d, not 0", what, p[0]);
  for (int64_t i = 0; i < n_img; ++i) {
    VLFB_REQUIRE(p[i + 1] >= p[i], "ava_match_tp: the %s CSR decreases at image %lld", what, (long long)i);
    VLFB_REQUIRE(p[i + 1] - p[i] <= limit, "ava_match_tp: image %lld has %d %s rows, more than the %d one workgroup holds", (long long)i,
                 p[i + 1] - p[i], what, limit);
  }
  *total = p[n_img];
  return VLFB_OK;
}

}  // namespace vlfb

int64_t vlfb_class_ap_voc_workspace_bytes_impl(int64_t n, int64_t cols) {
  if (n < 1 || cols < 1 || n > VLFB_CLASS_AP_MAX_N) return -1;
  return (int64_t)pad_pow2(n) * cols * 8;
}

extern "C" int vlfb_ava_match_tp(const float* scores, const double* det_box, int64_t n_rows, int64_t cols,
                                 const int32_t* img_det_ptr, const int32_t* det_rows, const int32_t* img_gt_ptr,
                                 const double* gt_box, const int32_t* gt_class, int64_t n_img, const int32_t* host_img_det_ptr,
                                 const int32_t* host_img_gt_ptr, const uint8_t* class_mask, uint8_t* tp, int32_t* n_gt,
                                 vlfb_stream_t stream) {
  VLFB_REQUIRE(n_rows >= 1 && n_rows < (1ll << 31) && cols >= 1 && cols < (1ll << 31) && n_rows * cols < (1ll << 40),
               "ava_match_tp: bad n_rows / cols %lld x %lld", (long long)n_rows, (long long)cols);
  VLFB_REQUIRE(n_img >= 0 && n_img < (1ll << 31), "ava_match_tp: bad n_img %lld", (long long)n_img);
  int64_t n_det = 0, n_gt_rows = 0;
  if (int rc = check_csr("detection", host_img_det_ptr, n_img, VLFB_AVA_MAX_DET, &n_det)) return rc;
  if (int rc = check_csr("ground-truth", host_img_gt_ptr, n_img, VLFB_AVA_MAX_GT, &n_gt_rows)) return rc;
  VLFB_REQUIRE(n_det <= n_rows, "ava_match_tp: %lld detections named for a table of %lld rows", (long long)n_det, (long long)n_rows);
  VLFB_REQUIRE(scores && class_mask && tp && n_gt, "ava_match_tp: scores, class_mask, tp and n_gt are required");
  VLFB_REQUIRE(n_img == 0 || (img_det_ptr && img_gt_ptr), "ava_match_tp: the device copies of both CSRs are required");
  VLFB_REQUIRE(n_det == 0 || (det_box && det_rows), "ava_match_tp: det_box and det_rows are required");
  VLFB_REQUIRE(n_gt_rows == 0 || (gt_box && gt_class), "ava_match_tp: gt_box and gt_class are required");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long cells = (long long)n_rows * cols;
  ava_fill_tp_kernel<<<(unsigned)std::min<long long>((cells + 255) / 256, 4096), 256, 0, s>>>(tp, cells);
  ava_count_gt_kernel<<<(unsigned)cols, 256, 0, s>>>(gt_class, (int)n_gt_rows, class_mask, n_gt);
  if (n_img > 0 && n_det > 0)
    ava_match_kernel<<<(unsigned)n_img, AVA_THREADS, 0, s>>>(scores, det_box, (int)n_rows, (int)cols, img_det_ptr, det_rows, (int)n_det,
                                                            img_gt_ptr, gt_box, gt_class, (int)n_gt_rows, class_mask, tp);
  return check_launch("ava_match_tp");
}

extern "C" int vlfb_class_ap_voc(const float* scores, const uint8_t* tp, const int32_t* n_gt, int64_t n, int64_t cols, double* ap,
                                 void* workspace, int64_t workspace_bytes, int flags, vlfb_stream_t stream) {
  VLFB_REQUIRE(n >= 1 && n <= VLFB_CLASS_AP_MAX_N, "class_ap_voc: n = %lld outside 1..%d", (long long)n, VLFB_CLASS_AP_MAX_N);
  VLFB_REQUIRE(cols >= 1 && cols < (1ll << 31), "class_ap_voc: bad cols %lld", (long long)cols);
  VLFB_REQUIRE(scores != nullptr && tp != nullptr && n_gt != nullptr, "class_ap_voc: scores, tp and n_gt are required");
  VLFB_REQUIRE(ap != nullptr, "class_ap_voc: ap is required");
  VLFB_REQUIRE((flags & ~VLFB_CLASS_AP_FORCE_GLOBAL) == 0, "class_ap_voc: unknown flags 0x%x", flags);
  const int npad = pad_pow2(n);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (npad <= VOC_LDS_MAX && !(flags & VLFB_CLASS_AP_FORCE_GLOBAL)) {
    class_ap_voc_lds_kernel<<<(unsigned)cols, AP_THREADS, 0, s>>>(scores, tp, n_gt, (int)n, (int)cols, npad, ap);
    return check_launch("class_ap_voc");
  }
  const int64_t need = vlfb_class_ap_voc_workspace_bytes_impl(n, cols);
  if (workspace == nullptr || workspace_bytes < need)
    return set_error(VLFB_ERR_WORKSPACE, "class_ap_voc: short workspace: %lld bytes given, %lld needed (n = %lld, cols = %lld)",
                     (long long)workspace_bytes, (long long)need, (long long)n, (long long)cols);
  class_ap_voc_global_kernel<<<(unsigned)cols, AP_THREADS, 0, s>>>(scores, tp, n_gt, (int)n, (int)cols, npad,
                                                                  static_cast<unsigned long long*>(workspace), ap);
  return check_launch("class_ap_voc");
}

// ---- AVA multi-crop merge (include/vlfb.h, "AVA multi-crop merge"): the three spatial shifts of one (scale, flip) ---------
namespace vlfb {

constexpr int MC_THREADS = 256;
constexpr long long MC_MAX_BLOCKS = 1 << 16;

// a logit as fp64: exact for every element type (fp64 logits are the ones parsed from score files)
template <typename T> __device__ __forceinline__ double mc_logit(const T* p) { return (double)Elem<T>::ld(p); }
template <> __device__ __forceinline__ double mc_logit<double>(const double* p) { return *p; }

// A thread owns one (row, class) element; the row's geometry is a handful of fp64 operations and is formed again by every
// thread of the row, so that no thread waits for another.  The thread of class 0 writes the row's mask.
template <typename T>
__global__ __launch_bounds__(MC_THREADS) void multicrop_merge_kernel(const T* __restrict__ logits, long long shift_stride, long long ld,
                                                                     const double* __restrict__ boxes, const int32_t* __restrict__ frame_hw,
                                                                     long long rows, int cols, int scale, int max_crop, int flip, int first,
                                                                     double* __restrict__ acc, float* __restrict__ out32,
                                                                     uint8_t* __restrict__ valid) {
  const long long n = rows * cols;
  for (long long i = (long long)blockIdx.x * MC_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * MC_THREADS) {
    const long long r = i / cols;
    const int c = (int)(i - r * cols);
    const long long height = frame_hw[2 * r], width = frame_hw[2 * r + 1];
    const double w = (double)(width * scale) / (double)height;
    const double nc = (double)(scale < max_crop ? scale : max_crop) / w;
    const double center_left = 0.5 - nc / 2.0, center_right = 0.5 + nc / 2.0;
    const double lcrop_right = nc, rcrop_left = 1.0 - nc;
    double x1 = boxes[4 * r], x2 = boxes[4 * r + 2];
    if (flip) {
      const double a = 1.0 - x2, b = 1.0 - x1;
      x1 = a;
      x2 = b;
    }
    const bool v[3] = {x1 < lcrop_right, x2 > center_left && x1 < center_right, x2 > rcrop_left};
    double sum = 0.0;
    int nv = 0;
#pragma unroll
    for (int s = 0; s < 3; ++s)
      if (v[s]) {                                                 // (a shift that does not see the box is not read)
        const double x = mc_logit<T>(logits + s * shift_stride + r * ld + c);
        sum += 1.0 / (1.0 + exp(-x));
        ++nv;
      }
    const double combined = sum / (double)nv;                     // 0 / 0 = NaN for a box no crop sees, like np.mean([])
    const double a = first ? combined : acc[i] + combined;
    acc[i] = a;
    if (out32) out32[i] = (float)a;
    if (valid && c == 0) valid[r] = (uint8_t)((v[0] ? 1 : 0) | (v[1] ? 2 : 0) | (v[2] ? 4 : 0));
  }
}

}  // namespace vlfb

extern "C" int vlfb_multicrop_merge(const void* logits, int dtype, int64_t shift_stride, int64_t ld, const double* boxes,
                                    const int32_t* frame_hw, int64_t rows, int64_t cols, int scale, int max_crop, int flip, int first,
                                    double* acc, float* out32, uint8_t* valid, vlfb_stream_t stream) {
  VLFB_REQUIRE(dtype_ok(dtype) || dtype == VLFB_F64, "multicrop_merge: unknown dtype %d", dtype);
  VLFB_REQUIRE(rows >= 0 && rows < (1ll << 31), "multicrop_merge: bad rows %lld", (long long)rows);
  VLFB_REQUIRE(cols >= 1 && cols < (1ll << 31), "multicrop_merge: bad cols %lld", (long long)cols);
  VLFB_REQUIRE(ld >= cols, "multicrop_merge: ld = %lld is less than cols = %lld", (long long)ld, (long long)cols);
  VLFB_REQUIRE(shift_stride >= 0, "multicrop_merge: negative shift_stride %lld", (long long)shift_stride);
  VLFB_REQUIRE(scale >= 1, "multicrop_merge: scale must be positive, got %d", scale);
  VLFB_REQUIRE(max_crop >= 1, "multicrop_merge: max_crop must be positive, got %d", max_crop);
  VLFB_REQUIRE(logits != nullptr, "multicrop_merge: logits is required");
  VLFB_REQUIRE(boxes != nullptr, "multicrop_merge: boxes is required");
  VLFB_REQUIRE(frame_hw != nullptr, "multicrop_merge: frame_hw is required");
  VLFB_REQUIRE(acc != nullptr, "multicrop_merge: acc is required");
  if (rows == 0) return VLFB_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long n = (long long)rows * cols;
  const unsigned grid = (unsigned)std::min<long long>((n + MC_THREADS - 1) / MC_THREADS, MC_MAX_BLOCKS);
  auto launch = [&](auto t) {
    using T = decltype(t);
    multicrop_merge_kernel<T><<<grid, MC_THREADS, 0, s>>>(static_cast<const T*>(logits), shift_stride, ld, boxes, frame_hw, rows, (int)cols,
                                                          scale, max_crop, flip ? 1 : 0, first ? 1 : 0, acc, out32, valid);
  };
  if (dtype == VLFB_F64) launch(double{});
  else with_elem(dtype, launch);
  return check_launch("multicrop_merge");
}

// ---- rank interleave: the global stream order of a pass rebuilt from the ranks' own row tables -------------------------
// A pure row copy (row_copy of csrc/vlfb_lfb.hip without the conversion): a wave per destination row, every destination
// byte has one writer, no atomics.  V is the widest access the host found legal for `row_bytes` and every base address.
namespace vlfb {

constexpr int IL_THREADS = 256, IL_MAX_BLOCKS = 65536;
struct InterleaveParts { const char* part[VLFB_ROWS_INTERLEAVE_MAX_WORLD]; };

template <typename V>
__global__ __launch_bounds__(IL_THREADS) void rows_interleave_kernel(InterleaveParts parts, int world, long long b, long long row_bytes,
                                                                     long long total, char* __restrict__ dst) {
  const int lane = threadIdx.x & 63, waves = IL_THREADS / 64;
  const long long per = row_bytes / (long long)sizeof(V);
  for (long long g = (long long)blockIdx.x * waves + (threadIdx.x >> 6); g < total; g += (long long)gridDim.x * waves) {
    const long long slice = g / b;
    const long long src_row = (slice / world) * b + g % b;
    const V* s = reinterpret_cast<const V*>(parts.part[slice % world] + src_row * row_bytes);
    V* d = reinterpret_cast<V*>(dst + g * row_bytes);
    for (long long i = lane; i < per; i += 64) d[i] = s[i];
  }
}

}  // namespace vlfb

extern "C" int vlfb_rows_interleave(const void* const* parts, const int64_t* part_rows, int world, int64_t b, int64_t row_bytes,
                                    int64_t total, void* dst, vlfb_stream_t stream) {
  VLFB_REQUIRE(world >= 1 && world <= VLFB_ROWS_INTERLEAVE_MAX_WORLD, "rows_interleave: world = %d outside 1..%d", world,
               VLFB_ROWS_INTERLEAVE_MAX_WORLD);
  VLFB_REQUIRE(b >= 1 && b < (1ll << 31), "rows_interleave: slice height b = %lld outside 1..2^31-1", (long long)b);
  VLFB_REQUIRE(row_bytes >= 1 && row_bytes < (1ll << 31), "rows_interleave: row_bytes = %lld outside 1..2^31-1", (long long)row_bytes);
  VLFB_REQUIRE(total >= 0 && total < (1ll << 40), "rows_interleave: total = %lld outside 0..2^40-1", (long long)total);
  VLFB_REQUIRE(parts != nullptr && part_rows != nullptr, "rows_interleave: parts and part_rows are required");
  if (total == 0) return VLFB_OK;
  VLFB_REQUIRE(dst != nullptr, "rows_interleave: dst is required");
  // part p is asked for b rows per complete global iteration, and for its share of the last, cut one
  const long long per_iter = (long long)b * world, full = total / per_iter, rem = total % per_iter;
  InterleaveParts ip;
  uintptr_t bits = reinterpret_cast<uintptr_t>(dst) | (uintptr_t)row_bytes;
  for (int p = 0; p < VLFB_ROWS_INTERLEAVE_MAX_WORLD; ++p) ip.part[p] = nullptr;
  for (int p = 0; p < world; ++p) {
    const long long need = full * b + std::min<long long>(std::max<long long>(rem - (long long)p * b, 0), b);
    VLFB_REQUIRE(part_rows[p] >= need, "rows_interleave: part %d holds %lld rows, %lld are asked of it", p, (long long)part_rows[p], need);
    VLFB_REQUIRE(need == 0 || parts[p] != nullptr, "rows_interleave: part %d is NULL, %lld rows are asked of it", p, need);
    ip.part[p] = static_cast<const char*>(parts[p]);
    if (need) bits |= reinterpret_cast<uintptr_t>(parts[p]);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long blocks = (total + IL_THREADS / 64 - 1) / (IL_THREADS / 64);
  const unsigned grid = (unsigned)std::min<long long>(blocks, IL_MAX_BLOCKS);
  char* d = static_cast<char*>(dst);
  if ((bits & 15) == 0) rows_interleave_kernel<uint4><<<grid, IL_THREADS, 0, s>>>(ip, world, b, row_bytes, total, d);
  else if ((bits & 3) == 0) rows_interleave_kernel<uint32_t><<<grid, IL_THREADS, 0, s>>>(ip, world, b, row_bytes, total, d);
  else rows_interleave_kernel<uint8_t><<<grid, IL_THREADS, 0, s>>>(ip, world, b, row_bytes, total, d);
  return check_launch("rows_interleave");
}
