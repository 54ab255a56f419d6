// Evaluation metrics on the device (include/vlfb.h, "Evaluation metrics"): top-k hit counters, the clip-merge score
// table, per-class average precision / ROC-AUC, EPIC action top-k.  Replaces the host meter of the reference's
// lib/utils/metrics.py and tools/evaluate_actions.py, which fetches `pred` and `labels` every iteration.
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
constexpr int TOPK_WAVES = 4;
template <typename T>
__global__ __launch_bounds__(TOPK_WAVES * 64) void topk_hits_kernel(const T* __restrict__ scores, const int32_t* __restrict__ labels,
                                                                    int rows, int cols, TopK ks, int64_t* __restrict__ hits) {
  __shared__ int part[TOPK_WAVES][MAX_K + 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int mine[MAX_K + 1] = {0, 0, 0, 0, 0};
  for (int r = wave; r < rows; r += TOPK_WAVES) {
    const int jl = labels[r];
    if (jl < 0 || jl >= cols) continue;                       // (wave-uniform)
    const T* row = scores + (size_t)r * cols;
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
  if (dtype == VLFB_F32)
    topk_hits_kernel<float><<<1, TOPK_WAVES * 64, 0, s>>>(static_cast<const float*>(scores), labels, (int)rows, (int)cols, tk, hits);
  else
    VLFB_WITH_T16(dtype, (topk_hits_kernel<T16><<<1, TOPK_WAVES * 64, 0, s>>>(static_cast<const T16*>(scores), labels, (int)rows,
                                                                               (int)cols, tk, hits)));
  return check_launch("topk_hits");
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
  if (dtype == VLFB_F32)
    merge_max_kernel<float><<<grid, MERGE_THREADS, 0, s>>>(static_cast<const float*>(scores), labels, (int)rows, (int)cols, table,
                                                          table_labels, n_items, total_rows, cur, mismatches);
  else
    VLFB_WITH_T16(dtype, (merge_max_kernel<T16><<<grid, MERGE_THREADS, 0, s>>>(static_cast<const T16*>(scores), labels, (int)rows,
                                                                                (int)cols, table, table_labels, n_items, total_rows,
                                                                                cur, mismatches)));
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
