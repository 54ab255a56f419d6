// Baseline JPEG decode of a batch of frames (include/vlfb.h, vlfb_jpeg_*): entropy decode, inverse DCT, upsample + colour.
// The format arithmetic is csrc/vlfb_jpeg_core.h; this file holds the three kernels around it, the checks of the host array
// and the host-compiled checker.
#include <vector>

#include "vlfb_common.h"
#include "vlfb_jpeg_core.h"

namespace vlfb {
namespace {

using namespace jpeg;

static_assert(sizeof(vlfb_jpeg_item) == VLFB_JPEG_ITEM_BYTES, "vlfb_jpeg_item has padding");

// ---- stage 1: entropy decode ------------------------------------------------------------------------------------------------
// One wave per segment (restart interval), grid (segment, item).  Lanes 0..3 build the four Huffman tables in LDS; the wave
// copies a window of the segment's bytes into LDS with 16-byte loads, lane 0 decodes whole MCUs from it into an LDS block
// buffer while the window still holds a worst-case MCU, and the wave stores each MCU's blocks (zeros included, so the
// workspace needs no clearing) with 16-byte stores.  Every loop is bounded by the segment's MCU count.
// par_subseq: 0 from vlfb_jpeg_decode_batch -- every item is this kernel's.  From vlfb_jpeg_decode_batch_par it is the
// subsequence size of the call: an item the routing rule gives to the parallel kernel is decoded here only if that kernel
// marked it (PAR_REDO_BIT of its status word), by the one wave such an item has, which takes the mark away.
constexpr int WIN_BYTES = 8192;
static_assert(WIN_BYTES >= 2 * MAX_MCU_BYTES + 64, "a window holds a worst-case MCU beside what the reader has buffered");

__global__ void __launch_bounds__(64) jpeg_entropy_kernel(const vlfb_jpeg_item* __restrict__ items, uint8_t* __restrict__ workspace,
                                                          int32_t* __restrict__ status, int par_subseq) {
  __shared__ Huff tabs[4];
  __shared__ __attribute__((aligned(16))) uint8_t win[WIN_BYTES];
  __shared__ __attribute__((aligned(16))) int16_t mcu_buf[MAX_MCU_BLOCKS * 64];
  __shared__ int32_t sh_pos, sh_err, sh_tab_bad, sh_redo;

  const vlfb_jpeg_item& it = items[blockIdx.y];
  const int lane = threadIdx.x;
  Geo g;
  const bool geo_ok = geometry(it, &g);
  const int32_t ri = it.restart_interval > 0 ? it.restart_interval : 0;
  const int64_t want = expected_segments(g, ri);
  const int64_t s = blockIdx.x;
  if (s >= want) return;
  if (par_subseq && vlfb_jpeg_item_is_parallel(it, par_subseq)) {     // want is 1: this wave alone reads and clears the mark
    if (lane == 0) sh_redo = atomicAnd(status + blockIdx.y, ~PAR_REDO_BIT) & PAR_REDO_BIT;
    __syncthreads();
    if (!sh_redo) return;
  }
  const int64_t mcus = total_mcus(g);
  const int64_t mcu0 = ri ? s * ri : 0;
  const int64_t mcu1 = ri ? (mcu0 + ri < mcus ? mcu0 + ri : mcus) : mcus;

  const uint8_t* scan = (const uint8_t*)it.scan;
  const uint32_t scan_bytes = it.scan_bytes < (1u << 30) ? it.scan_bytes : 0u;
  uint8_t* ws = workspace + it.ws_offset;

  if (lane == 0) sh_tab_bad = 0;
  __syncthreads();
  if (lane < 4 && !huff_build(it.huff[lane], &tabs[lane])) sh_tab_bad = 1;
  __syncthreads();

  int32_t seg_lo = 0, seg_hi = 0;
  int err = segment_range(scan, scan_bytes, (const uint32_t*)it.seg_offsets, it.n_segments, want, s, &seg_lo, &seg_hi);
  if (sh_tab_bad || !geo_ok) err |= VLFB_JPEG_BAD_CODE;
  if (err) seg_lo = seg_hi = 0;
  if (err && lane == 0) atomicOr(status + blockIdx.y, err);   // a segment that never runs (bad tables, a misplaced marker)

  Bits br;
  bits_init(&br, win, 0, seg_lo, seg_lo, 0);
  int pred[3] = {0, 0, 0};
  int32_t win_end = seg_lo;                  // the window holds stream bytes [win_base, win_end)
  int32_t pos = seg_lo;

  for (int64_t m = mcu0; m < mcu1; ++m) {
    if (!err && win_end < seg_hi && pos + MAX_MCU_BYTES + 16 > win_end) {
      // slide the window to the reader's position; 16-byte loads where all 16 bytes are inside the scan
      const int32_t base = pos - (int32_t)(((uintptr_t)scan + (uintptr_t)pos) & 15u);
      for (int v = lane; v < WIN_BYTES / 16; v += 64) {
        const int32_t off = base + v * 16;
        if (off >= 0 && (uint32_t)off + 16u <= scan_bytes) {
          *reinterpret_cast<uint4*>(win + v * 16) = *reinterpret_cast<const uint4*>(scan + off);
        } else {
          for (int k = 0; k < 16; ++k) win[v * 16 + k] = (off + k >= 0 && (uint32_t)(off + k) < scan_bytes) ? scan[off + k] : (uint8_t)0;
        }
      }
      win_end = base + WIN_BYTES < seg_hi ? base + WIN_BYTES : seg_hi;
      br.base = base;
      if (!br.ended) {                       // a reader that met a marker keeps its end
        br.hi = win_end;
        br.windowed = win_end < seg_hi ? 1 : 0;
      }
    }
    for (int k = lane; k < MAX_MCU_BLOCKS * 64 / 8; k += 64) reinterpret_cast<uint4*>(mcu_buf)[k] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    if (lane == 0) {
      int e = err;
      if (!e) e = decode_mcu(&br, g, tabs, it.td, it.ta, pred, mcu_buf);
      sh_err = e;
      sh_pos = br.pos;
    }
    __syncthreads();
    const int e = sh_err;
    pos = sh_pos;
    if (e && !err && lane == 0) atomicOr(status + blockIdx.y, e);
    // the MCU's blocks, 128 bytes each: 8 lanes per block; zeros once the segment has stopped
    const int blk = lane >> 3;
    if (blk < g.mcu_blocks && blk < MAX_MCU_BLOCKS) {
      int comp;
      int64_t block;
      mcu_block_place(g, m, blk, &comp, &block);
      const uint4 val = e ? make_uint4(0, 0, 0, 0) : reinterpret_cast<const uint4*>(mcu_buf)[lane];
      reinterpret_cast<uint4*>(ws + coef_offset(g, comp) + block * 128)[lane & 7] = val;
    }
    err = e;
    __syncthreads();
  }
}

// ---- stage 1, lane-parallel (csrc/vlfb_jpeg_core.h, "lane-parallel entropy decode") -----------------------------------------
// One workgroup of PAR_LANES lanes per item, grid n_items; items the routing rule refuses return at once.  The workgroup
// clears the coefficient area, destuffs the scan into LDS (count per slice, workgroup scan, compact), then per chunk of
// PAR_LANES subsequences: round 0 from guessed states, synchronisation rounds until no exit state changes (at most PAR_LANES
// rounds in all), a scan of the MCU counts, the write pass.  At the end one prefix sum per component turns the DC
// differences into coefficients.  Anything unusual marks the item for the serial kernel that follows in the same call.
// Every loop is bounded before it starts: slice bytes, 8 * subseq_bytes symbols, PAR_LANES rounds, ceil(scan / chunk) chunks.

// exclusive prefix sums over the workgroup of one value per lane, *total: their sum; every lane calls it
__device__ uint32_t par_block_scan(uint32_t v, uint32_t* sh, uint32_t* total) {
  const int lane = threadIdx.x;
  sh[lane] = v;
  __syncthreads();
  for (int d = 1; d < PAR_LANES; d <<= 1) {
    const uint32_t t = lane >= d ? sh[lane - d] : 0u;
    __syncthreads();
    sh[lane] += t;
    __syncthreads();
  }
  const uint32_t incl = sh[lane];
  *total = sh[PAR_LANES - 1];
  __syncthreads();
  return incl - v;
}

__global__ void __launch_bounds__(PAR_LANES) jpeg_entropy_par_kernel(const vlfb_jpeg_item* __restrict__ items,
                                                                     uint8_t* __restrict__ workspace, int32_t* __restrict__ status,
                                                                     int32_t* __restrict__ stats, int subseq, uint32_t stream_words) {
  extern __shared__ __attribute__((aligned(16))) uint32_t par_words[];   // stream_words: par_stream_words(largest parallel scan)
  __shared__ Huff tabs[4];
  __shared__ ParState sh_exit[PAR_LANES];
  __shared__ uint32_t sh_scan[PAR_LANES];
  __shared__ uint32_t sh_end;
  __shared__ int32_t sh_tab_bad;

  const int item = blockIdx.x, lane = threadIdx.x;
  const vlfb_jpeg_item& it = items[item];
  if (!vlfb_jpeg_item_is_parallel(it, subseq)) {
    if (stats && lane < 4) stats[4 * item + lane] = 0;
    return;
  }
  Geo g;
  const bool geo_ok = geometry(it, &g);
  const uint8_t* scan = (const uint8_t*)it.scan;
  const uint32_t n = it.scan_bytes;                  // <= PAR_MAX_SCAN by the rule
  uint8_t* ws = workspace + it.ws_offset;
  const int64_t total = total_mcus(g);

  if (lane == 0) { sh_tab_bad = 0; sh_end = n; }
  __syncthreads();
  if (lane < 4 && !huff_build(it.huff[lane], &tabs[lane])) sh_tab_bad = 1;
  __syncthreads();
  int32_t chunks = 0, rounds_sum = 0, rounds_max = 0;
  // uniform over the workgroup; a device record with a longer scan than the host array's (which sized par_words) is not decoded here
  int redo = (sh_tab_bad || !geo_ok || par_stream_words(n) > stream_words) ? 1 : 0;
  if (!redo) {
    for (int64_t i = lane; i < g.first_block[3] * 8; i += PAR_LANES) reinterpret_cast<uint4*>(ws)[i] = make_uint4(0, 0, 0, 0);

    // destuff: lane's slice [lo, hi) of the scan; the bytes it keeps in front of its first marker, the first marker of all
    const uint32_t slice = (n + PAR_LANES - 1) / PAR_LANES;
    const uint32_t lo = (uint32_t)lane * slice < n ? (uint32_t)lane * slice : n, hi = lo + slice < n ? lo + slice : n;
    uint32_t kept = 0, mark = n;
    for (uint32_t i = lo; i < hi; ++i) {
      if (par_is_marker(scan, n, i)) { mark = i; break; }
      if (!par_is_stuffing(scan, i)) ++kept;
    }
    if (mark < n) atomicMin(&sh_end, mark);
    __syncthreads();
    const uint32_t end = sh_end;
    if (lo >= end) kept = 0;                         // a slice behind the data's end; one that holds the end stopped there
    uint32_t stream_bytes;
    uint32_t at = par_block_scan(kept, sh_scan, &stream_bytes);
    uint8_t* bytes = reinterpret_cast<uint8_t*>(par_words);
    for (uint32_t i = lo; i < hi && i < end; ++i)
      if (!par_is_stuffing(scan, i)) bytes[par_byte_slot(at++)] = scan[i];
    for (uint32_t j = stream_bytes + lane; j < 4u * par_stream_words(stream_bytes); j += PAR_LANES) bytes[par_byte_slot(j)] = 0;
    __syncthreads();

    ParCtx cx;
    cx.words = par_words;
    cx.data_bits = stream_bytes * 8u;
    cx.tabs = tabs;
    cx.sel = par_table_select(g, it.td, it.ta);
    cx.mcu_blocks = g.mcu_blocks;
    const uint32_t chunk_bytes = (uint32_t)PAR_LANES * (uint32_t)subseq;
    const int32_t max_syms = 8 * subseq;
    chunks = (int32_t)((n + chunk_bytes - 1) / chunk_bytes);
    ParState carry = {0u, 0u};
    int64_t carry_mcu = 0;
    for (int32_t c = 0; c < chunks; ++c) {
      const uint32_t start_bit = ((uint32_t)c * chunk_bytes + (uint32_t)lane * (uint32_t)subseq) * 8u;   // < 8 * (n + chunk): 25 bits
      const uint32_t end_bit = start_bit + 8u * subseq < cx.data_bits ? start_bit + 8u * subseq : cx.data_bits;
      const int32_t live = par_live_lanes(cx.data_bits, (uint32_t)c * chunk_bytes * 8u, PAR_LANES, subseq);
      const ParState guess = {start_bit, 0u}, none = {PAR_NO_STATE, 0u};
      ParState my_in = lane >= live ? none : (lane == 0 ? carry : guess), my_exit;
      int32_t my_mcus;
      par_walk(cx, my_in, end_bit, max_syms, &my_exit, &my_mcus);
      sh_exit[lane] = my_exit;
      int32_t rounds = 1;
      __syncthreads();
      for (int r = 1; r < live; ++r) {
        const ParState in = lane >= live ? none : (lane == 0 ? carry : sh_exit[lane - 1]);
        __syncthreads();
        int moved = 0;
        if (!par_same(in, my_in)) {
          ParState out;
          par_walk(cx, in, end_bit, max_syms, &out, &my_mcus);
          my_in = in;
          moved = par_same(out, my_exit) ? 0 : 1;
          my_exit = out;
          sh_exit[lane] = out;
        }
        ++rounds;
        if (!__syncthreads_or(moved)) break;         // no exit state changed: every lane started from its neighbour's
      }
      uint32_t chunk_mcus;
      const uint32_t before = par_block_scan((uint32_t)my_mcus, sh_scan, &chunk_mcus);
      if (live > 0) carry = sh_exit[live - 1];
      if (lane < live && !par_write(cx, g, my_in, end_bit, max_syms, carry_mcu + before, total, ws)) redo = 1;
      carry_mcu += chunk_mcus;
      rounds_sum += rounds;
      rounds_max = rounds > rounds_max ? rounds : rounds_max;
      __syncthreads();                               // sh_exit is rewritten by the next chunk
    }
    if (carry_mcu < total) redo = 1;                 // the data ended before the last MCU
  }
  redo = __syncthreads_or(redo);
  if (stats && lane == 0) {
    stats[4 * item + 0] = redo ? 2 : 1;
    stats[4 * item + 1] = chunks;
    stats[4 * item + 2] = rounds_sum;
    stats[4 * item + 3] = rounds_max;
  }
  if (redo) {
    if (lane == 0) atomicOr(status + item, PAR_REDO_BIT);
    return;
  }
  // DC: lane's run of MCUs, the sums before it, the coefficients
  const int64_t per = (total + PAR_LANES - 1) / PAR_LANES;
  const int64_t m0 = lane * per < total ? lane * per : total, m1 = m0 + per < total ? m0 + per : total;
  uint32_t sums[3] = {0u, 0u, 0u}, pred[3], all;
  par_dc_sum(g, ws, m0, m1, sums);
  for (int k = 0; k < 3; ++k) pred[k] = par_block_scan(sums[k], sh_scan, &all);
  par_dc_apply(g, ws, m0, m1, pred);
}

// ---- stage 2: dequantise + inverse DCT ----------------------------------------------------------------------------------------
// 8 lanes per 8x8 block, 32 blocks per workgroup, grid (block group, item).  A lane loads one row of coefficients (16 bytes),
// dequantises it into LDS, transforms one column, then one row, and stores its 8 samples as one 8-byte store.
constexpr int IDCT_BLOCKS = 32;
constexpr int IDCT_STRIDE = 72;              // ints per block in LDS: 64 + 8, so that four blocks' columns fall on distinct banks

__global__ void __launch_bounds__(IDCT_BLOCKS * 8) jpeg_idct_kernel(const vlfb_jpeg_item* __restrict__ items,
                                                                     uint8_t* __restrict__ workspace) {
  __shared__ int32_t wsp[IDCT_BLOCKS * IDCT_STRIDE];
  __shared__ uint16_t quant[3][64];          // natural order
  const vlfb_jpeg_item& it = items[blockIdx.y];
  Geo g;
  geometry(it, &g);
  if ((int64_t)blockIdx.x * IDCT_BLOCKS >= g.first_block[3]) return;
  for (int i = threadIdx.x; i < 3 * 64; i += blockDim.x) quant[i / 64][natural_order(i % 64)] = it.quant[it.tq[i / 64] & 3][i % 64];
  __syncthreads();

  uint8_t* ws = workspace + it.ws_offset;
  const int grp = threadIdx.x >> 3, r = threadIdx.x & 7;
  const int64_t blk = (int64_t)blockIdx.x * IDCT_BLOCKS + grp;
  const bool live = blk < g.first_block[3];
  int c = 0;
  while (c < g.n_comp - 1 && blk >= g.first_block[c + 1]) ++c;
  const int64_t local = blk - g.first_block[c];
  int32_t* w = wsp + grp * IDCT_STRIDE;
  if (live) {
    const uint4 raw = reinterpret_cast<const uint4*>(ws + coef_offset(g, c) + local * 128)[r];
    const uint32_t word[4] = {raw.x, raw.y, raw.z, raw.w};
    for (int k = 0; k < 8; ++k) {
      const int16_t coef = (int16_t)((word[k >> 1] >> ((k & 1) * 16)) & 0xffffu);
      w[r * 8 + k] = (int32_t)coef * (int32_t)quant[c][r * 8 + k];
    }
  }
  __syncthreads();
  int32_t in[8], out[8];
  if (live) {
    for (int k = 0; k < 8; ++k) in[k] = w[k * 8 + r];        // column r
    idct_pass(in, out, IDCT_SHIFT_COLUMNS);
  }
  __syncthreads();
  if (live) for (int k = 0; k < 8; ++k) w[k * 8 + r] = out[k];
  __syncthreads();
  if (live) {
    for (int k = 0; k < 8; ++k) in[k] = w[r * 8 + k];        // row r
    idct_pass(in, out, IDCT_SHIFT_ROWS);
    uint32_t lo = 0, hi = 0;
    for (int k = 0; k < 4; ++k) {
      lo |= (uint32_t)idct_sample(out[k]) << (8 * k);
      hi |= (uint32_t)idct_sample(out[4 + k]) << (8 * k);
    }
    const int by = (int)(local / g.bw[c]), bx = (int)(local % g.bw[c]);
    uint8_t* plane = ws + plane_offset(g, c);
    *reinterpret_cast<uint2*>(plane + ((int64_t)by * 8 + r) * (g.bw[c] * 8) + bx * 8) = make_uint2(lo, hi);
  }
}

// ---- stage 3: upsample, convert, store --------------------------------------------------------------------------------------
// One lane per 4 pixels of a row, grid (pixel group, item); three 4-byte stores where the destination allows, bytes where not.
constexpr int PIX_THREADS = 256;

__global__ void __launch_bounds__(PIX_THREADS) jpeg_color_kernel(const vlfb_jpeg_item* __restrict__ items,
                                                                  const uint8_t* __restrict__ workspace) {
  const vlfb_jpeg_item& it = items[blockIdx.y];
  Geo g;
  if (!geometry(it, &g)) return;
  const int W = it.width, H = it.height;
  const int quads = (W + 3) / 4;
  const int64_t q = (int64_t)blockIdx.x * PIX_THREADS + threadIdx.x;
  if (q >= (int64_t)quads * H) return;
  const int y = (int)(q / quads), x0 = (int)(q % quads) * 4;
  const uint8_t* ws = workspace + it.ws_offset;
  const uint8_t* planes[3] = {ws + plane_offset(g, 0), ws + plane_offset(g, 1), ws + plane_offset(g, 2)};
  uint8_t* dst = (uint8_t*)it.dst + ((int64_t)y * W + x0) * 3;
  uint8_t px[12];
  const int n = W - x0 < 4 ? W - x0 : 4;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < n) pixel_bgr(g, planes, y, x0 + k, px + 3 * k);
  if (n == 4 && ((uintptr_t)dst & 3u) == 0) {
    uint32_t w3[3];
    for (int k = 0; k < 3; ++k)
      w3[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    d[0] = w3[0]; d[1] = w3[1]; d[2] = w3[2];
  } else {
    for (int k = 0; k < 3 * n; ++k) dst[k] = px[k];
  }
}

// ---- the host array ---------------------------------------------------------------------------------------------------------
// one item against the conditions of include/vlfb.h; need_src / need_dst: scan and seg_offsets / dst must not be NULL
int check_item(const char* what, int i, const vlfb_jpeg_item& it, bool need_src, bool need_dst, Geo* g) {
  VLFB_REQUIRE(it.width >= 1 && it.height >= 1 && it.width <= 65535 && it.height <= 65535, "%s: item %d has size %d x %d", what, i,
               it.width, it.height);
  VLFB_REQUIRE(it.n_comp == 1 || it.n_comp == 3, "%s: item %d has %d components (1 or 3 are supported)", what, i, it.n_comp);
  VLFB_REQUIRE(sampling_ok(it), "%s: item %d has unsupported sampling %dx%d %dx%d %dx%d", what, i, it.h[0], it.v[0], it.h[1], it.v[1],
               it.h[2], it.v[2]);
  for (int c = 0; c < it.n_comp; ++c)
    VLFB_REQUIRE(it.tq[c] < 4 && it.td[c] < 2 && it.ta[c] < 2, "%s: item %d component %d selects tables %d / %d / %d", what, i, c,
                 it.tq[c], it.td[c], it.ta[c]);
  VLFB_REQUIRE(((it.scan && it.seg_offsets) || !need_src) && (it.dst || !need_dst), "%s: item %d has a NULL address", what, i);
  VLFB_REQUIRE(it.scan_bytes < (1u << 30), "%s: item %d has a scan of %u bytes", what, i, it.scan_bytes);
  VLFB_REQUIRE(it.n_segments >= 1, "%s: item %d has no segment", what, i);
  VLFB_REQUIRE(it.restart_interval >= 0 && it.restart_interval <= 65535, "%s: item %d has restart interval %d", what, i,
               it.restart_interval);
  for (int t = 0; t < 4; ++t)
    VLFB_REQUIRE(huff_counts_ok(it.huff[t]), "%s: item %d Huffman table %d is not a prefix code", what, i, t);
  geometry(it, g);
  return VLFB_OK;
}

int check_batch(const char* what, const vlfb_jpeg_item* items_host, int n_items, bool need_dst, int64_t* bytes, int64_t* max_segments,
                int64_t* max_blocks, int64_t* max_quads) {
  VLFB_REQUIRE(items_host, "%s: NULL item array", what);
  VLFB_REQUIRE(n_items >= 1 && n_items <= 65535, "%s: n_items %d is not in 1..65535", what, n_items);
  *bytes = 0; *max_segments = 0; *max_blocks = 0; *max_quads = 0;
  for (int i = 0; i < n_items; ++i) {
    Geo g;
    const int rc = check_item(what, i, items_host[i], need_dst, need_dst, &g);
    if (rc != VLFB_OK) return rc;
    VLFB_REQUIRE(!need_dst || items_host[i].ws_offset == (uint64_t)*bytes, "%s: item %d has ws_offset %llu, the items before it take %lld",
                 what, i, (unsigned long long)items_host[i].ws_offset, (long long)*bytes);
    *bytes += item_workspace_bytes(g);
    const int64_t seg = expected_segments(g, items_host[i].restart_interval);
    const int64_t quads = (int64_t)((items_host[i].width + 3) / 4) * items_host[i].height;
    if (seg > *max_segments) *max_segments = seg;
    if (g.first_block[3] > *max_blocks) *max_blocks = g.first_block[3];
    if (quads > *max_quads) *max_quads = quads;
  }
  return VLFB_OK;
}

// stages 2 and 3 of the host checker: the coefficients of `ws` into the sample planes behind them, the planes into dst
void host_finish(const vlfb_jpeg_item& it, const Geo& g, uint8_t* wsp, uint8_t* dst) {
  for (int c = 0; c < g.n_comp; ++c) {
    int32_t q[64];
    for (int k = 0; k < 64; ++k) q[natural_order(k)] = it.quant[it.tq[c] & 3][k];
    uint8_t* plane = wsp + plane_offset(g, c);
    for (int64_t b = 0; b < (int64_t)g.bw[c] * g.bh[c]; ++b) {
      const int16_t* coef = reinterpret_cast<const int16_t*>(wsp + coef_offset(g, c) + b * 128);
      int32_t w[64], in[8], out[8];
      for (int col = 0; col < 8; ++col) {
        for (int k = 0; k < 8; ++k) in[k] = (int32_t)coef[k * 8 + col] * q[k * 8 + col];
        idct_pass(in, out, IDCT_SHIFT_COLUMNS);
        for (int k = 0; k < 8; ++k) w[k * 8 + col] = out[k];
      }
      const int by = (int)(b / g.bw[c]), bx = (int)(b % g.bw[c]);
      for (int r = 0; r < 8; ++r) {
        idct_pass(w + r * 8, out, IDCT_SHIFT_ROWS);
        for (int k = 0; k < 8; ++k) plane[((int64_t)by * 8 + r) * (g.bw[c] * 8) + bx * 8 + k] = idct_sample(out[k]);
      }
    }
  }
  const uint8_t* planes[3] = {wsp + plane_offset(g, 0), wsp + plane_offset(g, 1), wsp + plane_offset(g, 2)};
  for (int y = 0; y < it.height; ++y)
    for (int x = 0; x < it.width; ++x) pixel_bgr(g, planes, y, x, dst + ((int64_t)y * it.width + x) * 3);
}

}  // namespace
}  // namespace vlfb

using namespace vlfb;

extern "C" int64_t vlfb_jpeg_workspace_bytes(const vlfb_jpeg_item* items_host, int n_items) {
  int64_t bytes, seg, blocks, quads;
  const int rc = check_batch("jpeg_workspace_bytes", items_host, n_items, false, &bytes, &seg, &blocks, &quads);
  return rc != VLFB_OK ? (int64_t)rc : bytes;
}

extern "C" int vlfb_jpeg_decode_batch(const vlfb_jpeg_item* items_host, const vlfb_jpeg_item* items_dev, int n_items, void* workspace,
                                      int64_t workspace_bytes, int32_t* status_dev, vlfb_stream_t stream) {
  const char* what = "jpeg_decode_batch";
  int64_t bytes, seg, blocks, quads;
  const int rc = check_batch(what, items_host, n_items, true, &bytes, &seg, &blocks, &quads);
  if (rc != VLFB_OK) return rc;
  VLFB_REQUIRE(items_dev && workspace && status_dev, "%s: NULL buffer", what);
  VLFB_REQUIRE(((uintptr_t)workspace & 15u) == 0, "%s: the workspace is not 16-byte aligned", what);
  VLFB_REQUIRE(workspace_bytes >= bytes, "%s: the workspace has %lld bytes, the batch needs %lld", what, (long long)workspace_bytes,
               (long long)bytes);
  const int64_t idct_groups = (blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS, pix_groups = (quads + PIX_THREADS - 1) / PIX_THREADS;
  VLFB_REQUIRE(seg <= 0x7fffffffll && idct_groups <= 0x7fffffffll && pix_groups <= 0x7fffffffll, "%s: a frame too large for one grid", what);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(status_dev, 0, sizeof(int32_t) * (size_t)n_items, s) != hipSuccess) return check_launch(what);
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)seg, n_items), dim3(64), 0, s, items_dev, (uint8_t*)workspace, status_dev, 0);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)idct_groups, n_items), dim3(IDCT_BLOCKS * 8), 0, s, items_dev, (uint8_t*)workspace);
  hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)pix_groups, n_items), dim3(PIX_THREADS), 0, s, items_dev,
                     (const uint8_t*)workspace);
  return check_launch(what);
}

// The checker: csrc/vlfb_jpeg_core.h compiled for the host, one item, host addresses.
extern "C" int vlfb_jpeg_decode_host(const vlfb_jpeg_item* item, uint8_t* dst, int32_t* status) {
  const char* what = "jpeg_decode_host";
  VLFB_REQUIRE(item && dst && status, "%s: NULL buffer", what);
  Geo g;
  const int rc = check_item(what, 0, *item, true, false, &g);
  if (rc != VLFB_OK) return rc;
  const vlfb_jpeg_item& it = *item;
  std::vector<uint8_t> ws((size_t)item_workspace_bytes(g), 0);
  std::vector<jpeg::Huff> tabs(4);
  int st = 0;
  for (int t = 0; t < 4; ++t)
    if (!huff_build(it.huff[t], &tabs[t])) st |= VLFB_JPEG_BAD_CODE;
  const uint8_t* scan = (const uint8_t*)it.scan;
  const int64_t want = expected_segments(g, it.restart_interval), mcus = total_mcus(g);
  const int32_t ri = it.restart_interval;
  for (int64_t s = 0; s < want && !st; ++s) {
    const int64_t mcu0 = ri ? s * ri : 0, mcu1 = ri ? (mcu0 + ri < mcus ? mcu0 + ri : mcus) : mcus;
    int32_t lo, hi;
    int err = segment_range(scan, it.scan_bytes, (const uint32_t*)it.seg_offsets, it.n_segments, want, s, &lo, &hi);
    Bits br;
    bits_init(&br, scan, 0, lo, hi, 0);
    int pred[3] = {0, 0, 0};
    for (int64_t m = mcu0; m < mcu1 && !err; ++m) {
      int16_t buf[MAX_MCU_BLOCKS * 64] = {0};
      err = decode_mcu(&br, g, tabs.data(), it.td, it.ta, pred, buf);
      if (err) break;
      for (int b = 0; b < g.mcu_blocks; ++b) {
        int comp;
        int64_t block;
        mcu_block_place(g, m, b, &comp, &block);
        int16_t* out = reinterpret_cast<int16_t*>(ws.data() + coef_offset(g, comp) + block * 128);
        for (int k = 0; k < 64; ++k) out[k] = buf[b * 64 + k];
      }
    }
    if (err) { st |= err; break; }
  }
  host_finish(it, g, ws.data(), dst);
  *status = st;
  return VLFB_OK;
}

// ---- the lane-parallel path ---------------------------------------------------------------------------------------------------
namespace vlfb {
namespace {

int par_subseq_arg(const char* what, int subseq_bytes, int* subseq) {
  VLFB_REQUIRE(subseq_bytes == 0 || par_subseq_ok(subseq_bytes), "%s: subseq_bytes %d is not 0 or a multiple of 4 in 8..4096", what,
               subseq_bytes);
  *subseq = subseq_bytes ? subseq_bytes : PAR_SUBSEQ_DEFAULT;
  return VLFB_OK;
}

// Stage 1 of jpeg_entropy_par_kernel for one item with `lanes` lanes run one after another: the coefficients into ws (zeroed
// by the caller), stats[1..3].  false: the item is to be decoded serially.
bool host_par_entropy(const vlfb_jpeg_item& it, const Geo& g, int lanes, int subseq, uint8_t* ws, int32_t* stats) {
  std::vector<jpeg::Huff> tabs(4);
  bool tab_ok = true;
  for (int t = 0; t < 4; ++t) tab_ok = huff_build(it.huff[t], &tabs[t]) && tab_ok;
  if (!tab_ok) return false;
  const uint8_t* scan = (const uint8_t*)it.scan;
  const uint32_t n = it.scan_bytes;
  uint32_t end = n;
  for (uint32_t i = 0; i < n; ++i)
    if (par_is_marker(scan, n, i)) { end = i; break; }
  std::vector<uint32_t> words(par_stream_words(n), 0u);
  uint8_t* bytes = reinterpret_cast<uint8_t*>(words.data());
  uint32_t stream_bytes = 0;
  for (uint32_t i = 0; i < end; ++i)
    if (!par_is_stuffing(scan, i)) bytes[par_byte_slot(stream_bytes++)] = scan[i];

  ParCtx cx;
  cx.words = words.data();
  cx.data_bits = stream_bytes * 8u;
  cx.tabs = tabs.data();
  cx.sel = par_table_select(g, it.td, it.ta);
  cx.mcu_blocks = g.mcu_blocks;
  const int64_t total = total_mcus(g);
  const uint32_t chunk_bytes = (uint32_t)lanes * (uint32_t)subseq;
  const int32_t max_syms = 8 * subseq;
  const int32_t chunks = (int32_t)((n + chunk_bytes - 1) / chunk_bytes);
  std::vector<ParState> in(lanes), out(lanes), next(lanes);
  std::vector<int32_t> mcus(lanes);
  std::vector<uint32_t> end_bit(lanes);
  ParState carry = {0u, 0u};
  int64_t carry_mcu = 0;
  bool redo = false;
  stats[1] = chunks;
  for (int32_t c = 0; c < chunks; ++c) {
    const int32_t live = par_live_lanes(cx.data_bits, (uint32_t)c * chunk_bytes * 8u, lanes, subseq);
    for (int l = 0; l < live; ++l) {
      const uint32_t start_bit = ((uint32_t)c * chunk_bytes + (uint32_t)l * (uint32_t)subseq) * 8u;
      end_bit[l] = start_bit + 8u * subseq < cx.data_bits ? start_bit + 8u * subseq : cx.data_bits;
      in[l] = l == 0 ? carry : ParState{start_bit, 0u};
      par_walk(cx, in[l], end_bit[l], max_syms, &out[l], &mcus[l]);
    }
    int32_t rounds = 1;
    for (int r = 1; r < live; ++r) {
      for (int l = 0; l < live; ++l) next[l] = l == 0 ? carry : out[l - 1];   // every lane reads before any lane writes
      bool moved = false;
      for (int l = 0; l < live; ++l) {
        if (par_same(next[l], in[l])) continue;
        ParState o;
        par_walk(cx, next[l], end_bit[l], max_syms, &o, &mcus[l]);
        in[l] = next[l];
        moved = moved || !par_same(o, out[l]);
        out[l] = o;
      }
      ++rounds;
      if (!moved) break;
    }
    int64_t before = carry_mcu;
    for (int l = 0; l < live; ++l) {
      if (!par_write(cx, g, in[l], end_bit[l], max_syms, before, total, ws)) redo = true;
      before += mcus[l];
    }
    if (live > 0) carry = out[live - 1];
    carry_mcu = before;
    stats[2] += rounds;
    stats[3] = rounds > stats[3] ? rounds : stats[3];
  }
  if (carry_mcu < total || redo) return false;
  uint32_t pred[3] = {0u, 0u, 0u};
  par_dc_apply(g, ws, 0, total, pred);
  return true;
}

}  // namespace
}  // namespace vlfb

extern "C" int vlfb_jpeg_decode_batch_par(const vlfb_jpeg_item* items_host, const vlfb_jpeg_item* items_dev, int n_items, void* workspace,
                                          int64_t workspace_bytes, int32_t* status_dev, int subseq_bytes, int32_t* stats_dev,
                                          vlfb_stream_t stream) {
  const char* what = "jpeg_decode_batch_par";
  int64_t bytes, seg, blocks, quads;
  int rc = check_batch(what, items_host, n_items, true, &bytes, &seg, &blocks, &quads);
  if (rc != VLFB_OK) return rc;
  VLFB_REQUIRE(items_dev && workspace && status_dev, "%s: NULL buffer", what);
  VLFB_REQUIRE(((uintptr_t)workspace & 15u) == 0, "%s: the workspace is not 16-byte aligned", what);
  VLFB_REQUIRE(workspace_bytes >= bytes, "%s: the workspace has %lld bytes, the batch needs %lld", what, (long long)workspace_bytes,
               (long long)bytes);
  const int64_t idct_groups = (blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS, pix_groups = (quads + PIX_THREADS - 1) / PIX_THREADS;
  VLFB_REQUIRE(seg <= 0x7fffffffll && idct_groups <= 0x7fffffffll && pix_groups <= 0x7fffffffll, "%s: a frame too large for one grid", what);
  int subseq;
  rc = par_subseq_arg(what, subseq_bytes, &subseq);
  if (rc != VLFB_OK) return rc;
  uint32_t largest = 0;                              // the longest scan the parallel kernel takes: its LDS
  for (int i = 0; i < n_items; ++i)
    if (vlfb_jpeg_item_is_parallel(items_host[i], subseq) && items_host[i].scan_bytes > largest) largest = items_host[i].scan_bytes;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(status_dev, 0, sizeof(int32_t) * (size_t)n_items, s) != hipSuccess) return check_launch(what);
  // the limit covers the stream alone: the kernel's tables and lane states are static LDS beside it, 160 KiB in all
  static_assert(sizeof(uint32_t) * ((PAR_MAX_SCAN + 3) / 4 + 2) <= 144 * 1024, "the longest parallel scan fits the dynamic LDS limit");
  rc = launch_lds<jpeg_entropy_par_kernel, 144 * 1024>(dim3(n_items), dim3(PAR_LANES), sizeof(uint32_t) * par_stream_words(largest), s, what,
                                                        items_dev, (uint8_t*)workspace, status_dev, stats_dev, subseq,
                                                        par_stream_words(largest));
  if (rc != VLFB_OK) return rc;
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)seg, n_items), dim3(64), 0, s, items_dev, (uint8_t*)workspace, status_dev, subseq);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)idct_groups, n_items), dim3(IDCT_BLOCKS * 8), 0, s, items_dev, (uint8_t*)workspace);
  hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)pix_groups, n_items), dim3(PIX_THREADS), 0, s, items_dev,
                     (const uint8_t*)workspace);
  return check_launch(what);
}

extern "C" int vlfb_jpeg_decode_host_par(const vlfb_jpeg_item* item, uint8_t* dst, int32_t* status, int lanes, int subseq_bytes,
                                         int32_t* stats) {
  const char* what = "jpeg_decode_host_par";
  VLFB_REQUIRE(item && dst && status, "%s: NULL buffer", what);
  Geo g;
  int rc = check_item(what, 0, *item, true, false, &g);
  if (rc != VLFB_OK) return rc;
  VLFB_REQUIRE(lanes >= 1 && lanes <= 1024, "%s: lanes %d is not in 1..1024", what, lanes);
  int subseq;
  rc = par_subseq_arg(what, subseq_bytes, &subseq);
  if (rc != VLFB_OK) return rc;
  int32_t st[4] = {0, 0, 0, 0};
  if (vlfb_jpeg_item_is_parallel(*item, subseq)) {
    std::vector<uint8_t> ws((size_t)item_workspace_bytes(g), 0);
    st[0] = host_par_entropy(*item, g, lanes, subseq, ws.data(), st) ? 1 : 2;
    if (st[0] == 1) {
      host_finish(*item, g, ws.data(), dst);
      *status = 0;
    }
  }
  if (st[0] != 1) {                                  // by rule, or redone from scratch: the serial checker's pixels and status
    rc = vlfb_jpeg_decode_host(item, dst, status);
    if (rc != VLFB_OK) return rc;
  }
  if (stats)
    for (int k = 0; k < 4; ++k) stats[k] = st[k];
  return VLFB_OK;
}
