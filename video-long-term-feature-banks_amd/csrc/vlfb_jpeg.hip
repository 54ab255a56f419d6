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
constexpr int WIN_BYTES = 8192;
static_assert(WIN_BYTES >= 2 * MAX_MCU_BYTES + 64, "a window holds a worst-case MCU beside what the reader has buffered");

__global__ void __launch_bounds__(64) jpeg_entropy_kernel(const vlfb_jpeg_item* __restrict__ items, uint8_t* __restrict__ workspace,
                                                          int32_t* __restrict__ status) {
  __shared__ Huff tabs[4];
  __shared__ __attribute__((aligned(16))) uint8_t win[WIN_BYTES];
  __shared__ __attribute__((aligned(16))) int16_t mcu_buf[MAX_MCU_BLOCKS * 64];
  __shared__ int32_t sh_pos, sh_err, sh_tab_bad;

  const vlfb_jpeg_item& it = items[blockIdx.y];
  const int lane = threadIdx.x;
  Geo g;
  const bool geo_ok = geometry(it, &g);
  const int32_t ri = it.restart_interval > 0 ? it.restart_interval : 0;
  const int64_t want = expected_segments(g, ri);
  const int64_t s = blockIdx.x;
  if (s >= want) return;
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
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)seg, n_items), dim3(64), 0, s, items_dev, (uint8_t*)workspace, status_dev);
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
  for (int c = 0; c < g.n_comp; ++c) {
    int32_t q[64];
    for (int k = 0; k < 64; ++k) q[natural_order(k)] = it.quant[it.tq[c] & 3][k];
    uint8_t* plane = ws.data() + plane_offset(g, c);
    for (int64_t b = 0; b < (int64_t)g.bw[c] * g.bh[c]; ++b) {
      const int16_t* coef = reinterpret_cast<const int16_t*>(ws.data() + coef_offset(g, c) + b * 128);
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
  const uint8_t* planes[3] = {ws.data() + plane_offset(g, 0), ws.data() + plane_offset(g, 1), ws.data() + plane_offset(g, 2)};
  for (int y = 0; y < it.height; ++y)
    for (int x = 0; x < it.width; ++x) pixel_bgr(g, planes, y, x, dst + ((int64_t)y * it.width + x) * 3);
  *status = st;
  return VLFB_OK;
}
