// Clip preprocessing on the device: decoded uint8 BGR frames ->
// short-side scale (bilinear) -> crop -> horizontal flip -> /255 -> (x - mean) / std -> RGB, written
// straight into the model's `data` input in its device layout [T][crop][wl + crop + wr][c_pad].
// Replaces the per-frame cv2 / NumPy chain of lib/datasets/data_input_helper.py:70-139
// (images_and_boxes_preprocessing) and lib/datasets/image_processor.py:80-251.
//
// The resize is OpenCV's 8-bit INTER_LINEAR fixed-point algorithm (cfg.INTERPOLATION, config.py:238):
// the host computes the per-column / per-row source indices and 11-bit coefficients exactly as
// cv::resize does and the kernel does integer arithmetic only, so the result does not depend on
// floating-point contraction or rounding modes.  Built with -ffp-contract=off for the fp32
// normalisation tail (same operation order as the NumPy code: x / 255, - mean, / std).
//
// TRAIN.USE_COLOR_AUGMENTATION adds two kernels beside it: an integer per-frame channel-sum pass (the contrast
// jitter blends with the frame's grey mean) and the same walk with the colour chain before the normalisation.
//
// vlfb_clip_batch_* do the work of the three per-clip entry points for the clips of one minibatch in one launch each
// (lib/datasets/clip_loader.py): the same device functions, one record per clip read from device memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vlfb.h"
#include "vlfb_common.h"

namespace vlfb {
namespace {

struct ClipP {
  const uint8_t* src;     // [T][Hs][Ws][3]
  const int32_t* xofs;    // [Wr] left source column      (resized image column -> source)
  const int16_t* xcoef;   // [Wr][2] 11-bit weights of columns xofs, xofs + 1
  const int32_t* yofs;    // [Hr]
  const int16_t* ycoef;   // [Hr][2]
  int T, Hs, Ws, Hr, Wr;
  int resize;             // 0: Hr == Hs and Wr == Ws, frames are used as they are
  int crop_h, crop_w, y0, x0, flip;
  float mean[3], stdv[3]; // in the SOURCE channel order (BGR)
  int to_rgb;
  int wl, wtot, c_pad;    // destination row: wl zero pixels, crop_w pixels, rest zero; c_pad channels
};

__device__ __forceinline__ int resized_u8(const ClipP& p, const uint8_t* frame, int y, int x, int c) {
  if (!p.resize) return frame[((long long)y * p.Ws + x) * 3 + c];
  const int sx = p.xofs[x], sy = p.yofs[y];
  const int a0 = p.xcoef[2 * x], a1 = p.xcoef[2 * x + 1];
  const int b0 = p.ycoef[2 * y], b1 = p.ycoef[2 * y + 1];
  const int sx1 = min(sx + 1, p.Ws - 1), sy1 = min(sy + 1, p.Hs - 1);
  const uint8_t* r0 = frame + (long long)sy * p.Ws * 3;
  const uint8_t* r1 = frame + (long long)sy1 * p.Ws * 3;
  // horizontal pass (HResizeLinear: int = u8 * coef + u8 * coef), vertical pass with the staged
  // shifts of VResizeLinear<uchar>: ((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2
  const int h0 = r0[sx * 3 + c] * a0 + r0[sx1 * 3 + c] * a1;
  const int h1 = r1[sx * 3 + c] * a0 + r1[sx1 * 3 + c] * a1;
  const int v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

template <typename T>
__global__ void clip_preprocess_kernel(ClipP p, T* __restrict__ dst) {
  const long long total = (long long)p.T * p.crop_h * p.crop_w;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % p.crop_w);
    const long long ty = i / p.crop_w;
    const int y = (int)(ty % p.crop_h);
    const int t = (int)(ty / p.crop_h);
    const int xs = p.flip ? p.x0 - x : p.x0 + x;   // x0 = resized-frame column of output column 0; a flip walks left
    const int ys = p.y0 + y;
    const uint8_t* frame = p.src + (long long)t * p.Hs * p.Ws * 3;
    T* d = dst + ((long long)(t * p.crop_h + y) * p.wtot + p.wl + x) * p.c_pad;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float u = (float)resized_u8(p, frame, ys, xs, c);
      float v = u / 255.0f;
      v = v - p.mean[c];
      v = v / p.stdv[c];
      Elem<T>::st(d + (p.to_rgb ? 2 - c : c), v);
    }
  }
}

// ---- colour augmentation (TRAIN.USE_COLOR_AUGMENTATION): data_input_helper.py:120-151 color_augmentation_list,
// image_processor.py:252-336 lighting_list / blend / grayscale / saturation_list / brightness_list / contrast_list ----

struct ColorP {
  int n_ops, op[3];
  float alpha[3], light[3];
  const int64_t* sums;    // [T][VLFB_CLIP_SUM_BANDS][3] of clip_channel_sums_kernel, NULL without a contrast op
};

// One block per (band, frame): the integer B, G, R sums of the uint8 pixels clip_preprocess_kernel reads in crop rows
// [band * crop_h / 8, (band + 1) * crop_h / 8).  Integers, so the result does not depend on the block size or on the
// order of the reduction.  A thread takes every 256th pixel of the band: the wrapper bounds crop_h * crop_w so that
// its 32-bit counters cannot wrap; from the wave reduction on the sums are 64-bit.
constexpr int SUM_THREADS = 256;

// (`f` is the frame of p.src that destination frame t reads: t itself but for the _indexed entry points)
__device__ __forceinline__ void band_sums(const ClipP& p, int band, int t, int f, int64_t* __restrict__ sums) {
  const int r0 = (int)((long long)band * p.crop_h / VLFB_CLIP_SUM_BANDS);
  const int r1 = (int)((long long)(band + 1) * p.crop_h / VLFB_CLIP_SUM_BANDS);
  const long long n = (long long)(r1 - r0) * p.crop_w;
  const uint8_t* frame = p.src + (long long)f * p.Hs * p.Ws * 3;
  uint32_t acc[3] = {0u, 0u, 0u};
  for (long long i = threadIdx.x; i < n; i += SUM_THREADS) {
    const int x = (int)(i % p.crop_w);
    const int y = r0 + (int)(i / p.crop_w);
    const int xs = p.flip ? p.x0 - x : p.x0 + x;
    const int ys = p.y0 + y;
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += (uint32_t)resized_u8(p, frame, ys, xs, c);
  }
  __shared__ unsigned long long part[SUM_THREADS / 64][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    unsigned long long v = acc[c];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) part[wave][c] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t* out = sums + ((long long)t * VLFB_CLIP_SUM_BANDS + band) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      unsigned long long v = 0;
      for (int w = 0; w < SUM_THREADS / 64; ++w) v += part[w][c];
      out[c] = (int64_t)v;
    }
  }
}

__global__ void __launch_bounds__(SUM_THREADS) clip_channel_sums_kernel(ClipP p, int64_t* __restrict__ sums) {
  band_sums(p, blockIdx.x, blockIdx.y, blockIdx.y, sums);
}

// grey mean of frame t as the contrast op meets it: the exact mean of the un-augmented window, times the alphas of the
// brightness ops before it (a saturation blend keeps a pixel's grey value: the three weights add to one)
__device__ __forceinline__ float contrast_grey_mean(const ClipP& p, const ColorP& q, int t) {
  float grey_mean = 0.0f;
  if (q.sums) {
    int64_t s[3] = {0, 0, 0};
    for (int b = 0; b < VLFB_CLIP_SUM_BANDS; ++b)
      for (int c = 0; c < 3; ++c) s[c] += q.sums[((long long)t * VLFB_CLIP_SUM_BANDS + b) * 3 + c];
    const double num = 0.299 * (double)s[2] + 0.587 * (double)s[1] + 0.114 * (double)s[0];
    grey_mean = (float)(num / (255.0 * (double)((long long)p.crop_h * p.crop_w)));
    for (int k = 0; k < q.n_ops && q.op[k] != VLFB_COLOR_CONTRAST; ++k)
      if (q.op[k] == VLFB_COLOR_BRIGHTNESS) grey_mean = grey_mean * q.alpha[k];
  }
  return grey_mean;
}

// One pixel from the uint8 values of the resized frame to the normalised values in the SOURCE channel order: / 255, the
// jitter ops, the lighting offset, (v - mean) / std.  fp32 throughout, one rounding per operation (-ffp-contract=off), in
// the order the NumPy code applies them.
__device__ __forceinline__ void color_pixel(const ClipP& p, const ColorP& q, float grey_mean, const uint8_t* frame, int ys,
                                            int xs, float (&w)[3]) {
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = (float)resized_u8(p, frame, ys, xs, c) / 255.0f;
  for (int k = 0; k < q.n_ops; ++k) {
    const float a = q.alpha[k];
    if (q.op[k] == VLFB_COLOR_BRIGHTNESS) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = v[c] * a;
    } else {
      float other = grey_mean;
      if (q.op[k] == VLFB_COLOR_SATURATION) other = 0.299f * v[2] + 0.587f * v[1] + 0.114f * v[0];
      const float rest = other * (1.0f - a);
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = v[c] * a + rest;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    w[c] = v[c] + q.light[c];
    w[c] = w[c] - p.mean[c];
    w[c] = w[c] / p.stdv[c];
  }
}

// The walk of clip_preprocess_kernel with the frame on grid axis y and the colour chain between / 255 and the
// normalisation.
template <typename T>
__global__ void clip_preprocess_color_kernel(ClipP p, ColorP q, T* __restrict__ dst) {
  const int t = blockIdx.y;
  const float grey_mean = contrast_grey_mean(p, q, t);
  const uint8_t* frame = p.src + (long long)t * p.Hs * p.Ws * 3;
  const long long total = (long long)p.crop_h * p.crop_w;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % p.crop_w);
    const int y = (int)(i / p.crop_w);
    const int xs = p.flip ? p.x0 - x : p.x0 + x;
    const int ys = p.y0 + y;
    T* d = dst + ((long long)(t * p.crop_h + y) * p.wtot + p.wl + x) * p.c_pad;
    float w[3];
    color_pixel(p, q, grey_mean, frame, ys, xs, w);
#pragma unroll
    for (int c = 0; c < 3; ++c) Elem<T>::st(d + (p.to_rgb ? 2 - c : c), w[c]);
  }
}

// kernel parameters of a descriptor: on the host for the per-clip launches, on the device from a vlfb_clip_item
__host__ __device__ inline void fill_clip(ClipP* p, const vlfb_clip_desc& d, const uint8_t* frames, const int32_t* xofs,
                                          const int16_t* xcoef, const int32_t* yofs, const int16_t* ycoef) {
  p->src = frames; p->xofs = xofs; p->xcoef = xcoef; p->yofs = yofs; p->ycoef = ycoef;
  p->T = d.frames; p->Hs = d.src_h; p->Ws = d.src_w; p->Hr = d.resized_h; p->Wr = d.resized_w;
  p->resize = (d.resized_h != d.src_h || d.resized_w != d.src_w) ? 1 : 0;
  p->crop_h = d.crop_h; p->crop_w = d.crop_w; p->y0 = d.y0; p->x0 = d.x0; p->flip = d.flip;
  for (int c = 0; c < 3; ++c) { p->mean[c] = d.mean[c]; p->stdv[c] = d.std[c]; }
  p->to_rgb = d.to_rgb; p->wl = d.w_left; p->wtot = d.w_total; p->c_pad = d.c_pad;
}

__host__ __device__ inline void fill_color(ColorP* q, const vlfb_clip_color& c, const int64_t* sums) {
  bool contrast = false;
  q->n_ops = c.n_ops;
  for (int k = 0; k < 3; ++k) {
    q->op[k] = -1; q->alpha[k] = 1.0f; q->light[k] = c.light[k];
    if (k >= c.n_ops) continue;
    q->op[k] = c.op[k]; q->alpha[k] = c.alpha[k];
    contrast = contrast || c.op[k] == VLFB_COLOR_CONTRAST;
  }
  q->sums = contrast ? sums : nullptr;
}

// argument checks and kernel parameters shared by the colour and batch entry points (`with_dst`: the destination row too)
int clip_params(const char* what, const vlfb_clip_desc* d, const uint8_t* frames, const int32_t* xofs, const int16_t* xcoef,
                const int32_t* yofs, const int16_t* ycoef, bool with_dst, ClipP* p) {
  VLFB_REQUIRE(d && frames, "%s: NULL buffer", what);
  VLFB_REQUIRE(d->frames > 0 && d->src_h > 0 && d->src_w > 0 && d->crop_h > 0 && d->crop_w > 0, "%s: empty geometry", what);
  VLFB_REQUIRE(d->frames <= 65535, "%s: more than 65535 frames", what);
  const bool resize = d->resized_h != d->src_h || d->resized_w != d->src_w;
  VLFB_REQUIRE(!resize || (xofs && xcoef && yofs && ycoef), "%s: resize tables are required", what);
  VLFB_REQUIRE(d->y0 >= 0 && d->y0 + d->crop_h <= d->resized_h && d->x0 >= 0 && d->x0 < d->resized_w &&
                   (d->flip ? d->x0 - (d->crop_w - 1) >= 0 : d->x0 + d->crop_w <= d->resized_w),
               "%s: crop window leaves the resized frame", what);
  // one thread of the sums kernel adds at most ceil(crop_h * crop_w / 256) values of at most 255 into 32 bits
  VLFB_REQUIRE((long long)d->crop_h * d->crop_w <= (1ll << 31) - 1, "%s: crop window of more than 2^31 - 1 pixels", what);
  if (with_dst)
    VLFB_REQUIRE(d->c_pad >= 3 && d->w_left >= 0 && d->w_total >= d->w_left + d->crop_w, "%s: bad destination row", what);
  fill_clip(p, *d, frames, xofs, xcoef, yofs, ycoef);
  return VLFB_OK;
}

int color_params(const char* what, const vlfb_clip_color* c, const int64_t* sums, ColorP* q) {
  VLFB_REQUIRE(c->n_ops >= 0 && c->n_ops <= 3, "%s: n_ops %d is not in 0..3", what, c->n_ops);
  bool contrast = false;
  for (int k = 0; k < c->n_ops; ++k) {
    VLFB_REQUIRE(c->op[k] >= 0 && c->op[k] <= 2, "%s: op code %d is not in 0..2", what, c->op[k]);
    for (int j = 0; j < k; ++j)
      VLFB_REQUIRE(c->op[j] != c->op[k], "%s: op code %d appears twice", what, c->op[k]);
    contrast = contrast || c->op[k] == VLFB_COLOR_CONTRAST;
  }
  VLFB_REQUIRE(!contrast || sums, "%s: a contrast op needs the channel sums", what);
  fill_color(q, *c, sums);
  return VLFB_OK;
}

// ---- the clips of one minibatch in one launch (vlfb_clip_item, include/vlfb.h) ----
// The record of a workgroup's clip comes from device memory at an address that depends on blockIdx.z only: const and
// __restrict__, so the loads are scalar loads and the geometry lives in SGPRs, as the by-value ClipP of the per-clip kernels.
static_assert(sizeof(vlfb_clip_item) == VLFB_CLIP_ITEM_BYTES, "vlfb_clip_item layout (include/vlfb.h, vlfb/hip.py ClipItem)");
constexpr int TILE_W = 32, TILE_H = 8;     // 224 = 7 * 32: no idle lanes at the shipped crop; a wave stores 2 rows of 32 pixels

__device__ __forceinline__ void item_params(const vlfb_clip_item& it, ClipP* p, ColorP* q) {
  fill_clip(p, it.geo, (const uint8_t*)it.frames, (const int32_t*)it.xofs, (const int16_t*)it.xcoef, (const int32_t*)it.yofs,
            (const int16_t*)it.ycoef);
  fill_color(q, it.color, (const int64_t*)it.sums);
}

// The _indexed entry points read source frame index[item * index_stride + t] of the frame store `frames` points at.  The
// entry depends on blockIdx only (a uniform load, as the item record); `index` is NULL for the contiguous entry points,
// a constant after inlining, so their kernels are the ones they were.
__device__ __forceinline__ int source_frame(const int32_t* __restrict__ index, int index_stride, int t) {
  return index ? index[(long long)blockIdx.z * index_stride + t] : t;
}

__device__ __forceinline__ void batch_channel_sums(const vlfb_clip_item* __restrict__ items, const int32_t* __restrict__ index,
                                                   int index_stride) {
  const vlfb_clip_item& it = items[blockIdx.z];
  const int t = blockIdx.y;
  if (!it.sums || t >= it.geo.frames) return;
  ClipP p;
  ColorP q;
  item_params(it, &p, &q);
  band_sums(p, blockIdx.x, t, source_frame(index, index_stride, t), (int64_t*)it.sums);
}

__global__ void __launch_bounds__(SUM_THREADS) clip_batch_channel_sums_kernel(const vlfb_clip_item* __restrict__ items) {
  batch_channel_sums(items, nullptr, 0);
}

__global__ void __launch_bounds__(SUM_THREADS) clip_batch_channel_sums_indexed_kernel(
    const vlfb_clip_item* __restrict__ items, const int32_t* __restrict__ index, int index_stride) {
  batch_channel_sums(items, index, index_stride);
}

template <typename T>
__device__ __forceinline__ void batch_preprocess(const vlfb_clip_item* __restrict__ items, const int32_t* __restrict__ index,
                                                 int index_stride) {
  const vlfb_clip_item& it = items[blockIdx.z];
  const int t = blockIdx.y;
  const int tiles_x = (it.geo.crop_w + TILE_W - 1) / TILE_W;             // (uniform: one 32-bit division per workgroup)
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  if (t >= it.geo.frames || ty * TILE_H >= it.geo.crop_h) return;
  const int x = tx * TILE_W + (int)threadIdx.x, y = ty * TILE_H + (int)threadIdx.y;
  ClipP p;
  ColorP q;
  item_params(it, &p, &q);
  if (x >= p.crop_w || y >= p.crop_h) return;
  const float grey_mean = contrast_grey_mean(p, q, t);
  const int xs = p.flip ? p.x0 - x : p.x0 + x;
  const int ys = p.y0 + y;
  const uint8_t* frame = p.src + (long long)source_frame(index, index_stride, t) * p.Hs * p.Ws * 3;
  T* d = (T*)it.dst + ((long long)(t * p.crop_h + y) * p.wtot + p.wl + x) * p.c_pad;
  float w[3];
  color_pixel(p, q, grey_mean, frame, ys, xs, w);
  const float o0 = p.to_rgb ? w[2] : w[0], o2 = p.to_rgb ? w[0] : w[2];
  if (p.c_pad == 4 && it.dst % (4 * sizeof(T)) == 0) {                   // one store per pixel; the padding channel is zero
    if constexpr (sizeof(T) == 4)
      *reinterpret_cast<float4*>(d) = make_float4(o0, w[1], o2, 0.0f);
    else
      *reinterpret_cast<uint2*>(d) = make_uint2(Elem<T>::pack2(o0, w[1]), Elem<T>::pack2(o2, 0.0f));
  } else {
    Elem<T>::st(d, o0);
    Elem<T>::st(d + 1, w[1]);
    Elem<T>::st(d + 2, o2);
  }
}

template <typename T>
__global__ void __launch_bounds__(TILE_W * TILE_H) clip_batch_preprocess_kernel(const vlfb_clip_item* __restrict__ items) {
  batch_preprocess<T>(items, nullptr, 0);
}

template <typename T>
__global__ void __launch_bounds__(TILE_W * TILE_H) clip_batch_preprocess_indexed_kernel(
    const vlfb_clip_item* __restrict__ items, const int32_t* __restrict__ index, int index_stride) {
  batch_preprocess<T>(items, index, index_stride);
}

// every item of the host array against the conditions of the per-clip entry points; the grid extents over the items
int check_items(const char* what, const vlfb_clip_item* items_host, const vlfb_clip_item* items_dev, int n_items,
                int* max_frames, int* max_tiles, bool* any_sums) {
  VLFB_REQUIRE(items_host && items_dev, "%s: NULL item array", what);
  VLFB_REQUIRE(n_items >= 1 && n_items <= 65535, "%s: n_items %d is not in 1..65535", what, n_items);
  *max_frames = 0; *max_tiles = 0; *any_sums = false;
  for (int i = 0; i < n_items; ++i) {
    const vlfb_clip_item& it = items_host[i];
    ClipP p;
    ColorP q;
    int rc = clip_params(what, &it.geo, (const uint8_t*)it.frames, (const int32_t*)it.xofs, (const int16_t*)it.xcoef,
                         (const int32_t*)it.yofs, (const int16_t*)it.ycoef, true, &p);
    if (rc != VLFB_OK) return rc;
    VLFB_REQUIRE(it.dst, "%s: NULL buffer", what);
    rc = color_params(what, &it.color, (const int64_t*)it.sums, &q);
    if (rc != VLFB_OK) return rc;
    const long long tiles = (long long)((p.crop_w + TILE_W - 1) / TILE_W) * ((p.crop_h + TILE_H - 1) / TILE_H);
    VLFB_REQUIRE(tiles <= 0x7fffffffll, "%s: crop window of more than 2^31 - 1 tiles", what);
    if (p.T > *max_frames) *max_frames = p.T;
    if ((int)tiles > *max_tiles) *max_tiles = (int)tiles;
    *any_sums = *any_sums || it.sums != 0;
  }
  return VLFB_OK;
}

// the frame table of the _indexed entry points: item i reads index_host[i * index_stride + t], t < geo.frames, of a store of
// store_frames_host[i] frames
int check_index(const char* what, const vlfb_clip_item* items_host, int n_items, const int32_t* index_host,
                const int32_t* index_dev, int index_stride, const int32_t* store_frames_host) {
  VLFB_REQUIRE(index_host && index_dev && store_frames_host, "%s: NULL frame table", what);
  for (int i = 0; i < n_items; ++i) {
    const int frames = items_host[i].geo.frames;
    VLFB_REQUIRE(index_stride >= frames, "%s: item %d has %d frames, index_stride is %d", what, i, frames, index_stride);
    VLFB_REQUIRE(store_frames_host[i] >= 1, "%s: item %d reads a store of %d frames", what, i, store_frames_host[i]);
    for (int t = 0; t < frames; ++t) {
      const int f = index_host[(long long)i * index_stride + t];
      VLFB_REQUIRE(f >= 0 && f < store_frames_host[i], "%s: item %d entry %d is frame %d of a store of %d frames", what, i, t, f,
                   store_frames_host[i]);
    }
  }
  return VLFB_OK;
}

}  // namespace
}  // namespace vlfb

using namespace vlfb;

extern "C" int vlfb_clip_channel_sums(const vlfb_clip_desc* d, const uint8_t* frames, const int32_t* xofs,
                                      const int16_t* xcoef, const int32_t* yofs, const int16_t* ycoef,
                                      int64_t* sums, vlfb_stream_t stream) {
  ClipP p;
  const int rc = clip_params("clip_channel_sums", d, frames, xofs, xcoef, yofs, ycoef, false, &p);
  if (rc != VLFB_OK) return rc;
  VLFB_REQUIRE(sums, "clip_channel_sums: NULL sums");
  hipLaunchKernelGGL(clip_channel_sums_kernel, dim3(VLFB_CLIP_SUM_BANDS, p.T), dim3(SUM_THREADS), 0, (hipStream_t)stream, p, sums);
  return check_launch("clip_channel_sums");
}

extern "C" int vlfb_clip_preprocess_color(const vlfb_clip_desc* d, const vlfb_clip_color* c, const uint8_t* frames,
                                          const int32_t* xofs, const int16_t* xcoef, const int32_t* yofs,
                                          const int16_t* ycoef, const int64_t* sums, void* dst, int dst_dtype,
                                          vlfb_stream_t stream) {
  ClipP p;
  const int rc = clip_params("clip_preprocess_color", d, frames, xofs, xcoef, yofs, ycoef, true, &p);
  if (rc != VLFB_OK) return rc;
  VLFB_REQUIRE(c && dst, "clip_preprocess_color: NULL buffer");
  VLFB_REQUIRE(dst_dtype == VLFB_F32 || is16(dst_dtype), "clip_preprocess_color: dst dtype must be f32 or bf16");
  ColorP q;
  const int rq = color_params("clip_preprocess_color", c, sums, &q);
  if (rq != VLFB_OK) return rq;
  const dim3 grid(grid_for((int64_t)p.crop_h * p.crop_w, 256, 256), p.T);
  with_elem(dst_dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(clip_preprocess_color_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, p, q, (T*)dst);
  });
  return check_launch("clip_preprocess_color");
}

extern "C" int vlfb_clip_preprocess(const vlfb_clip_desc* d, const uint8_t* frames, const int32_t* xofs,
                                    const int16_t* xcoef, const int32_t* yofs, const int16_t* ycoef,
                                    void* dst, int dst_dtype, vlfb_stream_t stream) {
  VLFB_REQUIRE(d && frames && dst, "clip_preprocess: NULL buffer");
  VLFB_REQUIRE(d->frames > 0 && d->src_h > 0 && d->src_w > 0 && d->crop_h > 0 && d->crop_w > 0, "clip_preprocess: empty geometry");
  const bool resize = d->resized_h != d->src_h || d->resized_w != d->src_w;
  VLFB_REQUIRE(!resize || (xofs && xcoef && yofs && ycoef), "clip_preprocess: resize tables are required");
  VLFB_REQUIRE(d->y0 >= 0 && d->y0 + d->crop_h <= d->resized_h && d->x0 >= 0 && d->x0 < d->resized_w &&
                   (d->flip ? d->x0 - (d->crop_w - 1) >= 0 : d->x0 + d->crop_w <= d->resized_w),
               "clip_preprocess: crop window leaves the resized frame");
  VLFB_REQUIRE(d->c_pad >= 3 && d->w_left >= 0 && d->w_total >= d->w_left + d->crop_w, "clip_preprocess: bad destination row");
  VLFB_REQUIRE(dst_dtype == VLFB_F32 || is16(dst_dtype), "clip_preprocess: dst dtype must be f32 or bf16");
  ClipP p;
  p.src = frames; p.xofs = xofs; p.xcoef = xcoef; p.yofs = yofs; p.ycoef = ycoef;
  p.T = d->frames; p.Hs = d->src_h; p.Ws = d->src_w; p.Hr = d->resized_h; p.Wr = d->resized_w;
  p.resize = resize ? 1 : 0;
  p.crop_h = d->crop_h; p.crop_w = d->crop_w; p.y0 = d->y0; p.x0 = d->x0; p.flip = d->flip;
  for (int c = 0; c < 3; ++c) { p.mean[c] = d->mean[c]; p.stdv[c] = d->std[c]; }
  p.to_rgb = d->to_rgb; p.wl = d->w_left; p.wtot = d->w_total; p.c_pad = d->c_pad;
  const long long total = (long long)p.T * p.crop_h * p.crop_w;
  const int grid = grid_for(total, 256);
  with_elem(dst_dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(clip_preprocess_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, (T*)dst);
  });
  return check_launch("clip_preprocess");
}

extern "C" int vlfb_clip_batch_channel_sums(const vlfb_clip_item* items_host, const vlfb_clip_item* items_dev, int n_items,
                                            vlfb_stream_t stream) {
  int frames, tiles;
  bool any_sums;
  const int rc = check_items("clip_batch_channel_sums", items_host, items_dev, n_items, &frames, &tiles, &any_sums);
  if (rc != VLFB_OK) return rc;
  VLFB_REQUIRE(any_sums, "clip_batch_channel_sums: no item has a sums buffer");
  hipLaunchKernelGGL(clip_batch_channel_sums_kernel, dim3(VLFB_CLIP_SUM_BANDS, frames, n_items), dim3(SUM_THREADS), 0,
                     (hipStream_t)stream, items_dev);
  return check_launch("clip_batch_channel_sums");
}

extern "C" int vlfb_clip_batch_preprocess(const vlfb_clip_item* items_host, const vlfb_clip_item* items_dev, int n_items,
                                          int dst_dtype, vlfb_stream_t stream) {
  int frames, tiles;
  bool any_sums;
  const int rc = check_items("clip_batch_preprocess", items_host, items_dev, n_items, &frames, &tiles, &any_sums);
  if (rc != VLFB_OK) return rc;
  VLFB_REQUIRE(dst_dtype == VLFB_F32 || is16(dst_dtype), "clip_batch_preprocess: dst dtype must be f32 or bf16");
  const dim3 grid(tiles, frames, n_items), block(TILE_W, TILE_H);
  with_elem(dst_dtype, [&](auto t) {
    hipLaunchKernelGGL(clip_batch_preprocess_kernel<decltype(t)>, grid, block, 0, (hipStream_t)stream, items_dev);
  });
  return check_launch("clip_batch_preprocess");
}

extern "C" int vlfb_clip_batch_channel_sums_indexed(const vlfb_clip_item* items_host, const vlfb_clip_item* items_dev,
                                                    int n_items, const int32_t* index_host, const int32_t* index_dev,
                                                    int index_stride, const int32_t* store_frames_host, vlfb_stream_t stream) {
  const char* what = "clip_batch_channel_sums_indexed";
  int frames, tiles;
  bool any_sums;
  int rc = check_items(what, items_host, items_dev, n_items, &frames, &tiles, &any_sums);
  if (rc != VLFB_OK) return rc;
  rc = check_index(what, items_host, n_items, index_host, index_dev, index_stride, store_frames_host);
  if (rc != VLFB_OK) return rc;
  VLFB_REQUIRE(any_sums, "%s: no item has a sums buffer", what);
  hipLaunchKernelGGL(clip_batch_channel_sums_indexed_kernel, dim3(VLFB_CLIP_SUM_BANDS, frames, n_items), dim3(SUM_THREADS), 0,
                     (hipStream_t)stream, items_dev, index_dev, index_stride);
  return check_launch(what);
}

extern "C" int vlfb_clip_batch_preprocess_indexed(const vlfb_clip_item* items_host, const vlfb_clip_item* items_dev, int n_items,
                                                  const int32_t* index_host, const int32_t* index_dev, int index_stride,
                                                  const int32_t* store_frames_host, int dst_dtype, vlfb_stream_t stream) {
  const char* what = "clip_batch_preprocess_indexed";
  int frames, tiles;
  bool any_sums;
  int rc = check_items(what, items_host, items_dev, n_items, &frames, &tiles, &any_sums);
  if (rc != VLFB_OK) return rc;
  rc = check_index(what, items_host, n_items, index_host, index_dev, index_stride, store_frames_host);
  if (rc != VLFB_OK) return rc;
  VLFB_REQUIRE(dst_dtype == VLFB_F32 || is16(dst_dtype), "%s: dst dtype must be f32 or bf16", what);
  const dim3 grid(tiles, frames, n_items), block(TILE_W, TILE_H);
  with_elem(dst_dtype, [&](auto t) {
    hipLaunchKernelGGL(clip_batch_preprocess_indexed_kernel<decltype(t)>, grid, block, 0, (hipStream_t)stream, items_dev, index_dev, index_stride);
  });
  return check_launch(what);
}
