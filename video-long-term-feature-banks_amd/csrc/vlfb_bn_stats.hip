// Precise BN (lib/utils/bn_helper.py): the running statistics of every SpatialBN layer replaced by the average of the batch
// statistics of TRAIN.ITER_COMPUTE_PRECISE_BN training batches.  The reference fetches `_bn_sm` / `_bn_siv` of every layer
// to the host after every batch (two synchronising copies per layer and iteration); here the sums stay on the device:
//   accumulate (after each forward): sum_mean += sm; sum_mean2 += (1 / siv)^2 - eps + sm^2          (bn_helper.py:170-182)
//   finalize:   mean = sum_mean / n; var = sum_mean2 / n - mean^2; bad = #{var not > 0}              (:187-198)
//   update:     running_mean <- mean; running_var <- var                                             (:200-221)
// All three walk one layer table in device memory: a workgroup per layer (grid-stride), a thread per channel (block-
// stride), so the host needs nothing but the number of layers and the launch holds no per-iteration host value.  The
// kernels are launch-latency bound (a net has ~100 layers of 64..2048 channels).  Built with -ffp-contract=off: every
// result is compared bit for bit with the reference's float32 numpy chain, and the divisions are correctly rounded.
#include "vlfb_common.h"

namespace vlfb {
namespace {

constexpr int kStatThreads = 256;
constexpr int kStatMaxBlocks = 1024;

__global__ void __launch_bounds__(kStatThreads)
bn_precise_accumulate_kernel(const vlfb_bn_layer* __restrict__ table, int layers, float eps, float* __restrict__ sum_mean,
                             float* __restrict__ sum_mean2) {
  for (int l = blockIdx.x; l < layers; l += gridDim.x) {
    const vlfb_bn_layer L = table[l];
    for (int c = threadIdx.x; c < L.C; c += kStatThreads) {
      const float sm = L.save_mean[c];
      const float r = __fdiv_rn(1.f, L.save_inv_std[c]);
      const float var = r * r - eps;
      const float m2 = var + sm * sm;
      sum_mean[L.offset + c] += sm;
      sum_mean2[L.offset + c] += m2;
    }
  }
}

__global__ void __launch_bounds__(kStatThreads)
bn_precise_finalize_kernel(const vlfb_bn_layer* __restrict__ table, int layers, float normalize, float* __restrict__ sum_mean,
                           float* __restrict__ sum_mean2, int* __restrict__ bad) {
  __shared__ int part[kStatThreads / 64];
  int mine = 0;
  for (int l = blockIdx.x; l < layers; l += gridDim.x) {
    const vlfb_bn_layer L = table[l];
    for (int c = threadIdx.x; c < L.C; c += kStatThreads) {
      const float mean = __fdiv_rn(sum_mean[L.offset + c], normalize);
      const float m2 = __fdiv_rn(sum_mean2[L.offset + c], normalize);
      const float var = m2 - mean * mean;
      sum_mean[L.offset + c] = mean;
      sum_mean2[L.offset + c] = var;
      mine += var > 0.f ? 0 : 1;                     // (NaN counts)
    }
  }
  // integers only: the count does not depend on the launch geometry
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < kStatThreads / 64; ++w) s += part[w];
    if (s) atomicAdd(bad, s);
  }
}

__global__ void __launch_bounds__(kStatThreads)
bn_precise_update_kernel(const vlfb_bn_layer* __restrict__ table, int layers, const float* __restrict__ mean,
                         const float* __restrict__ var) {
  for (int l = blockIdx.x; l < layers; l += gridDim.x) {
    const vlfb_bn_layer L = table[l];
    for (int c = threadIdx.x; c < L.C; c += kStatThreads) {
      L.running_mean[c] = mean[L.offset + c];
      L.running_var[c] = var[L.offset + c];
    }
  }
}

inline dim3 stat_grid(int layers) { return dim3((unsigned)(layers < kStatMaxBlocks ? layers : kStatMaxBlocks)); }

}  // namespace
}  // namespace vlfb

using namespace vlfb;

static_assert(sizeof(vlfb_bn_layer) == VLFB_BN_LAYER_BYTES, "vlfb_bn_layer layout");

extern "C" int vlfb_bn_precise_accumulate(const vlfb_bn_layer* table, int layers, float eps, float* sum_mean,
                                          float* sum_mean2, vlfb_stream_t stream) {
  VLFB_REQUIRE(layers > 0, "bn_precise_accumulate: layers must be positive, got %d", layers);
  VLFB_REQUIRE(table != nullptr, "bn_precise_accumulate: the layer table is NULL");
  VLFB_REQUIRE(sum_mean && sum_mean2, "bn_precise_accumulate: NULL accumulator");
  hipLaunchKernelGGL(bn_precise_accumulate_kernel, stat_grid(layers), dim3(kStatThreads), 0, (hipStream_t)stream, table, layers,
                     eps, sum_mean, sum_mean2);
  return check_launch("bn_precise_accumulate");
}

extern "C" int vlfb_bn_precise_finalize(const vlfb_bn_layer* table, int layers, int normalize, float* sum_mean,
                                        float* sum_mean2, int32_t* bad, vlfb_stream_t stream) {
  VLFB_REQUIRE(layers > 0, "bn_precise_finalize: layers must be positive, got %d", layers);
  VLFB_REQUIRE(normalize > 0, "bn_precise_finalize: normalize must be positive, got %d", normalize);
  VLFB_REQUIRE(table != nullptr, "bn_precise_finalize: the layer table is NULL");
  VLFB_REQUIRE(sum_mean && sum_mean2, "bn_precise_finalize: NULL accumulator");
  VLFB_REQUIRE(bad != nullptr, "bn_precise_finalize: bad is NULL");
  hipError_t e = hipMemsetAsync(bad, 0, sizeof(int32_t), (hipStream_t)stream);
  if (e != hipSuccess) return set_error(VLFB_ERR_LAUNCH, "bn_precise_finalize: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(bn_precise_finalize_kernel, stat_grid(layers), dim3(kStatThreads), 0, (hipStream_t)stream, table, layers,
                     (float)normalize, sum_mean, sum_mean2, bad);
  return check_launch("bn_precise_finalize");
}

extern "C" int vlfb_bn_precise_update(const vlfb_bn_layer* table, int layers, const float* mean, const float* var,
                                      vlfb_stream_t stream) {
  VLFB_REQUIRE(layers > 0, "bn_precise_update: layers must be positive, got %d", layers);
  VLFB_REQUIRE(table != nullptr, "bn_precise_update: the layer table is NULL");
  VLFB_REQUIRE(mean && var, "bn_precise_update: NULL statistics");
  hipLaunchKernelGGL(bn_precise_update_kernel, stat_grid(layers), dim3(kStatThreads), 0, (hipStream_t)stream, table, layers,
                     mean, var);
  return check_launch("bn_precise_update");
}
