// What the tile kernels of the fused steps with small dense weights — drx_ncf_step, drx_gru_step (DESIGN.md sections 3.10, 3.11) — share
// beside the host frame of drx_step.hpp: a workgroup of the tile kernel adds its gradient of the flat small-weight array sw into ITS
// row of [grid, n_small] and its loss into one double; then
//   step_tile_grid     : the grid of such a tile kernel, min(tiles of 16, cap)
//   k_small_opt        : ONE launch adds the partial rows in workgroup order and updates sw by segments; it sums the loss too
//   set_dynamic_lds    : the dynamic-LDS attribute of a kernel that needs more than 64 KiB, set once per device and size
#pragma once
#include <atomic>
#include "drx_common.hpp"
#include "drx_opt.hpp"

namespace drx {

inline int step_tile_grid(int B, int cap) {
  const int tiles = B < 1 ? 1 : (B + 15) / 16;
  return tiles < cap ? tiles : cap;
}

// sw[j] <- rule(sum of the n_rows partials of j, rows ascending, + l2 of j's segment * sw[j]); one thread per small weight.
// thread 0 of block 0: loss_out[0] = (sum of the loss partials, ascending) / denom.
template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_small_opt(const float *__restrict__ part, int n_rows, int n, float *p, float *m, float *v,
                                                   DrxAdamSegments sg, int kind, float b1, float b2, float eps,
                                                   const double *__restrict__ loss_part, double denom, double *loss_out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j == 0 && loss_out) {
    double s = 0.0;
    for (int r = 0; r < n_rows; ++r) s += loss_part[r];
    loss_out[0] = s / denom;
  }
  if (j >= n) return;
  float t = 0.f;
  for (int r = 0; r < n_rows; ++r) t += part[(size_t)r * n + j];
  int sgi = -1;
  for (int k = 0; k < sg.n; ++k)
    if (j >= sg.start[k] && j < sg.start[k] + sg.len[k]) sgi = k;
  if (sgi < 0) return;
  const OptScalars o{kind, sg.alpha[sgi], 0.f, b1, b2, eps, sg.alpha[sgi]};
  const bool h1 = opt_has_s1(kind), h2 = opt_has_s2(kind);
  float pp = p[j], mm = h1 ? m[j] : 0.f, vv = h2 ? v[j] : 0.f;
  opt_update_dense<-1>(o, fmaf(sg.l2_coef[sgi], pp, t), pp, mm, vv);
  p[j] = pp;
  if (h1) m[j] = mm;
  if (h2) v[j] = vv;
}

// What a kernel has been granted, per device: one object per kernel, static at its launch site.
struct LdsGrant {
  std::atomic<size_t> by_device[64] = {};
};

// `bytes` of dynamic LDS for `kernel` on the current device.  Up to 64 KiB need nothing; above, hipFuncSetAttribute is called only
// when the device has not been granted that much yet — not on every step.
inline int set_dynamic_lds(const void *kernel, size_t bytes, LdsGrant &grant) {
  if (bytes <= 64 * 1024) return DRX_OK;
  int dev = 0;
  DRX_HIP(hipGetDevice(&dev));
  const bool kept = dev >= 0 && dev < 64;
  if (kept && grant.by_device[dev].load(std::memory_order_relaxed) >= bytes) return DRX_OK;
  DRX_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  if (kept) grant.by_device[dev].store(bytes, std::memory_order_relaxed);
  return DRX_OK;
}

}  // namespace drx
