// The host frame of a fused dense step — drx_bpr_step, drx_fpmc_step, drx_ncf_step (DESIGN.md sections 3.7, 3.9, 3.10) — and the two
// pieces of device code their pairwise losses share.  A step is: forward / backward into scratch -> the loss -> drx_batch_csr_device over
// its key lists -> ONE drx_rows_csr_opt_multi.  What differs per model is its kernel, its scratch struct and its carve function; what
// is the same lives here:
//   step_dry_carver / step_scratch_total : the size a *_step_scratch_bytes answers
//   step_carver                          : the live Carver over the scratch a step is given
//   step_tensors_ok                      : the rule's slots of every tensor, and the alignment of the tables
//   step_table / step_table_outer        : one DrxCsrAdamTable of the update launch
//   k_loss_mean, block_loss_partial      : the loss partials of a block and their mean, summed in a fixed order
#pragma once
#include "drx_common.hpp"
#include "drx_opt.hpp"

namespace drx {

// ---- scratch ---------------------------------------------------------------------------------------------------------------------------
// Sizes only: a Carver over a non-NULL base that is never dereferenced (drx_batch_csr_device_bytes asks whether the lists' arrays are
// given, not where they are).
inline Carver step_dry_carver() { return Carver(reinterpret_cast<void *>(uintptr_t(256)), 0); }

// what the dry Carver took, and 256 bytes more: step_carver aligns the base it is given
inline size_t step_scratch_total(const Carver &cv) { return align_up(cv.off, 256) + 256; }

// cv: a Carver over `scratch` from its first 256-byte boundary on; DRX_ESCRATCH when the buffer ends before it
inline int step_carver(void *scratch, size_t scratch_bytes, Carver &cv) {
  char *base = (char *)(((uintptr_t)scratch + 255) & ~uintptr_t(255));
  const size_t lead = (size_t)(base - (char *)scratch);
  if (scratch_bytes < lead) return DRX_ESCRATCH;
  cv = Carver(base, scratch_bytes - lead);
  return DRX_OK;
}

// ---- tensors and their slots -----------------------------------------------------------------------------------------------------------
struct StepTensor {
  float *p, *s1, *s2;
};

// Whether `kind` is a dense rule and every tensor brings the slots it has; the slots it lacks become NULL (they may be anything: they
// are not passed on).  The first n_tables tensors are tables read a float4 at a time: they and their slots must be 16-byte aligned.
// The tensors behind them (bias vectors, NeuMF's small weights) are read by the element.
inline bool step_tensors_ok(int kind, StepTensor *t, int n, int n_tables) {
  if (!opt_dense_kind(kind)) return false;
  for (int i = 0; i < n; ++i)
    if (!opt_slots_ok(kind, t[i].s1, t[i].s2)) return false;
  uintptr_t bits = 0;
  for (int i = 0; i < n; ++i) {
    if (!opt_has_s1(kind)) t[i].s1 = nullptr;
    if (!opt_has_s2(kind)) t[i].s2 = nullptr;
    if (i < n_tables) bits |= (uintptr_t)t[i].p | (uintptr_t)t[i].s1 | (uintptr_t)t[i].s2;
  }
  return !(bits & 15);
}

// ---- the tables of the update launch ---------------------------------------------------------------------------------------------------
// plain: row r of `t` gets the sum of the rows of src its lookups name
inline DrxCsrAdamTable step_table(const int32_t *row_ptr, const int32_t *order, const float *src, int ld, int n_rows, const StepTensor &t,
                                  float alpha, float l2_coef) {
  DrxCsrAdamTable T;
  memset(&T, 0, sizeof(T));
  T.row_ptr = row_ptr; T.order = order; T.src = src;
  T.group = 0; T.ld = ld; T.n_rows = n_rows;
  T.p = t.p; T.m = t.s1; T.v = t.s2;
  T.alpha = alpha; T.l2_coef = l2_coef;
  return T;
}

// the scaled outer-product form: lookup o adds scale[o] * src[o / group] to its row of `t` and scale[o] to its element of `bias`
inline DrxCsrAdamTable step_table_outer(const int32_t *row_ptr, const int32_t *order, const float *src, const float *scale, int group, int ld,
                                        int n_rows, const StepTensor &t, const StepTensor &bias, float alpha, float alpha_s, float l2_coef) {
  DrxCsrAdamTable T = step_table(row_ptr, order, src, ld, n_rows, t, alpha, l2_coef);
  T.scale = scale; T.group = group;
  T.p_s = bias.p; T.m_s = bias.s1; T.v_s = bias.s2;
  T.alpha_s = alpha_s;
  return T;
}

// ---- the loss ---------------------------------------------------------------------------------------------------------------------------
// The tail of a forward / backward block of GPB groups: lane 0 of every group hands in its group's loss, thread 0 adds the GPB values
// ascending in double into loss_part[block].  EVERY thread of the block calls it (it holds the block's barrier).
template <int GPB>
__device__ __forceinline__ void block_loss_partial(int lane, int gid, double loss, double *__restrict__ loss_part) {
  __shared__ double part[GPB];
  if (lane == 0) part[gid] = loss;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < GPB; ++k) s += part[k];
    loss_part[blockIdx.x] = s;
  }
}

// out[0] = (sum of the n partials) / denom: lane l adds partials l, l + 64, ... ascending, then a fixed shuffle tree.  One wavefront.
template <int DUMMY = 0>
__global__ __launch_bounds__(64) void k_loss_mean(const double *__restrict__ part, int n, double denom, double *__restrict__ out) {
  const int lane = threadIdx.x;
  double s = 0.0;
  for (int k = lane; k < n; k += 64) s += part[k];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  if (lane == 0) out[0] = s / denom;
}

}  // namespace drx
