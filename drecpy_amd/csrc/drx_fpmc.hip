// FPMC (Rendle, Freudenthaler, Schmidt-Thieme 2010; include/drx.h "FPMC"): the forward / backward kernel of the
// sequential pairwise step, the step itself — which hands the update to the dense family of drx_generic.hip — and the query rows of
// serving.
//   drx_fpmc_step       : k_fpmc_fwd_bwd -> drx_batch_csr_device (user keys, previous-item keys, item keys) -> ONE
//                         drx_rows_csr_opt_multi (P plain, M plain, QN with b in the outer-product form) -> the loss partials summed
//                         in a fixed order.  No atomics.
//   drx_fpmc_query_rows : [P[u] | mean of M over the user's basket] per requested user (the query rows of the fused scorer)
// Both build the context row with fpmc_context: one definition of the order in which the rows of M are summed.
#include "drx_common.hpp"
#include "drx_rows.hpp"
#include "drx_opt.hpp"
#include "drx_step.hpp"

namespace drx {

constexpr int kFpmcMaxL = 8;        // previous items of a window (Caser's window domain)
constexpr int kFpmcNegRound = 8;    // rows of QN in flight per round of negatives: 32 VGPRs of a lane
constexpr int kFpmcMaxNeg = 16;     // two rounds

// Float4 `lane` of the context row [P[u] | mean of M[ids[l]] over the ids present] (2 ld floats; lanes past the row hold zeros).
// ids[0..L): an id < 0 is an absent position.  The lanes of the second half load all L rows first, then add them positions ascending
// in fp32 and multiply ONCE by 1.0f / (the number present); no id present: zeros.  (An absent position adds +0 to a sum that is never
// -0: the sum's bits are those of the present rows alone.)
template <int G>
__device__ __forceinline__ float4 fpmc_context(const float *__restrict__ P, const float *__restrict__ M, int ld, int u,
                                               const int32_t *__restrict__ ids, int L, int lane) {
  const int h = ld >> 2;
  if (lane < h) return reinterpret_cast<const float4 *>(P + (size_t)u * ld)[lane];
  float4 acc = f4_zero();
  if (lane < 2 * h) {
    float4 m[kFpmcMaxL];
    int n = 0;
#pragma unroll
    for (int l = 0; l < kFpmcMaxL; ++l) {
      const int id = l < L ? ids[l] : -1;
      m[l] = id >= 0 ? reinterpret_cast<const float4 *>(M + (size_t)id * ld)[lane - h] : f4_zero();
      n += id >= 0;
    }
#pragma unroll
    for (int l = 0; l < kFpmcMaxL; ++l) f4_add(acc, m[l]);
    if (n) {
      const float s = 1.0f / (float)n;
      acc.x *= s; acc.y *= s; acc.z *= s; acc.w *= s;
    }
  }
  return acc;
}

// A group of G lanes per window, one float4 of a 2 ld row per lane (2 ld <= 4 G).  Per window: reads P[u] and the L rows of M once (the
// context c is formed ONCE, not once per negative), QN[i] and the r rows QN[j_k] in rounds of kFpmcNegRound, their biases and the ids;
// writes c (the update launch reads it: it rewrites P and M while it sums the gradients of QN), the first half of
// d = sum_k g_k (QN[i] - QN[j_k]) (the gradient row of P[u]), L copies of the second half times 1 / L (the gradient rows of M[l], l in S)
// and the 1 + r scales (sum_k g_k, -g_1 .. -g_r).  The item keys of the update are `after` itself.
// loss_part[block] = the block's sum over its windows (ascending) of sum_k softplus(-D_k) (k ascending) in double.
template <int G>
__global__ __launch_bounds__(kBlock) void k_fpmc_fwd_bwd(const float *__restrict__ P, const float *__restrict__ M, const float *__restrict__ QN,
                                                         const float *__restrict__ bq, int ld, const int32_t *__restrict__ uid,
                                                         const int32_t *__restrict__ before, const int32_t *__restrict__ after, int B, int L,
                                                         int r, float *__restrict__ ctx, float *__restrict__ dP, float *__restrict__ dM,
                                                         float *__restrict__ gs, double *__restrict__ loss_part) {
  constexpr int gpb = kBlock / G;
  const int lane = threadIdx.x % G, gid = threadIdx.x / G;
  const int w = blockIdx.x * gpb + gid;
  const int ld2 = 2 * ld, h = ld >> 2;
  double loss = 0.0;
  if (w < B) {                                         // (a group is live or idle as a whole: the shuffles stay inside live groups)
    const int32_t *items = after + (size_t)w * (1 + r);
    float4 c[1], qi[1];
    const int i = items[0];
    load_row<G, 1>(QN, (size_t)i, ld2, lane, qi);
    const float bi = bq[i];
    c[0] = fpmc_context<G>(P, M, ld, uid[w], before + (size_t)w * L, L, lane);
    const float scale = 1.0f / ((float)B * (float)r);
    float4 d = f4_zero();
    float gsum = 0.f;
    for (int k0 = 0; k0 < r; k0 += kFpmcNegRound) {
      float4 qj[kFpmcNegRound];
      float bj[kFpmcNegRound];
#pragma unroll
      for (int q = 0; q < kFpmcNegRound; ++q) {         // the round's loads, all issued before its first reduction
        const bool on = k0 + q < r;
        const int j = on ? items[1 + k0 + q] : i;
        float4 t[1];
        load_row<G, 1>(QN, (size_t)j, ld2, lane, t);
        qj[q] = t[0];
        bj[q] = bq[j];
      }
#pragma unroll
      for (int q = 0; q < kFpmcNegRound; ++q) {
        if (k0 + q < r) {                                // (uniform over the group)
          const float4 df = make_float4(qi[0].x - qj[q].x, qi[0].y - qj[q].y, qi[0].z - qj[q].z, qi[0].w - qj[q].w);
          const float delta = group_sum<G>(f4_dot(c[0], df)) + (bi - bj[q]);
          // g = -sigmoid(-delta) / (B r);  softplus(-delta) = max(-delta, 0) + log1p(exp(-|delta|))
          const float g = -(1.0f / (1.0f + expf(delta))) * scale;
          loss += (double)(fmaxf(-delta, 0.f) + log1pf(expf(-fabsf(delta))));
          f4_fma(d, g, df);
          gsum += g;
          if (lane == 0) gs[(size_t)w * (1 + r) + 1 + k0 + q] = -g;
        }
      }
    }
    if (lane == 0) gs[(size_t)w * (1 + r)] = gsum;
    store_row<G, 1>(ctx, (size_t)w, ld2, lane, c);
    if (lane < h) {
      reinterpret_cast<float4 *>(dP + (size_t)w * ld)[lane] = d;
    } else if (lane < 2 * h) {
      const float inv = 1.0f / (float)L;
      d.x *= inv; d.y *= inv; d.z *= inv; d.w *= inv;
      for (int l = 0; l < L; ++l) reinterpret_cast<float4 *>(dM + ((size_t)w * L + l) * ld)[lane - h] = d;
    }
  }
  block_loss_partial<gpb>(lane, gid, loss, loss_part);
}

template <int G>
__global__ __launch_bounds__(kBlock) void k_fpmc_query_rows(const float *__restrict__ P, const float *__restrict__ M, int ld,
                                                            const int32_t *__restrict__ baskets, int L, const int32_t *__restrict__ uid,
                                                            int n, float *__restrict__ out) {
  const int lane = threadIdx.x % G;
  constexpr int gpb = kBlock / G;
  for (int r = blockIdx.x * gpb + threadIdx.x / G; r < n; r += gridDim.x * gpb) {
    const int u = uid[r];
    float4 c[1];
    c[0] = fpmc_context<G>(P, M, ld, u, baskets + (size_t)u * L, L, lane);
    store_row<G, 1>(out, (size_t)r, 2 * ld, lane, c);
  }
}

struct FpmcScratch {
  float *ctx, *dP, *dM, *gs;
  int32_t *rp_u, *ord_u, *rp_m, *ord_m, *rp_i, *ord_i;
  double *loss_part;
  void *csr;
  size_t csr_bytes;
  int blocks;
};

// the three key lists of a step as drx_batch_csr_device takes them
static void fpmc_lists(const int32_t *uid, const int32_t *before, const int32_t *after, const FpmcScratch &S, int B, int L, int r,
                       int n_users, int n_items, DrxCsrList (&ls)[3]) {
  ls[0] = DrxCsrList{uid, B, n_users, S.rp_u, S.ord_u};
  ls[1] = DrxCsrList{before, B * L, n_items, S.rp_m, S.ord_m};
  ls[2] = DrxCsrList{after, B * (1 + r), n_items, S.rp_i, S.ord_i};
}

static bool fpmc_ld_ok(int ld) { return ld >= 4 && ld <= 128 && !(ld & 3); }

static bool fpmc_shape_ok(int64_t B, int L, int r, int ld, int n_users, int n_items) {
  return B >= 1 && B < (1 << 24) && L >= 1 && L <= kFpmcMaxL && r >= 1 && r <= kFpmcMaxNeg && n_users >= 1 && n_items >= 1 && fpmc_ld_ok(ld);
}

// carves the step's scratch; false when the description is invalid
static bool fpmc_carve(Carver &cv, int B, int L, int r, int ld, int n_users, int n_items, FpmcScratch &S) {
  if (!fpmc_shape_ok(B, L, r, ld, n_users, n_items)) return false;
  const int gpb = kBlock / pick_geom(2 * ld).G;
  S.blocks = (B + gpb - 1) / gpb;
  S.ctx = cv.take<float>((size_t)B * 2 * ld);
  S.dP = cv.take<float>((size_t)B * ld);
  S.dM = cv.take<float>((size_t)B * L * ld);
  S.gs = cv.take<float>((size_t)B * (1 + r));
  S.rp_u = cv.take<int32_t>((size_t)n_users + 1);
  S.ord_u = cv.take<int32_t>((size_t)B);
  S.rp_m = cv.take<int32_t>((size_t)n_items + 1);
  S.ord_m = cv.take<int32_t>((size_t)B * L);
  S.rp_i = cv.take<int32_t>((size_t)n_items + 1);
  S.ord_i = cv.take<int32_t>((size_t)B * (1 + r));
  S.loss_part = cv.take<double>((size_t)S.blocks);
  DrxCsrList ls[3];
  fpmc_lists(S.ord_u, S.ord_m, S.ord_i /* stand for the keys */, S, B, L, r, n_users, n_items, ls);
  S.csr_bytes = drx_batch_csr_device_bytes(ls, 3);
  if (!S.csr_bytes) return false;
  S.csr = cv.take<char>(S.csr_bytes);
  return true;
}

}  // namespace drx

extern "C" {

size_t drx_fpmc_step_scratch_bytes(int32_t B, int32_t L, int32_t neg_ratio, int32_t ld, int32_t n_users, int32_t n_items) {
  using namespace drx;
  Carver cv = step_dry_carver();
  FpmcScratch S;
  return fpmc_carve(cv, B, L, neg_ratio, ld, n_users, n_items, S) ? step_scratch_total(cv) : 0;
}

int drx_fpmc_step(float *P, float *M, float *QN, float *b, float *P_s1, float *P_s2, float *M_s1, float *M_s2, float *QN_s1, float *QN_s2,
                  float *b_s1, float *b_s2, int32_t ld, int32_t n_users, int32_t n_items, const int32_t *uid, const int32_t *before,
                  const int32_t *after, int32_t B, int32_t L, int32_t neg_ratio, const DrxOptRule *rule, const float *alphas, float reg,
                  double *loss_out, void *scratch, size_t scratch_bytes, void *stream) {
  using namespace drx;
  const int r = neg_ratio;
  if (!P || !M || !QN || !b || !uid || !before || !after || !rule || !alphas || !scratch || !fpmc_shape_ok(B, L, r, ld, n_users, n_items))
    return DRX_EINVAL;
  StepTensor t[4] = {{P, P_s1, P_s2}, {M, M_s1, M_s2}, {QN, QN_s1, QN_s2}, {b, b_s1, b_s2}};
  if (!step_tensors_ok(rule->kind, t, 4, 3)) return DRX_EINVAL;
  Carver cv(nullptr, 0);
  if (int rc = step_carver(scratch, scratch_bytes, cv)) return rc;
  FpmcScratch S;
  if (!fpmc_carve(cv, B, L, r, ld, n_users, n_items, S)) return DRX_EINVAL;
  if (!cv.ok()) return DRX_ESCRATCH;
  hipStream_t st = (hipStream_t)stream;
  int rc = dispatch_geom(2 * ld, [&](auto g) -> int {
    constexpr int G = decltype(g)::G;
    hipLaunchKernelGGL(k_fpmc_fwd_bwd<G>, dim3(S.blocks), dim3(kBlock), 0, st, P, M, QN, b, ld, uid, before, after, B, L, r, S.ctx, S.dP,
                       S.dM, S.gs, S.loss_part);
    DRX_LAUNCH_CHECK();
    return DRX_OK;
  });
  if (rc) return rc;
  if (loss_out) hipLaunchKernelGGL(k_loss_mean<>, dim3(1), dim3(64), 0, st, S.loss_part, S.blocks, (double)B * (double)r, loss_out);
  DrxCsrList ls[3];
  fpmc_lists(uid, before, after, S, B, L, r, n_users, n_items, ls);
  rc = drx_batch_csr_device(ls, 3, S.csr, S.csr_bytes, stream);
  if (rc) return rc;
  const DrxCsrAdamTable tabs[3] = {
      step_table(S.rp_u, S.ord_u, S.dP, ld, n_users, t[0], alphas[0], reg), step_table(S.rp_m, S.ord_m, S.dM, ld, n_items, t[1], alphas[1], reg),
      step_table_outer(S.rp_i, S.ord_i, S.ctx, S.gs, 1 + r, 2 * ld, n_items, t[2], t[3], alphas[2], alphas[3], reg)};
  return drx_rows_csr_opt_multi(tabs, 3, rule, stream);
}

int drx_fpmc_query_rows(const float *P, const float *M, int32_t ld, const int32_t *baskets, int32_t L, const int32_t *uid, int32_t n,
                        float *out, void *stream) {
  using namespace drx;
  if (!P || !M || !baskets || !uid || !out || n < 1 || L < 1 || L > kFpmcMaxL || !fpmc_ld_ok(ld) ||
      (((uintptr_t)P | (uintptr_t)M | (uintptr_t)out) & 15))
    return DRX_EINVAL;
  return dispatch_geom(2 * ld, [&](auto g) -> int {
    constexpr int G = decltype(g)::G;
    constexpr int gpb = kBlock / G;
    int blocks = (n + gpb - 1) / gpb;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_fpmc_query_rows<G>, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, P, M, ld, baskets, L, uid, n, out);
    DRX_LAUNCH_CHECK();
    return DRX_OK;
  });
}

}  // extern "C"
