// BPR-MF (Rendle et al. 2009; include/drx.h "BPR-MF"): the triple sampler, the forward / backward kernel of the
// pairwise step and the step itself, which hands the update to the dense family of drx_generic.hip.
//   drx_bpr_sample      : one thread per triple, three counters of the project's hash, no retry loop
//   drx_bpr_gather_rows : rows of a table by id (the query rows of the fused scorer)
//   drx_bpr_step        : k_bpr_fwd_bwd -> drx_batch_csr_device (user keys, item keys) -> ONE drx_rows_csr_opt_multi (P plain, Q with
//                         bq in the outer-product form) -> the loss partials summed in a fixed order.  No atomics.
#include "drx_common.hpp"
#include "drx_rows.hpp"
#include "drx_opt.hpp"
#include "drx_step.hpp"

namespace drx {

static __device__ __forceinline__ uint32_t bpr_bounded(uint32_t h, uint32_t n) { return (uint32_t)(((uint64_t)h * n) >> 32); }

// j-th (0-based) id of the ascending complement of held[0..nh): drx_sampler.hip's complement_at, restated for this translation unit
static __device__ __forceinline__ int32_t bpr_complement_at(const int32_t *__restrict__ held, int nh, uint32_t j) {
  int lo = 0, hi = nh;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)held[mid] - (int64_t)mid <= (int64_t)j) lo = mid + 1; else hi = mid;
  }
  return (int32_t)(j + (uint32_t)lo);
}

// H: the positives, R: every recorded pair (H itself where all recorded pairs are positives)
__global__ __launch_bounds__(kBlock) void k_bpr_sample(DrxHistory H, DrxHistory R, const int32_t *__restrict__ eligible, int n_eligible,
                                                       int n_items, int T, int r, uint64_t seed, int32_t *__restrict__ uid,
                                                       int32_t *__restrict__ pos, int32_t *__restrict__ neg) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= T) return;
  const uint32_t p = (uint32_t)(t / r);
  const int u = eligible[bpr_bounded(hash_u32(seed, p, 0u), (uint32_t)n_eligible)];
  const int64_t s = H.indptr[u];
  const int64_t deg = H.indptr[u + 1] - s;
  const int64_t rs = R.indptr[u];
  const int64_t nrec = R.indptr[u + 1] - rs;
  uid[t] = u;
  // (an eligible user has deg >= 1 and nrec < n_items; a listed user who is not gets -1 instead of a read past its row)
  pos[t] = deg >= 1 ? H.indices[s + bpr_bounded(hash_u32(seed, p, 1u), (uint32_t)deg)] : -1;
  neg[t] = nrec < n_items ? bpr_complement_at(R.indices + rs, (int)nrec, bpr_bounded(hash_u32(seed, (uint32_t)t, 2u), (uint32_t)(n_items - nrec)))
                          : -1;
}

template <int G>
__global__ __launch_bounds__(kBlock) void k_bpr_gather_rows(const float *__restrict__ table, int ld, const int32_t *__restrict__ ids, int n,
                                                            float *__restrict__ out) {
  const int lane = threadIdx.x % G;
  constexpr int gpb = kBlock / G;
  for (int r = blockIdx.x * gpb + threadIdx.x / G; r < n; r += gridDim.x * gpb) {
    float4 v[1];
    load_row<G, 1>(table, (size_t)ids[r], ld, lane, v);
    store_row<G, 1>(out, (size_t)r, ld, lane, v);
  }
}

// A group of G lanes per triple, one float4 of each row per lane (ld <= 4 G).  Per triple: reads P[u], Q[i], Q[j] once (3 ld floats),
// the three ids and two biases; writes the gradient row of P[u] and a copy of P[u] (2 ld floats), (g, -g) and the item keys (i, j).
// The update launch reads the copy, not P: it rewrites P's rows while it sums the item gradients.
// loss_part[block] = the block's sum of softplus(-D_t) in double, its triples ascending.
template <int G>
__global__ __launch_bounds__(kBlock) void k_bpr_fwd_bwd(const float *__restrict__ P, const float *__restrict__ Q, const float *__restrict__ bq,
                                                        int ld, const int32_t *__restrict__ uid, const int32_t *__restrict__ pos,
                                                        const int32_t *__restrict__ neg, int T, float *__restrict__ dP,
                                                        float *__restrict__ pu, float *__restrict__ gs, int32_t *__restrict__ ikeys,
                                                        double *__restrict__ loss_part) {
  constexpr int gpb = kBlock / G;
  const int lane = threadIdx.x % G, gid = threadIdx.x / G;
  const int t = blockIdx.x * gpb + gid;
  float loss = 0.f;
  if (t < T) {                                         // (a group is live or idle as a whole: the shuffles stay inside live groups)
    const int u = uid[t], i = pos[t], j = neg[t];
    float4 p[1], qi[1], qj[1];
    load_row<G, 1>(P, (size_t)u, ld, lane, p);
    load_row<G, 1>(Q, (size_t)i, ld, lane, qi);
    load_row<G, 1>(Q, (size_t)j, ld, lane, qj);
    float4 d[1];
    d[0] = make_float4(qi[0].x - qj[0].x, qi[0].y - qj[0].y, qi[0].z - qj[0].z, qi[0].w - qj[0].w);
    const float delta = group_sum<G>(f4_dot(p[0], d[0])) + (bq[i] - bq[j]);
    // g = -sigmoid(-delta) / T;  softplus(-delta) = max(-delta, 0) + log1p(exp(-|delta|))
    const float g = -(1.0f / (1.0f + expf(delta))) / (float)T;
    loss = fmaxf(-delta, 0.f) + log1pf(expf(-fabsf(delta)));
    d[0].x *= g; d[0].y *= g; d[0].z *= g; d[0].w *= g;
    store_row<G, 1>(dP, (size_t)t, ld, lane, d);
    store_row<G, 1>(pu, (size_t)t, ld, lane, p);
    if (lane == 0) {
      gs[2 * (size_t)t] = g;
      gs[2 * (size_t)t + 1] = -g;
      ikeys[2 * (size_t)t] = i;
      ikeys[2 * (size_t)t + 1] = j;
    }
  }
  block_loss_partial<gpb>(lane, gid, (double)loss, loss_part);
}

struct BprScratch {
  float *dP, *pu, *gs;
  int32_t *ikeys, *rp_u, *ord_u, *rp_i, *ord_i;
  double *loss_part;
  void *csr;
  size_t csr_bytes;
  int blocks;
};

// the two key lists of a step as drx_batch_csr_device takes them
static void bpr_lists(const int32_t *ukeys, const BprScratch &S, int T, int n_users, int n_items, DrxCsrList (&ls)[2]) {
  ls[0] = DrxCsrList{ukeys, T, n_users, S.rp_u, S.ord_u};
  ls[1] = DrxCsrList{S.ikeys, 2 * T, n_items, S.rp_i, S.ord_i};
}

static bool bpr_shape_ok(int64_t T, int ld, int n_users, int n_items) {
  return T >= 1 && T < (1 << 29) && n_users >= 1 && n_items >= 1 && ld >= 4 && ld <= 256 && !(ld & 3) && (int64_t)T * ld < (int64_t)1 << 40;
}

// carves the step's scratch; false when the description is invalid
static bool bpr_carve(Carver &cv, int T, int ld, int n_users, int n_items, BprScratch &S) {
  if (!bpr_shape_ok(T, ld, n_users, n_items)) return false;
  const int gpb = kBlock / pick_geom(ld).G;
  S.blocks = (T + gpb - 1) / gpb;
  S.dP = cv.take<float>((size_t)T * ld);
  S.pu = cv.take<float>((size_t)T * ld);
  S.gs = cv.take<float>(2 * (size_t)T);
  S.ikeys = cv.take<int32_t>(2 * (size_t)T);
  S.rp_u = cv.take<int32_t>((size_t)n_users + 1);
  S.ord_u = cv.take<int32_t>((size_t)T);
  S.rp_i = cv.take<int32_t>((size_t)n_items + 1);
  S.ord_i = cv.take<int32_t>(2 * (size_t)T);
  S.loss_part = cv.take<double>((size_t)S.blocks);
  DrxCsrList ls[2];
  bpr_lists(S.ord_u /* stands for the user keys */, S, T, n_users, n_items, ls);
  S.csr_bytes = drx_batch_csr_device_bytes(ls, 2);
  if (!S.csr_bytes) return false;
  S.csr = cv.take<char>(S.csr_bytes);
  return true;
}

}  // namespace drx

extern "C" {

int drx_bpr_sample(const DrxHistory *hist, const DrxHistory *recorded, const int32_t *eligible, int32_t n_eligible, int32_t n_items,
                   int32_t T, int32_t neg_ratio, uint64_t seed, int32_t *uid, int32_t *pos, int32_t *neg, void *stream) {
  using namespace drx;
  if (recorded && (!recorded->indptr || !recorded->indices)) return DRX_EINVAL;
  if (!hist || !hist->indptr || !hist->indices || !eligible || !uid || !pos || !neg || n_eligible < 1 || n_items < 1 || T < 1 || neg_ratio < 1)
    return DRX_EINVAL;
  hipLaunchKernelGGL(k_bpr_sample, dim3((T + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, *hist, recorded ? *recorded : *hist,
                     eligible, n_eligible, n_items, T, neg_ratio, seed, uid, pos, neg);
  DRX_LAUNCH_CHECK();
  return DRX_OK;
}

int drx_bpr_gather_rows(const float *table, int32_t ld, const int32_t *ids, int32_t n, float *out, void *stream) {
  using namespace drx;
  if (!table || !ids || !out || n < 1 || ld < 4 || (ld & 3) || ld > 256 || (((uintptr_t)table | (uintptr_t)out) & 15)) return DRX_EINVAL;
  return dispatch_geom(ld, [&](auto g) -> int {
    constexpr int G = decltype(g)::G;
    constexpr int gpb = kBlock / G;
    int blocks = (n + gpb - 1) / gpb;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_bpr_gather_rows<G>, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, table, ld, ids, n, out);
    DRX_LAUNCH_CHECK();
    return DRX_OK;
  });
}

size_t drx_bpr_step_scratch_bytes(int32_t T, int32_t ld, int32_t n_users, int32_t n_items) {
  using namespace drx;
  Carver cv = step_dry_carver();
  BprScratch S;
  return bpr_carve(cv, T, ld, n_users, n_items, S) ? step_scratch_total(cv) : 0;
}

int drx_bpr_step(float *P, float *Q, float *bq, float *P_s1, float *P_s2, float *Q_s1, float *Q_s2, float *bq_s1, float *bq_s2, int32_t ld,
                 int32_t n_users, int32_t n_items, const int32_t *uid, const int32_t *pos, const int32_t *neg, int32_t T,
                 const DrxOptRule *rule, const float *alphas, float reg, double *loss_out, void *scratch, size_t scratch_bytes,
                 void *stream) {
  using namespace drx;
  if (!P || !Q || !bq || !uid || !pos || !neg || !rule || !alphas || !scratch || !bpr_shape_ok(T, ld, n_users, n_items)) return DRX_EINVAL;
  StepTensor t[3] = {{P, P_s1, P_s2}, {Q, Q_s1, Q_s2}, {bq, bq_s1, bq_s2}};
  if (!step_tensors_ok(rule->kind, t, 3, 2)) return DRX_EINVAL;
  Carver cv(nullptr, 0);
  if (int rc = step_carver(scratch, scratch_bytes, cv)) return rc;
  BprScratch S;
  if (!bpr_carve(cv, T, ld, n_users, n_items, S)) return DRX_EINVAL;
  if (!cv.ok()) return DRX_ESCRATCH;
  hipStream_t st = (hipStream_t)stream;
  int rc = dispatch_geom(ld, [&](auto g) -> int {
    constexpr int G = decltype(g)::G;
    hipLaunchKernelGGL(k_bpr_fwd_bwd<G>, dim3(S.blocks), dim3(kBlock), 0, st, P, Q, bq, ld, uid, pos, neg, T, S.dP, S.pu, S.gs, S.ikeys,
                       S.loss_part);
    DRX_LAUNCH_CHECK();
    return DRX_OK;
  });
  if (rc) return rc;
  if (loss_out) hipLaunchKernelGGL(k_loss_mean<>, dim3(1), dim3(64), 0, st, S.loss_part, S.blocks, (double)T, loss_out);
  DrxCsrList ls[2];
  bpr_lists(uid, S, T, n_users, n_items, ls);
  rc = drx_batch_csr_device(ls, 2, S.csr, S.csr_bytes, stream);
  if (rc) return rc;
  const DrxCsrAdamTable tabs[2] = {step_table(S.rp_u, S.ord_u, S.dP, ld, n_users, t[0], alphas[0], reg),
                                   step_table_outer(S.rp_i, S.ord_i, S.pu, S.gs, 2, ld, n_items, t[1], t[2], alphas[1], alphas[2], reg)};
  return drx_rows_csr_opt_multi(tabs, 2, rule, stream);
}

}  // extern "C"
