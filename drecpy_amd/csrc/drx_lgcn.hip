// LightGCN (He et al. 2020; include/drx.h "LightGCN"): the sparse propagation out = scale (base + A in) over the
// symmetric normalised adjacency of the positives, the forward / backward kernel of the pairwise step, the dense gradient of the final
// embeddings and the step itself, which hands the update to drx_opt_dense.
//   drx_lgcn_propagate : k_lgcn_segments (a lane group per segment of at most kLgcnSplit entries of one row, kLgcnFlight neighbour rows
//                        in flight) -> k_lgcn_combine (the rows that were cut: their partial rows added in segment order)
//   drx_lgcn_final     : the Horner recurrence S <- E0 + A S, `layers` propagations, the last one scaled by 1 / (layers + 1)
//   drx_lgcn_step      : the same forward -> k_lgcn_fwd_bwd -> drx_batch_csr_device (the 3 T node keys) -> k_lgcn_dense_grad (every row of
//                        G, zeros included) -> the same recurrence on G -> drx_opt_dense on the user and the item half.  No atomics.
#include "drx_common.hpp"
#include "drx_rows.hpp"
#include "drx_opt.hpp"
#include "drx_step.hpp"

namespace drx {

// (variant builds: -DDRX_LGCN_SPLIT=..., -DDRX_LGCN_FLIGHT=...; DESIGN.md section 3.14 has what they measured)
#ifndef DRX_LGCN_SPLIT
#define DRX_LGCN_SPLIT 128
#endif
#ifndef DRX_LGCN_FLIGHT
#define DRX_LGCN_FLIGHT 4
#endif
constexpr int kLgcnSplit = DRX_LGCN_SPLIT;    // a row longer than this is cut into segments of this many entries (the last one shorter)
constexpr int kLgcnFlight = DRX_LGCN_FLIGHT;  // neighbour rows a lane group has in flight

// sum over entries [e0, e1) of the CSR, ascending, of w[c] * in[c, :] — this lane's float4 of it
template <int G>
__device__ __forceinline__ float4 lgcn_entries_sum(const DrxLgcnGraph &g, const float *in, int ld, int lane, int64_t e0, int64_t e1) {
  float4 acc = f4_zero();
  for (int64_t e = e0; e < e1; e += kLgcnFlight) {
    float4 v[kLgcnFlight][1];
    float wc[kLgcnFlight];
#pragma unroll
    for (int q = 0; q < kLgcnFlight; ++q) {
      wc[q] = 0.f;
      v[q][0] = f4_zero();
      if (e + q < e1) {
        const int32_t c = g.indices[e + q];
        wc[q] = g.w[c];
        load_row<G, 1>(in, (size_t)c, ld, lane, v[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < kLgcnFlight; ++q)
      if (e + q < e1) f4_fma(acc, wc[q], v[q][0]);
  }
  return acc;
}

// out[row, :] = scale * (base[row, :] + w[row] * acc)
template <int G>
__device__ __forceinline__ void lgcn_finish_row(const DrxLgcnGraph &g, const float *base, float *__restrict__ out, int row, int ld, int lane,
                                                const float4 &acc, float scale) {
  const float wr = g.w[row];
  float4 b[1], o[1];
  b[0] = f4_zero();
  if (base) load_row<G, 1>(base, (size_t)row, ld, lane, b);
  o[0] = make_float4(scale * (b[0].x + wr * acc.x), scale * (b[0].y + wr * acc.y), scale * (b[0].z + wr * acc.z), scale * (b[0].w + wr * acc.w));
  store_row<G, 1>(out, (size_t)row, ld, lane, o);
}

// A lane group per segment: a row of one segment is finished here, a cut row leaves part[segment, :].  (`base` may be `in`.)
template <int G>
__global__ __launch_bounds__(kBlock) void k_lgcn_segments(DrxLgcnGraph g, const float *base, const float *in, float *__restrict__ out,
                                                          float *__restrict__ part, int ld, float scale) {
  constexpr int gpb = kBlock / G;
  const int lane = threadIdx.x % G;
  const int s = blockIdx.x * gpb + threadIdx.x / G;
  if (s >= g.n_seg) return;
  const int row = g.seg_row[s];
  const int first = g.seg_ptr[row], n = g.seg_ptr[row + 1] - first;
  const int64_t r1 = g.indptr[row + 1];
  const int64_t e0 = g.indptr[row] + (int64_t)(s - first) * kLgcnSplit;
  const int64_t e1 = e0 + kLgcnSplit < r1 ? e0 + kLgcnSplit : r1;
  float4 acc[1];
  acc[0] = lgcn_entries_sum<G>(g, in, ld, lane, e0, e1);
  if (n == 1) lgcn_finish_row<G>(g, base, out, row, ld, lane, acc[0], scale);
  else store_row<G, 1>(part, (size_t)s, ld, lane, acc);
}

// A lane group per cut row: its partial rows added in segment order, then the row finished as above.
template <int G>
__global__ __launch_bounds__(kBlock) void k_lgcn_combine(DrxLgcnGraph g, const float *base, float *__restrict__ out,
                                                         const float *__restrict__ part, int ld, float scale) {
  constexpr int gpb = kBlock / G;
  const int lane = threadIdx.x % G;
  const int k = blockIdx.x * gpb + threadIdx.x / G;
  if (k >= g.n_cut) return;
  const int row = g.cut_rows[k];
  const int first = g.seg_ptr[row], n = g.seg_ptr[row + 1] - first;
  float4 acc = f4_zero();
  for (int q0 = 0; q0 < n; q0 += kLgcnFlight) {
    float4 v[kLgcnFlight][1];
#pragma unroll
    for (int q = 0; q < kLgcnFlight; ++q) {
      v[q][0] = f4_zero();
      if (q0 + q < n) load_row<G, 1>(part, (size_t)(first + q0 + q), ld, lane, v[q]);
    }
#pragma unroll
    for (int q = 0; q < kLgcnFlight; ++q)
      if (q0 + q < n) f4_add(acc, v[q][0]);
  }
  lgcn_finish_row<G>(g, base, out, row, ld, lane, acc, scale);
}

// A group of G lanes per triple, one float4 of each row per lane.  Reads Ebar[u], Ebar[n_users + i], Ebar[n_users + j] once and writes
// the three gradient rows of the triple (mat[3 t .. 3 t + 2]: g (ei - ej), g eu, -g eu) with their node keys.
// loss_part[block] = the block's sum of softplus(-D_t) in double, its triples ascending.
template <int G>
__global__ __launch_bounds__(kBlock) void k_lgcn_fwd_bwd(const float *__restrict__ E, int ld, int n_users, const int32_t *__restrict__ uid,
                                                         const int32_t *__restrict__ pos, const int32_t *__restrict__ neg, int T,
                                                         float *__restrict__ mat, int32_t *__restrict__ keys, double *__restrict__ loss_part) {
  constexpr int gpb = kBlock / G;
  const int lane = threadIdx.x % G, gid = threadIdx.x / G;
  const int t = blockIdx.x * gpb + gid;
  float loss = 0.f;
  if (t < T) {                                         // (a group is live or idle as a whole: the shuffles stay inside live groups)
    const int u = uid[t], i = n_users + pos[t], j = n_users + neg[t];
    float4 eu[1], ei[1], ej[1], d[1], a[1], b[1];
    load_row<G, 1>(E, (size_t)u, ld, lane, eu);
    load_row<G, 1>(E, (size_t)i, ld, lane, ei);
    load_row<G, 1>(E, (size_t)j, ld, lane, ej);
    d[0] = make_float4(ei[0].x - ej[0].x, ei[0].y - ej[0].y, ei[0].z - ej[0].z, ei[0].w - ej[0].w);
    const float delta = group_sum<G>(f4_dot(eu[0], d[0]));
    // g = -sigmoid(-delta) / T;  softplus(-delta) = max(-delta, 0) + log1p(exp(-|delta|))
    const float gr = -(1.0f / (1.0f + expf(delta))) / (float)T;
    loss = fmaxf(-delta, 0.f) + log1pf(expf(-fabsf(delta)));
    d[0].x *= gr; d[0].y *= gr; d[0].z *= gr; d[0].w *= gr;
    a[0] = make_float4(gr * eu[0].x, gr * eu[0].y, gr * eu[0].z, gr * eu[0].w);
    b[0] = make_float4(-a[0].x, -a[0].y, -a[0].z, -a[0].w);
    store_row<G, 1>(mat, 3 * (size_t)t, ld, lane, d);
    store_row<G, 1>(mat, 3 * (size_t)t + 1, ld, lane, a);
    store_row<G, 1>(mat, 3 * (size_t)t + 2, ld, lane, b);
    if (lane == 0) {
      keys[3 * (size_t)t] = u;
      keys[3 * (size_t)t + 1] = i;
      keys[3 * (size_t)t + 2] = j;
    }
  }
  block_loss_partial<gpb>(lane, gid, (double)loss, loss_part);
}

// A lane group per node: Gd[r, :] = the sum of mat[o, :] over the row's lookups in batch order; zeros for a row nothing names.
template <int G>
__global__ __launch_bounds__(kBlock) void k_lgcn_dense_grad(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ order,
                                                            const float *__restrict__ mat, int N, int ld, float *__restrict__ Gd) {
  constexpr int gpb = kBlock / G;
  const int lane = threadIdx.x % G;
  const int r = blockIdx.x * gpb + threadIdx.x / G;
  if (r >= N) return;
  const int q1 = row_ptr[r + 1];
  float4 acc[1];
  acc[0] = f4_zero();
  for (int q0 = row_ptr[r]; q0 < q1; q0 += kLgcnFlight) {
    float4 v[kLgcnFlight][1];
#pragma unroll
    for (int q = 0; q < kLgcnFlight; ++q) {
      v[q][0] = f4_zero();
      if (q0 + q < q1) load_row<G, 1>(mat, (size_t)order[q0 + q], ld, lane, v[q]);
    }
#pragma unroll
    for (int q = 0; q < kLgcnFlight; ++q)
      if (q0 + q < q1) f4_add(acc[0], v[q][0]);
  }
  store_row<G, 1>(Gd, (size_t)r, ld, lane, acc);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static bool lgcn_graph_ok(const DrxLgcnGraph *g) {
  return g && g->indptr && g->indices && g->w && g->seg_row && g->seg_ptr && g->N >= 1 && g->N < (1 << 30) && g->n_seg >= g->N &&
         g->n_seg < (1 << 30) && g->n_cut >= 0 && g->n_cut <= g->N && (g->n_cut == 0 || g->cut_rows);
}

static bool lgcn_ld_ok(int ld) { return ld >= 4 && ld <= 256 && !(ld & 3); }

// floats of the partial rows of one propagation (indexed by segment; none where no row is cut)
static size_t lgcn_part_floats(const DrxLgcnGraph &g, int ld) { return g.n_cut ? (size_t)g.n_seg * ld : 0; }

// out = scale (base + A in); everything checked by the caller
static int lgcn_propagate(const DrxLgcnGraph &g, const float *base, const float *in, float *out, float *part, int ld, float scale, hipStream_t st) {
  return dispatch_geom(ld, [&](auto gm) -> int {
    constexpr int G = decltype(gm)::G;
    constexpr int gpb = kBlock / G;
    hipLaunchKernelGGL(k_lgcn_segments<G>, dim3((g.n_seg + gpb - 1) / gpb), dim3(kBlock), 0, st, g, base, in, out, part, ld, scale);
    DRX_LAUNCH_CHECK();
    if (g.n_cut) {
      hipLaunchKernelGGL(k_lgcn_combine<G>, dim3((g.n_cut + gpb - 1) / gpb), dim3(kBlock), 0, st, g, base, out, (const float *)part, ld, scale);
      DRX_LAUNCH_CHECK();
    }
    return DRX_OK;
  });
}

// The Horner recurrence on x (layers >= 1): S <- x, `layers` times S <- x + A S, the last one times 1 / (layers + 1), into `out`; the
// steps before it alternate between tmp and out.  Forward (x = E0) and backward (x = G) are this one function.
static int lgcn_horner(const DrxLgcnGraph &g, const float *x, int layers, float *out, float *tmp, float *part, int ld, hipStream_t st) {
  const float *src = x;
  for (int l = 1; l <= layers; ++l) {
    float *dst = ((layers - l) & 1) ? tmp : out;
    if (int rc = lgcn_propagate(g, x, src, dst, part, ld, l == layers ? 1.0f / (float)(layers + 1) : 1.0f, st)) return rc;
    src = dst;
  }
  return DRX_OK;
}

struct LgcnScratch {
  float *ebar, *x, *y, *gd, *part, *mat;
  int32_t *keys, *rp, *ord;
  double *loss_part;
  void *csr;
  size_t csr_bytes;
  int blocks;
};

static bool lgcn_shape_ok(const DrxLgcnGraph *g, int64_t T, int ld, int n_users) {
  return lgcn_graph_ok(g) && lgcn_ld_ok(ld) && T >= 1 && T < (1 << 27) && n_users >= 1 && n_users < g->N;
}

// carves the step's scratch (ebar first: the forward's final embeddings stay there); false when the description is invalid
static bool lgcn_carve(Carver &cv, const DrxLgcnGraph *g, int T, int ld, int n_users, LgcnScratch &S) {
  if (!lgcn_shape_ok(g, T, ld, n_users)) return false;
  const size_t nl = (size_t)g->N * ld;
  const int gpb = kBlock / pick_geom(ld).G;
  S.blocks = (T + gpb - 1) / gpb;
  S.ebar = cv.take<float>(nl);
  S.x = cv.take<float>(nl);
  S.y = cv.take<float>(nl);
  S.gd = cv.take<float>(nl);
  S.part = cv.take<float>(lgcn_part_floats(*g, ld));
  S.mat = cv.take<float>(3 * (size_t)T * ld);
  S.keys = cv.take<int32_t>(3 * (size_t)T);
  S.rp = cv.take<int32_t>((size_t)g->N + 1);
  S.ord = cv.take<int32_t>(3 * (size_t)T);
  S.loss_part = cv.take<double>((size_t)S.blocks);
  const DrxCsrList ls{S.keys, 3 * T, g->N, S.rp, S.ord};
  S.csr_bytes = drx_batch_csr_device_bytes(&ls, 1);
  if (!S.csr_bytes) return false;
  S.csr = cv.take<char>(S.csr_bytes);
  return true;
}

}  // namespace drx

extern "C" {

int32_t drx_lgcn_row_split(void) { return drx::kLgcnSplit; }

size_t drx_lgcn_part_bytes(const DrxLgcnGraph *graph, int32_t ld) {
  using namespace drx;
  if (!lgcn_graph_ok(graph) || !lgcn_ld_ok(ld)) return 0;
  return lgcn_part_floats(*graph, ld) * sizeof(float) + 16;
}

int drx_lgcn_propagate(const DrxLgcnGraph *graph, const float *base, const float *in, float *out, int32_t ld, float scale, void *part,
                       size_t part_bytes, void *stream) {
  using namespace drx;
  if (!lgcn_graph_ok(graph) || !in || !out || !lgcn_ld_ok(ld) || in == out || base == out) return DRX_EINVAL;
  if (((uintptr_t)base | (uintptr_t)in | (uintptr_t)out | (uintptr_t)part) & 15) return DRX_EINVAL;
  if (graph->n_cut && !part) return DRX_EINVAL;
  if (graph->n_cut && part_bytes < lgcn_part_floats(*graph, ld) * sizeof(float)) return DRX_ESCRATCH;
  return lgcn_propagate(*graph, base, in, out, (float *)part, ld, scale, (hipStream_t)stream);
}

size_t drx_lgcn_final_scratch_bytes(const DrxLgcnGraph *graph, int32_t ld) {
  using namespace drx;
  if (!lgcn_graph_ok(graph) || !lgcn_ld_ok(ld)) return 0;
  Carver cv = step_dry_carver();
  cv.take<float>((size_t)graph->N * ld);
  cv.take<float>(lgcn_part_floats(*graph, ld));
  return step_scratch_total(cv);
}

int drx_lgcn_final(const float *E0, const DrxLgcnGraph *graph, int32_t layers, int32_t ld, float *out, void *scratch, size_t scratch_bytes,
                   void *stream) {
  using namespace drx;
  if (!E0 || !out || !scratch || E0 == out || !lgcn_graph_ok(graph) || !lgcn_ld_ok(ld) || layers < 0 || layers > DRX_LGCN_MAX_LAYERS)
    return DRX_EINVAL;
  if (((uintptr_t)E0 | (uintptr_t)out) & 15) return DRX_EINVAL;
  Carver cv(nullptr, 0);
  if (int rc = step_carver(scratch, scratch_bytes, cv)) return rc;
  float *tmp = cv.take<float>((size_t)graph->N * ld);
  float *part = cv.take<float>(lgcn_part_floats(*graph, ld));
  if (!cv.ok()) return DRX_ESCRATCH;
  if (layers == 0) {
    DRX_HIP(hipMemcpyAsync(out, E0, (size_t)graph->N * ld * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return DRX_OK;
  }
  return lgcn_horner(*graph, E0, layers, out, tmp, part, ld, (hipStream_t)stream);
}

size_t drx_lgcn_step_scratch_bytes(const DrxLgcnGraph *graph, int32_t T, int32_t ld, int32_t n_users) {
  using namespace drx;
  Carver cv = step_dry_carver();
  LgcnScratch S;
  return lgcn_carve(cv, graph, T, ld, n_users, S) ? step_scratch_total(cv) : 0;
}

int drx_lgcn_step(float *E0, float *P_s1, float *P_s2, float *Q_s1, float *Q_s2, int32_t ld, int32_t n_users, const DrxLgcnGraph *graph,
                  const int32_t *uid, const int32_t *pos, const int32_t *neg, int32_t T, int32_t layers, const DrxOptRule *rule,
                  const float *alphas, float reg, double *loss_out, void *scratch, size_t scratch_bytes, void *stream) {
  using namespace drx;
  if (!E0 || !uid || !pos || !neg || !rule || !alphas || !scratch || !lgcn_shape_ok(graph, T, ld, n_users) || layers < 0 ||
      layers > DRX_LGCN_MAX_LAYERS)
    return DRX_EINVAL;
  const int N = graph->N;
  const size_t nu = (size_t)n_users * ld, ni = (size_t)(N - n_users) * ld;
  StepTensor t[2] = {{E0, P_s1, P_s2}, {E0 + nu, Q_s1, Q_s2}};
  if (!step_tensors_ok(rule->kind, t, 2, 2)) return DRX_EINVAL;
  Carver cv(nullptr, 0);
  if (int rc = step_carver(scratch, scratch_bytes, cv)) return rc;
  LgcnScratch S;
  if (!lgcn_carve(cv, graph, T, ld, n_users, S)) return DRX_EINVAL;
  if (!cv.ok()) return DRX_ESCRATCH;
  hipStream_t st = (hipStream_t)stream;
  // 1. the final embeddings (layers == 0: E0 itself)
  const float *ebar = E0;
  if (layers > 0) {
    if (int rc = lgcn_horner(*graph, E0, layers, S.ebar, S.x, S.part, ld, st)) return rc;
    ebar = S.ebar;
  }
  // 2. the triples
  int rc = dispatch_geom(ld, [&](auto gm) -> int {
    constexpr int G = decltype(gm)::G;
    hipLaunchKernelGGL(k_lgcn_fwd_bwd<G>, dim3(S.blocks), dim3(kBlock), 0, st, ebar, ld, n_users, uid, pos, neg, T, S.mat, S.keys, S.loss_part);
    DRX_LAUNCH_CHECK();
    return DRX_OK;
  });
  if (rc) return rc;
  if (loss_out) hipLaunchKernelGGL(k_loss_mean<>, dim3(1), dim3(64), 0, st, S.loss_part, S.blocks, (double)T, loss_out);
  // 3. G, dense
  const DrxCsrList ls{S.keys, 3 * T, N, S.rp, S.ord};
  rc = drx_batch_csr_device(&ls, 1, S.csr, S.csr_bytes, stream);
  if (rc) return rc;
  rc = dispatch_geom(ld, [&](auto gm) -> int {
    constexpr int G = decltype(gm)::G;
    constexpr int gpb = kBlock / G;
    hipLaunchKernelGGL(k_lgcn_dense_grad<G>, dim3((N + gpb - 1) / gpb), dim3(kBlock), 0, st, S.rp, S.ord, S.mat, N, ld, S.gd);
    DRX_LAUNCH_CHECK();
    return DRX_OK;
  });
  if (rc) return rc;
  // 4. dE0 (layers == 0: G itself)
  const float *dE0 = S.gd;
  if (layers > 0) {
    if ((rc = lgcn_horner(*graph, S.gd, layers, S.x, S.y, S.part, ld, st))) return rc;
    dE0 = S.x;
  }
  // 5. the dense rule on the two halves, each with its step size
  DrxOptRule r = *rule;
  r.lr = alphas[0];
  if ((rc = drx_opt_dense(t[0].p, t[0].s1, t[0].s2, dE0, (int64_t)nu, &r, reg, stream))) return rc;
  r.lr = alphas[1];
  return drx_opt_dense(t[1].p, t[1].s1, t[1].s2, dE0 + nu, (int64_t)ni, &r, reg, stream);
}

}  // extern "C"
