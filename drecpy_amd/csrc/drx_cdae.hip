// CDAE, the sampled step, for MI355X (gfx950): one (user, item, label) triple per row group — embedding-bag hidden layer, ONE output
// unit, Keras BCE/MSE, backward, and the sparse Adagrad / Adam updates of the rows the batch touched through the segmented reduction
// (drx_segreduce.hpp / drx_segstream.hpp) over the prepared touch list (drx_prep.hpp); the column-sharded step's two halves; the hot
// head.  This file and the headers it includes hold every line of device code a sampled step executes, and nothing else:
//   reference ("dense") mode and inference    drx_cdae_dense.hip
//   the touch list prepared in parts          drx_cdae_parts.hip
//   version, error strings, events, streams   drx_runtime.hip
//   the input-bag gather both modes share     drx_rows.hpp (gather_bag)
//
// Replaces, per fit() iteration, the TensorFlow eager ops issued by DRecPy/Recommender/cdae.py:50-82 and
// DRecPy/Recommender/recommender_abc.py:190-204,328-334 (see include/drx.h for the per-entry mapping).
//
// Thread geometry: a table row (ld floats) is owned by a GROUP of G lanes (G = 8..64, power of two,
// sub-wave), each lane holding J float4 -> one coalesced 16 B/lane access per row; K=128 is a half-wave
// (two rows per wave64), K=50 (ld 52) a 16-lane group (four rows per wave).
#include "drx_common.hpp"
#include "drx_rows.hpp"
#include "drx_segreduce.hpp"
#include <cstring>
#include "drx_scan.hpp"
#include "drx_prep.hpp"
#include "drx_segstream.hpp"
#include "drx_cdae_host.hpp"
#include <type_traits>
#include <mutex>
#include <unordered_map>

#ifdef DRX_STAMPS
static unsigned long long *h_stamps = nullptr;       // device buffer [110000 x 16], handed to the sparse step's kernels in their arguments
extern "C" int drx_debug_set_stamps(unsigned long long *buf, unsigned int) { h_stamps = buf; return 0; }
#endif

namespace drx {

// ------------------------------------------------------------------------------------------------
// sampled-output mode: one group per (u, i, y) triple — gather, hidden, one output unit, loss,
// backward to dz1 / g2 rows, and the (row key, sample) touch list for the inverted index.
// key space: [0,N) W rows, [N,2N) W2T rows, [2N, 2N+U) V rows.
// ------------------------------------------------------------------------------------------------
struct SparseBufs {
  float *dz1;       // [B, ld]
  float *g2;        // [B, ld]  dz2_b * h_b
  float *dz2;       // [B]
  float *lossb;     // [B]
  float *phead, *ptail;                       // [n_chunks, ld]
  float *phs, *pts;                           // [n_chunks] scalar (b2) partials
  float *pblock, *pbs;                        // [n_blocks, ld], [n_blocks]: partials of all-inner workgroups (k_seg_reduce_planned)
  float *bpart;                               // [n_bpart, ld]
  const uint8_t *solo_v, *solo_o;             // [B] each or nullptr: sample b is the ONLY toucher of its V / W2T row
  unsigned long long *stamps;                 // diagnostic builds (DRX_STAMPS) only
  const int32_t *order;                       // [B] or nullptr: launch order of the forward kernel's triples (k_order_by_degree)
  // DRX_BATCH_SHARE_USERS (k_items_fwd_bwd): the batch's work items (drx_prep.hpp PrepBufs); dz1 then holds B more rows behind the
  // samples': the items' summed gradients.  Else nullptr.
  const int32_t *usamp, *worder, *n_items;
  const WorkItem *witem;
  int T, n_chunks, n_bpart;
};

template <int G, int J, int KIND = -1>
__device__ __forceinline__ void sparse_apply(const DrxCdaeParams &P, const DrxOptim &opt, int B, uint32_t key, int lane,
                                             const float4 (&g)[J], float gs) {
  const uint32_t N = (uint32_t)P.n_items;
  // read every candidate pointer as a scalar first, then select VALUES (a dynamic index into the kernarg pointer
  // arrays would become a vector load + s_waitcnt vmcnt(0))
  float *const tW = P.W, *const tO = P.W2T, *const tV = P.V;
  float *const a0 = opt.s1[0], *const a1 = opt.s1[1], *const a2 = opt.s1[2];
  float *const c0 = opt.s2[0], *const c1 = opt.s2[1], *const c2 = opt.s2[2];
  const int var = key < N ? 0 : (key < 2 * N ? 1 : 2);
  const size_t row = key - (uint32_t)var * N;
  float *const tab = var == 0 ? tW : (var == 1 ? tO : tV);
  float *const s1 = var == 0 ? a0 : (var == 1 ? a1 : a2);
  float *const s2 = var == 0 ? c0 : (var == 1 ? c1 : c2);
  OptScalars o = opt_for(opt, 0, B);
  o.inv_k = 1.0f / (float)P.k;
  float4 w[J];
  load_row<G, J>(tab, row, P.ld, lane, w);
  row_update<G, J, KIND>(o, tab, s1, s2, row, P.ld, lane, w, g);
  if (var == 1 && lane == 0) {
    const int kind = KIND >= 0 ? KIND : o.kind;
    float pb = P.b2[row], m = opt.s1[4][row], v = kind == DRX_OPT_ADAM ? opt.s2[4][row] : 0.f;
    o.rb = 0.f;
    opt_update1<KIND>(o, gs, pb, m, v);
    P.b2[row] = pb; opt.s1[4][row] = m;
    if (kind == DRX_OPT_ADAM) opt.s2[4][row] = v;
  }
}

// One triple after its input bag is known, in two halves.  sampled_hidden: hidden layer and the dot product with the
// sampled output row (on the columns this table holds).  sampled_rest: loss, backward, gradient rows (and the in-place update
// of rows only this triple touches) from the COMPLETE dot product — the same value in the single-GPU step, the sum over ranks
// of the partial dots in the column-sharded one.
template <int G, int J>
__device__ __forceinline__ float sampled_hidden(const DrxCdaeParams &P, const DrxBatch &bt, float scale, int b, int lane,
                                                const float4 (&acc)[J], float4 (&h)[J], float4 (&w2)[J]) {
  hidden_act<G, J>(P, bt.uid[b], scale, lane, acc, h);
  load_row<G, J>(P.W2T, (size_t)bt.iid[b], P.ld, lane, w2);
  float d = 0.f;
#pragma unroll
  for (int j = 0; j < J; ++j) d += f4_dot(w2[j], h[j]);
  return group_sum<G>(d);
}

template <int G, int J, int KIND = -1>
__device__ __forceinline__ void sampled_rest(const DrxCdaeParams &P, const DrxOptim &opt, const DrxHistory &H, const DrxBatch &bt,
                                             float scale, uint32_t qthr, int loss_kind, const SparseBufs &S, int b, int lane,
                                             float d, const float4 (&h)[J], const float4 (&w2)[J],
                                             float4 (*dz1_out)[J] = nullptr) {
  const int u = bt.uid[b], i = bt.iid[b];
  const float y = bt.y[b];
  const float p = sigmoidf_(d + P.b2[i]);
  const float invB = 1.0f / (float)bt.B;
  float lval, dp;
  if (loss_kind == DRX_LOSS_BCE) { lval = bce_elem(y, p); dp = bce_grad(y, p) * invB; }
  else { lval = (p - y) * (p - y); dp = 2.0f * (p - y) * invB; }
  const float dz2 = dp * p * (1.0f - p);
  float4 dz1[J], g2[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    dz1[j].x = dz2 * w2[j].x * h[j].x * (1.0f - h[j].x); dz1[j].y = dz2 * w2[j].y * h[j].y * (1.0f - h[j].y);
    dz1[j].z = dz2 * w2[j].z * h[j].z * (1.0f - h[j].z); dz1[j].w = dz2 * w2[j].w * h[j].w * (1.0f - h[j].w);
    g2[j].x = dz2 * h[j].x; g2[j].y = dz2 * h[j].y; g2[j].z = dz2 * h[j].z; g2[j].w = dz2 * h[j].w;
  }
  store_row<G, J>(S.dz1, (size_t)b, P.ld, lane, dz1);
  if (lane == 0) S.lossb[b] = lval;
  const uint8_t *const pv = S.solo_v, *const po = S.solo_o;
  const bool solo_v = pv && pv[b], solo_o = po && po[b];
  if (solo_o) {      // this sample alone touches W2T[i] and b2[i]: update them here (same arithmetic as the segment path)
    sparse_apply<G, J, KIND>(P, opt, bt.B, (uint32_t)P.n_items + (uint32_t)i, lane, g2, dz2);
  } else {
    store_row<G, J>(S.g2, (size_t)b, P.ld, lane, g2);
    if (lane == 0) S.dz2[b] = dz2;
  }
  if (solo_v) sparse_apply<G, J, KIND>(P, opt, bt.B, 2u * (uint32_t)P.n_items + (uint32_t)u, lane, dz1, 0.f);
  if (dz1_out) {
#pragma unroll
    for (int j = 0; j < J; ++j) (*dz1_out)[j] = dz1[j];
  }
}

template <int G, int J, int KIND = -1>
__device__ __forceinline__ void sampled_finish(const DrxCdaeParams &P, const DrxOptim &opt, const DrxHistory &H, const DrxBatch &bt,
                                               float scale, uint32_t qthr, int loss_kind, const SparseBufs &S, int b, int lane,
                                               const float4 (&acc)[J]) {
  float4 h[J], w2[J];
#ifdef DRX_STAMPS
  if (acc[0].x == acc[0].x) DRX_STAMP(S.stamps, b, 5, lane);          // (uses acc: behind the gather)
#endif
  const float d = sampled_hidden<G, J>(P, bt, scale, b, lane, acc, h, w2);
#ifdef DRX_STAMPS
  if (d == d) DRX_STAMP(S.stamps, b, 6, lane);                        // (uses d: V[u], b and W2T[i] have landed)
#endif
  sampled_rest<G, J, KIND>(P, opt, H, bt, scale, qthr, loss_kind, S, b, lane, d, h, w2);
  DRX_STAMP(S.stamps, b, 7, lane);                                    // (behind the stores of the in-place updates)
}

// ---- column-sharded ("K-sharded") step: the two halves as kernels of their own, the all-reduce of dot[] between them ----------
template <int G, int J>
__global__ __launch_bounds__(kBlock) void k_kshard_fwd(DrxCdaeParams P, DrxHistory H, DrxBatch bt, float scale, uint32_t qthr,
                                                       float *__restrict__ h_out, float *__restrict__ dot_out,
                                                       const int32_t *__restrict__ order) {
  const int lane = threadIdx.x % G;
  const int slot = blockIdx.x * (kBlock / G) + threadIdx.x / G;
  if (slot >= bt.B) return;
  const int b = order ? order[slot] : slot;        // longest histories first, similar lengths side by side (k_degree_counts)
  float4 acc[J], h[J], w2[J];
  DenseAux none{};
  gather_bag<G, J, 0>(P, H, bt, qthr, b, lane, acc, none, nullptr, nullptr, 0);
  const float d = sampled_hidden<G, J>(P, bt, scale, b, lane, acc, h, w2);
  store_row<G, J>(h_out, (size_t)b, P.ld, lane, h);
  if (lane == 0) dot_out[b] = d;
}

// (long histories / small batches: one workgroup per triple, like k_sampled_fwd_bwd_wg)
template <int G, int J>
__global__ __launch_bounds__(kBlock) void k_kshard_fwd_wg(DrxCdaeParams P, DrxHistory H, DrxBatch bt, float scale, uint32_t qthr,
                                                          float *__restrict__ h_out, float *__restrict__ dot_out) {
  extern __shared__ __align__(16) float lds[];   // [R, ld]
  constexpr int R = kBlock / G;
  const int lane = threadIdx.x % G, r = threadIdx.x / G;
  const int b = blockIdx.x;
  float4 acc[J], h[J], w2[J];
  DenseAux none{};
  gather_bag<G, J, 0>(P, H, bt, qthr, b, lane, acc, none, nullptr, nullptr, 0, r, R);
  store_row<G, J>(lds, (size_t)r, P.ld, lane, acc);
  __syncthreads();
  if (r != 0) return;
#pragma unroll
  for (int j = 0; j < J; ++j) acc[j] = f4_zero();
#pragma unroll 8
  for (int rr = 0; rr < R; ++rr) {
    float4 v[J];
    load_row<G, J>(lds, (size_t)rr, P.ld, lane, v);
#pragma unroll
    for (int j = 0; j < J; ++j) f4_add(acc[j], v[j]);
  }
  const float d = sampled_hidden<G, J>(P, bt, scale, b, lane, acc, h, w2);
  store_row<G, J>(h_out, (size_t)b, P.ld, lane, h);
  if (lane == 0) dot_out[b] = d;
}

template <int G, int J>
__global__ __launch_bounds__(kBlock) void k_kshard_rest(DrxCdaeParams P, DrxOptim opt, DrxHistory H, DrxBatch bt, float scale,
                                                        uint32_t qthr, int loss_kind, SparseBufs S,
                                                        const float *__restrict__ h_in, const float *__restrict__ dot_total) {
  const int lane = threadIdx.x % G;
  const int b = blockIdx.x * (kBlock / G) + threadIdx.x / G;
  if (b >= bt.B) return;
  float4 h[J], w2[J];
  load_row<G, J>(h_in, (size_t)b, P.ld, lane, h);
  load_row<G, J>(P.W2T, (size_t)bt.iid[b], P.ld, lane, w2);
  sampled_rest<G, J>(P, opt, H, bt, scale, qthr, loss_kind, S, b, lane, dot_total[b], h, w2);
}

template <int G, int J, int KIND = -1>
__global__ __launch_bounds__(kBlock) void k_sampled_fwd_bwd(DrxCdaeParams P, DrxOptim opt, DrxHistory H, DrxBatch bt, float scale,
                                                            uint32_t qthr, int loss_kind, SparseBufs S) {
  const int lane = threadIdx.x % G;
  const int slot = blockIdx.x * (kBlock / G) + threadIdx.x / G;
#ifdef DRX_STAMPS
  const unsigned long long t_in = wall_clock64();
#endif
  if (slot >= bt.B) return;
  const int32_t *const ord = S.order;
  const int b = ord ? ord[slot] : slot;            // longest histories first, similar lengths side by side (k_degree_counts)
  float4 acc[J];
  DenseAux none{};
#ifdef DRX_STAMPS
  if (lane == 0 && S.stamps && (unsigned)b < 110000u) S.stamps[(size_t)b * 16] = t_in;          // stamp 0: the group's start
  if (bt.uid[b] >= 0) DRX_STAMP(S.stamps, b, 1, lane);                                           // (uses uid: it has landed)
#endif
  gather_bag<G, J, 0>(P, H, bt, qthr, b, lane, acc, none, nullptr, nullptr, 0, 0, 1, S.stamps);
  sampled_finish<G, J, KIND>(P, opt, H, bt, scale, qthr, loss_kind, S, b, lane, acc);
}

// DRX_BATCH_SHARE_USERS: one WORKGROUP per work item — up to kShareTriples (16) triples of ONE user (drx_prep.hpp k_tp_item_*).
// Every row of the user's history is loaded ONCE for all the item's triples (the plain kernel: once per triple):
//   A. the bags of the item's triples are a small masked matrix product [16 triples x history] x [history x K]: the workgroup's waves
//      split the history, 16 rows per wave and round, and v_mfma_f32_16x16x4_f32 adds them into the 16 bags under the 0 / 1 keep
//      coefficients — fp32 products with 0 or 1 are exact; the sums run in the instruction's fixed order.  The coefficient a lane
//      feeds the instruction is the one (triple, row) pair whose mask bit it evaluates: no ballot, no broadcast;
//   B. the waves' partial bags meet in LDS; row group r (the G x J geometry of every other kernel) sums those of triples r, r + R, ...
//      in wave order, then forward / loss / backward as in k_sampled_fwd_bwd;
//   C. the item's summed gradient row dz1[B + item] = sum of its triples' dz1 (per group, then in group order): what the touch
//      list's shared entries (sample field B + item) name.
// At the ml-1m shape (6 040 users, 65 536 triples: 11 per user, 165 rows per history) the plain kernel gathers 8.6 M rows in 350 us;
// summing every user's rows once and subtracting each triple's dropped rows (4.1 M rows): 222 us; the masked product on the vector
// ALUs (a v_readlane + a packed FMA per row and triple: the kernel was bound by instruction issue): 200 us.
template <int G, int J, int KIND = -1>
__global__ __launch_bounds__(kItemThreads, (4 * G * J <= 128 ? 5 : 1)) void k_items_fwd_bwd(DrxCdaeParams P, DrxOptim opt, DrxHistory H, DrxBatch bt, float scale,
                                                          uint32_t qthr, int loss_kind, SparseBufs S) {
  extern __shared__ __align__(16) float lds[];   // [NWV * RT, ld] floats, then RT sample ids
  constexpr int R = kItemThreads / G, NWV = kItemThreads / 64, RT = kShareTriples;
  constexpr int NH = 4 * G * J / 64;                               // blocks of 64 columns of a row
  static_assert(NH >= 1 && NH <= 8 && RT == 16, "rows of 64 .. 512 floats; the 16 x 16 x 4 matrix instruction");
  constexpr int NF = NH <= 2 ? 16 : (NH == 4 ? 8 : 4);             // rows in flight per wave
  constexpr int TPG = (RT + R - 1) / R;                            // triples per row group in B
  if ((int)blockIdx.x >= S.n_items[0]) return;
  const int w = S.worder[blockIdx.x];              // longest histories first
  const WorkItem wi = S.witem[w];
  const int p0 = wi.p0, n = wi.n, u = wi.user;
  const int64_t s = wi.hist_start, e = s + wi.deg;
  const int lane = threadIdx.x % G, r = threadIdx.x / G;
  int *lb = (int *)(lds + (size_t)NWV * RT * P.ld);
  if ((int)threadIdx.x < RT) lb[threadIdx.x] = (int)threadIdx.x < n ? S.usamp[p0 + threadIdx.x] : 0;
  // the user's row of V (B needs it, not the bags): under way before A's rounds
  float4 vrow[J];
  load_row<G, J>(P.V, (size_t)u, P.ld, lane, vrow);
  const int n_waves = (int)min((int64_t)NWV, (e - s + NF - 1) / NF);         // waves that have rows at all
  {  // A
    // v_mfma_f32_16x16x4_f32 per (4 rows, 16 columns): A[m][k] = the keep coefficient of (triple m, row k) — lane l supplies
    // A[l % 16][l / 16], the very pair whose mask bit it evaluates; B[k][n] = lane l's column of row k = l / 16.  A lane loads float4s
    // (columns 64 h + 4 (l % 16) ...), so the tile of (h, j) holds columns 64 h + 4 n + j: C[4 (l / 16) + i][l % 16] in register i.
    typedef float f4v __attribute__((ext_vector_type(4)));
    const int wl = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int kr = wl >> 4, nc = wl & 15;            // this lane's row of a group of 4, its triple (A) / its column quad (B)
    f4v acc[NH][4];
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[h][j] = f4v{0.f, 0.f, 0.f, 0.f};
    const int64_t c0 = s + (int64_t)wv * NF;
    int ridx[NF / 4];
#pragma unroll
    for (int g = 0; g < NF / 4; ++g) ridx[g] = c0 + 4 * g + kr < e ? H.indices[c0 + 4 * g + kr] : 0;
    __syncthreads();                                 // (lb)
    const int bmine = lb[nc];
    for (int64_t c = c0; c < e; c += (int64_t)NWV * NF) {
      const int64_t cn = c + (int64_t)NWV * NF;
      int ridx_n[NF / 4];
#pragma unroll
      for (int g = 0; g < NF / 4; ++g) ridx_n[g] = cn + 4 * g + kr < e ? H.indices[cn + 4 * g + kr] : 0;      // (under way while this round's rows are)
      float4 bv[NF / 4][NH];
#pragma unroll
      for (int g = 0; g < NF / 4; ++g)
#pragma unroll
        for (int h = 0; h < NH; ++h) {
          bv[g][h] = f4_zero();
          if (c + 4 * g + kr < e && 64 * h + 4 * nc < P.ld)
            bv[g][h] = *reinterpret_cast<const float4 *>(P.W + (size_t)ridx[g] * P.ld + 64 * h + 4 * nc);
        }
#pragma unroll
      for (int g = 0; g < NF / 4; ++g) {
        const int64_t row = c + 4 * g + kr;
        bool kf = false;
        if (nc < n && row < e) {
          const uint32_t jj = (uint32_t)(row - s);
          kf = bt.keep ? (bt.keep[bt.keep_off[bmine] + jj] != 0) : (hash_u32(bt.mask_seed, (uint32_t)bmine, jj) >= qthr);
        }
        const float a = kf ? 1.0f : 0.0f;
#pragma unroll
        for (int h = 0; h < NH; ++h) {
          acc[h][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[g][h].x, acc[h][0], 0, 0, 0);
          acc[h][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[g][h].y, acc[h][1], 0, 0, 0);
          acc[h][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[g][h].z, acc[h][2], 0, 0, 0);
          acc[h][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[g][h].w, acc[h][3], 0, 0, 0);
        }
      }
#pragma unroll
      for (int g = 0; g < NF / 4; ++g) ridx[g] = ridx_n[g];
    }
    if (wv < n_waves) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = 4 * kr + i;
        if (t < n) {
#pragma unroll
          for (int h = 0; h < NH; ++h)
            if (64 * h + 4 * nc < P.ld)
              *reinterpret_cast<float4 *>(lds + (size_t)(wv * RT + t) * P.ld + 64 * h + 4 * nc) =
                  make_float4(acc[h][0][i], acc[h][1][i], acc[h][2][i], acc[h][3][i]);
        }
      }
    }
  }
  __syncthreads();
  // B
  float4 dsum[J];
#pragma unroll
  for (int j = 0; j < J; ++j) dsum[j] = f4_zero();
#pragma unroll
  for (int kt = 0; kt < TPG; ++kt) {
    const int t = r + kt * R;
    if (t < n) {
      const int b = lb[t];
      float4 acc[J], h[J], w2[J], dz1[J];
#pragma unroll
      for (int j = 0; j < J; ++j) acc[j] = f4_zero();
      for (int wv = 0; wv < n_waves; ++wv) {
        float4 x[J];
        load_row<G, J>(lds, (size_t)(wv * RT + t), P.ld, lane, x);
#pragma unroll
        for (int j = 0; j < J; ++j) f4_add(acc[j], x[j]);
      }
      float4 brow[J];
      load_row<G, J>(P.b, 0, P.ld, lane, brow);
      hidden_act_rows<G, J>(P, scale, lane, acc, vrow, brow, h);
      load_row<G, J>(P.W2T, (size_t)bt.iid[b], P.ld, lane, w2);
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < J; ++j) d += f4_dot(w2[j], h[j]);
      d = group_sum<G>(d);
      sampled_rest<G, J, KIND>(P, opt, H, bt, scale, qthr, loss_kind, S, b, lane, d, h, w2, &dz1);
#pragma unroll
      for (int j = 0; j < J; ++j) f4_add(dsum[j], dz1[j]);
    }
  }
  // C
  __syncthreads();                                   // (every group has read its partial bags)
  if (r < n) store_row<G, J>(lds, (size_t)r, P.ld, lane, dsum);
  __syncthreads();
  if (r == 0) {
    float4 t[J];
#pragma unroll
    for (int j = 0; j < J; ++j) t[j] = f4_zero();
    for (int rr = 0; rr < min(n, R); ++rr) {
      float4 x[J];
      load_row<G, J>(lds, (size_t)rr, P.ld, lane, x);
#pragma unroll
      for (int j = 0; j < J; ++j) f4_add(t[j], x[j]);
    }
    store_row<G, J>(S.dz1, (size_t)bt.B + w, P.ld, lane, t);
  }
}

// Small batches of long histories (ml-1m: 155 items per user, B of a few thousand): with one group per triple the gather is
// a chain of ~20 dependent load rounds on a chip that is mostly idle (measured 143 us at B = 4096).  Here one WORKGROUP
// takes a triple: its 256/G groups split the history, the partial bags are summed in LDS in group order.
template <int G, int J>
__global__ __launch_bounds__(kBlock) void k_sampled_fwd_bwd_wg(DrxCdaeParams P, DrxOptim opt, DrxHistory H, DrxBatch bt, float scale,
                                                               uint32_t qthr, int loss_kind, SparseBufs S) {
  extern __shared__ __align__(16) float lds[];   // [R, ld]
  constexpr int R = kBlock / G;
  const int lane = threadIdx.x % G, r = threadIdx.x / G;
  const int b = blockIdx.x;
  float4 acc[J];
  DenseAux none{};
  gather_bag<G, J, 0>(P, H, bt, qthr, b, lane, acc, none, nullptr, nullptr, 0, r, R);
  store_row<G, J>(lds, (size_t)r, P.ld, lane, acc);
  __syncthreads();
  if (r != 0) return;
#pragma unroll
  for (int j = 0; j < J; ++j) acc[j] = f4_zero();
#pragma unroll 8
  for (int rr = 0; rr < R; ++rr) {
    float4 v[J];
    load_row<G, J>(lds, (size_t)rr, P.ld, lane, v);
#pragma unroll
    for (int j = 0; j < J; ++j) f4_add(acc[j], v[j]);
  }
  sampled_finish<G, J>(P, opt, H, bt, scale, qthr, loss_kind, S, b, lane, acc);
}

// Policy of the single-GPU sparse step for the generic segmented reduction (drx_segreduce.hpp):
// key space [0,N) W rows (contribution dz1[b] * 1/(1-q)), [N,2N) W2T rows (g2[b], scalar dz2[b] for b2), [2N,2N+U) V rows.
template <int KIND>
struct DirectPolicyT {
  DrxCdaeParams P;
  DrxOptim opt;
  int B;
  float scale;
  // contribution rows: dz1 [B,ld] and g2 [B,ld]; g2 is addressed as dz1 + g2_off so that the choice between them is
  // a VALUE select (a select between the two kernarg pointer FIELDS makes hipcc fetch the pointer with a vector load
  // and an s_waitcnt vmcnt(0) in front of every row load, which serialises the loads: measured 0.26 -> 0.33 ms)
  const float *dz1;
  long long g2_off;
  const float *dz2;
  template <int G, int J>
  __device__ __forceinline__ void load(uint32_t key, uint32_t bv, int lane, float4 (&row)[J], float &sc, float &coef) const {
    const uint32_t N = (uint32_t)P.n_items;
    const bool is_out = key >= N && key < 2 * N;
    // (DRX_BATCH_SHARE_USERS lists: the top bit of a W touch's sample field says "subtract"; fields >= B name a user's summed row,
    // stored behind the samples' rows)
    const uint32_t b = bv & 0x7FFFFFFFu;
    load_row<G, J>(dz1 + (is_out ? g2_off : 0ll), (size_t)b, P.ld, lane, row);
    if (is_out) sc = dz2[b];
    coef = key < N ? ((bv >> 31) ? -scale : scale) : 1.0f;
  }
  template <int G, int J>
  __device__ __forceinline__ void finish(uint32_t key, int, int lane, const float4 (&g)[J], float gs) const {
    sparse_apply<G, J, KIND>(P, opt, B, key, lane, g, gs);
  }
  // what the streamed reduction (drx_segstream.hpp) needs to know — the key space as three row arrays: W rows (touches carry the sample
  // whose dz1 row they add, with the coefficient 1/(1-q)), W2T rows (g2 rows, coefficient 1, and the scalar dz2 for the output bias),
  // V rows (dz1 rows, coefficient 1); the optimizer is element-wise with one slot (Adagrad: KIND says so at compile time); a row's
  // own value enters its gradient with reg/B (sparse_apply -> row_update), the output bias's does not
  static constexpr bool kStreamParks = false;                  // every finished row is applied to its table
  __device__ __forceinline__ StreamArrays stream_arrays() const {
    const uint32_t N = (uint32_t)P.n_items;
    return StreamArrays{{0u, N, 2u * N}, {dz1, dz1 + g2_off, dz1}, {P.W, P.W2T, P.V}, {opt.s1[0], opt.s1[1], opt.s1[2]},
                        {scale, 1.0f, 1.0f}, {nullptr, dz2, nullptr}, {nullptr, P.b2, nullptr}, {nullptr, opt.s1[4], nullptr}};
  }
  __device__ __forceinline__ float stream_decay() const { return opt.reg_rate / (float)B; }
  __device__ __forceinline__ void stream_update(float g, float &p, float &a) const {
    static_assert(KIND == DRX_OPT_ADAGRAD || KIND < 0, "one slot per element");
    OptScalars o = opt_for(opt, 0, B);
    float unused = 0.f;
    opt_update1<DRX_OPT_ADAGRAD>(o, g, p, a, unused);
  }
  __device__ __forceinline__ void stream_update_scalar(float g, float &p, float &a) const { stream_update(g, p, a); }      // sparse_apply's output-bias half
};
using DirectPolicy = DirectPolicyT<-1>;                      // optimizer chosen at run time
using DirectPolicyAdagrad = DirectPolicyT<DRX_OPT_ADAGRAD>;  // the throughput configuration's optimizer, known at compile time

template <int G, int J, int NT>
__device__ __forceinline__ void bias_final_body(const DrxCdaeParams &P, const DrxOptim &opt, const BiasArgs &A,
                                                float *lds /* [NT/G, ld] */, float *red) {
  constexpr int R = NT / G;
  const int lane = threadIdx.x % G, r = threadIdx.x / G;
  float4 acc[J];
#pragma unroll
  for (int j = 0; j < J; ++j) acc[j] = f4_zero();
  constexpr int NB = J == 1 ? 8 : 2;
  for (int i = r; i < A.n_part; i += NB * R) {
    float4 v[NB][J];
#pragma unroll
    for (int q = 0; q < NB; ++q) {
#pragma unroll
      for (int j = 0; j < J; ++j) v[q][j] = f4_zero();
      if (i + q * R < A.n_part) load_row<G, J>(A.part, (size_t)(i + q * R), P.ld, lane, v[q]);
    }
#pragma unroll
    for (int q = 0; q < NB; ++q)
#pragma unroll
      for (int j = 0; j < J; ++j) f4_add(acc[j], v[q][j]);
  }
  store_row<G, J>(lds, (size_t)r, P.ld, lane, acc);
  __syncthreads();
  if (r == 0) {
    float4 g[J], w[J];
#pragma unroll
    for (int j = 0; j < J; ++j) g[j] = f4_zero();
#pragma unroll 8
    for (int rr = 0; rr < R; ++rr) {
      float4 v[J];
      load_row<G, J>(lds, (size_t)rr, P.ld, lane, v);
#pragma unroll
      for (int j = 0; j < J; ++j) f4_add(g[j], v[j]);
    }
    load_row<G, J>(P.b, 0, P.ld, lane, w);
    OptScalars o = opt_for(opt, 0, A.B);
    if (o.kind == DRX_OPT_ROWWISE_ADAGRAD) o.kind = DRX_OPT_ADAGRAD;      // the bias vectors keep one accumulator per element
    o.rb = 0.f;
    row_update<G, J>(o, P.b, opt.s1[3], opt.s2[3], 0, P.ld, lane, w, g);
  }
  if (A.loss_out) {   // mean of the per-sample losses from the per-block partials, fixed order
    const float *lp = A.part + (size_t)A.n_part * P.ld;
    float a = 0.f;
    for (int b = threadIdx.x; b < A.n_part; b += NT) a += lp[b];
    float t = block_sum(a, red);
    if (threadIdx.x == 0) { A.loss_out[0] = t / (float)A.B; A.loss_out[1] = 0.f; }
  }
}

// The two stages of the hidden-bias gradient ride along with the planned segmented reduction (drx_segreduce.hpp): the column-sum
// partials of dz1 as extra workgroups of k_seg_reduce_planned (they depend on the forward kernel only), the final sum + update of b
// (+ the mean loss) as one extra workgroup of k_span_planned.  The sparse step is three launches: forward/backward, reduction, spans.
template <int G, int J>
struct BiasFinalExtra {
  DrxCdaeParams P;
  DrxOptim opt;
  BiasArgs A;
  __device__ __forceinline__ void operator()(float *lds) const {
    __shared__ float red[kFixBlock / 64];
    bias_final_body<G, J, kFixBlock>(P, opt, A, lds, red);
  }
};

// ------------------------------------------------------------------------------------------------
// The HOT HEAD (include/drx.h DrxHotHead): the W rows of the H hottest items take no part in the touch list; their gradients are the
// dense product (1/(1-q)) * M^T * dz1 of the batch's transposed 0/1 kept-mask M [H, B] (k_sparse_touches) with dz1 [B, ld], read once
// as a stream instead of one random row gather per touch.  Two stages riding in the launches the step already has:
//   partials: extra workgroups of k_seg_reduce_stream — one WAVE per (slice of kHotSlice samples, strip of 16 columns, group of up to 64
//             hot rows): up to four 16 x 16 tiles of P[s] = M_slice^T * dz1_slice on v_mfma_f32_16x16x32_bf16, so dz1 is read ONCE per
//             row group (H <= 64: once).  dz1 is split exactly into hi + mid + lo bf16 (8 significant bits each: 24 = the fp32
//             significand), so three MFMAs per k-step and tile sum the fp32 values; a 0/1 A operand is exact in bf16; accumulation is
//             fp32.  16 accumulators per lane: the launch keeps its 64-VGPR budget.  The waves of row group 0 hold every dz1 element of
//             their (slice, strip) in registers: they also leave the slice's column sums — the hidden bias's partials, BiasArgs::part
//             with a head — and the wave of strip 0 the slice's loss partial; the launch carries no BiasPartialExtra workgroups then;
//   finish:   extra workgroups of k_span_planned — one per hot row: the slices' partials summed in a fixed order, the row's Adagrad
//             update as the segment path's (DirectPolicyAdagrad::stream_update); rows no sample kept are not touched.
// ------------------------------------------------------------------------------------------------
constexpr int kHotSlice = 512;       // samples per partial (P: [B / kHotSlice, H, ld] floats)
constexpr int kHotGroup = 64;        // hot rows a partial wave takes: four 16-row tiles
// (rows of 64 / 128 floats only: kHotMaxG, drx_prep.hpp)

struct HotArgs {
  const float *dz1;             // [B, ld]
  const uint32_t *mask;         // [H, Bw] (drx_prep.hpp PrepBufs::hmask)
  float *part;                  // [S, H, ld]
  uint32_t *any;                // [S, H / 32]: bit r of word (s, hb) = hot row 32 hb + r has a kept sample in slice s
  const int32_t *item;          // [H]
  float scale;                  // 1 / (1 - q)
  int B, H, Bw, S, first;       // first: the launch's first workgroup of this stage
  float *bpart;                 // [S, ld] the slices' column sums of dz1, then [S] their loss partials (BiasArgs::part of a step with a head)
  const float *lossb;           // [B], or nullptr: no loss wanted
};

static inline int hot_slices(int B) { return (B + kHotSlice - 1) / kHotSlice; }
static inline int hot_groups(int H) { return (H + kHotGroup - 1) / kHotGroup; }

typedef __bf16 hot_bf16x8 __attribute__((ext_vector_type(8)));
typedef float hot_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t hot_u32x4 __attribute__((ext_vector_type(4)));

// NT: threads of the launch it rides in (k_seg_reduce_stream<LD>: (kSegBlock / (LD / 4)) waves)
template <int LD, int NT>
struct HotPartialExtra {
  HotArgs A;
  __device__ __forceinline__ void operator()(float *) const {
    constexpr int CS = LD / 16, NW = NT / 64;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int ngr = (A.H + kHotGroup - 1) / kHotGroup;
    const int task = ((int)blockIdx.x - A.first) * NW + wv;        // column strip fastest: the waves of a workgroup read neighbouring
    if (task >= A.S * ngr * CS) return;                            // 64-byte pieces of the same dz1 rows
    const int cs = task % CS, rg = (task / CS) % ngr, s = task / (CS * ngr);
    const int c = lane & 15, kq = lane >> 4;                       // A[row c][k = 8 kq + j], B[k = 8 kq + j][col c]
    const int nt = min(kHotGroup, A.H - rg * kHotGroup) / 16;      // row tiles of this group: 4, or 2 (H a multiple of 32)
    // (wave-uniform bases in scalar registers + one 32-bit offset per lane: a slice of dz1 is 512 rows, a tile's mask rows 16 * Bw words)
    const int b_begin = s * kHotSlice, b_end = min(A.B, b_begin + kHotSlice);
    const uint32_t *const mgrp = A.mask + (size_t)rg * kHotGroup * A.Bw;
    const float *const slice = A.dz1 + (size_t)b_begin * LD + cs * 16;
    const uint32_t mlane = (uint32_t)c * (uint32_t)A.Bw, xlane = (uint32_t)(8 * kq * LD + c);
    hot_f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = hot_f32x4{0.f, 0.f, 0.f, 0.f};
    uint32_t seen = 0u;                                            // bit t: this lane's row of tile t has a kept sample in the slice
    float bsum = 0.f;                                              // this lane's share of the column sum (row group 0)
    for (int b0 = b_begin; b0 < b_end; b0 += 32) {                // one mask word: one k-step of 32 samples
      float x[8];
      uint32_t w[4];
      {
        const float *const rows = slice + (size_t)(b0 - b_begin) * LD;
        const uint32_t *const words = mgrp + (b0 >> 5);
        const int left = A.B - b0 - 8 * kq;                        // rows past the batch (the batch's last k-step only) read as 0
        if (left >= 8) {
#pragma unroll
          for (int j = 0; j < 8; ++j) x[j] = rows[xlane + (uint32_t)(j * LD)];
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) x[j] = j < left ? rows[xlane + (uint32_t)(j * LD)] : 0.f;
        }
        // (a group of two tiles reads its second tile's words twice and drops them: no branch around an MFMA, whose accumulators the
        // compiler would otherwise move through VGPRs at every k-step)
#pragma unroll
        for (int t = 0; t < 4; ++t) w[t] = (words + (size_t)(16 * min(t, nt - 1)) * A.Bw)[mlane] & (t < nt ? ~0u : 0u);
      }
      // (a k-step without a mask bit is not skipped: its dz1 values are the bias's)
      hot_u32x4 bh, bm, bl;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uint32_t hv[2], mv[2], lv[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {                              // v = hi + mid + lo exactly (truncations; the rests are exact)
          const float v = x[2 * i + e];
          bsum += v;                                               // (k-steps ascending, j = 0 .. 7 inside a step)
          hv[e] = __float_as_uint(v) & 0xFFFF0000u;
          const float r1 = v - __uint_as_float(hv[e]);
          mv[e] = __float_as_uint(r1) & 0xFFFF0000u;
          lv[e] = __float_as_uint(r1 - __uint_as_float(mv[e])) & 0xFFFF0000u;
        }
        bh[i] = (hv[0] >> 16) | hv[1];
        bm[i] = (mv[0] >> 16) | mv[1];
        bl[i] = (lv[0] >> 16) | lv[1];
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {                                // (a tile past the group's last: A = 0)
        seen |= (w[t] != 0u ? 1u : 0u) << t;
        const uint32_t bits = (w[t] >> (8 * kq)) & 0xFFu;
        hot_u32x4 a;
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = ((bits >> (2 * i)) & 1u) * 0x3F80u | ((bits >> (2 * i + 1)) & 1u) * 0x3F800000u;      // bf16 1.0 or 0
        const hot_bf16x8 av = __builtin_bit_cast(hot_bf16x8, a);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, __builtin_bit_cast(hot_bf16x8, bh), acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, __builtin_bit_cast(hot_bf16x8, bm), acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, __builtin_bit_cast(hot_bf16x8, bl), acc[t], 0, 0, 0);
      }
    }
    // D of tile t: column c, row 4 kq + register
    float *const out = A.part + ((size_t)s * A.H + rg * kHotGroup) * LD + cs * 16 + c;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (t < nt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) out[(size_t)(16 * t + 4 * kq + i) * LD] = acc[t][i];
      }
    if (cs == 0) {                                                 // the rows of this group a sample of the slice kept (lanes c, c + 16, .. read the same row)
      uint32_t rows[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) rows[t] = (uint32_t)__ballot((seen >> t) & 1u) & 0xFFFFu;
      if (lane == 0) {
        uint32_t *const any = A.any + (size_t)s * (A.H / 32) + rg * (kHotGroup / 32);
        any[0] = rows[0] | (rows[1] << 16);
        if (nt > 2) any[1] = rows[2] | (rows[3] << 16);
      }
    }
    if (rg == 0) {
      // the slice's column sums of these 16 columns: the four lane groups in a fixed order
      const float g1 = __shfl(bsum, c + 16, 64), g2 = __shfl(bsum, c + 32, 64), g3 = __shfl(bsum, c + 48, 64);
      if (kq == 0) A.bpart[(size_t)s * LD + cs * 16 + c] = ((bsum + g1) + g2) + g3;
      if (cs == 0 && A.lossb) {                                    // ... and the slice's loss partial, a fixed order too
        float l = 0.f;
        for (int b = b_begin + lane; b < b_end; b += 64) l += A.lossb[b];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) l += __shfl_xor(l, o, 64);
        if (lane == 0) A.bpart[(size_t)A.S * LD + s] = l;
      }
    }
  }
};

// one workgroup of kFixBlock threads per hot row: NQ = kFixBlock / LD groups each sum a run of consecutive slices in slice order, the
// runs are added in group order (a fixed order: bit-reproducible), then the row's Adagrad update
template <int LD, class Policy>
struct HotFinishExtra {
  HotArgs A;
  Policy pol;
  __device__ __forceinline__ void operator()(float *lds) const {
    constexpr int NT = kFixBlock, NQ = NT / LD;
    static_assert(NQ >= 1 && NT % LD == 0, "a row per workgroup");
    const int h = (int)blockIdx.x - A.first;
    if (h >= A.H) return;
    const uint32_t bit = 1u << (h & 31);
    bool touched = false;
    for (int s = (int)threadIdx.x; s < A.S; s += NT) touched |= (A.any[(size_t)s * (A.H / 32) + (h >> 5)] & bit) != 0u;
    if (!__syncthreads_or(touched)) return;                        // no sample kept this row: it stays bit-equal
    const int c = (int)threadIdx.x % LD, q = (int)threadIdx.x / LD;
    const int per = (A.S + NQ - 1) / NQ, s0 = q * per, s1 = min(A.S, s0 + per);
    float sum = 0.f;
#pragma unroll 8
    for (int s = s0; s < s1; ++s) sum += A.part[((size_t)s * A.H + h) * LD + c];
    lds[q * LD + c] = sum;
    __syncthreads();
    if (q == 0) {
      float t = lds[c];
#pragma unroll
      for (int k = 1; k < NQ; ++k) t += lds[k * LD + c];
      const StreamArrays SA = pol.stream_arrays();
      const size_t off = (size_t)A.item[h] * LD + c;
      float pv = SA.table[0][off], av = SA.slot[0][off];
      pol.stream_update(fmaf(pol.stream_decay(), pv, A.scale * t), pv, av);
      SA.table[0][off] = pv;
      SA.slot[0][off] = av;
    }
  }
};

// two kinds of extra workgroups in one launch: [.., n1) the first, the rest the second
template <class E1, class E2>
struct ExtraPair {
  E1 e1;
  int n1;
  E2 e2;
  __device__ __forceinline__ void operator()(float *lds) const {
    if ((int)blockIdx.x < n1) e1(lds);
    else e2(lds);
  }
};

static SparseBufs sparse_layout(Carver &cv, const DrxCdaeParams &P, int B, int n_touch_slots) {
  SparseBufs S{};
  S.T = n_touch_slots + 2 * B;
  const int chunk = seg_chunk(long_segments(S.T, P));           // (as prep_layout: the list's chunks)
  S.n_chunks = (S.T + chunk - 1) / chunk;
  S.n_bpart = 1024;      // (256: each row group of a bias block summed 32 rows one load at a time; tail_a 25.0 -> 23.5 us)
  S.dz1 = cv.take<float>((size_t)2 * B * P.ld);       // (the second half: the work items' summed rows of DRX_BATCH_SHARE_USERS)
  S.g2 = cv.take<float>((size_t)B * P.ld);
  S.dz2 = cv.take<float>(B);
  S.lossb = cv.take<float>(B);
  S.phead = cv.take<float>((size_t)S.n_chunks * P.ld);
  S.ptail = cv.take<float>((size_t)S.n_chunks * P.ld);
  S.phs = cv.take<float>(S.n_chunks);
  S.pts = cv.take<float>(S.n_chunks);
  {
    const int cpb = kSegBlock / pick_geom(P.ld).G;
    const int n_blocks = (S.n_chunks + cpb - 1) / cpb;
    S.pblock = cv.take<float>((size_t)n_blocks * P.ld);
    S.pbs = cv.take<float>(n_blocks);
  }
  S.bpart = cv.take<float>((size_t)S.n_bpart * (P.ld + 1));     // partial rows + per-block loss partials
  return S;
}

// Which prepared buffers carry a hot head, and of how many rows: the preparation's record, kept on the HOST — a step entry is queued
// while the preparation may still be running on another stream, and reading a word of the device buffer would wait for that stream
// (the pipeline's run-ahead would be gone).  Keyed by the buffer's address: every preparation into an address rewrites its entry (a plain
// one drops it), drx_cdae_prep_forget drops it when the caller releases the buffer.  A step given another H than its list's is refused.
static std::mutex g_hot_mu;
static std::unordered_map<const void *, int> g_hot_of;
static void hot_record(const void *prepared, int H) {
  std::lock_guard<std::mutex> lk(g_hot_mu);
  if (H > 0) g_hot_of[prepared] = H;
  else g_hot_of.erase(prepared);
}
static int hot_recorded(const void *prepared) {
  std::lock_guard<std::mutex> lk(g_hot_mu);
  const auto it = g_hot_of.find(prepared);
  return it == g_hot_of.end() ? 0 : it->second;
}

// the hot head's partials and row flags (behind the step's other buffers: a step without a head keeps its layout)
// (+ the hidden bias's and the loss's partials of a step with a head, one row per slice: SparseBufs::bpart has 1024 rows, a batch of more
// than 1024 slices would not fit them)
struct HotBufs { float *part; uint32_t *any; float *bpart; };
static HotBufs hot_layout(Carver &cv, const DrxCdaeParams &P, int B, int H) {
  HotBufs HB{nullptr, nullptr, nullptr};
  if (H <= 0) return HB;
  HB.part = cv.take<float>((size_t)hot_slices(B) * H * P.ld);
  HB.any = cv.take<uint32_t>((size_t)hot_slices(B) * (H / 32));
  HB.bpart = cv.take<float>((size_t)hot_slices(B) * (P.ld + 1));
  return HB;
}

// ---- the sampled step's three launches: forward/backward, the segmented reduction, the span finish ----------------------------------
// (which variant of each: drx_prep.hpp forward_form / reduce_form / hot_head_fits; the reduction's launches: drx_segstream.hpp)
template <int G, int J>
static void launch_forward(ForwardForm form, const DrxCdaeParams &P, const DrxOptim &opt, const DrxHistory &hist, const DrxBatch &bt,
                           float scale, uint32_t qthr, int32_t loss_kind, const SparseBufs &S, const float *ks_h, const float *ks_dot,
                           hipStream_t st) {
  constexpr int gpb = kBlock / G;
  const dim3 groups((bt.B + gpb - 1) / gpb);
  const bool adagrad = opt.kind == DRX_OPT_ADAGRAD;        // (compiled in: the throughput configuration's optimizer)
  switch (form) {
  case ForwardForm::ColumnShard:
    hipLaunchKernelGGL((k_kshard_rest<G, J>), groups, dim3(kBlock), 0, st, P, opt, hist, bt, scale, qthr, loss_kind, S, ks_h, ks_dot);
    break;
  case ForwardForm::SharedUsers:
    if constexpr (G >= 16 && J <= 2) {                      // (share_users(): rows of 64 .. 512 floats)
      // work items: at most one per distinct user + one per full item, never more than triples
      const long long wmax = (long long)(P.n_users < bt.B ? P.n_users : bt.B) + bt.B / share_item_triples(P.ld) + 1;
      hipLaunchKernelGGL((adagrad ? k_items_fwd_bwd<G, J, DRX_OPT_ADAGRAD> : k_items_fwd_bwd<G, J>), dim3((unsigned)(wmax < bt.B ? wmax : bt.B)),
                         dim3(kItemThreads), share_item_lds_bytes(P.ld), st, P, opt, hist, bt, scale, qthr, loss_kind, S);
    }
    break;
  case ForwardForm::PerWorkgroup:
    hipLaunchKernelGGL((k_sampled_fwd_bwd_wg<G, J>), dim3(bt.B), dim3(kBlock), (size_t)gpb * P.ld * 4, st, P, opt, hist, bt, scale, qthr,
                       loss_kind, S);
    break;
  case ForwardForm::PerGroup:
    hipLaunchKernelGGL((adagrad ? k_sampled_fwd_bwd<G, J, DRX_OPT_ADAGRAD> : k_sampled_fwd_bwd<G, J>), groups, dim3(kBlock), 0, st, P, opt, hist,
                       bt, scale, qthr, loss_kind, S);
    break;
  }
}

// the segmented reduction (+ the bias column sums as extra workgroups) and the ONE launch that combines the chunk-crossing segments
// (+ the bias update), phase event 3 between them; with a hot head (HA.H > 0: the streamed form, hot_head_fits) both launches carry
// its workgroups too — the partials, one wave per (slice, 16 columns, up to 64 hot rows), which leave the bias column sums as well (BA.part
// is their carve then: no BiasPartialExtra workgroups in front) — and the finish, one workgroup per hot row
template <int G, int J, class Policy>
static int reduce_and_finish(ReduceForm form, const DrxCdaeParams &P, const DrxOptim &opt, const SparseBufs &S, const SegBufs &SB,
                             const PlanBufs &PB, const SpanPlan &plan, const BiasArgs &BA, const HotArgs &HA, void *const *events,
                             hipStream_t st) {
  const Policy pol{P, opt, BA.B, HA.scale, S.dz1, (long long)(S.g2 - S.dz1), S.dz2};
  const BiasFinalExtra<G, J> bias{P, opt, BA};
  int rc = DRX_EINVAL;
  if (HA.H == 0) rc = launch_reduce<G, J>(form, SB, PB, plan, pol, BA, st);
  else if constexpr (kHotBuilt<G, J, Policy>) {
    constexpr int NT = kStreamThreads<G>;
    HotArgs part = HA;
    part.first = 0;
    const int n_hot = (HA.S * hot_groups(HA.H) * (G / 4) + NT / 64 - 1) / (NT / 64);      // waves: (slice, row group, strip of 16 columns)
    rc = launch_reduce_streamed<G, J>(SB, PB, plan, pol, n_hot, HotPartialExtra<4 * G, NT>{part}, st);
  }
  if (rc) return rc;
  DRX_HIP(phase_event(events, 3, st));
  rc = DRX_EINVAL;
  if (HA.H == 0) rc = launch_spans<G, J>(SB, PB, plan, pol, 1, bias, st);
  else if constexpr (kHotBuilt<G, J, Policy>) {
    HotArgs fin = HA;
    fin.first = kSpanBlocks + 1;                            // (behind the hidden bias's workgroup)
    using Finish = ExtraPair<BiasFinalExtra<G, J>, HotFinishExtra<4 * G, Policy>>;
    rc = launch_spans<G, J>(SB, PB, plan, pol, 1 + HA.H, Finish{bias, fin.first, {fin, pol}}, st);
  }
  if (rc) return rc;
  DRX_HIP(phase_event(events, 4, st));
  DRX_HIP(phase_event(events, 5, st));
  return DRX_OK;
}

}  // namespace drx

using namespace drx;

extern "C" {

size_t drx_cdae_scratch_bytes(const DrxCdaeParams *p, int32_t B, int32_t n_touch_slots, int32_t dense_mode) {
  if (!p || B < 1 || n_touch_slots < 0) return 0;
  Carver c(nullptr, 0);
  if (dense_mode) {
    c.off = dense_layout_bytes(*p, B);
  } else {
    (void)sparse_layout(c, *p, B, n_touch_slots);
    (void)prep_layout(c, *p, B, n_touch_slots);
  }
  return align_up(c.off, 256) + 256;
}

// (drx_debug_cdae_reduce: the caller's gradient rows stand in for the forward kernel's; form 1: the planned form where reduce_form()
// answers Streamed)
struct GivenGradients { const float *dz1, *g2, *dz2; int32_t form; };

static int step_sparse_impl(const DrxCdaeParams *p, const DrxOptim *opt, const DrxHistory *hist, const DrxBatch *bt,
                            int32_t loss_kind, const void *prepared, size_t prepared_bytes, void *scratch, size_t scratch_bytes,
                            float *loss_out, void *const *events, void *stream, const float *ks_h = nullptr,
                            const float *ks_dot = nullptr, const DrxHotHead *hot = nullptr, const GivenGradients *given = nullptr) {
  int rc = check_params(p);
  if (rc) return rc;
  rc = check_batch(hist, bt);
  if (rc || !opt || !scratch || !bt->iid || (!bt->y && !given) || !bt->keep_off) return DRX_EINVAL;
  if (opt->kind != DRX_OPT_ADAM && opt->kind != DRX_OPT_ADAGRAD && opt->kind != DRX_OPT_ROWWISE_ADAGRAD) return DRX_EINVAL;
  for (int i = 0; i < 5; ++i)
    if (!opt->s1[i] || (opt->kind == DRX_OPT_ADAM && !opt->s2[i])) return DRX_EINVAL;
  if ((uint64_t)2 * p->n_items + p->n_users + 1 >= 0xFFFFFFFFull) return DRX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int H = hot ? hot->H : 0;
  if (prepared && hot_recorded(prepared) != H) return DRX_EINVAL;     // (a list prepared with another head, or none)
  Carver cv(scratch, scratch_bytes);
  SparseBufs S = sparse_layout(cv, *p, bt->B, bt->n_touch_slots);
  const HotBufs HB = hot_layout(cv, *p, bt->B, H);
  PrepBufs R{};
  if (prepared) {
    Carver cp(const_cast<void *>(prepared), prepared_bytes);
    R = prep_layout(cp, *p, bt->B, bt->n_touch_slots, H);
    if (!cp.ok()) return DRX_ESCRATCH;
  } else {
    R = prep_layout(cv, *p, bt->B, bt->n_touch_slots, H);
  }
  if (!cv.ok()) return DRX_ESCRATCH;
  const float scale = 1.0f / (1.0f - bt->q);
  const uint32_t qthr = q_threshold(bt->q);
  const int rows_per_block = (bt->B + S.n_bpart - 1) / S.n_bpart;
  const int n_bpart = (bt->B + rows_per_block - 1) / rows_per_block;
  S.solo_v = prepared ? R.solo_v : nullptr;
  S.solo_o = prepared ? R.solo_o : nullptr;
  S.order = prepared ? R.order : nullptr;
  SegBufs SB{R.keys_s, R.vals_s, S.phead, S.ptail, S.phs, S.pts, nullptr, nullptr, nullptr, nullptr, S.T, S.n_chunks, p->ld, nullptr};
#ifdef DRX_STAMPS
  S.stamps = SB.stamps = h_stamps;
#endif
  PlanBufs PB{S.pblock, S.pbs};
  // DRX_BATCH_SHARE_USERS (lists prepared ahead through the history's transpose only): one forward workgroup per work item
  // (k_items_fwd_bwd); the reduction reads the items' summed gradient rows
  // (a list in the shared form has no gradient row per triple: the column-sharded step's forward kernels cannot read it)
  if (prepared && ks_h && share_users(p, hist, bt, R)) return DRX_EINVAL;
  const bool share = prepared && !ks_h && share_users(p, hist, bt, R);
  S.usamp = share ? R.usamp : nullptr;
  S.witem = share ? R.witem : nullptr;
  S.worder = share ? R.worder : nullptr;
  S.n_items = share ? R.n_du : nullptr;
  // which variant of each launch (drx_prep.hpp)
  ReduceForm form = reduce_form(opt->kind, bt->B, S.T, *p);
  const ForwardForm fwd = forward_form(ks_h != nullptr, share, bt->B, bt->n_touch_slots);
  if (H > 0 && !hot_head_fits(form, p->ld, share, ks_h != nullptr)) return DRX_EINVAL;
  if (given) {
    if (share || (given->form == 1 && (H > 0 || form == ReduceForm::PlannedLong))) return DRX_EINVAL;
    if (given->form == 1) form = ReduceForm::PlannedShort;
  }
  const HotArgs HA{S.dz1, R.hmask, HB.part, HB.any, hot ? hot->item : nullptr, scale, bt->B, H, R.Bw, hot_slices(bt->B), 0, HB.bpart,
                   loss_out ? S.lossb : nullptr};
  // (with a head the hidden bias's partials are the slices' column sums its partial waves leave)
  const BiasArgs BA = H > 0 ? BiasArgs{S.dz1, HB.bpart, S.lossb, loss_out, bt->B, hot_slices(bt->B), kHotSlice}
                            : BiasArgs{S.dz1, S.bpart, S.lossb, loss_out, bt->B, n_bpart, rows_per_block};
  DRX_HIP(phase_event(events, 0, st));
  if (given) {
    const size_t row_bytes = (size_t)bt->B * p->ld * sizeof(float);
    DRX_HIP(hipMemcpyAsync(S.dz1, given->dz1, row_bytes, hipMemcpyDeviceToDevice, st));
    DRX_HIP(hipMemcpyAsync(S.g2, given->g2, row_bytes, hipMemcpyDeviceToDevice, st));
    DRX_HIP(hipMemcpyAsync(S.dz2, given->dz2, (size_t)bt->B * sizeof(float), hipMemcpyDeviceToDevice, st));
    DRX_HIP(hipMemsetAsync(S.lossb, 0, (size_t)bt->B * sizeof(float), st));
  } else {
    (void)dispatch_geom(p->ld, [&](auto g) -> int {
      launch_forward<decltype(g)::G, decltype(g)::J>(fwd, *p, *opt, *hist, *bt, scale, qthr, loss_kind, S, ks_h, ks_dot, st);
      return DRX_OK;                                                   // (launch errors: DRX_LAUNCH_CHECK below)
    });
  }
  DRX_HIP(phase_event(events, 1, st));
  if (!prepared) {
    rc = prepare_impl(p, hist, bt, R, st, false, TouchPresence{nullptr, WireGeo{1, 0, 1}}, hot ? hot->slot : nullptr,
                      hot ? hot->item : nullptr);
    if (rc) return rc;
  }
  DRX_HIP(phase_event(events, 2, st));
  rc = dispatch_geom(p->ld, [&](auto g) -> int {
    constexpr int G = decltype(g)::G, J = decltype(g)::J;
    return opt->kind == DRX_OPT_ADAGRAD
        ? reduce_and_finish<G, J, DirectPolicyAdagrad>(form, *p, *opt, S, SB, PB, R.plan, BA, HA, events, st)
        : reduce_and_finish<G, J, DirectPolicy>(form, *p, *opt, S, SB, PB, R.plan, BA, HA, events, st);
  });
  if (rc) return rc;
  DRX_LAUNCH_CHECK();
  return DRX_OK;
}

size_t drx_cdae_prep_bytes(const DrxCdaeParams *p, int32_t B, int32_t n_touch_slots) {
  if (!p || B < 1 || n_touch_slots < 0) return 0;
  Carver c(nullptr, 0);
  (void)prep_layout(c, *p, B, n_touch_slots);
  return align_up(c.off, 256) + 256;
}

int drx_cdae_sparse_prepare(const DrxCdaeParams *p, const DrxHistory *hist, const DrxBatch *bt, void *prepared,
                            size_t prepared_bytes, void *stream) {
  int rc = check_params(p);
  if (rc) return rc;
  rc = check_batch(hist, bt);
  if (rc || !prepared || !bt->iid || !bt->keep_off) return DRX_EINVAL;
  Carver cp(prepared, prepared_bytes);
  PrepBufs R = prep_layout(cp, *p, bt->B, bt->n_touch_slots);
  if (!cp.ok()) return DRX_ESCRATCH;
  hot_record(prepared, 0);                                           // (a list without a head from now on)
  rc = prepare_impl(p, hist, bt, R, (hipStream_t)stream, true);      // touches, sort, span plan + sole-toucher marks (+ launch order)
  if (rc) return rc;
  if (p->ld <= 16) order_by_degree(bt, R, (hipStream_t)stream, true);
  DRX_LAUNCH_CHECK();
  return DRX_OK;
}

size_t drx_cdae_prep_result_bytes(const DrxCdaeParams *p, int32_t B, int32_t n_touch_slots) {
  if (!p || B < 1 || n_touch_slots < 0) return 0;
  Carver c(nullptr, 0);
  return prep_layout(c, *p, B, n_touch_slots).result_bytes;
}

int drx_cdae_step_sparse_prepared(const DrxCdaeParams *p, const DrxOptim *opt, const DrxHistory *hist, const DrxBatch *bt,
                                  int32_t loss_kind, const void *prepared, size_t prepared_bytes, void *scratch,
                                  size_t scratch_bytes, float *loss_out, void *const *events, void *stream) {
  if (!prepared) return DRX_EINVAL;
  return step_sparse_impl(p, opt, hist, bt, loss_kind, prepared, prepared_bytes, scratch, scratch_bytes, loss_out, events, stream);
}

int drx_cdae_kshard_forward(const DrxCdaeParams *p, const DrxHistory *hist, const DrxBatch *bt, float *h_out, float *dot_partial,
                            void *stream) {
  return drx_cdae_kshard_forward_prepared(p, hist, bt, nullptr, 0, h_out, dot_partial, stream);
}

int drx_cdae_kshard_forward_prepared(const DrxCdaeParams *p, const DrxHistory *hist, const DrxBatch *bt, const void *prepared,
                                     size_t prepared_bytes, float *h_out, float *dot_partial, void *stream) {
  int rc = check_params(p);
  if (rc) return rc;
  rc = check_batch(hist, bt);
  if (rc || !bt->iid || !bt->keep_off || !h_out || !dot_partial) return DRX_EINVAL;
  const int32_t *order = nullptr;                  // the launch order built with the prepared list (drx_cdae_sparse_prepare*)
  if (prepared) {
    Carver cp(const_cast<void *>(prepared), prepared_bytes);
    const PrepBufs R = prep_layout(cp, *p, bt->B, bt->n_touch_slots);
    if (!cp.ok()) return DRX_ESCRATCH;
    order = R.order;
  }
  hipStream_t st = (hipStream_t)stream;
  const float scale = 1.0f / (1.0f - bt->q);
  const uint32_t qthr = q_threshold(bt->q);
  const bool per_wg = forward_per_workgroup(bt->B, bt->n_touch_slots);
  return dispatch_geom(p->ld, [&](auto g) -> int {
    constexpr int G = decltype(g)::G, J = decltype(g)::J;
    constexpr int gpb = kBlock / G;
    if (per_wg)
      hipLaunchKernelGGL((k_kshard_fwd_wg<G, J>), dim3(bt->B), dim3(kBlock), (size_t)gpb * p->ld * 4, st, *p, *hist, *bt, scale, qthr,
                         h_out, dot_partial);
    else
      hipLaunchKernelGGL((k_kshard_fwd<G, J>), dim3((bt->B + gpb - 1) / gpb), dim3(kBlock), 0, st, *p, *hist, *bt, scale, qthr, h_out,
                         dot_partial, order);
    DRX_LAUNCH_CHECK();
    return DRX_OK;
  });
}

int drx_cdae_kshard_step(const DrxCdaeParams *p, const DrxOptim *opt, const DrxHistory *hist, const DrxBatch *bt, int32_t loss_kind,
                         const float *h, const float *dot_total, const void *prepared, size_t prepared_bytes, void *scratch,
                         size_t scratch_bytes, float *loss_out, void *const *events, void *stream) {
  if (!h || !dot_total) return DRX_EINVAL;
  if (opt && opt->kind == DRX_OPT_ROWWISE_ADAGRAD) return DRX_EINVAL;      // its row statistic would cover the local columns only
  return step_sparse_impl(p, opt, hist, bt, loss_kind, prepared, prepared_bytes, scratch, scratch_bytes, loss_out, events, stream,
                          h, dot_total);
}

int drx_cdae_step_sparse(const DrxCdaeParams *p, const DrxOptim *opt, const DrxHistory *hist, const DrxBatch *bt,
                         int32_t loss_kind, void *scratch, size_t scratch_bytes, float *loss_out, void *stream) {
  return step_sparse_impl(p, opt, hist, bt, loss_kind, nullptr, 0, scratch, scratch_bytes, loss_out, nullptr, stream);
}

int drx_cdae_step_sparse_timed(const DrxCdaeParams *p, const DrxOptim *opt, const DrxHistory *hist, const DrxBatch *bt,
                               int32_t loss_kind, void *scratch, size_t scratch_bytes, float *loss_out, void *const *events,
                               void *stream) {
  if (!events) return DRX_EINVAL;
  return step_sparse_impl(p, opt, hist, bt, loss_kind, nullptr, 0, scratch, scratch_bytes, loss_out, events, stream);
}

// ---- the hot head (include/drx.h DrxHotHead) ----------------------------------------------------------------------------------
static int hot_rows(const DrxCdaeParams *p, int32_t H) {
  if (!p || H < 0 || H > DRX_MAX_HOT || H % 32 || H > p->n_items) return -1;
  return H;
}

static bool hot_ok(const DrxCdaeParams *p, const DrxHotHead *hot) {
  return hot && hot_rows(p, hot->H) >= 0 && (hot->H == 0 || (hot->slot && hot->item && p->ld <= 4 * kHotMaxG));
}

size_t drx_cdae_prep_bytes_hot(const DrxCdaeParams *p, int32_t B, int32_t n_touch_slots, int32_t H) {
  if (!p || B < 1 || n_touch_slots < 0 || hot_rows(p, H) < 0) return 0;
  Carver c(nullptr, 0);
  (void)prep_layout(c, *p, B, n_touch_slots, H);
  return align_up(c.off, 256) + 256;
}

size_t drx_cdae_scratch_bytes_hot(const DrxCdaeParams *p, int32_t B, int32_t n_touch_slots, int32_t H) {
  if (!p || B < 1 || n_touch_slots < 0 || hot_rows(p, H) < 0) return 0;
  Carver c(nullptr, 0);
  (void)sparse_layout(c, *p, B, n_touch_slots);
  (void)hot_layout(c, *p, B, H);
  (void)prep_layout(c, *p, B, n_touch_slots, H);
  return align_up(c.off, 256) + 256;
}

int drx_cdae_sparse_prepare_hot(const DrxCdaeParams *p, const DrxHistory *hist, const DrxBatch *bt, const DrxHotHead *hot,
                                void *prepared, size_t prepared_bytes, void *stream) {
  int rc = check_params(p);
  if (rc) return rc;
  rc = check_batch(hist, bt);
  if (rc || !prepared || !bt->iid || !bt->keep_off || !hot_ok(p, hot)) return DRX_EINVAL;
  Carver cp(prepared, prepared_bytes);
  PrepBufs R = prep_layout(cp, *p, bt->B, bt->n_touch_slots, hot->H);
  if (!cp.ok()) return DRX_ESCRATCH;
  hot_record(prepared, 0);
  rc = prepare_impl(p, hist, bt, R, (hipStream_t)stream, true, TouchPresence{nullptr, WireGeo{1, 0, 1}}, hot->slot, hot->item);
  if (rc) return rc;
  hot_record(prepared, hot->H);
  if (p->ld <= 16) order_by_degree(bt, R, (hipStream_t)stream, true);
  DRX_LAUNCH_CHECK();
  return DRX_OK;
}

// (include/drx.h: the first two launches of a preparation — touch kernel, then the sort's counting launch or its fold — and copies of
// what they leave, for a test to read before a sort trusts it)
int drx_debug_prep_counts(const DrxCdaeParams *p, const DrxHistory *hist, const DrxBatch *bt, const DrxHotHead *hot, uint8_t *present,
                          int32_t ipr, int32_t cshift, int32_t world, void *prepared, size_t prepared_bytes, uint32_t *hist_out,
                          uint32_t *buckets_out, uint32_t *keys_out, uint32_t *vals_out, uint32_t *mask_out, int32_t *info_out,
                          void *stream) {
  int rc = check_params(p);
  if (rc) return rc;
  rc = check_batch(hist, bt);
  if (rc || !prepared || !bt->iid || !bt->keep_off || !hist_out || !buckets_out || !keys_out || !vals_out || !info_out) return DRX_EINVAL;
  if ((uint64_t)2 * p->n_items + p->n_users + 1 >= 0xFFFFFFFFull) return DRX_EINVAL;
  if (hot && !hot_ok(p, hot)) return DRX_EINVAL;
  if (present && (ipr < 1 || cshift < 0 || cshift > 30 || world < 1)) return DRX_EINVAL;
  const int H = hot ? hot->H : 0;
  if (H > 0 && !mask_out) return DRX_EINVAL;
  Carver cp(prepared, prepared_bytes);
  const PrepBufs R = prep_layout(cp, *p, bt->B, bt->n_touch_slots, H);
  if (!cp.ok()) return DRX_ESCRATCH;
  if (H > 0 && !hot_list_fits(R.T, *p, present != nullptr)) return DRX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hot_record(prepared, 0);                                           // (no list stands in this buffer)
  launch_touches(p, hist, bt, R, st, TouchPresence{present, WireGeo{present ? ipr : 1, present ? cshift : 0, present ? world : 1}},
                 H > 0 ? hot->slot : nullptr, H > 0 ? hot->item : nullptr);
  const SortRider rider{bt->keep_off, bt->B, R.order_work, R.partials, R.partial_rows};
  const uint32_t *h = nullptr;
  rc = sort_first_counts(R.sort_temp, R.sort_bytes, R.keys, (size_t)R.T, R.bits, true, st, rider, &h);
  if (rc) return rc;
  const int dbits = sort_first_digit_bits(R.bits);
  DRX_HIP(hipMemcpyAsync(hist_out, h, sizeof(uint32_t) << dbits, hipMemcpyDeviceToDevice, st));
  DRX_HIP(hipMemcpyAsync(buckets_out, R.order_work, 256 * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  DRX_HIP(hipMemcpyAsync(keys_out, R.keys, (size_t)R.T * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  DRX_HIP(hipMemcpyAsync(vals_out, R.vals, (size_t)R.T * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  if (H > 0) DRX_HIP(hipMemcpyAsync(mask_out, R.hmask, (size_t)H * R.Bw * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  info_out[0] = dbits;
  info_out[1] = R.partials ? R.partial_rows : 0;
  info_out[2] = R.T;
  info_out[3] = DRX_PREP_ROUNDS ? touch_grid(bt->B) : (bt->B + 15) / 16;
  DRX_LAUNCH_CHECK();
  return DRX_OK;
}

// (include/drx.h: copies of what a finished preparation left in `prepared` — nothing is launched, the buffer is only read)
int drx_debug_prep_result(const DrxCdaeParams *p, int32_t B, int32_t n_touch_slots, int32_t H, const void *prepared, size_t prepared_bytes,
                          uint32_t *keys_s_out, uint32_t *vals_s_out, uint8_t *solo_v_out, uint8_t *solo_o_out, int32_t *order_out,
                          void *stream) {
  int rc = check_params(p);
  if (rc) return rc;
  if (B < 1 || n_touch_slots < 0 || hot_rows(p, H) < 0 || !prepared || !keys_s_out || !vals_s_out || !solo_v_out || !solo_o_out || !order_out)
    return DRX_EINVAL;
  Carver cp(const_cast<void *>(prepared), prepared_bytes);
  const PrepBufs R = prep_layout(cp, *p, B, n_touch_slots, H);
  if (!cp.ok()) return DRX_ESCRATCH;
  hipStream_t st = (hipStream_t)stream;
  DRX_HIP(hipMemcpyAsync(keys_s_out, R.keys_s, (size_t)R.T * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  DRX_HIP(hipMemcpyAsync(vals_s_out, R.vals_s, (size_t)R.T * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  DRX_HIP(hipMemcpyAsync(solo_v_out, R.solo_v, (size_t)B, hipMemcpyDeviceToDevice, st));
  DRX_HIP(hipMemcpyAsync(solo_o_out, R.solo_o, (size_t)B, hipMemcpyDeviceToDevice, st));
  DRX_HIP(hipMemcpyAsync(order_out, R.order, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  return DRX_OK;
}

// (include/drx.h: the step's reduction and span launches alone, on gradient rows the caller gives)
int drx_debug_cdae_reduce(const DrxCdaeParams *p, const DrxOptim *opt, const DrxHistory *hist, const DrxBatch *bt, const DrxHotHead *hot,
                          const void *prepared, size_t prepared_bytes, const float *dz1_in, const float *g2_in, const float *dz2_in,
                          int32_t form, void *scratch, size_t scratch_bytes, void *stream) {
  if (!dz1_in || !g2_in || !dz2_in || (form != 0 && form != 1) || (hot && !hot_ok(p, hot))) return DRX_EINVAL;
  const GivenGradients given{dz1_in, g2_in, dz2_in, form};
  return step_sparse_impl(p, opt, hist, bt, DRX_LOSS_BCE, prepared, prepared_bytes, scratch, scratch_bytes, nullptr, nullptr, stream,
                          nullptr, nullptr, hot && hot->H > 0 ? hot : nullptr, &given);
}

// (include/drx.h: copies of the span plan a finished preparation left — nothing is launched)
int drx_debug_span_plan(const DrxCdaeParams *p, int32_t B, int32_t n_touch_slots, int32_t H, const void *prepared, size_t prepared_bytes,
                        uint8_t *ext_out, uint32_t *desc_out, uint32_t *cnt_out, void *stream) {
  int rc = check_params(p);
  if (rc) return rc;
  if (B < 1 || n_touch_slots < 0 || hot_rows(p, H) < 0 || !prepared || !ext_out || !desc_out || !cnt_out) return DRX_EINVAL;
  Carver cp(const_cast<void *>(prepared), prepared_bytes);
  const PrepBufs R = prep_layout(cp, *p, B, n_touch_slots, H);
  if (!cp.ok()) return DRX_ESCRATCH;
  hipStream_t st = (hipStream_t)stream;
  DRX_HIP(hipMemcpyAsync(ext_out, R.plan.ext, (size_t)R.n_chunks, hipMemcpyDeviceToDevice, st));
  DRX_HIP(hipMemcpyAsync(desc_out, R.plan.desc, (size_t)R.n_chunks * sizeof(uint2), hipMemcpyDeviceToDevice, st));
  DRX_HIP(hipMemcpyAsync(cnt_out, R.plan.cnt, 2 * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  return DRX_OK;
}

int drx_cdae_step_sparse_hot(const DrxCdaeParams *p, const DrxOptim *opt, const DrxHistory *hist, const DrxBatch *bt,
                             const DrxHotHead *hot, int32_t loss_kind, const void *prepared, size_t prepared_bytes, void *scratch,
                             size_t scratch_bytes, float *loss_out, void *const *events, void *stream) {
  if (!hot_ok(p, hot)) return DRX_EINVAL;
  return step_sparse_impl(p, opt, hist, bt, loss_kind, prepared, prepared_bytes, scratch, scratch_bytes, loss_out, events, stream,
                          nullptr, nullptr, hot);
}

int32_t drx_cdae_hot_rows_for(const DrxCdaeParams *p, int32_t opt_kind, int32_t B, int32_t n_touch_slots, int32_t H) {
  if (B < 1 || n_touch_slots < 0 || hot_rows(p, H) <= 0) return 0;
  // (a list of shared users is one of long segments: never the streamed form)
  return hot_head_fits(reduce_form(opt_kind, B, n_touch_slots + 2 * B, *p), p->ld, false, false) ? H : 0;
}

void drx_cdae_prep_forget(const void *prepared) {
  if (prepared) hot_record(prepared, 0);
}

}  // extern "C"
