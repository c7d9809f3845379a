// CDAE, reference ("dense") mode and inference, for MI355X (gfx950): embedding-bag hidden layer, the output layer over ALL units,
// Keras BCE/MSE against the batch-mean / per-row target, backward and the fused dense Adam / Adagrad sweep over every row; the quiet
// fit() loop of that mode in one call (drx_cdae_fit_dense); drx_cdae_forward.  None of this runs in a sampled step (drx_cdae.hip);
// the input-bag gather the two modes share is gather_bag in drx_rows.hpp.
//
// Replaces, per fit() iteration, the TensorFlow eager ops issued by DRecPy/Recommender/cdae.py:50-82 and
// DRecPy/Recommender/recommender_abc.py:190-204,328-334 (see include/drx.h for the per-entry mapping).
#include "drx_common.hpp"
#include "drx_rows.hpp"
#include "drx_opt.hpp"
#include "drx_cdae_host.hpp"

namespace drx {

template <int G, int J, int MODE>
__global__ __launch_bounds__(kBlock) void k_hidden_fwd(DrxCdaeParams P, DrxHistory H, DrxBatch bt, float scale,
                                                       uint32_t qthr, float *__restrict__ hout, DenseAux aux) {
  const int lane = threadIdx.x % G;
  const int b = blockIdx.x * (kBlock / G) + threadIdx.x / G;
  if (b >= bt.B) return;
  float4 acc[J], h[J];
  gather_bag<G, J, MODE>(P, H, bt, qthr, b, lane, acc, aux, nullptr, nullptr, 0);
  const int u = bt.uid[b];
  if (MODE == 1 && lane == 0) atomicOr(&aux.vm[(size_t)u * aux.Bw + (b >> 5)], 1u << (b & 31));
  hidden_act<G, J>(P, u, scale, lane, acc, h);
  store_row<G, J>(hout, (size_t)b, P.ld, lane, h);
}

// Small batches (the reference's own B = 32..64): one WORKGROUP per batch row — its 256/G groups split the user's history,
// each keeps 4 row loads in flight, and the partial bags are combined in LDS in group order.  With one group per row a
// 155-item history is a chain of ~40 dependent load batches on 8 workgroups of the whole chip (measured 94 us at ml-1m).
template <int G, int J, int MODE, int THREADS = kBlock>
__global__ __launch_bounds__(THREADS) void k_hidden_fwd_wg(DrxCdaeParams P, DrxHistory H, DrxBatch bt, float scale,
                                                          uint32_t qthr, float *__restrict__ hout, DenseAux aux) {
  extern __shared__ __align__(16) float lds[];   // [R, ld]
  constexpr int R = THREADS / G;
  const int lane = threadIdx.x % G, r = threadIdx.x / G;
  const int b = blockIdx.x;
  float4 acc[J], h[J];
  gather_bag<G, J, MODE>(P, H, bt, qthr, b, lane, acc, aux, nullptr, nullptr, 0, r, R);
  store_row<G, J>(lds, (size_t)r, P.ld, lane, acc);
  __syncthreads();
  if (r == 0) {
#pragma unroll
    for (int j = 0; j < J; ++j) acc[j] = f4_zero();
#pragma unroll 8
    for (int rr = 0; rr < R; ++rr) {
      float4 v[J];
      load_row<G, J>(lds, (size_t)rr, P.ld, lane, v);
#pragma unroll
      for (int j = 0; j < J; ++j) f4_add(acc[j], v[j]);
    }
    const int u = bt.uid[b];
    if (MODE == 1 && lane == 0) atomicOr(&aux.vm[(size_t)u * aux.Bw + (b >> 5)], 1u << (b & 31));
    hidden_act<G, J>(P, u, scale, lane, acc, h);
    store_row<G, J>(hout, (size_t)b, P.ld, lane, h);
  }
}

// pred[b,n] = sigmoid(h_b . W2T[n] + b2[n]) for all b, n  (inference; cdae.py:76)
template <int G, int J>
__global__ __launch_bounds__(kBlock) void k_out_fwd(DrxCdaeParams P, const float *__restrict__ h, int B,
                                                    float *__restrict__ pred) {
  const int lane = threadIdx.x % G;
  const int gpb = kBlock / G;
  for (int n = blockIdx.x * gpb + threadIdx.x / G; n < P.n_items; n += gridDim.x * gpb) {
    float4 w[J];
    load_row<G, J>(P.W2T, (size_t)n, P.ld, lane, w);
    const float bias = P.b2[n];
    for (int b = 0; b < B; ++b) {
      float4 hv[J];
      load_row<G, J>(h, (size_t)b, P.ld, lane, hv);
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < J; ++j) d += f4_dot(w[j], hv[j]);
      d = group_sum<G>(d);
      if (lane == 0) pred[(size_t)b * P.n_items + n] = sigmoidf_(d + bias);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// reference mode, output layer: forward over ALL units, loss vs batch-mean / per-row target, dz2,
// dW2T/db2 (+L2) with fused Adam, and the per-workgroup partial of dh = dz2 . W_^T.
// One GROUP owns one output unit (its W2T row stays in registers), the sub-batch's hidden rows live
// in LDS; workgroups are persistent over tiles of R = 256/G units.
// ------------------------------------------------------------------------------------------------
struct OutDenseArgs {
  const float *h;         // [B, ld]
  int32_t *cnt;           // [N]  (zeroed again by the tile that read it: the next step finds it clean)
  const uint32_t *tb;     // [B, Nw] or null
  int Nw;
  int B, Bs, n_sub;       // sub-batch rows resident in LDS, number of sub-batches
  float *gbuf;            // [N, ld] gradient accumulator across sub-batches (n_sub > 1)
  float *gb2buf;          // [N]
  float *dh_slab;         // [grid, B, ld]
  float *loss_part;       // [grid] prediction-loss partials
  float *reg_part;        // [grid] sum w^2 partials of W2T
  int loss_kind;
};

// KIND (here and in k_out_dense_tile, k_in_sweep): < 0 — Adam or Adagrad, opt.kind deciding at run time as ever; >= 0 — one of the other
// dense rules, known at compile time (csrc/drx_opt.hpp)
template <int G, int J, bool WANT_LOSS, int KIND>
__global__ __launch_bounds__(kBlock) void k_out_dense(DrxCdaeParams P, DrxOptim opt, OutDenseArgs A) {
  extern __shared__ __align__(16) float lds[];
  constexpr int R = kBlock / G;
  const int ld = P.ld;
  float *h_s = lds;                        // [Bs, ld]
  float *dh_s = h_s + (size_t)A.Bs * ld;   // [Bs, ld]
  float *w_s = dh_s + (size_t)A.Bs * ld;   // [R, ld]
  float *dz_s = w_s + (size_t)R * ld;      // [Bs, R]
  __shared__ float red[kBlock / 64];
  const int lane = threadIdx.x % G, r = threadIdx.x / G;
  const int n_tiles = (P.n_items + R - 1) / R;
  const OptScalars oW = opt_for(opt, 1, A.B), oB = opt_for(opt, 4, A.B);
  const float invBN = 1.0f / ((float)A.B * (float)P.n_items);
  const float invB = 1.0f / (float)A.B;
  float loss_acc = 0.f, reg_acc = 0.f;

  for (int sb = 0; sb < A.n_sub; ++sb) {
    const int b0 = sb * A.Bs;
    const int nb = min(A.Bs, A.B - b0);
    __syncthreads();
    for (int i = threadIdx.x; i < nb * ld / 4; i += kBlock) {
      reinterpret_cast<float4 *>(h_s)[i] = reinterpret_cast<const float4 *>(A.h + (size_t)b0 * ld)[i];
      reinterpret_cast<float4 *>(dh_s)[i] = f4_zero();
    }
    __syncthreads();
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
      const int n = tile * R + r;
      const bool live = n < P.n_items;
      float4 w[J], gw[J];
#pragma unroll
      for (int j = 0; j < J; ++j) { w[j] = f4_zero(); gw[j] = f4_zero(); }
      float bias = 0.f, tbar = 0.f, gb2 = 0.f;
      if (live) {
        load_row<G, J>(P.W2T, (size_t)n, ld, lane, w);
        bias = P.b2[n];
        tbar = (float)A.cnt[n] * invB;
        if (lane == 0 && sb + 1 == A.n_sub) A.cnt[n] = 0;       // (every lane of the group has read it: same instruction)
      }
      store_row<G, J>(w_s, (size_t)r, ld, lane, w);
      for (int b = 0; b < nb; ++b) {
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) {
          const int c = lane + j * G;
          if (4 * c < ld) d += f4_dot(w[j], reinterpret_cast<const float4 *>(h_s + (size_t)b * ld)[c]);
        }
        d = group_sum<G>(d);
        float dz = 0.f;
        if (live) {
          const float p = sigmoidf_(d + bias);
          float t = tbar;
          if (A.tb) t = (A.tb[(size_t)(b0 + b) * A.Nw + (n >> 5)] >> (n & 31)) & 1u ? 1.0f : 0.0f;
          float dp;
          if (A.loss_kind == DRX_LOSS_BCE) {
            if (WANT_LOSS) loss_acc += bce_elem(t, p);
            dp = bce_grad(t, p) * invBN;
          } else {
            const float df = p - t;
            // (B,B,N) broadcast of squared error: (p - tbar)^2 + var(t) for binary targets
            if (WANT_LOSS) loss_acc += df * df + (A.tb ? 0.f : t * (1.0f - t));
            dp = 2.0f * df * invBN;
          }
          dz = dp * p * (1.0f - p);
          gb2 += dz;
#pragma unroll
          for (int j = 0; j < J; ++j) {
            const int c = lane + j * G;
            if (4 * c < ld) f4_fma(gw[j], dz, reinterpret_cast<const float4 *>(h_s + (size_t)b * ld)[c]);
          }
        }
        if (lane == 0) dz_s[b * R + r] = dz;
      }
      __syncthreads();
      // dh_s[b,:] += sum_r dz_s[b,r] * w_s[r,:]   (each thread owns fixed (b, col) cells)
      for (int i = threadIdx.x; i < nb * (ld / 4); i += kBlock) {
        const int b = i / (ld / 4), c = i % (ld / 4);
        float4 a = reinterpret_cast<float4 *>(dh_s + (size_t)b * ld)[c];
#pragma unroll
        for (int rr = 0; rr < R; ++rr) f4_fma(a, dz_s[b * R + rr], reinterpret_cast<const float4 *>(w_s + (size_t)rr * ld)[c]);
        reinterpret_cast<float4 *>(dh_s + (size_t)b * ld)[c] = a;
      }
      // weight update of unit n (gradient complete after the last sub-batch)
      if (live) {
        if (A.n_sub > 1) {
          float4 acc[J];
          if (sb > 0) load_row<G, J>(A.gbuf, (size_t)n, ld, lane, acc);
          if (sb > 0) {
#pragma unroll
            for (int j = 0; j < J; ++j) f4_add(gw[j], acc[j]);
            gb2 += A.gb2buf[n];
          }
          if (sb + 1 < A.n_sub) {
            store_row<G, J>(A.gbuf, (size_t)n, ld, lane, gw);
            if (lane == 0) A.gb2buf[n] = gb2;
          }
        }
        if (sb + 1 == A.n_sub) {
          reg_acc += row_update_rule<G, J, KIND>(oW, P.W2T, opt.s1[1], opt.s2[1], (size_t)n, ld, lane, w, gw);
          if (lane == 0) {
            float pb = bias, m = rule_has_s1<KIND>(oB) ? opt.s1[4][n] : 0.f, v = rule_has_s2<KIND>(oB) ? opt.s2[4][n] : 0.f;
            OptScalars ob = oB; ob.rb = 0.f;
            opt_update_rule<KIND>(ob, gb2, pb, m, v);
            P.b2[n] = pb;
            if (rule_has_s1<KIND>(oB)) opt.s1[4][n] = m;
            if (rule_has_s2<KIND>(oB)) opt.s2[4][n] = v;
          }
        }
      }
      __syncthreads();
    }
    // this workgroup's partial of dh for the sub-batch rows
    for (int i = threadIdx.x; i < nb * ld / 4; i += kBlock)
      reinterpret_cast<float4 *>(A.dh_slab + ((size_t)blockIdx.x * A.B + b0) * ld)[i] = reinterpret_cast<float4 *>(dh_s)[i];
  }
  // every lane of a group accumulated the same loss terms; count them once (lane 0)
  float lsum = block_sum(lane == 0 ? loss_acc : 0.f, red);
  float rsum = block_sum(reg_acc, red);
  if (threadIdx.x == 0) { A.loss_part[blockIdx.x] = lsum * invBN; A.reg_part[blockIdx.x] = rsum; }
}

// The same output-layer step for batches that fit LDS whole (the reference's own B = 64): k_out_dense walks the batch rows one
// after the other with a cross-lane reduction per (row, unit) — a chain of B dependent shuffles that leaves the chip idle when
// there are only N/R tiles to spread.  Here a tile of kTileR units is three small register-tiled products out of LDS:
//   A  every thread owns (row, unit) pairs and forms their dot products serially over the columns -> p, loss, dz
//   B  every thread owns one float4 of one unit's gradient row: sum_b dz[b] h[b,:] in batch order, then the optimizer update
//   C  every thread owns (row, float4) cells of the tile's contribution to dh
// h rows and W2T rows are padded by 4 floats in LDS so that 8 different rows read by a wave fall on different banks.
constexpr int kTileR = 8;

__host__ __device__ inline size_t out_tile_lds_floats(int B, int ld) {
  return (size_t)B * (ld + 4) + (size_t)B * ld + (size_t)kTileR * (ld + 4) + (size_t)B * kTileR + 2 * kTileR;
}

template <bool WANT_LOSS, int KIND>
__global__ __launch_bounds__(kBlock) void k_out_dense_tile(DrxCdaeParams P, DrxOptim opt, OutDenseArgs A) {
  constexpr int R = kTileR;
  extern __shared__ __align__(16) float lds[];
  const int ld = P.ld, ldp = ld + 4, B = A.B, c4n = ld / 4;
  float *h_s = lds;                              // [B, ldp]
  float *dh_s = h_s + (size_t)B * ldp;           // [B, ld]
  float *w_s = dh_s + (size_t)B * ld;            // [R, ldp]
  float *dz_s = w_s + (size_t)R * ldp;           // [B, R]
  float *bias_s = dz_s + (size_t)B * R;          // [R]
  float *tbar_s = bias_s + R;                    // [R]
  __shared__ float red[kBlock / 64];
  const int n_tiles = (P.n_items + R - 1) / R;
  const OptScalars oW = opt_for(opt, 1, B), oB = opt_for(opt, 4, B);
  const float invBN = 1.0f / ((float)B * (float)P.n_items);
  const float invB = 1.0f / (float)B;
  float loss_acc = 0.f, reg_acc = 0.f;

  for (int i = threadIdx.x; i < B * c4n; i += kBlock) {
    const int b = i / c4n, c = i % c4n;
    reinterpret_cast<float4 *>(h_s + (size_t)b * ldp)[c] = reinterpret_cast<const float4 *>(A.h + (size_t)b * ld)[c];
    reinterpret_cast<float4 *>(dh_s + (size_t)b * ld)[c] = f4_zero();
  }
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    __syncthreads();                             // previous tile's readers of w_s / dz_s are done (and h_s is loaded)
    for (int i = threadIdx.x; i < R * c4n; i += kBlock) {
      const int r = i / c4n, c = i % c4n, n = tile * R + r;
      reinterpret_cast<float4 *>(w_s + (size_t)r * ldp)[c] =
          n < P.n_items ? reinterpret_cast<const float4 *>(P.W2T + (size_t)n * ld)[c] : f4_zero();
    }
    if (threadIdx.x < R) {
      const int n = tile * R + threadIdx.x;
      bias_s[threadIdx.x] = n < P.n_items ? P.b2[n] : 0.f;
      tbar_s[threadIdx.x] = n < P.n_items ? (float)A.cnt[n] * invB : 0.f;
      if (n < P.n_items) A.cnt[n] = 0;
    }
    __syncthreads();
    // A: dot products, predictions, dz
    for (int pair = threadIdx.x; pair < B * R; pair += kBlock) {
      const int r = pair % R, b = pair / R, n = tile * R + r;
      const float4 *wr = reinterpret_cast<const float4 *>(w_s + (size_t)r * ldp);
      const float4 *hr = reinterpret_cast<const float4 *>(h_s + (size_t)b * ldp);
      float d0 = 0.f, d1 = 0.f;
      int c = 0;
#pragma unroll 4
      for (; c + 1 < c4n; c += 2) { d0 += f4_dot(wr[c], hr[c]); d1 += f4_dot(wr[c + 1], hr[c + 1]); }
      if (c < c4n) d0 += f4_dot(wr[c], hr[c]);
      float dz = 0.f;
      if (n < P.n_items) {
        const float p = sigmoidf_((d0 + d1) + bias_s[r]);
        float t = tbar_s[r];
        if (A.tb) t = (A.tb[(size_t)b * A.Nw + (n >> 5)] >> (n & 31)) & 1u ? 1.0f : 0.0f;
        float dp;
        if (A.loss_kind == DRX_LOSS_BCE) {
          if (WANT_LOSS) loss_acc += bce_elem(t, p);
          dp = bce_grad(t, p) * invBN;
        } else {
          const float df = p - t;
          if (WANT_LOSS) loss_acc += df * df + (A.tb ? 0.f : t * (1.0f - t));
          dp = 2.0f * df * invBN;
        }
        dz = dp * p * (1.0f - p);
      }
      dz_s[b * R + r] = dz;
    }
    __syncthreads();
    // C: dh_s[b,:] += sum_r dz[b,r] * w[r,:]
    for (int i = threadIdx.x; i < B * c4n; i += kBlock) {
      const int b = i / c4n, c = i % c4n;
      float4 a = reinterpret_cast<float4 *>(dh_s + (size_t)b * ld)[c];
#pragma unroll
      for (int rr = 0; rr < R; ++rr) f4_fma(a, dz_s[b * R + rr], reinterpret_cast<const float4 *>(w_s + (size_t)rr * ldp)[c]);
      reinterpret_cast<float4 *>(dh_s + (size_t)b * ld)[c] = a;
    }
    // B: gradient row of each unit (batch order) and its update; one thread per (unit, float4)
    for (int i = threadIdx.x; i < R * c4n; i += kBlock) {
      const int r = i / c4n, c = i % c4n, n = tile * R + r;
      if (n >= P.n_items) continue;
      float4 g = f4_zero();
#pragma unroll 8
      for (int b = 0; b < B; ++b) f4_fma(g, dz_s[b * R + r], reinterpret_cast<const float4 *>(h_s + (size_t)b * ldp)[c]);
      float4 p = reinterpret_cast<const float4 *>(w_s + (size_t)r * ldp)[c];
      float4 *pw = reinterpret_cast<float4 *>(P.W2T + (size_t)n * ld) + c;
      const bool h1 = rule_has_s1<KIND>(oW);         // (KIND < 0: a constant true)
      float4 *p1 = h1 ? reinterpret_cast<float4 *>(opt.s1[1] + (size_t)n * ld) + c : nullptr;
      float4 *p2 = rule_has_s2<KIND>(oW) ? reinterpret_cast<float4 *>(opt.s2[1] + (size_t)n * ld) + c : nullptr;
      float4 m = h1 ? *p1 : f4_zero(), v = p2 ? *p2 : f4_zero();
      reg_acc += f4_dot(p, p);
      opt_update_rule<KIND>(oW, fmaf(oW.rb, p.x, g.x), p.x, m.x, v.x);
      opt_update_rule<KIND>(oW, fmaf(oW.rb, p.y, g.y), p.y, m.y, v.y);
      opt_update_rule<KIND>(oW, fmaf(oW.rb, p.z, g.z), p.z, m.z, v.z);
      opt_update_rule<KIND>(oW, fmaf(oW.rb, p.w, g.w), p.w, m.w, v.w);
      *pw = p;
      if (h1) *p1 = m;
      if (p2) *p2 = v;
    }
    if (threadIdx.x >= kBlock - R) {             // the last R threads (idle in B for every supported width): the unit's bias
      const int r = threadIdx.x - (kBlock - R), n = tile * R + r;
      if (n < P.n_items) {
        float gb2 = 0.f;
        for (int b = 0; b < B; ++b) gb2 += dz_s[b * R + r];
        float pb = bias_s[r], m = rule_has_s1<KIND>(oB) ? opt.s1[4][n] : 0.f, v = rule_has_s2<KIND>(oB) ? opt.s2[4][n] : 0.f;
        OptScalars ob = oB; ob.rb = 0.f;
        opt_update_rule<KIND>(ob, gb2, pb, m, v);
        P.b2[n] = pb;
        if (rule_has_s1<KIND>(oB)) opt.s1[4][n] = m;
        if (rule_has_s2<KIND>(oB)) opt.s2[4][n] = v;
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < B * c4n; i += kBlock)
    reinterpret_cast<float4 *>(A.dh_slab + (size_t)blockIdx.x * B * ld)[i] = reinterpret_cast<float4 *>(dh_s)[i];
  float lsum = block_sum(loss_acc, red);
  float rsum = block_sum(reg_acc, red);
  if (threadIdx.x == 0) { A.loss_part[blockIdx.x] = lsum * invBN; A.reg_part[blockIdx.x] = rsum; }
}

// dz1[b,:] = (sum_slabs dh) * h (1-h)      one workgroup per batch row, groups stride over slabs
template <int G, int J, int THREADS = kBlock>
__global__ __launch_bounds__(THREADS) void k_hidden_bwd(int ld, int B, int n_slabs, const float *__restrict__ slab,
                                                       const float *__restrict__ h, float *__restrict__ dz1) {
  extern __shared__ __align__(16) float lds[];   // [R, ld]
  constexpr int R = THREADS / G;
  const int lane = threadIdx.x % G, r = threadIdx.x / G;
  const int b = blockIdx.x;
  float4 acc[J];
#pragma unroll
  for (int j = 0; j < J; ++j) acc[j] = f4_zero();
  for (int s = r; s < n_slabs; s += 4 * R) {            // 4 independent slab rows in flight, folded in slab order
    float4 v[4][J];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int j = 0; j < J; ++j) v[u][j] = f4_zero();
      if (s + u * R < n_slabs) load_row<G, J>(slab, (size_t)(s + u * R) * B + b, ld, lane, v[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < J; ++j) f4_add(acc[j], v[u][j]);
  }
  store_row<G, J>(lds, (size_t)r, ld, lane, acc);
  __syncthreads();
  if (r == 0) {
    float4 t[J], hv[J];
#pragma unroll
    for (int j = 0; j < J; ++j) t[j] = f4_zero();
#pragma unroll 8
    for (int rr = 0; rr < R; ++rr) {
      float4 v[J];
      load_row<G, J>(lds, (size_t)rr, ld, lane, v);
#pragma unroll
      for (int j = 0; j < J; ++j) f4_add(t[j], v[j]);
    }
    load_row<G, J>(h, (size_t)b, ld, lane, hv);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      t[j].x *= hv[j].x * (1.0f - hv[j].x); t[j].y *= hv[j].y * (1.0f - hv[j].y);
      t[j].z *= hv[j].z * (1.0f - hv[j].z); t[j].w *= hv[j].w * (1.0f - hv[j].w);
    }
    store_row<G, J>(dz1, (size_t)b, ld, lane, t);
  }
}

// Dense sweep over W rows [0,N) and V rows [N, N+U): gradient from the per-row batch bitmasks (bits
// ascending => deterministic sum order) + L2, Adam.  The last workgroup updates the hidden bias b.
struct DensePrefetch {          // n16 16-byte words from src (pinned host memory) to dst (device), or n16 == 0
  const uint4 *src;
  uint4 *dst;
  size_t n16;
};

template <int G, int J, int KIND>
__global__ __launch_bounds__(kBlock) void k_in_sweep(DrxCdaeParams P, DrxOptim opt, int B, float scale, DenseAux aux,
                                                     const float *__restrict__ dz1, float *reg_part, DensePrefetch pf) {
  __shared__ float red[kBlock / 64];
  const int lane = threadIdx.x % G;
  const int gpb = kBlock / G;
  const int ld = P.ld;
  float reg_acc = 0.f;
  if (blockIdx.x == gridDim.x - 1) {   // hidden bias: g = sum_b dz1[b,:]   (no L2 on biases, cdae.py:82)
    // the next batch, if the caller has it: from its pinned staging slot into device memory while the sweep runs (16-byte words)
    for (size_t i = threadIdx.x; i < pf.n16; i += kBlock) pf.dst[i] = pf.src[i];
    // every group sums the rows b = group, group + gpb, ...; the first group adds the partial sums up in group order
    __shared__ float4 part[kBlock / G][G * J];
    const int grp = threadIdx.x / G;
    float4 g[J], w[J];
#pragma unroll
    for (int j = 0; j < J; ++j) g[j] = f4_zero();
    for (int b = grp; b < B; b += gpb) {
      float4 v[J];
      load_row<G, J>(dz1, (size_t)b, ld, lane, v);
#pragma unroll
      for (int j = 0; j < J; ++j) f4_add(g[j], v[j]);
    }
#pragma unroll
    for (int j = 0; j < J; ++j) part[grp][j * G + lane] = g[j];
    __syncthreads();
    if (threadIdx.x < G) {
      for (int q = 1; q < gpb; ++q) {
#pragma unroll
        for (int j = 0; j < J; ++j) f4_add(g[j], part[q][j * G + lane]);
      }
      load_row<G, J>(P.b, 0, ld, lane, w);
      OptScalars o = opt_for(opt, 3, B);
      o.rb = 0.f;
      row_update_rule<G, J, KIND>(o, P.b, opt.s1[3], opt.s2[3], 0, ld, lane, w, g);
    }
    if (threadIdx.x == 0) reg_part[blockIdx.x] = 0.f;
    return;
  }
  const int total = P.n_items + P.n_users;
  const OptScalars oW = opt_for(opt, 0, B), oV = opt_for(opt, 2, B);
  for (int row = blockIdx.x * gpb + threadIdx.x / G; row < total; row += (gridDim.x - 1) * gpb) {
    const bool isW = row < P.n_items;
    const size_t rr = isW ? row : row - P.n_items;
    uint32_t *mask = isW ? aux.km + rr * aux.Bw : aux.vm + rr * aux.Bw;
    float4 g[J], w[J];
#pragma unroll
    for (int j = 0; j < J; ++j) g[j] = f4_zero();
    for (int wd = 0; wd < aux.Bw; ++wd) {
      uint32_t m = mask[wd];
      if (m && lane == 0) mask[wd] = 0;            // consumed (all lanes of the group loaded it with the same instruction): clean for the next step
      while (m) {
        const int b = wd * 32 + __builtin_ctz(m);
        m &= m - 1;
        float4 v[J];
        load_row<G, J>(dz1, (size_t)b, ld, lane, v);
#pragma unroll
        for (int j = 0; j < J; ++j) f4_add(g[j], v[j]);
      }
    }
    if (isW) {
#pragma unroll
      for (int j = 0; j < J; ++j) { g[j].x *= scale; g[j].y *= scale; g[j].z *= scale; g[j].w *= scale; }
      load_row<G, J>(P.W, rr, ld, lane, w);
      reg_acc += row_update_rule<G, J, KIND>(oW, P.W, opt.s1[0], opt.s2[0], rr, ld, lane, w, g);
    } else {
      load_row<G, J>(P.V, rr, ld, lane, w);
      reg_acc += row_update_rule<G, J, KIND>(oV, P.V, opt.s1[2], opt.s2[2], rr, ld, lane, w, g);
    }
  }
  float rsum = block_sum(reg_acc, red);
  if (threadIdx.x == 0) reg_part[blockIdx.x] = rsum;
}

__global__ void k_loss_final(const float *lp, int nl, const float *rp1, int n1, const float *rp2, int n2, float reg_half_rb,
                             float *out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float l = 0.f, r = 0.f;
    for (int i = 0; i < nl; ++i) l += lp[i];
    for (int i = 0; i < n1; ++i) r += rp1[i];
    for (int i = 0; i < n2; ++i) r += rp2[i];
    out[0] = l;
    out[1] = r * reg_half_rb;
  }
}

// ------------------------------------------------------------------------------------------------
// scratch layouts (shared by the sizing entry point and the step functions)
// ------------------------------------------------------------------------------------------------
constexpr int kSmallBatch = 1024;    // at or below: one workgroup per batch row in the hidden-layer gather
constexpr int kFewRows = 128;        // at or below: that workgroup has 1024 threads (fewer rows than CUs: spread each row wider)
constexpr int kOutGrid = 512;        // persistent workgroups of k_out_dense (two per CU when LDS allows)
constexpr int kSweepGrid = 1024;
constexpr size_t kLdsBudget = 144 * 1024;

struct DenseLayout {
  float *h, *dz1, *dh_slab, *loss_part, *reg_part1, *reg_part2, *gbuf, *gb2buf;
  int32_t *cnt;
  uint32_t *km, *vm, *tb;
  size_t zero_begin, zero_end;
  int Bw, Nw, Bs, n_sub, out_grid;
  size_t lds_bytes;
  bool tile_path;               // k_out_dense_tile: the whole batch in LDS
};

static DenseLayout dense_layout(Carver &cv, const DrxCdaeParams &P, int B, bool per_row) {
  DenseLayout L{};
  const Geom gm = pick_geom(P.ld);
  const int R = kBlock / gm.G;
  const int n_tiles = (P.n_items + R - 1) / R;
  L.out_grid = n_tiles < kOutGrid ? n_tiles : kOutGrid;
  // LDS: 2*Bs*ld + R*ld + Bs*R floats
  size_t fixed = (size_t)R * P.ld * 4;
  size_t per_b = ((size_t)2 * P.ld + R) * 4;
  int Bs = (int)((kLdsBudget - fixed) / per_b);
  if (Bs > B) Bs = B;
  if (Bs < 1) Bs = 1;
  L.Bs = Bs;
  L.n_sub = (B + Bs - 1) / Bs;
  L.lds_bytes = fixed + per_b * Bs;
  L.tile_path = out_tile_lds_floats(B, P.ld) * 4 <= kLdsBudget / 2 && B <= 256;      // two workgroups per CU
  if (L.tile_path) {
    const int nt = (P.n_items + kTileR - 1) / kTileR;
    L.out_grid = nt < kOutGrid ? nt : kOutGrid;
    L.Bs = B; L.n_sub = 1;
    L.lds_bytes = out_tile_lds_floats(B, P.ld) * 4;
  }
  L.Bw = (B + 31) / 32;
  L.Nw = (P.n_items + 31) / 32;
  L.h = cv.take<float>((size_t)B * P.ld);
  L.dz1 = cv.take<float>((size_t)B * P.ld);
  L.dh_slab = cv.take<float>((size_t)L.out_grid * B * P.ld);
  L.loss_part = cv.take<float>(L.out_grid);
  L.reg_part1 = cv.take<float>(L.out_grid);
  L.reg_part2 = cv.take<float>(kSweepGrid + 1);
  L.gbuf = L.n_sub > 1 ? cv.take<float>((size_t)P.n_items * P.ld) : nullptr;
  L.gb2buf = L.n_sub > 1 ? cv.take<float>(P.n_items) : nullptr;
  cv.off = align_up(cv.off, 256);
  L.zero_begin = cv.off;
  L.cnt = cv.take<int32_t>(P.n_items);
  L.km = cv.take<uint32_t>((size_t)P.n_items * L.Bw);
  L.vm = cv.take<uint32_t>((size_t)P.n_users * L.Bw);
  L.tb = cv.take<uint32_t>((size_t)B * L.Nw);      // always reserved so the size does not depend on the mode
  L.zero_end = cv.off;
  (void)per_row;
  return L;
}

size_t dense_layout_bytes(const DrxCdaeParams &P, int B) {
  Carver c(nullptr, 0);
  (void)dense_layout(c, P, B, true);
  return c.off;
}

// the output layer's launch: its dynamic LDS may exceed the default limit, so the kernel is told first
using OutDenseKernel = void (*)(DrxCdaeParams, DrxOptim, OutDenseArgs);
static int launch_out_dense(OutDenseKernel kernel, const DenseLayout &L, const DrxCdaeParams &P, const DrxOptim &opt,
                            const OutDenseArgs &A, hipStream_t st) {
  DRX_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds_bytes));
  hipLaunchKernelGGL(kernel, dim3(L.out_grid), dim3(kBlock), L.lds_bytes, st, P, opt, A);
  return DRX_OK;
}

}  // namespace drx

using namespace drx;

extern "C" {

int drx_cdae_forward(const DrxCdaeParams *p, const DrxHistory *hist, const DrxBatch *bt, float *h, float *pred,
                     void *stream) {
  int rc = check_params(p);
  if (rc) return rc;
  rc = check_batch(hist, bt);
  if (rc || !h) return DRX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const float scale = 1.0f / (1.0f - bt->q);
  const uint32_t qthr = q_threshold(bt->q);
  DenseAux none{};
  return dispatch_geom(p->ld, [&](auto g) -> int {
    constexpr int G = decltype(g)::G, J = decltype(g)::J;
    constexpr int gpb = kBlock / G;
    if (bt->B <= kSmallBatch)
      hipLaunchKernelGGL((k_hidden_fwd_wg<G, J, 0>), dim3(bt->B), dim3(kBlock), (size_t)gpb * p->ld * 4, st, *p, *hist, *bt, scale, qthr,
                         h, none);
    else
      hipLaunchKernelGGL((k_hidden_fwd<G, J, 0>), dim3((bt->B + gpb - 1) / gpb), dim3(kBlock), 0, st, *p, *hist, *bt, scale, qthr, h,
                         none);
    if (pred) {
      int blocks = (p->n_items + gpb - 1) / gpb;
      if (blocks > 2048) blocks = 2048;
      hipLaunchKernelGGL((k_out_fwd<G, J>), dim3(blocks), dim3(kBlock), 0, st, *p, h, bt->B, pred);
    }
    DRX_LAUNCH_CHECK();
    return DRX_OK;
  });
}

static int step_dense_impl(const DrxCdaeParams *p, const DrxOptim *opt, const DrxHistory *hist, const DrxBatch *bt,
                           int32_t loss_kind, int32_t targets_kind, void *scratch, size_t scratch_bytes, float *loss_out,
                           void *stream, const DensePrefetch &pf) {
  int rc = check_params(p);
  if (rc) return rc;
  rc = check_batch(hist, bt);
  if (rc || !opt || !scratch) return DRX_EINVAL;
  if (!opt_dense_kind(opt->kind)) return DRX_EINVAL;
  for (int i = 0; i < 5; ++i)
    if (!opt_slots_ok(opt->kind, opt->s1[i], opt->s2[i])) return DRX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  Carver cv(scratch, scratch_bytes);
  // DRX_DENSE_AUX_CLEAN: the caller vouches that the batch-membership arrays in `scratch` are all zero — true for zero-initialised
  // scratch and after every completed dense step of the same batch size, because the kernels that consume an entry clear it
  const bool aux_clean = (targets_kind & DRX_DENSE_AUX_CLEAN) != 0;
  targets_kind &= 0xFF;
  const bool per_row = targets_kind == DRX_TARGETS_PER_ROW;
  DenseLayout L = dense_layout(cv, *p, bt->B, per_row);
  if (!cv.ok()) return DRX_ESCRATCH;
  const float scale = 1.0f / (1.0f - bt->q);
  const uint32_t qthr = q_threshold(bt->q);
  if (!aux_clean) DRX_HIP(hipMemsetAsync((char *)scratch + L.zero_begin, 0, L.zero_end - L.zero_begin, st));
  else if (per_row) DRX_HIP(hipMemsetAsync(L.tb, 0, (size_t)bt->B * L.Nw * 4, st));      // (target bits are shared by tiles: no single consumer)
  DenseAux aux{L.cnt, L.km, L.vm, per_row ? L.tb : nullptr, L.Bw, L.Nw};
  OutDenseArgs A{};
  A.h = L.h; A.cnt = L.cnt; A.tb = aux.tb; A.Nw = L.Nw; A.B = bt->B; A.Bs = L.Bs; A.n_sub = L.n_sub;
  A.gbuf = L.gbuf; A.gb2buf = L.gb2buf; A.dh_slab = L.dh_slab; A.loss_part = L.loss_part; A.reg_part = L.reg_part1;
  A.loss_kind = loss_kind;
  const int total_rows = p->n_items + p->n_users;
  return dispatch_opt_kind_keep_adam(opt->kind, [&](auto kc) -> int {
  constexpr int KIND = decltype(kc)::value;
  return dispatch_geom(p->ld, [&](auto g) -> int {
    constexpr int G = decltype(g)::G, J = decltype(g)::J;
    constexpr int gpb = kBlock / G;
    // a 256-thread workgroup keeps 4 * gpb history rows in flight per round: go wide when a row needs more than two rounds
    const bool wide_fwd = bt->B <= kFewRows && (int64_t)bt->n_touch_slots > (int64_t)bt->B * 8 * gpb;
    if (wide_fwd)               // few rows with long histories: 1024 threads per batch row (32 groups split the history)
      hipLaunchKernelGGL((k_hidden_fwd_wg<G, J, 1, 1024>), dim3(bt->B), dim3(1024), (size_t)(1024 / G) * p->ld * 4, st, *p, *hist, *bt,
                         scale, qthr, L.h, aux);
    else if (bt->B <= kSmallBatch)
      hipLaunchKernelGGL((k_hidden_fwd_wg<G, J, 1>), dim3(bt->B), dim3(kBlock), (size_t)gpb * p->ld * 4, st, *p, *hist, *bt, scale, qthr,
                         L.h, aux);
    else
      hipLaunchKernelGGL((k_hidden_fwd<G, J, 1>), dim3((bt->B + gpb - 1) / gpb), dim3(kBlock), 0, st, *p, *hist, *bt, scale, qthr, L.h,
                         aux);
    const OutDenseKernel out = L.tile_path ? (loss_out ? k_out_dense_tile<true, KIND> : k_out_dense_tile<false, KIND>)
                                           : (loss_out ? k_out_dense<G, J, true, KIND> : k_out_dense<G, J, false, KIND>);
    const int orc = launch_out_dense(out, L, *p, *opt, A, st);
    if (orc) return orc;
    if (bt->B <= kFewRows && L.out_grid > 16 * gpb)          // many partial slabs per row: 1024 threads fold them
      hipLaunchKernelGGL((k_hidden_bwd<G, J, 1024>), dim3(bt->B), dim3(1024), (size_t)(1024 / G) * p->ld * 4, st, p->ld, bt->B, L.out_grid,
                         L.dh_slab, L.h, L.dz1);
    else
      hipLaunchKernelGGL((k_hidden_bwd<G, J>), dim3(bt->B), dim3(kBlock), (size_t)gpb * p->ld * 4, st, p->ld, bt->B, L.out_grid,
                         L.dh_slab, L.h, L.dz1);
    int sweep = (total_rows + gpb - 1) / gpb;
    if (sweep > kSweepGrid) sweep = kSweepGrid;
    hipLaunchKernelGGL((k_in_sweep<G, J, KIND>), dim3(sweep + 1), dim3(kBlock), 0, st, *p, *opt, bt->B, scale, aux, L.dz1, L.reg_part2, pf);
    if (loss_out)
      hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(64), 0, st, L.loss_part, L.out_grid, L.reg_part1, L.out_grid, L.reg_part2, sweep + 1,
                         0.5f * opt->reg_rate / (float)bt->B, loss_out);
    DRX_LAUNCH_CHECK();
    return DRX_OK;
  });
  });
}

int drx_cdae_step_dense(const DrxCdaeParams *p, const DrxOptim *opt, const DrxHistory *hist, const DrxBatch *bt,
                        int32_t loss_kind, int32_t targets_kind, void *scratch, size_t scratch_bytes, float *loss_out,
                        void *stream) {
  return step_dense_impl(p, opt, hist, bt, loss_kind, targets_kind, scratch, scratch_bytes, loss_out, stream, DensePrefetch{});
}

// ---- the quiet fit() loop of reference mode in one call -------------------------------------------------------------------------
// What RecommenderABC.fit() does per epoch when nobody watches single steps (recommender_abc.py:189-205 with verbose off and no
// early-stopping rule): take the next drawn batch, queue its training step, keep the draw-ahead workers fed.  A staging slot
// (pinned, device-addressable) is laid out
//   [uid int32 B | keep_off int32 B+1 | keep u8 keep_capacity | iid int32 B | value f64 B | is_negative u8 B], every array 16-byte
// aligned: what a step reads comes first.  The step of batch s copies that prefix of batch s+1 into device memory from the last
// workgroup of its parameter sweep (k_in_sweep: one PCIe round trip hidden behind the sweep), so that the gather kernel of step
// s+1 reads its batch from HBM: 7.8 instead of 12.2 us at the ml-100k shape; only the first batch of a call is read in place.
struct FitSlot {
  size_t uid, keep_off, keep, iid, val, neg, total;
};
static FitSlot fit_slot_layout(int32_t B, int64_t keep_capacity) {
  FitSlot s{};
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off = align_up(off + bytes, 16); return at; };
  s.uid = take((size_t)B * 4);
  s.keep_off = take((size_t)(B + 1) * 4);
  s.keep = take((size_t)(keep_capacity > 0 ? keep_capacity : 1));
  s.iid = take((size_t)B * 4);
  s.val = take((size_t)B * 8);
  s.neg = take((size_t)B);
  s.total = align_up(off, 256);
  return s;
}

size_t drx_cdae_fit_slot_bytes(int32_t B, int64_t keep_capacity) {
  if (B < 1 || keep_capacity < 0) return 0;
  return fit_slot_layout(B, keep_capacity).total;
}

int drx_cdae_fit_dense(const DrxCdaeParams *p, const DrxOptim *opt, const DrxHistory *hist, DrxDrawAhead *draws, int64_t *cursor,
                       int32_t B, float q, int64_t keep_capacity, int32_t loss_kind, int32_t targets_kind, int64_t n_steps,
                       const float *h_alphas, void *h_slots, size_t slot_bytes, int32_t n_slots, void *d_stage,
                       size_t d_stage_bytes, void *scratch, size_t scratch_bytes, void *stream) {
  constexpr int kAhead = 4;             // draws in flight beyond the two batches the loop holds: two per worker
  constexpr int kMaxSlots = 64;
  if (!p || !opt || !hist || !draws || !cursor || !h_alphas || !h_slots || !scratch || B < 1 || n_steps < 0 || keep_capacity < 0)
    return DRX_EINVAL;
  if (n_slots < kAhead + 4 || n_slots > kMaxSlots) return DRX_EINVAL;
  const FitSlot S = fit_slot_layout(B, keep_capacity);
  if (slot_bytes < S.total) return DRX_ESCRATCH;
  if (d_stage && d_stage_bytes < 2 * S.iid) return DRX_ESCRATCH;       // two device copies of the prefix a step reads
  hipStream_t st = (hipStream_t)stream;
  hipEvent_t ev[kMaxSlots] = {};
  bool busy[kMaxSlots] = {};
  for (int k = 0; k < n_slots; ++k)
    if (hipEventCreateWithFlags(&ev[k], hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess) {
      for (int j = 0; j < k; ++j) (void)hipEventDestroy(ev[j]);
      return DRX_EINVAL;
    }
  int64_t ticket = cursor[0];
  uint64_t mask_pos = (uint64_t)cursor[1], mask_at[2] = {(uint64_t)cursor[2], (uint64_t)cursor[3]};
  const uint64_t words = (uint64_t)2 * (uint64_t)p->n_items * (uint64_t)B;      // cdae.py:63: N uniform draws per batch row
  struct Pending { int gen; int64_t job; int slot; } ring[kAhead + 1];
  int head = 0, count = 0;
  int64_t next_slot = 0, submitted = 0;
  int rc = DRX_OK;
  hipError_t herr = hipSuccess;
  auto slot_at = [&](int k) { return (char *)h_slots + (size_t)k * slot_bytes; };
  auto submit = [&]() -> int {
    const int k = (int)(next_slot % n_slots);
    if (busy[k]) {                      // the step that last read this slot must have finished before a worker refills it
      if ((herr = hipEventSynchronize(ev[k])) != hipSuccess) return (int)herr;
      busy[k] = false;
    }
    char *b = slot_at(k);
    const int gen = (int)(ticket & 1);
    const int64_t job = drx_drawahead_submit(draws, gen, ticket, mask_pos - mask_at[gen], B, (double)q, (int32_t *)(b + S.uid),
                                             (int32_t *)(b + S.iid), (double *)(b + S.val), (uint8_t *)(b + S.neg),
                                             (int32_t *)(b + S.keep_off), (uint8_t *)(b + S.keep), keep_capacity > 0 ? keep_capacity : 1);
    if (job < 0) return (int)job;
    ++next_slot; ++ticket; ++submitted;
    mask_pos += words;
    mask_at[gen] = mask_pos;
    ring[(head + count) % (kAhead + 1)] = Pending{gen, job, k};
    ++count;
    return DRX_OK;
  };
  // never beyond the last step: the sampler and corruption streams end where the reference's do
  auto refill = [&]() { while (rc == DRX_OK && count < kAhead && submitted < n_steps) rc = submit(); };
  auto take = [&](Pending &out) {       // the oldest draw in flight, completed
    out = ring[head];
    head = (head + 1) % (kAhead + 1);
    --count;
    const int wrc = drx_drawahead_wait(draws, out.gen, out.job);
    if (rc == DRX_OK) rc = wrc;
  };
  DrxOptim o = *opt;
  Pending cur{}, nxt{};
  bool have_nxt = false;
  int64_t s = 0;
  if (n_steps > 0) {
    refill();
    if (rc == DRX_OK) take(cur);
  }
  for (; s < n_steps && rc == DRX_OK; ++s) {
    refill();
    if (rc) break;
    have_nxt = false;
    if (s + 1 < n_steps) {
      take(nxt);
      have_nxt = true;
      refill();
      if (rc) break;
    }
    const char *hb = slot_at(cur.slot);
    const bool on_device = d_stage && s > 0;          // (copied there by the previous step's sweep)
    const char *b = on_device ? (const char *)d_stage + (size_t)(s & 1) * S.iid : hb;
    DrxBatch bt{};
    bt.B = B;
    bt.uid = (const int32_t *)(b + S.uid);
    bt.keep_off = (const int32_t *)(b + S.keep_off);
    bt.keep = (const uint8_t *)(b + S.keep);
    bt.q = q;
    bt.n_touch_slots = ((const int32_t *)(hb + S.keep_off))[B];
    DensePrefetch pf{};
    if (have_nxt && d_stage) {
      const char *nb = slot_at(nxt.slot);
      const int32_t n_keep = ((const int32_t *)(nb + S.keep_off))[B];
      pf.src = (const uint4 *)nb;
      pf.dst = (uint4 *)((char *)d_stage + (size_t)((s + 1) & 1) * S.iid);
      pf.n16 = (S.keep + (size_t)(n_keep > 0 ? n_keep : 1) + 15) / 16;
    }
    for (int j = 0; j < 5; ++j) o.alpha[j] = h_alphas[s * 5 + j];
    rc = step_dense_impl(p, &o, hist, &bt, loss_kind, targets_kind | DRX_DENSE_AUX_CLEAN, scratch, scratch_bytes, nullptr, stream, pf);
    if (rc) break;
    // this step is the last reader of its own slot when it read it in place, and of the next batch's slot when it copied it
    const int released = pf.n16 ? nxt.slot : (on_device ? -1 : cur.slot);
    if (!on_device && pf.n16) {         // (first step of a call: both)
      if ((herr = hipEventRecord(ev[cur.slot], st)) != hipSuccess) { rc = (int)herr; break; }
      busy[cur.slot] = true;
    }
    if (released >= 0) {
      if ((herr = hipEventRecord(ev[released], st)) != hipSuccess) { rc = (int)herr; break; }
      busy[released] = true;
    }
    cur = nxt;
  }
  // draws still in flight write into the caller's slots: wait for them whatever happened (their place in the streams is consumed)
  while (count > 0) { Pending drop; take(drop); }
  cursor[0] = ticket;
  cursor[1] = (int64_t)mask_pos;
  cursor[2] = (int64_t)mask_at[0];
  cursor[3] = (int64_t)mask_at[1];
  // the slots are free for the caller's next run once the steps queued here have read them (the events do not outlive the call)
  herr = hipStreamSynchronize(st);
  if (rc == DRX_OK && herr != hipSuccess) rc = (int)herr;
  for (int k = 0; k < n_slots; ++k) (void)hipEventDestroy(ev[k]);
  return rc;
}

}  // extern "C"
