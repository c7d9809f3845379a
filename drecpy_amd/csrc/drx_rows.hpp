// Row-group device helpers shared by the libdrx.so kernels (gfx950): coalesced float4 row access for a group of G
// lanes, the hidden-layer activation, the embedding-bag gather, Keras optimizer updates, deterministic block reduction.
#pragma once
#include "drx_common.hpp"

#ifndef DRX_GATHER_ROWS
#define DRX_GATHER_ROWS 8
#endif
// 1: a round's rows in flight are formed from the history's KEPT entries only (gather_bag, groups of up to 32 lanes); 0 (a variant
// build): from consecutive entries, a dropped one leaving its place empty
#ifndef DRX_GATHER_PACKED
#define DRX_GATHER_PACKED 1
#endif

namespace drx {

template <int G, int J>
__device__ __forceinline__ void load_row(const float *base, size_t row, int ld, int lane, float4 (&v)[J]) {
  const float4 *r = reinterpret_cast<const float4 *>(base + row * (size_t)ld);
#pragma unroll
  for (int j = 0; j < J; ++j) {
    int c = lane + j * G;
    v[j] = (4 * c < ld) ? r[c] : f4_zero();
  }
}

template <int G, int J>
__device__ __forceinline__ void store_row(float *base, size_t row, int ld, int lane, const float4 (&v)[J]) {
  float4 *r = reinterpret_cast<float4 *>(base + row * (size_t)ld);
#pragma unroll
  for (int j = 0; j < J; ++j) {
    int c = lane + j * G;
    if (4 * c < ld) r[c] = v[j];
  }
}

// the lanes of this thread's row group for which f holds (bit i: lane i of the group)
template <int G>
__device__ __forceinline__ unsigned long long group_ballot(bool f) {
  const unsigned long long m = __ballot(f);
  if (G >= 64) return m;
  const int sh = ((int)(threadIdx.x & 63) / G) * G;
  return (m >> sh) & ((1ull << (G & 63)) - 1ull);
}

__device__ __forceinline__ float colmask(int col, int k, float v) { return col < k ? v : 0.0f; }

// h = sigmoid(scale*bag + V[u] + b), zero in the padding columns (v, bb: the rows V[u] and b).
template <int G, int J>
__device__ __forceinline__ void hidden_act_rows(const DrxCdaeParams &P, float scale, int lane, const float4 (&acc)[J], const float4 (&v)[J],
                                                const float4 (&bb)[J], float4 (&h)[J]) {
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int col = 4 * (lane + j * G);
    h[j].x = colmask(col + 0, P.k, sigmoidf_(fmaf(scale, acc[j].x, v[j].x + bb[j].x)));
    h[j].y = colmask(col + 1, P.k, sigmoidf_(fmaf(scale, acc[j].y, v[j].y + bb[j].y)));
    h[j].z = colmask(col + 2, P.k, sigmoidf_(fmaf(scale, acc[j].z, v[j].z + bb[j].z)));
    h[j].w = colmask(col + 3, P.k, sigmoidf_(fmaf(scale, acc[j].w, v[j].w + bb[j].w)));
  }
}
template <int G, int J>
__device__ __forceinline__ void hidden_act(const DrxCdaeParams &P, int u, float scale, int lane,
                                           const float4 (&acc)[J], float4 (&h)[J]) {
  float4 v[J], bb[J];
  load_row<G, J>(P.V, (size_t)u, P.ld, lane, v);
  load_row<G, J>(P.b, 0, P.ld, lane, bb);
  hidden_act_rows<G, J>(P, scale, lane, acc, v, bb, h);
}

// ------------------------------------------------------------------------------------------------
// the input bag of one batch row (both modes: the sampled step's forward kernels in drx_cdae.hip, reference mode's in
// drx_cdae_dense.hip) and the auxiliary per-step index the hidden-layer kernel builds in reference ("dense") mode
// ------------------------------------------------------------------------------------------------
struct DenseAux {
  int32_t *cnt;    // [N]       #batch rows having item n as a positive  -> batch-mean target
  uint32_t *km;    // [N, Bw]   bit b set: item n is a surviving (kept) input of batch row b
  uint32_t *vm;    // [U, Bw]   bit b set: batch row b belongs to user u
  uint32_t *tb;    // [B, Nw]   per-row target bits (DRX_TARGETS_PER_ROW) or nullptr
  int32_t Bw, Nw;
};

// Gathers scale * sum_{kept} W[n] for one batch row.  MODE 0: plain; 1: also builds DenseAux;
// 2: also emits the (key,val) touch list of the sampled mode.
template <int G, int J, int MODE>
__device__ __forceinline__ void gather_bag(const DrxCdaeParams &P, const DrxHistory &H, const DrxBatch &bt,
                                           uint32_t qthr, int b, int lane, float4 (&acc)[J],
                                           const DenseAux &aux, uint32_t *tkeys, uint32_t *tvals,
                                           int touch_base, int part = 0, int nparts = 1, unsigned long long *stamps = nullptr) {
  (void)stamps;
#pragma unroll
  for (int j = 0; j < J; ++j) acc[j] = f4_zero();
  const int u = bt.uid[b];
  const int64_t s = H.indptr[u], e = H.indptr[u + 1];
#ifdef DRX_STAMPS
  if (s >= 0) DRX_STAMP(stamps, b, 2, lane);          // (uses s: the stamp waits for the row pointers)
  bool first_rows = true;
#endif
  const uint8_t *kp = bt.keep ? bt.keep + bt.keep_off[b] : nullptr;
  // a group fetches CH history entries per round: its G lanes hold IPL each, so that narrow groups (rows of <= 32 floats:
  // G = 4 or 8) do not walk the history in rounds of 4 or 8 dependent index loads
  constexpr int IPL = G >= 16 ? 1 : 16 / G;
  constexpr int CH = G * IPL;
  for (int64_t c = s + (int64_t)part * CH; c < e; c += (int64_t)nparts * CH) {
    int idx[IPL], kf[IPL];
#pragma unroll
    for (int r = 0; r < IPL; ++r) {
      const int64_t j = c + r * G + lane;
      idx[r] = -1; kf[r] = 0;
      if (j < e) {
        idx[r] = H.indices[j];
        const uint32_t jj = (uint32_t)(j - s);
        kf[r] = kp ? (kp[jj] != 0) : (hash_u32(bt.mask_seed, (uint32_t)b, jj) >= qthr);
        if (MODE == 1) {
          atomicAdd(&aux.cnt[idx[r]], 1);
          if (aux.tb) atomicOr(&aux.tb[(size_t)b * aux.Nw + (idx[r] >> 5)], 1u << (idx[r] & 31));
          if (kf[r]) atomicOr(&aux.km[(size_t)idx[r] * aux.Bw + (b >> 5)], 1u << (b & 31));
        }
        if (MODE == 2) {
          tkeys[touch_base + jj] = kf[r] ? (uint32_t)idx[r] : DRX_KEY_NONE;
          tvals[touch_base + jj] = (uint32_t)b;
        }
      }
    }
    constexpr int NF = J == 1 ? DRX_GATHER_ROWS : 4;       // rows in flight per group
#ifdef DRX_STAMPS
    if (first_rows && idx[0] >= -1) DRX_STAMP(stamps, b, 3, lane);      // (uses idx: the stamp waits for the indices)
#endif
    // the rows in flight of a round are the next NF KEPT entries, in history order: a dropped entry takes no place among them (bit tt of
    // `left`: entry tt of this fetch is kept and not yet loaded; the same value in every lane of the group).  The kept rows enter acc in
    // the order they always did, and the all-zero rows that no longer stand between them changed no sum.  (Groups of 64 lanes keep
    // consecutive entries: a 64-bit mask costs their kernels the eighth wave per SIMD.)
    if constexpr (DRX_GATHER_PACKED != 0 && CH <= 32) {
      uint32_t left = 0;
#pragma unroll
      for (int rr = 0; rr < IPL; ++rr) left |= (uint32_t)group_ballot<G>(kf[rr] != 0) << (rr * G);
      while (left) {
        float4 r[NF][J];
#pragma unroll
        for (int q = 0; q < NF; ++q) {
          const bool on = left != 0;
          const int tt = on ? __builtin_ctz(left) : 0;
          left &= left - 1;                                   // (0 stays 0)
          int si = idx[0];
#pragma unroll
          for (int rr = 1; rr < IPL; ++rr) si = (tt / G == rr) ? idx[rr] : si;
          const int iq = __shfl(si, tt % G, G);
#pragma unroll
          for (int jx = 0; jx < J; ++jx) r[q][jx] = f4_zero();
          if (on) load_row<G, J>(P.W, (size_t)iq, P.ld, lane, r[q]);
        }
#pragma unroll
        for (int q = 0; q < NF; ++q)
#pragma unroll
          for (int jx = 0; jx < J; ++jx) f4_add(acc[jx], r[q][jx]);
#ifdef DRX_STAMPS
        if (first_rows && acc[0].x == acc[0].x) { DRX_STAMP(stamps, b, 4, lane); first_rows = false; }      // (uses acc: after the first rows landed)
#endif
      }
    } else {
      const int n_here = (int)((e - c) < (int64_t)CH ? (e - c) : (int64_t)CH);
      for (int t = 0; t < n_here; t += NF) {
        float4 r[NF][J];
#pragma unroll
        for (int q = 0; q < NF; ++q) {
          const int tt = t + q;
          int si = idx[0], sk = kf[0];
#pragma unroll
          for (int rr = 1; rr < IPL; ++rr) { si = (tt / G == rr) ? idx[rr] : si; sk = (tt / G == rr) ? kf[rr] : sk; }
          const int iq = __shfl(si, tt % G, G);
          const int kq = (tt < n_here) ? __shfl(sk, tt % G, G) : 0;
#pragma unroll
          for (int jx = 0; jx < J; ++jx) r[q][jx] = f4_zero();
          if (kq) load_row<G, J>(P.W, (size_t)iq, P.ld, lane, r[q]);
        }
#pragma unroll
        for (int q = 0; q < NF; ++q)
#pragma unroll
          for (int jx = 0; jx < J; ++jx) f4_add(acc[jx], r[q][jx]);
#ifdef DRX_STAMPS
        if (first_rows && acc[0].x == acc[0].x) { DRX_STAMP(stamps, b, 4, lane); first_rows = false; }      // (uses acc: after the first rows landed)
#endif
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// optimizer row updates (fp32, Keras formulas)
// ------------------------------------------------------------------------------------------------
struct OptScalars {
  int kind;
  float lr, rb;              // rb = reg_rate / B
  float b1, b2, eps, alpha;  // alpha = Keras-Adam lr_t of the variable being updated
  float inv_k = 0.f;         // 1 / K (row-wise Adagrad: mean of the squared gradient over the K columns)
};

// KIND >= 0: the optimizer is known at compile time (the sparse step's Adagrad instantiation: the segmented reduction then needs 64
// instead of 90 VGPRs — 8 waves per SIMD instead of 5); KIND < 0: o.kind decides at run time.
template <int KIND = -1>
__device__ __forceinline__ void opt_update1(const OptScalars &o, float g, float &p, float &s1, float &s2) {
  const int kind = KIND >= 0 ? KIND : o.kind;
  if (kind == DRX_OPT_ADAM) {
    // TF's ApplyAdam functor, operation for operation (1 - beta is formed in fp32 there too)
    s1 = s1 + (g - s1) * (1.0f - o.b1);
    s2 = s2 + (g * g - s2) * (1.0f - o.b2);
    p = p - (s1 * o.alpha) / (sqrtf(s2) + o.eps);
  } else {
    s1 = s1 + g * g;
    p = p - o.lr * g / (sqrtf(s1) + o.eps);
  }
}

// Applies g (data gradient, already complete) + rb*p to one row of `tab` with slots s1/s2.
template <int G, int J, int KIND = -1>
__device__ __forceinline__ float row_update(const OptScalars &o, float *tab, float *s1, float *s2, size_t row, int ld,
                                            int lane, const float4 (&w)[J], const float4 (&g)[J]) {
  float sq = 0.f;
  float4 *pr = reinterpret_cast<float4 *>(tab + row * (size_t)ld);
  const int kind = KIND >= 0 ? KIND : o.kind;
  if (kind == DRX_OPT_ROWWISE_ADAGRAD) {
    // one accumulator per row (first float of the row's slot): the optimizer state costs 4 bytes of traffic per row, not 4K
    float4 gg[J];
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const float4 p = w[j];
      gg[j].x = fmaf(o.rb, p.x, g[j].x); gg[j].y = fmaf(o.rb, p.y, g[j].y);
      gg[j].z = fmaf(o.rb, p.z, g[j].z); gg[j].w = fmaf(o.rb, p.w, g[j].w);
      q += f4_dot(gg[j], gg[j]);
      sq += f4_dot(p, p);
    }
    q = group_sum<G>(q) * o.inv_k;
    const float acc = s1[row * (size_t)ld] + q;
    const float step = o.lr / (sqrtf(acc) + o.eps);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int c = lane + j * G;
      if (4 * c < ld) {
        float4 p = w[j];
        p.x -= step * gg[j].x; p.y -= step * gg[j].y; p.z -= step * gg[j].z; p.w -= step * gg[j].w;
        pr[c] = p;
      }
    }
    if (lane == 0) s1[row * (size_t)ld] = acc;
    return sq;
  }
  float4 *a1 = reinterpret_cast<float4 *>(s1 + row * (size_t)ld);
  float4 *a2 = (kind == DRX_OPT_ADAM) ? reinterpret_cast<float4 *>(s2 + row * (size_t)ld) : nullptr;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int c = lane + j * G;
    if (4 * c < ld) {
      float4 p = w[j];
      float4 m = a1[c];
      float4 v = a2 ? a2[c] : f4_zero();
      sq += f4_dot(p, p);
      opt_update1<KIND>(o, fmaf(o.rb, p.x, g[j].x), p.x, m.x, v.x);
      opt_update1<KIND>(o, fmaf(o.rb, p.y, g[j].y), p.y, m.y, v.y);
      opt_update1<KIND>(o, fmaf(o.rb, p.z, g[j].z), p.z, m.z, v.z);
      opt_update1<KIND>(o, fmaf(o.rb, p.w, g[j].w), p.w, m.w, v.w);
      pr[c] = p;
      a1[c] = m;
      if (a2) a2[c] = v;
    }
  }
  return sq;   // partial |row|^2 of this lane (pre-update), for the L2 loss value
}

__device__ __forceinline__ OptScalars opt_for(const DrxOptim &opt, int var, int B) {
  OptScalars o;
  o.kind = opt.kind; o.lr = opt.lr; o.rb = opt.reg_rate / (float)B;
  o.b1 = opt.beta1; o.b2 = opt.beta2; o.eps = opt.eps; o.alpha = opt.alpha[var];
  return o;
}

// Deterministic block reduction of one float per thread -> thread 0 holds the sum.
__device__ __forceinline__ float block_sum(float v, float *red /* [blockDim.x/64] in LDS */) {
  v = group_sum<64>(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x == 0)
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
  return t;
}

}  // namespace drx
