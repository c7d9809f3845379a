// NeuMF (He et al. 2017; include/drx.h "NeuMF"): the fused GMF + MLP training step, the half rows of serving and
// the all-item / pair scorer.  Every dense product runs on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate) out of LDS, M = a tile of 16
// samples / rows / pairs.  Operand layout (lane l): A[l % 16][l / 16], B[l / 16][l % 16], C register r = C[4 (l / 16) + r][l % 16].
//   drx_ncf_step        : k_ncf_tile -> k_small_opt (drx_small.hpp: partials in workgroup order + the rule on sw) -> drx_batch_csr_device (user keys,
//                         item keys) -> ONE drx_rows_csr_opt_multi (U plain, V plain).  No atomics.
//   drx_ncf_half_rows   : [W_1 half^T row + b_1 | hg (.) Pg]  /  [W_1 half^T row | Qg]
//   drx_ncf_score_rows / drx_ncf_pair_scores : ncf_tile_logit, ONE definition of a pair's sums, for strips of the catalogue and for pairs.
#include "drx_common.hpp"
#include "drx_rows.hpp"
#include "drx_opt.hpp"
#include "drx_step.hpp"
#include "drx_small.hpp"

namespace drx {

typedef float ncf_f4v __attribute__((ext_vector_type(4)));
constexpr int kNcfMaxW = 64;                      // the widest layer and the widest half of a table row
constexpr int kNcfTS = 68;                        // floats per row of a 16-row tile in LDS (rows fall in 16 different bank quads)
constexpr int kNcfTS0 = 132;                      // the same for rows of up to 128 floats (a_0 = [Pm | Qm] and its gradient)
constexpr int kNcfMaxGrid = 256;

static int ncf_round4(int x) { return (x + 3) & ~3; }

// the dims describe the layout of include/drx.h exactly
static bool ncf_dims_ok(const DrxNcfDims *D) {
  if (!D || D->n_users < 1 || D->n_items < 1 || D->kg < 1 || D->kg > kNcfMaxW || D->km < 1 || D->km > kNcfMaxW) return false;
  if (D->ldg != ncf_round4(D->kg) || D->ldm != ncf_round4(D->km) || D->n_layers < 1 || D->n_layers > DRX_NCF_MAX_LAYERS) return false;
  int off = 0, fin = 2 * D->km;
  for (int l = 0; l < D->n_layers; ++l) {
    const int fo = D->f[l];
    if (fo < 1 || fo > kNcfMaxW || D->off_w[l] != off || D->off_b[l] != off + fin * fo) return false;
    off += fin * fo + fo;
    fin = fo;
  }
  return D->off_h == off && D->off_b0 == off + D->kg + fin && D->n_small == off + D->kg + fin + 1;
}

// acc (16 x 16) = X [16 x fin] (rows of xs floats) . W [fin x fo] (row-major), columns col0 .. col0 + 15: k ascending in steps of 4
__device__ __forceinline__ ncf_f4v ncf_mfma_xw(const float *X, int xs, const float *W, int fin, int fo, int col0, int m16, int q4) {
  ncf_f4v acc = {0.f, 0.f, 0.f, 0.f};
  const int col = col0 + m16;
  for (int k0 = 0; k0 < fin; k0 += 4) {
    const int kk = k0 + q4;
    const float a = kk < fin ? X[m16 * xs + kk] : 0.f;
    const float b = (kk < fin && col < fo) ? W[kk * fo + col] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// acc (16 x 16) = G [16 x fo] (rows of gs floats) . W^T (W [fin x fo] row-major), columns (rows of W) row0 .. row0 + 15
__device__ __forceinline__ ncf_f4v ncf_mfma_gwt(const float *G, int gs, const float *W, int fin, int fo, int row0, int m16, int q4) {
  ncf_f4v acc = {0.f, 0.f, 0.f, 0.f};
  const int row = row0 + m16;
  for (int k0 = 0; k0 < fo; k0 += 4) {
    const int kk = k0 + q4;
    const float a = kk < fo ? G[m16 * gs + kk] : 0.f;
    const float b = (kk < fo && row < fin) ? W[row * fo + kk] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

__device__ __forceinline__ int ncf_fin(const DrxNcfDims &D, int l) { return l == 0 ? 2 * D.km : D.f[l - 1]; }

// ---- the step ----------------------------------------------------------------------------------------------------------------------------
// LDS: [n_small] weights | A0 [16][132] | A [4][16][68] | G [16][132] | GP, GQ [16][68] | gsm [16] | le [16]
static size_t ncf_tile_lds(const DrxNcfDims *D) {
  return sizeof(float) * ((size_t)ncf_round4(D->n_small) + 2 * 16 * kNcfTS0 + (DRX_NCF_MAX_LAYERS + 2) * 16 * kNcfTS + 32);
}

__global__ __launch_bounds__(256) void k_ncf_tile(DrxNcfDims D, const float *__restrict__ U, const float *__restrict__ V,
                                                  const float *__restrict__ sw, const int32_t *__restrict__ uid,
                                                  const int32_t *__restrict__ iid, const float *__restrict__ y, int B,
                                                  float *__restrict__ dU, float *__restrict__ dV, float *__restrict__ gsw_part,
                                                  double *__restrict__ loss_part) {
  extern __shared__ __align__(16) float lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m16 = lane & 15, q4 = lane >> 4;
  const int ts = threadIdx.x >> 4, tj = threadIdx.x & 15;            // the row-wise passes: 16 threads per sample
  float *const swl = lds;
  float *const A0 = swl + ((D.n_small + 3) & ~3);
  float *const A = A0 + 16 * kNcfTS0;                                 // A[(l) * 16 * 68 + s * 68 + c] = a_{l + 1}
  float *const G = A + DRX_NCF_MAX_LAYERS * 16 * kNcfTS;
  float *const GP = G + 16 * kNcfTS0;
  float *const GQ = GP + 16 * kNcfTS;
  float *const gsm = GQ + 16 * kNcfTS;
  float *const le = gsm + 16;
  for (int i = threadIdx.x; i < D.n_small; i += 256) swl[i] = sw[i];
  const int ld = D.ldg + D.ldm, n = D.n_layers, fn = D.f[n - 1];
  const float inv_b = 1.0f / (float)B;
  const float *const hg = swl + D.off_h, *const hm = hg + D.kg;
  float *const part = gsw_part + (size_t)blockIdx.x * D.n_small;
  const int n_tiles = (B + 15) / 16;
  double loss = 0.0;
  bool first = true;                                                  // the workgroup's first tile writes its row of partials, the others add
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int b0 = tile * 16;
    __syncthreads();                                                  // (the weights' copy; the previous tile's rows are free)
    // ---- gather: the two table rows of each sample; the GMF halves to GP / GQ, the MLP halves side by side to A0
    {
      const int b = b0 + ts;
      const size_t u = b < B ? (size_t)uid[b] : 0, i = b < B ? (size_t)iid[b] : 0;
      for (int c = tj; c < ld / 4; c += 16) {
        float4 pu = f4_zero(), qi = f4_zero();
        if (b < B) {
          pu = reinterpret_cast<const float4 *>(U + u * ld)[c];
          qi = reinterpret_cast<const float4 *>(V + i * ld)[c];
        }
        const float pa[4] = {pu.x, pu.y, pu.z, pu.w}, qa[4] = {qi.x, qi.y, qi.z, qi.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = 4 * c + e;
          if (col < D.ldg) {
            GP[ts * kNcfTS + col] = pa[e];
            GQ[ts * kNcfTS + col] = qa[e];
          } else if (col - D.ldg < D.km) {
            A0[ts * kNcfTS0 + col - D.ldg] = pa[e];
            A0[ts * kNcfTS0 + D.km + col - D.ldg] = qa[e];
          }
        }
      }
    }
    __syncthreads();
    // ---- forward: a wave takes the 16-column tile `wv` of every layer
#pragma unroll 1
    for (int l = 0; l < n; ++l) {
      const int fin = ncf_fin(D, l), fo = D.f[l];
      if (wv * 16 < fo) {
        const ncf_f4v acc = l == 0 ? ncf_mfma_xw(A0, kNcfTS0, swl + D.off_w[0], fin, fo, wv * 16, m16, q4)
                                   : ncf_mfma_xw(A + (l - 1) * 16 * kNcfTS, kNcfTS, swl + D.off_w[l], fin, fo, wv * 16, m16, q4);
        const int col = wv * 16 + m16;
        const float bias = col < fo ? swl[D.off_b[l] + col] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) A[l * 16 * kNcfTS + (4 * q4 + r) * kNcfTS + col] = col < fo ? fmaxf(acc[r] + bias, 0.f) : 0.f;
      }
      __syncthreads();
    }
    // ---- per sample (wave 0; lane = sample m16, quarter q4 of the columns): logit, loss, g
    if (wv == 0) {
      const float *const an = A + (n - 1) * 16 * kNcfTS + m16 * kNcfTS;
      float s = 0.f, gm = 0.f;
      for (int c = q4 * 16; c < q4 * 16 + 16 && c < fn; ++c) s = fmaf(hm[c], an[c], s);
      for (int k = q4 * 16; k < q4 * 16 + 16 && k < D.kg; ++k) gm = fmaf(hg[k] * GP[m16 * kNcfTS + k], GQ[m16 * kNcfTS + k], gm);
      s += __shfl_xor(s, 16); s += __shfl_xor(s, 32);
      gm += __shfl_xor(gm, 16); gm += __shfl_xor(gm, 32);
      const float x = (s + gm) + swl[D.off_b0];
      const int b = b0 + m16;
      if (q4 == 0) {
        const float yb = b < B ? y[b] : 0.f;
        gsm[m16] = b < B ? (1.0f / (1.0f + expf(-x)) - yb) * inv_b : 0.f;
        le[m16] = b < B ? fmaxf(x, 0.f) - yb * x + log1pf(expf(-fabsf(x))) : 0.f;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int s_ = 0; s_ < 16; ++s_) loss += (double)le[s_];
    // ---- dZ_n = g hm where a_n > 0; the gradients of h and b0 (one thread per entry, samples ascending)
    for (int c = tj; c < fn; c += 16) G[ts * kNcfTS0 + c] = A[(n - 1) * 16 * kNcfTS + ts * kNcfTS + c] > 0.f ? gsm[ts] * hm[c] : 0.f;
    {
      const int t = threadIdx.x;
      if (t <= D.kg + fn) {
        float g = 0.f;
        if (t < D.kg) {
          for (int s_ = 0; s_ < 16; ++s_) g = fmaf(gsm[s_], GP[s_ * kNcfTS + t] * GQ[s_ * kNcfTS + t], g);
        } else if (t < D.kg + fn) {
          for (int s_ = 0; s_ < 16; ++s_) g = fmaf(gsm[s_], A[(n - 1) * 16 * kNcfTS + s_ * kNcfTS + t - D.kg], g);
        } else {
          for (int s_ = 0; s_ < 16; ++s_) g += gsm[s_];
        }
        part[D.off_h + t] = first ? g : part[D.off_h + t] + g;
      }
    }
    __syncthreads();
    // ---- backward: G holds dZ_l; db_l, dW_l = A_{l-1}^T dZ_l, then dA_{l-1} = dZ_l W_l^T -> dZ_{l-1} overwrites G
#pragma unroll 1
    for (int l = n - 1; l >= 0; --l) {
      const int fin = ncf_fin(D, l), fo = D.f[l];
      const float *const Ain = l == 0 ? A0 : A + (l - 1) * 16 * kNcfTS;
      const int as = l == 0 ? kNcfTS0 : kNcfTS;
      if ((int)threadIdx.x < fo) {
        float g = 0.f;
        for (int s_ = 0; s_ < 16; ++s_) g += G[s_ * kNcfTS0 + threadIdx.x];
        const int at = D.off_b[l] + threadIdx.x;
        part[at] = first ? g : part[at] + g;
      }
      const int nto = (fo + 15) / 16, nti = (fin + 15) / 16;
      for (int ti = wv; ti < nti * nto; ti += 4) {                    // dW_l tile (mi, ni): M = 16 rows of W_l, K = the 16 samples
        const int mi = ti / nto, ni = ti % nto;
        const int arow = mi * 16 + m16, gcol = ni * 16 + m16;
        ncf_f4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int kk = 4 * ks + q4;
          const float a = arow < fin ? Ain[kk * as + arow] : 0.f;
          const float b = gcol < fo ? G[kk * kNcfTS0 + gcol] : 0.f;
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = mi * 16 + 4 * q4 + r;
          if (row < fin && gcol < fo) {
            const int at = D.off_w[l] + row * fo + gcol;
            part[at] = first ? acc[r] : part[at] + acc[r];
          }
        }
      }
      ncf_f4v da[2] = {ncf_f4v{0.f, 0.f, 0.f, 0.f}, ncf_f4v{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int j = 0; j < 2; ++j)                                     // this wave's tiles of the up to 8 of dA_{l-1}
        if ((wv + 4 * j) * 16 < fin) da[j] = ncf_mfma_gwt(G, kNcfTS0, swl + D.off_w[l], fin, fo, (wv + 4 * j) * 16, m16, q4);
      __syncthreads();                                                // (every wave has read dZ_l: the tile may be overwritten)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = (wv + 4 * j) * 16 + m16;
        if (col < fin) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int s_ = 4 * q4 + r;
            G[s_ * kNcfTS0 + col] = (l == 0 || Ain[s_ * as + col] > 0.f) ? da[j][r] : 0.f;
          }
        }
      }
      __syncthreads();
    }
    // ---- the samples' gradient rows: [g hg (.) other side's GMF half | the side's half of dA_0], padding zero
    {
      const int b = b0 + ts;
      if (b < B) {
        const float g = gsm[ts];
        for (int c = tj; c < ld / 4; c += 16) {
          float vu[4], vv[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int col = 4 * c + e, k = col - D.ldg;
            if (col < D.ldg) {
              const float gh = col < D.kg ? g * hg[col] : 0.f;
              vu[e] = gh * GQ[ts * kNcfTS + col];
              vv[e] = gh * GP[ts * kNcfTS + col];
            } else {
              vu[e] = k < D.km ? G[ts * kNcfTS0 + k] : 0.f;
              vv[e] = k < D.km ? G[ts * kNcfTS0 + D.km + k] : 0.f;
            }
          }
          reinterpret_cast<float4 *>(dU + (size_t)b * ld)[c] = make_float4(vu[0], vu[1], vu[2], vu[3]);
          reinterpret_cast<float4 *>(dV + (size_t)b * ld)[c] = make_float4(vv[0], vv[1], vv[2], vv[3]);
        }
      }
    }
    first = false;
  }
  if (threadIdx.x == 0) loss_part[blockIdx.x] = loss;
}

struct NcfScratch {
  float *dU, *dV, *gsw_part;
  double *loss_part;
  int32_t *rp_u, *ord_u, *rp_i, *ord_i;
  void *csr;
  size_t csr_bytes;
  int grid;
};

static void ncf_lists(const DrxNcfDims *D, const int32_t *uid, const int32_t *iid, const NcfScratch &S, int B, DrxCsrList (&ls)[2]) {
  ls[0] = DrxCsrList{uid, B, D->n_users, S.rp_u, S.ord_u};
  ls[1] = DrxCsrList{iid, B, D->n_items, S.rp_i, S.ord_i};
}

static bool ncf_carve(Carver &cv, const DrxNcfDims *D, int B, NcfScratch &S) {
  if (!ncf_dims_ok(D) || B < 1 || B >= (1 << 24)) return false;
  const int ld = D->ldg + D->ldm;
  S.grid = drx_ncf_grid(B);
  S.dU = cv.take<float>((size_t)B * ld);
  S.dV = cv.take<float>((size_t)B * ld);
  S.gsw_part = cv.take<float>((size_t)S.grid * D->n_small);
  S.loss_part = cv.take<double>((size_t)S.grid);
  S.rp_u = cv.take<int32_t>((size_t)D->n_users + 1);
  S.ord_u = cv.take<int32_t>((size_t)B);
  S.rp_i = cv.take<int32_t>((size_t)D->n_items + 1);
  S.ord_i = cv.take<int32_t>((size_t)B);
  DrxCsrList ls[2];
  ncf_lists(D, S.ord_u, S.ord_i /* stand for the keys */, S, B, ls);
  S.csr_bytes = drx_batch_csr_device_bytes(ls, 2);
  if (!S.csr_bytes) return false;
  S.csr = cv.take<char>(S.csr_bytes);
  return true;
}

// ---- serving -----------------------------------------------------------------------------------------------------------------------------
// 16 rows per workgroup: wave w the 16-column tile w of [W_1 half^T row (+ b_1)], then the GMF half row-wise
__global__ __launch_bounds__(256) void k_ncf_half_rows(DrxNcfDims D, const float *__restrict__ table, const float *__restrict__ sw,
                                                       const int32_t *__restrict__ ids, int n, int side, float *__restrict__ out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m16 = lane & 15, q4 = lane >> 4;
  const int ld = D.ldg + D.ldm, f1 = D.f[0], f1p = (f1 + 3) & ~3, hw = f1p + D.ldg;
  const float *const W = sw + D.off_w[0] + (size_t)side * D.km * f1;
  for (int r0 = blockIdx.x * 16; r0 < n; r0 += gridDim.x * 16) {
    if (wv * 16 < f1) {
      const int ra = r0 + m16;
      const size_t row = ra < n ? (size_t)(ids ? ids[ra] : ra) : 0;
      const int col = wv * 16 + m16;
      ncf_f4v acc = {0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < D.km; k0 += 4) {
        const int kk = k0 + q4;
        const float a = (kk < D.km && ra < n) ? table[row * ld + D.ldg + kk] : 0.f;
        const float b = (kk < D.km && col < f1) ? W[kk * f1 + col] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
      }
      const float bias = (side == 0 && col < f1) ? sw[D.off_b[0] + col] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ro = r0 + 4 * q4 + r;
        if (ro < n && col < f1p) out[(size_t)ro * hw + col] = col < f1 ? acc[r] + bias : 0.f;
      }
    }
    const int ro = r0 + (threadIdx.x >> 4);
    if (ro < n) {
      const size_t row = (size_t)(ids ? ids[ro] : ro);
      for (int k = threadIdx.x & 15; k < D.ldg; k += 16) {
        const float t = table[row * ld + k];
        out[(size_t)ro * hw + f1p + k] = k < D.kg ? (side == 0 ? sw[D.off_h + k] * t : t) : 0.f;
      }
    }
  }
}

// what the scorers keep of sw in LDS: W_2 .. b_n, h, b0 (contiguous in the layout); `wbase` = the offset of its first float
__device__ __host__ __forceinline__ int ncf_serve_base(const DrxNcfDims &D) { return D.n_layers > 1 ? D.off_w[1] : D.off_h; }

// The logit of the wave's 16 pairs: pair m16 has the half rows ua (user) and ib (item); every lane of a pair returns its logit.
// Za, Zb: the wave's two tiles [16][68] in LDS.  Every wave of the workgroup calls this together (the barriers are the workgroup's).
// A pair's sums: Z_1 = relu(A_u + B_i) element-wise; every layer k ascending in steps of 4 (row m16 of the tile plays no part in the
// order); hm and the GMF dot quarter by quarter of 16 columns ascending, the quarters as (q ^ 1) then (q ^ 2); (mlp + gmf) + b0.
__device__ __forceinline__ float ncf_tile_logit(const DrxNcfDims &D, const float *swl, int wbase, float *Za, float *Zb, const float *ua,
                                                const float *ib, int m16, int q4) {
  const int f1 = D.f[0], f1p = (f1 + 3) & ~3;
  for (int c = q4 * 16; c < q4 * 16 + 16; ++c) Za[m16 * kNcfTS + c] = c < f1 ? fmaxf(ua[c] + ib[c], 0.f) : 0.f;
  __syncthreads();
  float *in = Za, *out = Zb;
#pragma unroll 1
  for (int l = 1; l < D.n_layers; ++l) {
    const int fin = D.f[l - 1], fo = D.f[l];
    const float *const W = swl + (D.off_w[l] - wbase), *const bl = swl + (D.off_b[l] - wbase);
    for (int nt = 0; nt * 16 < fo; ++nt) {
      const ncf_f4v acc = ncf_mfma_xw(in, kNcfTS, W, fin, fo, nt * 16, m16, q4);
      const int col = nt * 16 + m16;
      const float bias = col < fo ? bl[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(4 * q4 + r) * kNcfTS + col] = col < fo ? fmaxf(acc[r] + bias, 0.f) : 0.f;
    }
    __syncthreads();
    float *t = in; in = out; out = t;
  }
  const int fn = D.f[D.n_layers - 1];
  const float *const hm = swl + (D.off_h - wbase) + D.kg;
  float s = 0.f, gm = 0.f;
  for (int c = q4 * 16; c < q4 * 16 + 16 && c < fn; ++c) s = fmaf(hm[c], in[m16 * kNcfTS + c], s);
  for (int k = q4 * 16; k < q4 * 16 + 16 && k < D.kg; ++k) gm = fmaf(ua[f1p + k], ib[f1p + k], gm);
  s += __shfl_xor(s, 16); s += __shfl_xor(s, 32);
  gm += __shfl_xor(gm, 16); gm += __shfl_xor(gm, 32);
  __syncthreads();                                                    // (the tiles are free for the next call)
  return (s + gm) + swl[D.off_b0 - wbase];
}

constexpr int kNcfStrip = 64;                     // items of a workgroup's strip: 16 per wave
constexpr int kNcfUserBlock = 32;                 // users of a workgroup's block at most

static size_t ncf_serve_weights(const DrxNcfDims *D) { return (size_t)ncf_round4(D->n_small - ncf_serve_base(*D)); }
static size_t ncf_score_lds(const DrxNcfDims *D, int ub) {
  const int hw = drx_ncf_half_width(D);
  return sizeof(float) * (ncf_serve_weights(D) + (size_t)(kNcfStrip + ub) * hw + 8 * 16 * kNcfTS);
}

// LDS: weights | IS [64][hw] | US [ub][hw] | Z [4 waves][2][16][68]
__global__ __launch_bounds__(256) void k_ncf_score_rows(DrxNcfDims D, const float *__restrict__ sw, const float *__restrict__ uhalf,
                                                        const float *__restrict__ ihalf, int R, int ub, float *__restrict__ out) {
  extern __shared__ __align__(16) float lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m16 = lane & 15, q4 = lane >> 4;
  const int hw = ((D.f[0] + 3) & ~3) + D.ldg, wbase = ncf_serve_base(D), nw = D.n_small - wbase;
  float *const swl = lds;
  float *const IS = swl + ((nw + 3) & ~3);
  float *const US = IS + kNcfStrip * hw;
  float *const Z = US + ub * hw + wv * 2 * 16 * kNcfTS;
  const int i0 = blockIdx.x * kNcfStrip, u0 = blockIdx.y * ub;
  for (int i = threadIdx.x; i < nw; i += 256) swl[i] = sw[wbase + i];
  for (int i = threadIdx.x; i < kNcfStrip * hw / 4; i += 256) {       // the strip's half rows, once for all the block's users
    const int row = i / (hw / 4);
    reinterpret_cast<float4 *>(IS)[i] = i0 + row < D.n_items ? reinterpret_cast<const float4 *>(ihalf + (size_t)i0 * hw)[i] : f4_zero();
  }
  for (int i = threadIdx.x; i < ub * hw / 4; i += 256) {
    const int row = i / (hw / 4);
    reinterpret_cast<float4 *>(US)[i] = u0 + row < R ? reinterpret_cast<const float4 *>(uhalf + (size_t)u0 * hw)[i] : f4_zero();
  }
  __syncthreads();
  const int item = i0 + wv * 16 + m16;
  for (int r = 0; r < ub && u0 + r < R; ++r) {                        // (uniform over the workgroup)
    const float x = ncf_tile_logit(D, swl, wbase, Z, Z + 16 * kNcfTS, US + r * hw, IS + (wv * 16 + m16) * hw, m16, q4);
    if (q4 == 0 && item < D.n_items) out[(size_t)(u0 + r) * D.n_items + item] = x;
  }
}

// LDS: weights | Z [4 waves][2][16][68]; 64 pairs per workgroup, the half rows read where they lie
__global__ __launch_bounds__(256) void k_ncf_pair_scores(DrxNcfDims D, const float *__restrict__ sw, const float *__restrict__ uhalf,
                                                         const float *__restrict__ ihalf, const int32_t *__restrict__ urow,
                                                         const int32_t *__restrict__ irow, int P, float *__restrict__ out) {
  extern __shared__ __align__(16) float lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m16 = lane & 15, q4 = lane >> 4;
  const int hw = ((D.f[0] + 3) & ~3) + D.ldg, wbase = ncf_serve_base(D), nw = D.n_small - wbase;
  float *const swl = lds;
  float *const Z = swl + ((nw + 3) & ~3) + wv * 2 * 16 * kNcfTS;
  for (int i = threadIdx.x; i < nw; i += 256) swl[i] = sw[wbase + i];
  __syncthreads();
  const int p = blockIdx.x * 64 + wv * 16 + m16;
  const size_t ur = p < P ? (size_t)urow[p] : 0, ir = p < P ? (size_t)irow[p] : 0;
  const float x = ncf_tile_logit(D, swl, wbase, Z, Z + 16 * kNcfTS, uhalf + ur * hw, ihalf + ir * hw, m16, q4);
  if (q4 == 0 && p < P) out[p] = x;
}

}  // namespace drx

extern "C" {

int drx_ncf_grid(int32_t B) { return drx::step_tile_grid(B, drx::kNcfMaxGrid); }

size_t drx_ncf_step_scratch_bytes(const DrxNcfDims *D, int32_t B) {
  using namespace drx;
  Carver cv = step_dry_carver();
  NcfScratch S;
  return ncf_carve(cv, D, B, S) ? step_scratch_total(cv) : 0;
}

int drx_ncf_step(const DrxNcfDims *D, float *U, float *V, float *sw, float *U_s1, float *U_s2, float *V_s1, float *V_s2, float *sw_s1,
                 float *sw_s2, const int32_t *uid, const int32_t *iid, const float *y, int32_t B, const DrxOptRule *rule,
                 const float *alphas, float reg, double *loss_out, void *scratch, size_t scratch_bytes, void *stream) {
  using namespace drx;
  if (!D || !U || !V || !sw || !uid || !iid || !y || !rule || !alphas || !scratch || !ncf_dims_ok(D) || B < 1 || B >= (1 << 24))
    return DRX_EINVAL;
  const int kind = rule->kind;
  StepTensor t[3] = {{U, U_s1, U_s2}, {V, V_s1, V_s2}, {sw, sw_s1, sw_s2}};
  if (!step_tensors_ok(kind, t, 3, 2)) return DRX_EINVAL;
  Carver cv(nullptr, 0);
  if (int rc = step_carver(scratch, scratch_bytes, cv)) return rc;
  NcfScratch S;
  if (!ncf_carve(cv, D, B, S)) return DRX_EINVAL;
  if (!cv.ok()) return DRX_ESCRATCH;
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = ncf_tile_lds(D);
  static LdsGrant grant;
  if (int rc = set_dynamic_lds((const void *)k_ncf_tile, lds, grant)) return rc;
  hipLaunchKernelGGL(k_ncf_tile, dim3(S.grid), dim3(256), lds, st, *D, U, V, sw, uid, iid, y, B, S.dU, S.dV, S.gsw_part, S.loss_part);
  DRX_LAUNCH_CHECK();
  DrxAdamSegments sg;
  memset(&sg, 0, sizeof(sg));
  auto seg = [&](int start, int len, float l2) {
    sg.start[sg.n] = start; sg.len[sg.n] = len; sg.alpha[sg.n] = alphas[2]; sg.l2_coef[sg.n] = l2;
    ++sg.n;
  };
  for (int l = 0; l < D->n_layers; ++l) {
    seg(D->off_w[l], D->off_b[l] - D->off_w[l], reg);
    seg(D->off_b[l], D->f[l], 0.f);
  }
  seg(D->off_h, D->off_b0 - D->off_h, reg);
  seg(D->off_b0, 1, 0.f);
  hipLaunchKernelGGL(k_small_opt<>, dim3((D->n_small + 255) / 256), dim3(256), 0, st, S.gsw_part, S.grid, D->n_small, sw, t[2].s1, t[2].s2,
                     sg, kind, rule->mu, rule->mu2, rule->eps, S.loss_part, (double)B, loss_out);
  DRX_LAUNCH_CHECK();
  DrxCsrList ls[2];
  ncf_lists(D, uid, iid, S, B, ls);
  int rc = drx_batch_csr_device(ls, 2, S.csr, S.csr_bytes, stream);
  if (rc) return rc;
  const int ld = D->ldg + D->ldm;
  const DrxCsrAdamTable tabs[2] = {step_table(S.rp_u, S.ord_u, S.dU, ld, D->n_users, t[0], alphas[0], reg),
                                   step_table(S.rp_i, S.ord_i, S.dV, ld, D->n_items, t[1], alphas[1], reg)};
  return drx_rows_csr_opt_multi(tabs, 2, rule, stream);
}

int32_t drx_ncf_half_width(const DrxNcfDims *D) { return D ? ((D->f[0] + 3) & ~3) + D->ldg : 0; }

int drx_ncf_half_rows(const DrxNcfDims *D, const float *table, const float *sw, const int32_t *ids, int32_t n, int32_t side, float *out,
                      void *stream) {
  using namespace drx;
  if (!D || !table || !sw || !out || n < 1 || (side != 0 && side != 1) || !ncf_dims_ok(D) || (((uintptr_t)table | (uintptr_t)out) & 15))
    return DRX_EINVAL;
  int blocks = (n + 15) / 16;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(k_ncf_half_rows, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *D, table, sw, ids, n, side, out);
  DRX_LAUNCH_CHECK();
  return DRX_OK;
}

int drx_ncf_score_rows(const DrxNcfDims *D, const float *sw, const float *uhalf, const float *ihalf, int32_t R, float *out, void *stream) {
  using namespace drx;
  if (!D || !sw || !uhalf || !ihalf || !out || R < 1 || !ncf_dims_ok(D) || (((uintptr_t)uhalf | (uintptr_t)ihalf) & 15)) return DRX_EINVAL;
  const int ub = R < kNcfUserBlock ? R : kNcfUserBlock;
  const size_t lds = ncf_score_lds(D, ub);
  static LdsGrant grant;
  if (int rc = set_dynamic_lds((const void *)k_ncf_score_rows, lds, grant)) return rc;
  const int strips = (D->n_items + kNcfStrip - 1) / kNcfStrip, blocks = (R + ub - 1) / ub;
  if (blocks > 65535) return DRX_EINVAL;
  hipLaunchKernelGGL(k_ncf_score_rows, dim3(strips, blocks), dim3(256), lds, (hipStream_t)stream, *D, sw, uhalf, ihalf, R, ub, out);
  DRX_LAUNCH_CHECK();
  return DRX_OK;
}

int drx_ncf_pair_scores(const DrxNcfDims *D, const float *sw, const float *uhalf, const float *ihalf, const int32_t *urow,
                        const int32_t *irow, int32_t P, float *out, void *stream) {
  using namespace drx;
  if (!D || !sw || !uhalf || !ihalf || !urow || !irow || !out || P < 1 || !ncf_dims_ok(D) || (((uintptr_t)uhalf | (uintptr_t)ihalf) & 15))
    return DRX_EINVAL;
  const size_t lds = sizeof(float) * (ncf_serve_weights(D) + 8 * 16 * kNcfTS);
  static LdsGrant grant;
  if (int rc = set_dynamic_lds((const void *)k_ncf_pair_scores, lds, grant)) return rc;
  hipLaunchKernelGGL(k_ncf_pair_scores, dim3((P + 63) / 64), dim3(256), lds, (hipStream_t)stream, *D, sw, uhalf, ihalf, urow, irow, P, out);
  DRX_LAUNCH_CHECK();
  return DRX_OK;
}

}  // extern "C"
