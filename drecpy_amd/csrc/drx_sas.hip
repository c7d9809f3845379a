// SASRec (Kang & McAuley 2018; include/drx.h "SASRec"): the self-attention tile kernel of the pairwise step, the
// step itself and the query rows of serving.  Every dense product runs on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate); the
// row-wise layer normalisation, softmax and ReLU run on the VALU.  ONE WINDOW IS ONE MFMA TILE: its 16 rows are the positions (rows
// >= L and absent positions are masked), so S = q k^T is one 16 x 16 accumulator and a row's bits cannot depend on another window.
// Operand layout (lane l): A[l % 16][l / 16], B[l / 16][l % 16], C register r = C[4 (l / 16) + r][l % 16].
//   drx_sas_step       : k_sas_tile -> k_small_opt (drx_small.hpp: partials in workgroup order + the rule on sw) -> drx_batch_csr_device (input
//                        keys, item keys) -> ONE drx_rows_csr_opt_multi (E plain, Q with b in the outer-product form).  No atomics.
//   drx_sas_query_rows : h of a user's basket, one user per tile
// Both run sas_forward: one definition of every sum of the forward pass.
// Where things live: the weights stay in global memory and are read as MFMA B operands (L2 holds them); LDS
// keeps EVERY activation of the forward pass of the one window in flight (per block X, A, q, k, v, X', F, relu and P), nothing is
// recomputed but the LN statistics and nothing goes to the scratch carve; a wave keeps its 16-column tiles of the five weight gradients
// of every block in registers over all windows of its workgroup; the gradients of Pos, the biases and the LN vectors add up in LDS.
#include "drx_common.hpp"
#include "drx_rows.hpp"
#include "drx_opt.hpp"
#include "drx_step.hpp"
#include "drx_small.hpp"

namespace drx {

typedef float sas_f4v __attribute__((ext_vector_type(4)));
constexpr int kSasMaxH = 64;
constexpr int kSasMaxL = 16;
constexpr int kSasMaxBlocks = 2;
constexpr int kSasMaxNeg = 16;
constexpr int kSasTS = 68;                        // floats per row of a 16-row tile of activations in LDS
constexpr int kSasTile = 16 * kSasTS;
constexpr int kSasPS = 17;                        // floats per row of a 16 x 16 tile (P, dS)
constexpr int kSasPTile = 16 * kSasPS;
constexpr int kSasMaxGrid = 256;
constexpr float kSasEps = 1e-5f;
// the tiles of one block's forward pass, in this order; the X of block b + 1 (after the last block: the input of the final LN) is tile 0
// of the next group
enum { SAS_X = 0, SAS_A, SAS_Q, SAS_K, SAS_V, SAS_X1, SAS_F, SAS_R, SAS_PER_BLOCK };
// the vectors of one block behind off_vec, h floats each
enum { SAS_B1 = 0, SAS_B2, SAS_LN1G, SAS_LN1B, SAS_LN2G, SAS_LN2B, SAS_VEC_PER_BLOCK };

static int sas_round4(int x) { return (x + 3) & ~3; }

// the dims describe the layout of include/drx.h exactly
static bool sas_dims_ok(const DrxSasDims *D) {
  if (!D || D->n_items < 1 || D->h < 1 || D->h > kSasMaxH || D->L < 1 || D->L > kSasMaxL || D->blocks < 1 || D->blocks > kSasMaxBlocks)
    return false;
  const int H = D->h, HH = H * H;
  return D->ldh == sas_round4(H) && D->off_pos == 0 && D->off_blk == D->L * H && D->off_vec == D->off_blk + 5 * HH * D->blocks &&
         D->off_lnf == D->off_vec + SAS_VEC_PER_BLOCK * H * D->blocks && D->n_small == D->off_lnf + 2 * H;
}

// ---- the five product forms ----------------------------------------------------------------------------------------------------------
// acc (16 x 16) = X [16 x n] (LDS, rows of xs floats) . W [n x n] (global, row-major), columns col0 .. col0 + 15: k ascending by 4
__device__ __forceinline__ sas_f4v sas_xw(const float *X, int xs, const float *__restrict__ W, int n, int col0, int m16, int q4) {
  sas_f4v acc = {0.f, 0.f, 0.f, 0.f};
  const int col = col0 + m16;
  for (int k0 = 0; k0 < n; k0 += 4) {
    const int kk = k0 + q4;
    const float a = kk < n ? X[m16 * xs + kk] : 0.f;
    const float b = (kk < n && col < n) ? W[kk * n + col] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// acc = G [16 x n] (LDS) . W^T (W [n x n] global, row-major), columns (rows of W) row0 .. row0 + 15, added to acc
__device__ __forceinline__ sas_f4v sas_gwt(const float *G, int gs, const float *__restrict__ W, int n, int row0, int m16, int q4,
                                           sas_f4v acc) {
  const int row = row0 + m16;
  for (int k0 = 0; k0 < n; k0 += 4) {
    const int kk = k0 + q4;
    const float a = kk < n ? G[m16 * gs + kk] : 0.f;
    const float b = (kk < n && row < n) ? W[row * n + kk] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// acc (16 x 16) = X [16 x n] . Y^T, Y [16 x n], both in LDS with rows of kSasTS floats (q k^T, dO v^T)
__device__ __forceinline__ sas_f4v sas_abt(const float *X, const float *Y, int n, int m16, int q4) {
  sas_f4v acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < n; k0 += 4) {
    const int kk = k0 + q4;
    const float a = kk < n ? X[m16 * kSasTS + kk] : 0.f;
    const float b = kk < n ? Y[m16 * kSasTS + kk] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// acc (16 x 16) = S [16 x 16] (LDS, rows of kSasPS) . Y [16 x n] (LDS, rows of kSasTS), columns col0 .. col0 + 15 (P v, dS k)
__device__ __forceinline__ sas_f4v sas_ab(const float *S, const float *Y, int n, int col0, int m16, int q4) {
  sas_f4v acc = {0.f, 0.f, 0.f, 0.f};
  const int col = col0 + m16;
#pragma unroll
  for (int k0 = 0; k0 < 16; k0 += 4) {
    const int kk = k0 + q4;
    const float a = S[m16 * kSasPS + kk];
    const float b = col < n ? Y[kk * kSasTS + col] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// acc (16 x 16) += X^T . Y over the 16 positions: rows row0 .. row0 + 15 of X's nx columns (X in LDS, rows of xs floats), columns col0
// .. col0 + 15 of Y's ny columns (LDS, rows of kSasTS): the weight gradients A^T dY, and P^T dO, dS^T q at xs = kSasPS
__device__ __forceinline__ sas_f4v sas_atb(const float *X, int xs, int nx, int row0, const float *Y, int ny, int col0, int m16, int q4,
                                           sas_f4v acc) {
  const int row = row0 + m16, col = col0 + m16;
#pragma unroll
  for (int k0 = 0; k0 < 16; k0 += 4) {
    const int kk = k0 + q4;
    const float a = row < nx ? X[kk * xs + row] : 0.f;
    const float b = col < ny ? Y[kk * kSasTS + col] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// C (this wave's 16 x 16 accumulator) -> the columns col0 .. of a tile in LDS
__device__ __forceinline__ void sas_put(float *T, sas_f4v c, int n, int col0, int m16, int q4) {
  const int col = col0 + m16;
  if (col < n) {
#pragma unroll
    for (int r = 0; r < 4; ++r) T[(4 * q4 + r) * kSasTS + col] = c[r];
  }
}

// ---- the row-wise passes: 16 threads per position (ts the row, tj the lane of it) ----------------------------------------------------
struct SasStat {
  float mean, rstd;
};
__device__ __forceinline__ SasStat sas_stat(const float *x, int H, int tj) {
  float s = 0.f;
  for (int c = tj; c < H; c += 16) s += x[c];
  SasStat st;
  st.mean = group_sum<16>(s) / (float)H;
  float v = 0.f;
  for (int c = tj; c < H; c += 16) {
    const float d = x[c] - st.mean;
    v = fmaf(d, d, v);
  }
  st.rstd = 1.0f / sqrtf(group_sum<16>(v) / (float)H + kSasEps);
  return st;
}

// Y row = LN(X row; g, beta)
__device__ __forceinline__ void sas_ln_row(const float *x, float *y, const float *__restrict__ g, const float *__restrict__ beta, int H,
                                           int tj) {
  const SasStat st = sas_stat(x, H, tj);
  for (int c = tj; c < H; c += 16) y[c] = fmaf((x[c] - st.mean) * st.rstd, g[c], beta[c]);
}

// the backward pass of y = LN(x): res row += dx; dyx row <- dy (.) xhat (its column sums are the gain's gradient).  No contraction
// here: dy g must be the SAME rounded product in the mean and in the difference from it, or at a variance near zero (h = 1: exactly
// zero, rstd = 316) the product's rounding error, which a fused multiply-subtract would keep, comes out as a gradient
__device__ __forceinline__ void sas_ln_back_row(const float *x, const float *dy, const float *__restrict__ g, float *res, float *dyx, int H,
                                                int tj) {
#pragma clang fp contract(off)
  const SasStat st = sas_stat(x, H, tj);
  float s1 = 0.f, s2 = 0.f;
  for (int c = tj; c < H; c += 16) {
    const float xh = (x[c] - st.mean) * st.rstd, dxh = dy[c] * g[c];
    s1 += dxh;
    s2 = fmaf(dxh, xh, s2);
  }
  s1 = group_sum<16>(s1) / (float)H;
  s2 = group_sum<16>(s2) / (float)H;
  for (int c = tj; c < H; c += 16) {
    const float xh = (x[c] - st.mean) * st.rstd, dxh = dy[c] * g[c];
    res[c] += st.rstd * (dxh - s1 - xh * s2);
    dyx[c] = dy[c] * xh;
  }
}

// acc[c] += the column sums (the 16 rows ascending) of tile A by threads 0 .. H - 1 and of tile B by threads 64 .. 64 + H - 1
__device__ __forceinline__ void sas_colsums(const float *A, float *acc_a, const float *B, float *acc_b, int H) {
  const int t = threadIdx.x;
  const float *src = t < 64 ? A : B;
  float *dst = t < 64 ? acc_a : acc_b;
  const int c = t & 63;
  if (t < 128 && c < H && src) {
    float g = 0.f;
    for (int s = 0; s < 16; ++s) g += src[s * kSasTS + c];
    dst[c] += g;
  }
}

__device__ __forceinline__ const float *sas_w(const DrxSasDims &D, const float *sw, int b, int j) {
  return sw + D.off_blk + (5 * b + j) * D.h * D.h;
}
__device__ __forceinline__ const float *sas_vec(const DrxSasDims &D, const float *sw, int b, int j) {
  return sw + D.off_vec + (SAS_VEC_PER_BLOCK * b + j) * D.h;
}

// The forward pass of ONE sequence.  ids [16] (LDS): the item at position t, < 0 = absent (and every t >= L).  Fills the activation
// tiles act [blocks * 8 + 1] and P [blocks], and hrow [kSasTS] <- h = LN(X_{L-1}; lnf), zero when position L - 1 is absent, zero in
// the columns h .. 67.  Every thread of the workgroup calls it; it ends with the workgroup's barrier.
template <int NB>
__device__ __forceinline__ void sas_forward(const DrxSasDims &D, const float *__restrict__ E, const float *__restrict__ sw, const int *ids,
                                            float *act, float *Ps, float *hrow) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m16 = lane & 15, q4 = lane >> 4;
  const int ts = threadIdx.x >> 4, tj = threadIdx.x & 15;
  const int H = D.h, L = D.L;
  const bool on = ids[ts] >= 0;
  {
    const int id = ids[ts];
    for (int c = tj; c < H; c += 16) act[ts * kSasTS + c] = on ? E[(size_t)id * D.ldh + c] + sw[D.off_pos + ts * H + c] : 0.f;
  }
  __syncthreads();
  const float inv = 1.0f / sqrtf((float)H);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    float *const T = act + b * SAS_PER_BLOCK * kSasTile;
    float *const X = T + SAS_X * kSasTile, *const A = T + SAS_A * kSasTile, *const Qt = T + SAS_Q * kSasTile;
    float *const Kt = T + SAS_K * kSasTile, *const V = T + SAS_V * kSasTile, *const X1 = T + SAS_X1 * kSasTile;
    float *const F = T + SAS_F * kSasTile, *const R = T + SAS_R * kSasTile, *const Xn = T + SAS_PER_BLOCK * kSasTile;
    float *const P = Ps + b * kSasPTile;
    sas_ln_row(X + ts * kSasTS, A + ts * kSasTS, sas_vec(D, sw, b, SAS_LN1G), sas_vec(D, sw, b, SAS_LN1B), H, tj);
    __syncthreads();
    if (wv * 16 < H) {
      sas_put(Qt, sas_xw(A, kSasTS, sas_w(D, sw, b, 0), H, wv * 16, m16, q4), H, wv * 16, m16, q4);
      sas_put(Kt, sas_xw(A, kSasTS, sas_w(D, sw, b, 1), H, wv * 16, m16, q4), H, wv * 16, m16, q4);
      sas_put(V, sas_xw(A, kSasTS, sas_w(D, sw, b, 2), H, wv * 16, m16, q4), H, wv * 16, m16, q4);
    }
    __syncthreads();
    if (wv == 0) {                                                    // S, the masks and the softmax of a row: 16 lanes, in registers
      const sas_f4v s = sas_abt(Qt, Kt, H, m16, q4);
      const bool key = ids[m16] >= 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * q4 + r;
        const bool ok = key && m16 <= row && ids[row] >= 0;
        const float v = ok ? s[r] * inv : -3.0e38f;
        float top = v;
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) top = fmaxf(top, __shfl_xor(top, m, kWave));
        const float e = ok ? expf(v - top) : 0.f;
        const float den = group_sum<16>(e);
        P[row * kSasPS + m16] = den > 0.f ? e / den : 0.f;
      }
    }
    __syncthreads();
    if (wv * 16 < H) {
      const sas_f4v o = sas_ab(P, V, H, wv * 16, m16, q4);
      const int col = wv * 16 + m16;
      if (col < H) {
#pragma unroll
        for (int r = 0; r < 4; ++r) X1[(4 * q4 + r) * kSasTS + col] = X[(4 * q4 + r) * kSasTS + col] + o[r];
      }
    }
    __syncthreads();
    sas_ln_row(X1 + ts * kSasTS, F + ts * kSasTS, sas_vec(D, sw, b, SAS_LN2G), sas_vec(D, sw, b, SAS_LN2B), H, tj);
    __syncthreads();
    if (wv * 16 < H) {
      const sas_f4v u = sas_xw(F, kSasTS, sas_w(D, sw, b, 3), H, wv * 16, m16, q4);
      const int col = wv * 16 + m16;
      if (col < H) {
        const float b1 = sas_vec(D, sw, b, SAS_B1)[col];
#pragma unroll
        for (int r = 0; r < 4; ++r) R[(4 * q4 + r) * kSasTS + col] = fmaxf(u[r] + b1, 0.f);
      }
    }
    __syncthreads();
    if (wv * 16 < H) {
      const sas_f4v y = sas_xw(R, kSasTS, sas_w(D, sw, b, 4), H, wv * 16, m16, q4);
      const int col = wv * 16 + m16;
      if (col < H) {
        const float b2 = sas_vec(D, sw, b, SAS_B2)[col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 4 * q4 + r;
          Xn[row * kSasTS + col] = ids[row] >= 0 ? X1[row * kSasTS + col] + (y[r] + b2) : 0.f;
        }
      }
    }
    __syncthreads();
  }
  if (ts == L - 1) {
    const float *x = act + NB * SAS_PER_BLOCK * kSasTile + ts * kSasTS;
    const SasStat st = sas_stat(x, H, tj);
    for (int c = tj; c < kSasTS; c += 16)
      hrow[c] = (on && c < H) ? fmaf((x[c] - st.mean) * st.rstd, sw[D.off_lnf + c], sw[D.off_lnf + H + c]) : 0.f;
  }
  __syncthreads();
}

// ---- the step ----------------------------------------------------------------------------------------------------------------------------
// LDS (floats): act [8 blocks + 1] tiles | P [blocks] | G [5] tiles | dS | hrow [68] | dh [68] | vacc [L h + 6 h blocks + 2 h] | ids [16]
static size_t sas_vacc(const DrxSasDims *D) { return (size_t)D->L * D->h + (size_t)(SAS_VEC_PER_BLOCK * D->blocks + 2) * D->h; }
static size_t sas_forward_floats(int blocks) { return (size_t)(SAS_PER_BLOCK * blocks + 1) * kSasTile + (size_t)blocks * kSasPTile; }
static size_t sas_tile_lds(const DrxSasDims *D) {
  return sizeof(float) * (sas_forward_floats(D->blocks) + 5 * kSasTile + kSasPTile + 2 * kSasTS + sas_vacc(D) + 16);
}
// act | P | hrow | ids
static size_t sas_query_lds(const DrxSasDims *D) { return sizeof(float) * (sas_forward_floats(D->blocks) + kSasTS + 16); }

template <int NB>
__global__ __launch_bounds__(256) void k_sas_tile(DrxSasDims D, const float *__restrict__ E, const float *__restrict__ sw,
                                                  const float *__restrict__ Q, const float *__restrict__ bq,
                                                  const int32_t *__restrict__ before, const int32_t *__restrict__ after, int B, int r,
                                                  float *__restrict__ dE, float *__restrict__ hL, float *__restrict__ gs,
                                                  float *__restrict__ gsw_part, double *__restrict__ loss_part) {
  extern __shared__ __align__(16) float lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m16 = lane & 15, q4 = lane >> 4;
  const int ts = threadIdx.x >> 4, tj = threadIdx.x & 15;
  const int H = D.h, L = D.L;
  float *const act = lds;
  float *const Ps = act + (SAS_PER_BLOCK * NB + 1) * kSasTile;
  float *const G0 = Ps + NB * kSasPTile;
  float *const G1 = G0 + kSasTile, *const G2 = G1 + kSasTile, *const G3 = G2 + kSasTile, *const G4 = G3 + kSasTile;
  float *const DS = G4 + kSasTile;
  float *const hrow = DS + kSasPTile;
  float *const dh = hrow + kSasTS;
  float *const vacc = dh + kSasTS;                                    // Pos [L h], then the vectors in the order behind off_vec
  const int n_vacc = L * H + (SAS_VEC_PER_BLOCK * NB + 2) * H;
  int *const ids = reinterpret_cast<int *>(vacc + n_vacc);
  float *const vvec = vacc + L * H;
  for (int i = threadIdx.x; i < n_vacc; i += 256) vacc[i] = 0.f;
  sas_f4v gw[NB][5][4];                                               // this wave's column tile wv of dWq, dWk, dWv, dW1, dW2: row tile mi
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) gw[b][j][mi] = sas_f4v{0.f, 0.f, 0.f, 0.f};
  const float scale = 1.0f / ((float)B * (float)r);
  const float inv = 1.0f / sqrtf((float)H);
  const int col0 = wv * 16;
  const bool wave_on = col0 < H;
  double loss = 0.0;
#pragma unroll 1
  for (int w = blockIdx.x; w < B; w += gridDim.x) {
    __syncthreads();                                                  // (the previous window's tiles are free)
    if (threadIdx.x < 16) ids[threadIdx.x] = (int)threadIdx.x < L ? before[(size_t)w * L + threadIdx.x] : -1;
    __syncthreads();
    sas_forward<NB>(D, E, sw, ids, act, Ps, hrow);
    // ---- the window's 16 lanes, a float4 of a row of Q each: D_wk, the loss, g_wk, dh = sum_k g_wk (Q[i] - Q[j_k])
    if (threadIdx.x < 16) {
      const bool col_on = 4 * tj < D.ldh;
      const int32_t *items = after + (size_t)w * (1 + r);
      const float4 h = *reinterpret_cast<const float4 *>(hrow + 4 * tj);
      const int i = items[0];
      const float4 qi = col_on ? reinterpret_cast<const float4 *>(Q + (size_t)i * D.ldh)[tj] : f4_zero();
      const float bi = bq[i];
      float4 d = f4_zero();
      float gsum = 0.f;
      double lw = 0.0;
      for (int k = 0; k < r; ++k) {
        const int j = items[1 + k];
        const float4 qj = col_on ? reinterpret_cast<const float4 *>(Q + (size_t)j * D.ldh)[tj] : f4_zero();
        const float4 df = make_float4(qi.x - qj.x, qi.y - qj.y, qi.z - qj.z, qi.w - qj.w);
        const float delta = group_sum<16>(f4_dot(h, df)) + (bi - bq[j]);
        // g = -sigmoid(-delta) / (B r);  softplus(-delta) = max(-delta, 0) + log1p(exp(-|delta|))
        const float g = -(1.0f / (1.0f + expf(delta))) * scale;
        lw += (double)(fmaxf(-delta, 0.f) + log1pf(expf(-fabsf(delta))));
        f4_fma(d, g, df);
        gsum += g;
        if (tj == 0) gs[(size_t)w * (1 + r) + 1 + k] = -g;
      }
      if (tj == 0) gs[(size_t)w * (1 + r)] = gsum;
      if (col_on) reinterpret_cast<float4 *>(hL + (size_t)w * D.ldh)[tj] = h;
      *reinterpret_cast<float4 *>(dh + 4 * tj) = d;
      if (tj == 0) loss += lw;
    }
    __syncthreads();
    // ---- backward.  G0 holds the gradient of the block's output X''; the final LN touches row L - 1 alone
    {
      const float *x = act + NB * SAS_PER_BLOCK * kSasTile + ts * kSasTS;
      for (int c = tj; c < H; c += 16) G0[ts * kSasTS + c] = 0.f;
      if (ts == L - 1) {
        sas_ln_back_row(x, dh, sw + D.off_lnf, G0 + ts * kSasTS, G1 + ts * kSasTS, H, tj);
        for (int c = tj; c < H; c += 16) {
          vvec[SAS_VEC_PER_BLOCK * NB * H + c] += G1[ts * kSasTS + c];
          vvec[(SAS_VEC_PER_BLOCK * NB + 1) * H + c] += dh[c];
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int b = NB - 1; b >= 0; --b) {
      float *const T = act + b * SAS_PER_BLOCK * kSasTile;
      float *const X = T + SAS_X * kSasTile, *const A = T + SAS_A * kSasTile, *const Qt = T + SAS_Q * kSasTile;
      float *const Kt = T + SAS_K * kSasTile, *const V = T + SAS_V * kSasTile, *const X1 = T + SAS_X1 * kSasTile;
      float *const F = T + SAS_F * kSasTile, *const R = T + SAS_R * kSasTile;
      float *const P = Ps + b * kSasPTile;
      float *const vb = vvec + SAS_VEC_PER_BLOCK * b * H;
      // (1) the second FFN layer: dW2 += relu^T dY, db2 += colsum dY, G1 <- dU = (dY W2^T) (.) [relu > 0]
      sas_colsums(G0, vb + SAS_B2 * H, nullptr, nullptr, H);
      if (wave_on) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
          if (mi * 16 < H) gw[b][4][mi] = sas_atb(R, kSasTS, H, mi * 16, G0, H, col0, m16, q4, gw[b][4][mi]);
        const sas_f4v dr = sas_gwt(G0, kSasTS, sas_w(D, sw, b, 4), H, col0, m16, q4, sas_f4v{0.f, 0.f, 0.f, 0.f});
        const int col = col0 + m16;
        if (col < H) {
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const int at = (4 * q4 + rr) * kSasTS + col;
            G1[at] = R[at] > 0.f ? dr[rr] : 0.f;
          }
        }
      }
      __syncthreads();
      // (2) the first: dW1 += F^T dU, db1 += colsum dU, G2 <- dF = dU W1^T
      sas_colsums(G1, vb + SAS_B1 * H, nullptr, nullptr, H);
      if (wave_on) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
          if (mi * 16 < H) gw[b][3][mi] = sas_atb(F, kSasTS, H, mi * 16, G1, H, col0, m16, q4, gw[b][3][mi]);
        sas_put(G2, sas_gwt(G1, kSasTS, sas_w(D, sw, b, 3), H, col0, m16, q4, sas_f4v{0.f, 0.f, 0.f, 0.f}), H, col0, m16, q4);
      }
      __syncthreads();
      // (3) LN2: G0 <- dX' = dY + LN'(dF), G3 <- dF (.) xhat
      sas_ln_back_row(X1 + ts * kSasTS, G2 + ts * kSasTS, sas_vec(D, sw, b, SAS_LN2G), G0 + ts * kSasTS, G3 + ts * kSasTS, H, tj);
      __syncthreads();
      sas_colsums(G2, vb + SAS_LN2B * H, G3, vb + SAS_LN2G * H, H);
      // (4) attention: wave 0 dS = P (.) (dP - rowsum(P (.) dP)) / sqrt(h), dP = dO v^T; every wave G1 <- dv = P^T dO
      if (wv == 0) {
        const sas_f4v dp = sas_abt(G0, V, H, m16, q4);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int row = 4 * q4 + rr;
          const float p = P[row * kSasPS + m16];
          const float dot = group_sum<16>(p * dp[rr]);
          DS[row * kSasPS + m16] = p * (dp[rr] - dot) * inv;
        }
      }
      if (wave_on) sas_put(G1, sas_atb(P, kSasPS, 16, 0, G0, H, col0, m16, q4, sas_f4v{0.f, 0.f, 0.f, 0.f}), H, col0, m16, q4);
      __syncthreads();
      // G2 <- dq = dS k, G3 <- dk = dS^T q
      if (wave_on) {
        sas_put(G2, sas_ab(DS, Kt, H, col0, m16, q4), H, col0, m16, q4);
        sas_put(G3, sas_atb(DS, kSasPS, 16, 0, Qt, H, col0, m16, q4, sas_f4v{0.f, 0.f, 0.f, 0.f}), H, col0, m16, q4);
      }
      __syncthreads();
      // dWq, dWk, dWv += A^T (dq, dk, dv);  G4 <- dA = dq Wq^T + dk Wk^T + dv Wv^T
      if (wave_on) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
          if (mi * 16 < H) {
            gw[b][0][mi] = sas_atb(A, kSasTS, H, mi * 16, G2, H, col0, m16, q4, gw[b][0][mi]);
            gw[b][1][mi] = sas_atb(A, kSasTS, H, mi * 16, G3, H, col0, m16, q4, gw[b][1][mi]);
            gw[b][2][mi] = sas_atb(A, kSasTS, H, mi * 16, G1, H, col0, m16, q4, gw[b][2][mi]);
          }
        sas_f4v da = sas_gwt(G2, kSasTS, sas_w(D, sw, b, 0), H, col0, m16, q4, sas_f4v{0.f, 0.f, 0.f, 0.f});
        da = sas_gwt(G3, kSasTS, sas_w(D, sw, b, 1), H, col0, m16, q4, da);
        da = sas_gwt(G1, kSasTS, sas_w(D, sw, b, 2), H, col0, m16, q4, da);
        sas_put(G4, da, H, col0, m16, q4);
      }
      __syncthreads();
      // (5) LN1: G0 <- dX = dX' + LN'(dA), G1 <- dA (.) xhat
      sas_ln_back_row(X + ts * kSasTS, G4 + ts * kSasTS, sas_vec(D, sw, b, SAS_LN1G), G0 + ts * kSasTS, G1 + ts * kSasTS, H, tj);
      __syncthreads();
      sas_colsums(G4, vb + SAS_LN1B * H, G1, vb + SAS_LN1G * H, H);
      __syncthreads();
    }
    // ---- G0 = dX0: the gradient rows of E, padding zero, and Pos
    if (ts < L) {
      for (int c = tj; c < D.ldh; c += 16) dE[((size_t)w * L + ts) * D.ldh + c] = c < H ? G0[ts * kSasTS + c] : 0.f;
      for (int c = tj; c < H; c += 16) vacc[ts * H + c] += G0[ts * kSasTS + c];
    }
  }
  // ---- the workgroup's row of partial sums: every entry of it is written
  float *const part = gsw_part + (size_t)blockIdx.x * D.n_small;
  const int col = col0 + m16;
  if (col < H) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const int row = mi * 16 + 4 * q4 + rr;
            if (row < H) part[D.off_blk + (5 * b + j) * H * H + row * H + col] = gw[b][j][mi][rr];
          }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_vacc; i += 256) part[i < L * H ? D.off_pos + i : D.off_vec + (i - L * H)] = vacc[i];
  if (threadIdx.x == 0) loss_part[blockIdx.x] = loss;
}

// ---- serving -----------------------------------------------------------------------------------------------------------------------------
// one user per tile: out[q] = h of the basket of uid[q], stored left-aligned and shifted here so that its newest item is at L - 1
template <int NB>
__global__ __launch_bounds__(256) void k_sas_query_rows(DrxSasDims D, const float *__restrict__ E, const float *__restrict__ sw,
                                                        const int32_t *__restrict__ baskets, const int32_t *__restrict__ uid, int n,
                                                        float *__restrict__ out) {
  extern __shared__ __align__(16) float lds[];
  const int L = D.L;
  float *const act = lds;
  float *const Ps = act + (SAS_PER_BLOCK * NB + 1) * kSasTile;
  float *const hrow = Ps + NB * kSasPTile;
  int *const ids = reinterpret_cast<int *>(hrow + kSasTS);
#pragma unroll 1
  for (int q = blockIdx.x; q < n; q += gridDim.x) {
    __syncthreads();
    if (threadIdx.x < 16) {
      const int32_t *row = baskets + (size_t)uid[q] * L;
      int m = 0;
      for (int t = 0; t < L; ++t) m += row[t] >= 0;
      const int t = (int)threadIdx.x - (L - m);                       // the basket's entry that position threadIdx.x holds
      ids[threadIdx.x] = ((int)threadIdx.x < L && t >= 0) ? row[t] : -1;
    }
    __syncthreads();
    sas_forward<NB>(D, E, sw, ids, act, Ps, hrow);
    if (4 * threadIdx.x < (unsigned)D.ldh)
      reinterpret_cast<float4 *>(out + (size_t)q * D.ldh)[threadIdx.x] = *reinterpret_cast<const float4 *>(hrow + 4 * threadIdx.x);
  }
}

struct SasScratch {
  float *dE, *hL, *gs, *gsw_part;
  double *loss_part;
  int32_t *rp_e, *ord_e, *rp_i, *ord_i;
  void *csr;
  size_t csr_bytes;
  int grid;
};

static void sas_lists(const DrxSasDims *D, const int32_t *before, const int32_t *after, const SasScratch &S, int B, int r,
                      DrxCsrList (&ls)[2]) {
  ls[0] = DrxCsrList{before, B * D->L, D->n_items, S.rp_e, S.ord_e};
  ls[1] = DrxCsrList{after, B * (1 + r), D->n_items, S.rp_i, S.ord_i};
}

static bool sas_shape_ok(const DrxSasDims *D, int64_t B, int r) {
  return sas_dims_ok(D) && B >= 1 && B < (1 << 24) && r >= 1 && r <= kSasMaxNeg;
}

static bool sas_carve(Carver &cv, const DrxSasDims *D, int B, int r, SasScratch &S) {
  if (!sas_shape_ok(D, B, r)) return false;
  S.grid = drx_sas_grid(B);
  // dE first, hL second: engine_sas.py SasEngine.step_hidden reads hL at this place (tests/test_gpu_sasrec.py holds serving's rows to
  // its bits); whoever moves one of the two moves the accessor
  S.dE = cv.take<float>((size_t)B * D->L * D->ldh);
  S.hL = cv.take<float>((size_t)B * D->ldh);
  S.gs = cv.take<float>((size_t)B * (1 + r));
  S.gsw_part = cv.take<float>((size_t)S.grid * D->n_small);
  S.loss_part = cv.take<double>((size_t)S.grid);
  S.rp_e = cv.take<int32_t>((size_t)D->n_items + 1);
  S.ord_e = cv.take<int32_t>((size_t)B * D->L);
  S.rp_i = cv.take<int32_t>((size_t)D->n_items + 1);
  S.ord_i = cv.take<int32_t>((size_t)B * (1 + r));
  DrxCsrList ls[2];
  sas_lists(D, S.ord_e, S.ord_i /* stand for the keys */, S, B, r, ls);
  S.csr_bytes = drx_batch_csr_device_bytes(ls, 2);
  if (!S.csr_bytes) return false;
  S.csr = cv.take<char>(S.csr_bytes);
  return true;
}

}  // namespace drx

extern "C" {

int drx_sas_grid(int32_t B) {
  const int n = B < 1 ? 1 : B;                                        // a tile is one window
  return n < drx::kSasMaxGrid ? n : drx::kSasMaxGrid;
}

size_t drx_sas_step_scratch_bytes(const DrxSasDims *D, int32_t B, int32_t neg_ratio) {
  using namespace drx;
  Carver cv = step_dry_carver();
  SasScratch S;
  return sas_carve(cv, D, B, neg_ratio, S) ? step_scratch_total(cv) : 0;
}

int drx_sas_step(const DrxSasDims *D, float *E, float *sw, float *Q, float *b, float *E_s1, float *E_s2, float *sw_s1, float *sw_s2,
                 float *Q_s1, float *Q_s2, float *b_s1, float *b_s2, const int32_t *before, const int32_t *after, int32_t B,
                 int32_t neg_ratio, const DrxOptRule *rule, const float *alphas, float reg, double *loss_out, void *scratch,
                 size_t scratch_bytes, void *stream) {
  using namespace drx;
  const int r = neg_ratio;
  if (!D || !E || !sw || !Q || !b || !before || !after || !rule || !alphas || !scratch || !sas_shape_ok(D, B, r)) return DRX_EINVAL;
  const int kind = rule->kind;
  StepTensor t[4] = {{E, E_s1, E_s2}, {Q, Q_s1, Q_s2}, {sw, sw_s1, sw_s2}, {b, b_s1, b_s2}};
  if (!step_tensors_ok(kind, t, 4, 2)) return DRX_EINVAL;
  Carver cv(nullptr, 0);
  if (int rc = step_carver(scratch, scratch_bytes, cv)) return rc;
  SasScratch S;
  if (!sas_carve(cv, D, B, r, S)) return DRX_EINVAL;
  if (!cv.ok()) return DRX_ESCRATCH;
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = sas_tile_lds(D);
  if (D->blocks == 1) {
    static LdsGrant tile_lds;
    if (int rc = set_dynamic_lds((const void *)k_sas_tile<1>, lds, tile_lds)) return rc;
    hipLaunchKernelGGL(k_sas_tile<1>, dim3(S.grid), dim3(256), lds, st, *D, E, sw, Q, b, before, after, B, r, S.dE, S.hL, S.gs, S.gsw_part,
                       S.loss_part);
  } else {
    static LdsGrant tile_lds;
    if (int rc = set_dynamic_lds((const void *)k_sas_tile<2>, lds, tile_lds)) return rc;
    hipLaunchKernelGGL(k_sas_tile<2>, dim3(S.grid), dim3(256), lds, st, *D, E, sw, Q, b, before, after, B, r, S.dE, S.hL, S.gs, S.gsw_part,
                       S.loss_part);
  }
  DRX_LAUNCH_CHECK();
  DrxAdamSegments sg;
  memset(&sg, 0, sizeof(sg));
  sg.n = 2;                                                           // [Pos | the matrices] regularised, the vectors not
  sg.start[0] = 0; sg.len[0] = D->off_vec; sg.alpha[0] = alphas[1]; sg.l2_coef[0] = reg;
  sg.start[1] = D->off_vec; sg.len[1] = D->n_small - D->off_vec; sg.alpha[1] = alphas[1]; sg.l2_coef[1] = 0.f;
  hipLaunchKernelGGL(k_small_opt<>, dim3((D->n_small + 255) / 256), dim3(256), 0, st, S.gsw_part, S.grid, D->n_small, sw, t[2].s1, t[2].s2,
                     sg, kind, rule->mu, rule->mu2, rule->eps, S.loss_part, (double)B * (double)r, loss_out);
  DRX_LAUNCH_CHECK();
  DrxCsrList ls[2];
  sas_lists(D, before, after, S, B, r, ls);
  int rc = drx_batch_csr_device(ls, 2, S.csr, S.csr_bytes, stream);
  if (rc) return rc;
  const DrxCsrAdamTable tabs[2] = {
      step_table(S.rp_e, S.ord_e, S.dE, D->ldh, D->n_items, t[0], alphas[0], reg),
      step_table_outer(S.rp_i, S.ord_i, S.hL, S.gs, 1 + r, D->ldh, D->n_items, t[1], t[3], alphas[2], alphas[2], reg)};
  return drx_rows_csr_opt_multi(tabs, 2, rule, stream);
}

int drx_sas_query_rows(const float *E, const float *sw, const DrxSasDims *D, const int32_t *baskets, const int32_t *uid, int32_t n,
                       float *out, void *stream) {
  using namespace drx;
  if (!E || !sw || !D || !baskets || !uid || !out || n < 1 || !sas_dims_ok(D) || (((uintptr_t)E | (uintptr_t)out) & 15)) return DRX_EINVAL;
  const size_t lds = sas_query_lds(D);
  const int blocks = n < 4096 ? n : 4096;
  if (D->blocks == 1) {
    static LdsGrant query_lds;
    if (int rc = set_dynamic_lds((const void *)k_sas_query_rows<1>, lds, query_lds)) return rc;
    hipLaunchKernelGGL(k_sas_query_rows<1>, dim3(blocks), dim3(256), lds, (hipStream_t)stream, *D, E, sw, baskets, uid, n, out);
  } else {
    static LdsGrant query_lds;
    if (int rc = set_dynamic_lds((const void *)k_sas_query_rows<2>, lds, query_lds)) return rc;
    hipLaunchKernelGGL(k_sas_query_rows<2>, dim3(blocks), dim3(256), lds, (hipStream_t)stream, *D, E, sw, baskets, uid, n, out);
  }
  DRX_LAUNCH_CHECK();
  return DRX_OK;
}

}  // extern "C"
