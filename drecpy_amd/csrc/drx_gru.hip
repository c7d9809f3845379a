// GRU4Rec (Hidasi, Karatzoglou, Baltrunas, Tikk 2016; include/drx.h "GRU4Rec"): the recurrent tile kernel of
// the pairwise step, the step itself and the query rows of serving.  Every dense product runs on v_mfma_f32_16x16x4_f32 (fp32 in, fp32
// accumulate), M = a tile of 16 windows / users.  Operand layout (lane l): A[l % 16][l / 16], B[l / 16][l % 16], C register r =
// C[4 (l / 16) + r][l % 16].
//   drx_gru_step       : k_gru_tile -> k_small_opt (drx_small.hpp: partials in workgroup order + the rule on sw) -> drx_batch_csr_device (input
//                        keys, item keys) -> ONE drx_rows_csr_opt_multi (E plain, Q with b in the outer-product form).  No atomics.
//   drx_gru_query_rows : h after the cell has run over a user's basket, for tiles of 16 users
// Both run the recurrence with gru_forward: one definition of every sum of the forward pass.
// Where things live: Wx, Wh stay in global memory and are read as MFMA B operands (96 KiB at K = H = 64: L2
// holds them, LDS could not next to the activations); LDS holds x_1 .. x_L, h_0 .. h_L and the pre-activations of ONE step; the backward
// pass recomputes a step's gates from x_t and h_{t-1} with the forward's own function; a wave keeps its tiles of dWx, dWh in registers
// over all steps and tiles of its workgroup.
#include "drx_common.hpp"
#include "drx_rows.hpp"
#include "drx_opt.hpp"
#include "drx_step.hpp"
#include "drx_small.hpp"

namespace drx {

typedef float gru_f4v __attribute__((ext_vector_type(4)));
constexpr int kGruMaxW = 64;                      // K and H at most
constexpr int kGruMaxL = 8;
constexpr int kGruMaxNeg = 16;
constexpr int kGruTS = 68;                        // floats per row of a 16-row tile of x_t / h_t in LDS
constexpr int kGruPS = 196;                       // floats per row of a 16-row tile of the 3 H pre-activations
constexpr int kGruTile = 16 * kGruTS;
constexpr int kGruMaxGrid = 256;

static int gru_round4(int x) { return (x + 3) & ~3; }

// the dims describe the layout of include/drx.h exactly
static bool gru_dims_ok(const DrxGruDims *D) {
  if (!D || D->n_items < 1 || D->k < 1 || D->k > kGruMaxW || D->h < 1 || D->h > kGruMaxW) return false;
  if (D->ldk != gru_round4(D->k) || D->ldh != gru_round4(D->h)) return false;
  const int g = 3 * D->h;
  return D->off_wx == 0 && D->off_wh == D->k * g && D->off_bx == (D->k + D->h) * g && D->off_bhn == D->off_bx + g &&
         D->n_small == D->off_bhn + D->h;
}

// acc (16 x 16) = X [16 x fin] (LDS, rows of xs floats) . W [fin x fo] (global, row-major), columns col0 .. col0 + 15: k ascending in
// steps of 4
__device__ __forceinline__ gru_f4v gru_mfma_xw(const float *X, int xs, const float *__restrict__ W, int fin, int fo, int col0, int m16,
                                               int q4) {
  gru_f4v acc = {0.f, 0.f, 0.f, 0.f};
  const int col = col0 + m16;
  for (int k0 = 0; k0 < fin; k0 += 4) {
    const int kk = k0 + q4;
    const float a = kk < fin ? X[m16 * xs + kk] : 0.f;
    const float b = (kk < fin && col < fo) ? W[kk * fo + col] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// acc (16 x 16) = G [16 x fo] (LDS, rows of gs floats) . W^T (W [fin x fo] global, row-major), columns (rows of W) row0 .. row0 + 15
__device__ __forceinline__ gru_f4v gru_mfma_gwt(const float *G, int gs, const float *__restrict__ W, int fin, int fo, int row0, int m16,
                                                int q4) {
  gru_f4v acc = {0.f, 0.f, 0.f, 0.f};
  const int row = row0 + m16;
  for (int k0 = 0; k0 < fo; k0 += 4) {
    const int kk = k0 + q4;
    const float a = kk < fo ? G[m16 * gs + kk] : 0.f;
    const float b = (kk < fo && row < fin) ? W[row * fo + kk] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

__device__ __forceinline__ float gru_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// the gates of one element from its pre-activations: px = x_t Wx + bx, ph = h_{t-1} Wh (+ bhn in the n block)
struct GruGates {
  float z, r, n, hn;
};
__device__ __forceinline__ GruGates gru_gates(const float *PX, const float *PH, int s, int c, int H) {
  GruGates g;
  g.z = gru_sigmoid(PX[s * kGruPS + c] + PH[s * kGruPS + c]);
  g.r = gru_sigmoid(PX[s * kGruPS + H + c] + PH[s * kGruPS + H + c]);
  g.hn = PH[s * kGruPS + 2 * H + c];
  g.n = tanhf(fmaf(g.r, g.hn, PX[s * kGruPS + 2 * H + c]));
  return g;
}

// PX, PH [16][196] <- the pre-activations of one step from Xt, Hp [16][68]: wave wv takes the 16-column tiles wv, wv + 4, wv + 8 of the
// 3 H gate columns.  Every thread of the workgroup calls it; it ends with the workgroup's barrier.
__device__ __forceinline__ void gru_preact(const DrxGruDims &D, const float *__restrict__ sw, const float *Xt, const float *Hp, float *PX,
                                           float *PH, int wv, int m16, int q4) {
  const int G3 = 3 * D.h;
#pragma unroll 1
  for (int ct = wv; ct * 16 < G3; ct += 4) {
    const gru_f4v ax = gru_mfma_xw(Xt, kGruTS, sw + D.off_wx, D.k, G3, ct * 16, m16, q4);
    const gru_f4v ah = gru_mfma_xw(Hp, kGruTS, sw + D.off_wh, D.h, G3, ct * 16, m16, q4);
    const int col = ct * 16 + m16;
    if (col < G3) {
      const float bx = sw[D.off_bx + col];
      const float bh = col >= 2 * D.h ? sw[D.off_bhn + col - 2 * D.h] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        PX[(4 * q4 + r) * kGruPS + col] = ax[r] + bx;
        PH[(4 * q4 + r) * kGruPS + col] = ah[r] + bh;
      }
    }
  }
  __syncthreads();
}

// The forward recurrence of a tile of 16 rows.  idl [L][16]: the item of row s at step t, < 0 = no step (the row keeps its h).
// Gathers x_t = E[idl[t][s]] into X [L][16][68] (a row without a step: zeros), then for t ascending h_t into Hs[t + 1]; Hs[0] must hold
// zeros (h_0) and the columns >= H of every Hs tile are never written.  A row's sums do not depend on the other rows of its tile.
__device__ __forceinline__ void gru_forward(const DrxGruDims &D, const float *__restrict__ E, const float *__restrict__ sw, const int *idl,
                                            int L, float *X, float *Hs, float *PX, float *PH) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m16 = lane & 15, q4 = lane >> 4;
  const int ts = threadIdx.x >> 4, tj = threadIdx.x & 15;
  for (int t = 0; t < L; ++t) {
    const int id = idl[t * 16 + ts];
    if (4 * tj < D.ldk) {
      const float4 v = id >= 0 ? reinterpret_cast<const float4 *>(E + (size_t)id * D.ldk)[tj] : f4_zero();
      *reinterpret_cast<float4 *>(X + t * kGruTile + ts * kGruTS + 4 * tj) = v;
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int t = 0; t < L; ++t) {
    const float *Hp = Hs + t * kGruTile;
    float *Hn = Hs + (t + 1) * kGruTile;
    gru_preact(D, sw, X + t * kGruTile, Hp, PX, PH, wv, m16, q4);
    const bool on = idl[t * 16 + ts] >= 0;
    for (int c = tj; c < D.h; c += 16) {
      const float hp = Hp[ts * kGruTS + c];
      float hn = hp;
      if (on) {
        const GruGates g = gru_gates(PX, PH, ts, c, D.h);
        hn = fmaf(g.z, hp, (1.0f - g.z) * g.n);
      }
      Hn[ts * kGruTS + c] = hn;
    }
    __syncthreads();
  }
}

// ---- the step ----------------------------------------------------------------------------------------------------------------------------
// LDS (floats): X [L][16][68] | Hs [L + 1][16][68] | PX, PH [16][196] | DH [16][68] | bacc [256] | le (double) [16] | idl (int) [L][16]
static size_t gru_tile_lds(int L) {
  return sizeof(float) * ((size_t)(2 * L + 2) * kGruTile + 2 * 16 * kGruPS + 256 + 32 + (size_t)L * 16);
}
// X | Hs | PX, PH | idl
static size_t gru_query_lds(int L) { return sizeof(float) * ((size_t)(2 * L + 1) * kGruTile + 2 * 16 * kGruPS + (size_t)L * 16); }

__global__ __launch_bounds__(256) void k_gru_tile(DrxGruDims D, const float *__restrict__ E, const float *__restrict__ sw,
                                                  const float *__restrict__ Q, const float *__restrict__ bq,
                                                  const int32_t *__restrict__ before, const int32_t *__restrict__ after, int B, int L, int r,
                                                  float *__restrict__ dE, float *__restrict__ hL, float *__restrict__ gs,
                                                  float *__restrict__ gsw_part, double *__restrict__ loss_part) {
  extern __shared__ __align__(16) float lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m16 = lane & 15, q4 = lane >> 4;
  const int ts = threadIdx.x >> 4, tj = threadIdx.x & 15;            // the row-wise passes: 16 threads per window
  float *const X = lds;
  float *const Hs = X + L * kGruTile;
  float *const PX = Hs + (L + 1) * kGruTile;
  float *const PH = PX + 16 * kGruPS;
  float *const DH = PH + 16 * kGruPS;
  float *const bacc = DH + kGruTile;
  double *const le = reinterpret_cast<double *>(bacc + 256);
  int *const idl = reinterpret_cast<int *>(bacc + 256 + 32);
  const int K = D.k, H = D.h, G3 = 3 * H;
  for (int i = threadIdx.x; i < (L + 1) * kGruTile; i += 256) Hs[i] = 0.f;
  bacc[threadIdx.x] = 0.f;
  gru_f4v awx[3][4], awh[3][4];                                       // this wave's tiles of dWx, dWh: column tile wv + 4 j, row tile mi
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      awx[j][mi] = gru_f4v{0.f, 0.f, 0.f, 0.f};
      awh[j][mi] = gru_f4v{0.f, 0.f, 0.f, 0.f};
    }
  const float scale = 1.0f / ((float)B * (float)r);
  const int n_tiles = (B + 15) / 16;
  double loss = 0.0;
#pragma unroll 1
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int b0 = tile * 16;
    __syncthreads();                                                  // (the previous tile's rows are free)
    for (int i = threadIdx.x; i < L * 16; i += 256) {
      const int t = i >> 4, w = b0 + (i & 15);
      idl[i] = w < B ? before[(size_t)w * L + t] : -1;
    }
    __syncthreads();
    gru_forward(D, E, sw, idl, L, X, Hs, PX, PH);
    // ---- per window (16 lanes, a float4 of a row of Q each): D_wk, the loss, g_wk, dh_L = sum_k g_wk (Q[i] - Q[j_k])
    {
      const int w = b0 + ts;
      const bool col_on = 4 * tj < D.ldh;
      float4 d = f4_zero();
      double lw = 0.0;
      if (w < B) {                                                    // (a group of 16 lanes is live or idle as a whole)
        const int32_t *items = after + (size_t)w * (1 + r);
        const float4 h = col_on ? *reinterpret_cast<const float4 *>(Hs + L * kGruTile + ts * kGruTS + 4 * tj) : f4_zero();
        const int i = items[0];
        const float4 qi = col_on ? reinterpret_cast<const float4 *>(Q + (size_t)i * D.ldh)[tj] : f4_zero();
        const float bi = bq[i];
        float gsum = 0.f;
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
      }
      *reinterpret_cast<float4 *>(DH + ts * kGruTS + 4 * tj) = d;
      if (tj == 0) le[ts] = lw;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int s_ = 0; s_ < 16; ++s_) loss += le[s_];
    // ---- backward through time: DH holds dh_t
#pragma unroll 1
    for (int t = L - 1; t >= 0; --t) {
      const float *Xt = X + t * kGruTile, *Hp = Hs + t * kGruTile;
      gru_preact(D, sw, Xt, Hp, PX, PH, wv, m16, q4);
      // the gates again, then the gradients of the pre-activations in their place: PX <- [da_z | da_r | da_n], PH <- [da_z | da_r |
      // da_n r]; DH <- dh_t z (the direct path to h_{t-1}); a row without a step passes dh on and has zero gate gradients
      {
        const bool on = idl[t * 16 + ts] >= 0;
        for (int c = tj; c < H; c += 16) {
          const float dh = DH[ts * kGruTS + c];
          float daz = 0.f, dar = 0.f, dan = 0.f, danr = 0.f, dhp = dh;
          if (on) {
            const GruGates g = gru_gates(PX, PH, ts, c, H);
            const float hp = Hp[ts * kGruTS + c];
            dan = dh * (1.0f - g.z) * (1.0f - g.n * g.n);
            daz = dh * (hp - g.n) * g.z * (1.0f - g.z);
            dar = dan * g.hn * g.r * (1.0f - g.r);
            danr = dan * g.r;
            dhp = dh * g.z;
          }
          PX[ts * kGruPS + c] = daz; PX[ts * kGruPS + H + c] = dar; PX[ts * kGruPS + 2 * H + c] = dan;
          PH[ts * kGruPS + c] = daz; PH[ts * kGruPS + H + c] = dar; PH[ts * kGruPS + 2 * H + c] = danr;
          DH[ts * kGruTS + c] = dhp;
        }
      }
      __syncthreads();
      // the biases: one thread per entry of [bx | bhn], the tile's windows ascending
      if ((int)threadIdx.x < 4 * H) {
        const int c = threadIdx.x;
        const float *src = c < G3 ? PX + c : PH + 2 * H + (c - G3);
        float g = 0.f;
        for (int s_ = 0; s_ < 16; ++s_) g += src[s_ * kGruPS];
        bacc[c] += g;
      }
      // dWx += x_t^T dgx, dWh += h_{t-1}^T dgh: M = 16 rows of W, K = the 16 windows
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int ct = wv + 4 * j;
        if (ct * 16 < G3) {
          const int gcol = ct * 16 + m16;
#pragma unroll
          for (int mi = 0; mi < 4; ++mi) {
            const int arow = mi * 16 + m16;
            if (mi * 16 < K) {
#pragma unroll
              for (int ks = 0; ks < 4; ++ks) {
                const int kk = 4 * ks + q4;
                const float a = arow < K ? Xt[kk * kGruTS + arow] : 0.f;
                const float b = gcol < G3 ? PX[kk * kGruPS + gcol] : 0.f;
                awx[j][mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, awx[j][mi], 0, 0, 0);
              }
            }
            if (mi * 16 < H) {
#pragma unroll
              for (int ks = 0; ks < 4; ++ks) {
                const int kk = 4 * ks + q4;
                const float a = arow < H ? Hp[kk * kGruTS + arow] : 0.f;
                const float b = gcol < G3 ? PH[kk * kGruPS + gcol] : 0.f;
                awh[j][mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, awh[j][mi], 0, 0, 0);
              }
            }
          }
        }
      }
      // dx_t = dgx Wx^T -> the gradient rows of E (wave wv the 16 columns wv of up to 64), padding zero
      if (wv * 16 < D.ldk) {
        const gru_f4v dx = gru_mfma_gwt(PX, kGruPS, sw + D.off_wx, K, G3, wv * 16, m16, q4);
        const int col = wv * 16 + m16;
        if (col < D.ldk) {
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const int w = b0 + 4 * q4 + rr;
            if (w < B) dE[((size_t)w * L + t) * D.ldk + col] = col < K ? dx[rr] : 0.f;
          }
        }
      }
      // dh_{t-1} = dh_t z + dgh Wh^T
      if (wv * 16 < H) {
        const gru_f4v dhp = gru_mfma_gwt(PH, kGruPS, sw + D.off_wh, H, G3, wv * 16, m16, q4);
        const int col = wv * 16 + m16;
        if (col < H) {
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) DH[(4 * q4 + rr) * kGruTS + col] += dhp[rr];
        }
      }
      __syncthreads();
    }
  }
  // ---- the workgroup's row of partial sums: every entry of it is written
  float *const part = gsw_part + (size_t)blockIdx.x * D.n_small;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int ct = wv + 4 * j;
    const int gcol = ct * 16 + m16;
    if (gcol < G3) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int row = mi * 16 + 4 * q4 + rr;
          if (row < K) part[D.off_wx + row * G3 + gcol] = awx[j][mi][rr];
          if (row < H) part[D.off_wh + row * G3 + gcol] = awh[j][mi][rr];
        }
      }
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < 4 * H) part[D.off_bx + threadIdx.x] = bacc[threadIdx.x];
  if (threadIdx.x == 0) loss_part[blockIdx.x] = loss;
}

// ---- serving -----------------------------------------------------------------------------------------------------------------------------
// tiles of 16 users: out[q] = h after the steps of the basket of uid[q] (the positions present, ascending), padding zero
__global__ __launch_bounds__(256) void k_gru_query_rows(DrxGruDims D, const float *__restrict__ E, const float *__restrict__ sw,
                                                        const int32_t *__restrict__ baskets, int L, const int32_t *__restrict__ uid, int n,
                                                        float *__restrict__ out) {
  extern __shared__ __align__(16) float lds[];
  const int ts = threadIdx.x >> 4, tj = threadIdx.x & 15;
  float *const X = lds;
  float *const Hs = X + L * kGruTile;
  float *const PX = Hs + (L + 1) * kGruTile;
  float *const PH = PX + 16 * kGruPS;
  int *const idl = reinterpret_cast<int *>(PH + 16 * kGruPS);
  for (int i = threadIdx.x; i < (L + 1) * kGruTile; i += 256) Hs[i] = 0.f;
  const int n_tiles = (n + 15) / 16;
#pragma unroll 1
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int r0 = tile * 16;
    __syncthreads();
    for (int i = threadIdx.x; i < L * 16; i += 256) {
      const int t = i >> 4, q = r0 + (i & 15);
      idl[i] = q < n ? baskets[(size_t)uid[q] * L + t] : -1;
    }
    __syncthreads();
    gru_forward(D, E, sw, idl, L, X, Hs, PX, PH);
    const int q = r0 + ts;
    if (q < n && 4 * tj < D.ldh)
      reinterpret_cast<float4 *>(out + (size_t)q * D.ldh)[tj] = *reinterpret_cast<const float4 *>(Hs + L * kGruTile + ts * kGruTS + 4 * tj);
  }
}

struct GruScratch {
  float *dE, *hL, *gs, *gsw_part;
  double *loss_part;
  int32_t *rp_e, *ord_e, *rp_i, *ord_i;
  void *csr;
  size_t csr_bytes;
  int grid;
};

static void gru_lists(const DrxGruDims *D, const int32_t *before, const int32_t *after, const GruScratch &S, int B, int L, int r,
                      DrxCsrList (&ls)[2]) {
  ls[0] = DrxCsrList{before, B * L, D->n_items, S.rp_e, S.ord_e};
  ls[1] = DrxCsrList{after, B * (1 + r), D->n_items, S.rp_i, S.ord_i};
}

static bool gru_shape_ok(const DrxGruDims *D, int64_t B, int L, int r) {
  return gru_dims_ok(D) && B >= 1 && B < (1 << 24) && L >= 1 && L <= kGruMaxL && r >= 1 && r <= kGruMaxNeg;
}

static bool gru_carve(Carver &cv, const DrxGruDims *D, int B, int L, int r, GruScratch &S) {
  if (!gru_shape_ok(D, B, L, r)) return false;
  S.grid = drx_gru_grid(B);
  S.dE = cv.take<float>((size_t)B * L * D->ldk);
  S.hL = cv.take<float>((size_t)B * D->ldh);
  S.gs = cv.take<float>((size_t)B * (1 + r));
  S.gsw_part = cv.take<float>((size_t)S.grid * D->n_small);
  S.loss_part = cv.take<double>((size_t)S.grid);
  S.rp_e = cv.take<int32_t>((size_t)D->n_items + 1);
  S.ord_e = cv.take<int32_t>((size_t)B * L);
  S.rp_i = cv.take<int32_t>((size_t)D->n_items + 1);
  S.ord_i = cv.take<int32_t>((size_t)B * (1 + r));
  DrxCsrList ls[2];
  gru_lists(D, S.ord_e, S.ord_i /* stand for the keys */, S, B, L, r, ls);
  S.csr_bytes = drx_batch_csr_device_bytes(ls, 2);
  if (!S.csr_bytes) return false;
  S.csr = cv.take<char>(S.csr_bytes);
  return true;
}

}  // namespace drx

extern "C" {

int drx_gru_grid(int32_t B) { return drx::step_tile_grid(B, drx::kGruMaxGrid); }

size_t drx_gru_step_scratch_bytes(const DrxGruDims *D, int32_t B, int32_t L, int32_t neg_ratio) {
  using namespace drx;
  Carver cv = step_dry_carver();
  GruScratch S;
  return gru_carve(cv, D, B, L, neg_ratio, S) ? step_scratch_total(cv) : 0;
}

int drx_gru_step(const DrxGruDims *D, float *E, float *sw, float *Q, float *b, float *E_s1, float *E_s2, float *sw_s1, float *sw_s2,
                 float *Q_s1, float *Q_s2, float *b_s1, float *b_s2, const int32_t *before, const int32_t *after, int32_t B, int32_t L,
                 int32_t neg_ratio, const DrxOptRule *rule, const float *alphas, float reg, double *loss_out, void *scratch,
                 size_t scratch_bytes, void *stream) {
  using namespace drx;
  const int r = neg_ratio;
  if (!D || !E || !sw || !Q || !b || !before || !after || !rule || !alphas || !scratch || !gru_shape_ok(D, B, L, r)) return DRX_EINVAL;
  const int kind = rule->kind;
  StepTensor t[4] = {{E, E_s1, E_s2}, {Q, Q_s1, Q_s2}, {sw, sw_s1, sw_s2}, {b, b_s1, b_s2}};
  if (!step_tensors_ok(kind, t, 4, 2)) return DRX_EINVAL;
  Carver cv(nullptr, 0);
  if (int rc = step_carver(scratch, scratch_bytes, cv)) return rc;
  GruScratch S;
  if (!gru_carve(cv, D, B, L, r, S)) return DRX_EINVAL;
  if (!cv.ok()) return DRX_ESCRATCH;
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = gru_tile_lds(L);
  static LdsGrant tile_lds;
  if (int rc = set_dynamic_lds((const void *)k_gru_tile, lds, tile_lds)) return rc;
  hipLaunchKernelGGL(k_gru_tile, dim3(S.grid), dim3(256), lds, st, *D, E, sw, Q, b, before, after, B, L, r, S.dE, S.hL, S.gs, S.gsw_part,
                     S.loss_part);
  DRX_LAUNCH_CHECK();
  DrxAdamSegments sg;
  memset(&sg, 0, sizeof(sg));
  sg.n = 2;                                                           // [Wx | Wh] regularised, [bx | bhn] not
  sg.start[0] = D->off_wx; sg.len[0] = D->off_bx - D->off_wx; sg.alpha[0] = alphas[1]; sg.l2_coef[0] = reg;
  sg.start[1] = D->off_bx; sg.len[1] = D->n_small - D->off_bx; sg.alpha[1] = alphas[1]; sg.l2_coef[1] = 0.f;
  hipLaunchKernelGGL(k_small_opt<>, dim3((D->n_small + 255) / 256), dim3(256), 0, st, S.gsw_part, S.grid, D->n_small, sw, t[2].s1, t[2].s2,
                     sg, kind, rule->mu, rule->mu2, rule->eps, S.loss_part, (double)B * (double)r, loss_out);
  DRX_LAUNCH_CHECK();
  DrxCsrList ls[2];
  gru_lists(D, before, after, S, B, L, r, ls);
  int rc = drx_batch_csr_device(ls, 2, S.csr, S.csr_bytes, stream);
  if (rc) return rc;
  const DrxCsrAdamTable tabs[2] = {
      step_table(S.rp_e, S.ord_e, S.dE, D->ldk, D->n_items, t[0], alphas[0], reg),
      step_table_outer(S.rp_i, S.ord_i, S.hL, S.gs, 1 + r, D->ldh, D->n_items, t[1], t[3], alphas[2], alphas[2], reg)};
  return drx_rows_csr_opt_multi(tabs, 2, rule, stream);
}

int drx_gru_query_rows(const float *E, const float *sw, const DrxGruDims *D, const int32_t *baskets, int32_t L, const int32_t *uid,
                       int32_t n, float *out, void *stream) {
  using namespace drx;
  if (!E || !sw || !D || !baskets || !uid || !out || n < 1 || L < 1 || L > kGruMaxL || !gru_dims_ok(D) ||
      (((uintptr_t)E | (uintptr_t)out) & 15))
    return DRX_EINVAL;
  const size_t lds = gru_query_lds(L);
  static LdsGrant query_lds;
  if (int rc = set_dynamic_lds((const void *)k_gru_query_rows, lds, query_lds)) return rc;
  int blocks = (n + 15) / 16;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_gru_query_rows, dim3(blocks), dim3(256), lds, (hipStream_t)stream, *D, E, sw, baskets, L, uid, n, out);
  DRX_LAUNCH_CHECK();
  return DRX_OK;
}

}  // extern "C"
