// Mult-VAE / Mult-DAE (Liang et al. 2018; include/drx.h "Mult-VAE"): the full-softmax training step, its noise
// and the query rows of serving.  Every dense product runs on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate) in tiles of 16 batch
// rows; tanh, exp, the log-sum-exp and the KL terms run on the VALU.
// Operand layout (lane l): A[l % 16][l / 16], B[l / 16][l % 16], C register r = C[4 (l / 16) + r][l % 16].
//   drx_vae_step : k_vae_encode (bag of W_in rows, h1, [mu | logvar], z, h2 per row tile; the keys and scales of the W_in update)
//                  -> k_vae_lse (pass 1 over the catalogue: a (max, sum) per row and workgroup) -> k_vae_lse_combine (workgroup order)
//                  -> k_vae_out (pass 2: the logits again, dlogit, dW_out / db_out of an item tile over ALL rows and the dense rule
//                     on them in place, the workgroup's slab of dh2 = dlogit W_out, the data loss)
//                  -> k_vae_back (slabs summed in slab order, the decoder and encoder backward, dx1, small-weight partials)
//                  -> k_small_opt (drx_small.hpp) -> drx_batch_csr_device + k_vae_remap -> ONE drx_rows_csr_opt_multi (W_in, outer form)
//   drx_vae_query_rows : h2 of a user's positives, 16 users per tile
// Both run vae_forward: one definition of every sum of the forward pass.  No array of B x n_items floats exists: the logits of a
// 16 x 16 tile live in one accumulator, twice.  No float atomics; every sum runs in an order fixed by the arguments.
#include "drx_common.hpp"
#include "drx_rows.hpp"
#include "drx_opt.hpp"
#include "drx_step.hpp"
#include "drx_small.hpp"

namespace drx {

typedef float vae_f4v __attribute__((ext_vector_type(4)));
constexpr int kVaeMaxH = 128;
constexpr int kVaeMaxL = 64;
constexpr int kVaeTS = 132;                       // floats per row of a 16-row tile in LDS
constexpr int kVaeTile = 16 * kVaeTS;
constexpr int kVaeDS = 17;                        // floats per row of a 16 x 16 tile of dlogit
constexpr int kVaeRowGrid = 256;                  // workgroups of the row-tile kernels at most
constexpr int kVaeItemGrid = 128;                 // persistent workgroups of the two catalogue passes at most: the number of slabs
constexpr int kVaeMaxB = 1 << 16;
constexpr int kVaeChunk = 512;                    // rows whose membership masks of an item tile pass 2 keeps in LDS

static int vae_round4(int x) { return (x + 3) & ~3; }

// the dims describe the layout of include/drx.h exactly
static bool vae_dims_ok(const DrxVaeDims *D) {
  if (!D || D->n_items < 1 || D->h < 1 || D->h > kVaeMaxH || D->latent < 1 || D->latent > kVaeMaxL) return false;
  if (D->variational != 0 && D->variational != 1) return false;
  const int e = D->variational ? 2 * D->latent : D->latent;
  return D->e == e && D->ldh == vae_round4(D->h) && D->off_we == 0 && D->off_wd == D->h * e && D->off_vec == D->off_wd + D->latent * D->h &&
         D->n_small == D->off_vec + 2 * D->h + e;
}

static int vae_item_tiles(const DrxVaeDims *D) { return (D->n_items + 15) / 16; }
static int vae_item_grid(const DrxVaeDims *D) {
  const int t = vae_item_tiles(D);
  return t < kVaeItemGrid ? t : kVaeItemGrid;
}

// ---- the product forms -----------------------------------------------------------------------------------------------------------------
// acc (16 x 16) = X [16 x n] (LDS, rows of kVaeTS floats) . W [n x ncols] (global, row-major), columns col0 .. col0 + 15
__device__ __forceinline__ vae_f4v vae_xw(const float *X, const float *__restrict__ W, int n, int ncols, int col0, int m16, int q4) {
  vae_f4v acc = {0.f, 0.f, 0.f, 0.f};
  const int col = col0 + m16;
  for (int k0 = 0; k0 < n; k0 += 4) {
    const int kk = k0 + q4;
    const float a = kk < n ? X[m16 * kVaeTS + kk] : 0.f;
    const float b = (kk < n && col < ncols) ? W[kk * ncols + col] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// acc = G [16 x n] (LDS) . W^T, W [nrows x n] global row-major: columns (rows of W) row0 .. row0 + 15
__device__ __forceinline__ vae_f4v vae_gwt(const float *G, const float *__restrict__ W, int nrows, int n, int row0, int m16, int q4) {
  vae_f4v acc = {0.f, 0.f, 0.f, 0.f};
  const int row = row0 + m16;
  for (int k0 = 0; k0 < n; k0 += 4) {
    const int kk = k0 + q4;
    const float a = kk < n ? G[m16 * kVaeTS + kk] : 0.f;
    const float b = (kk < n && row < nrows) ? W[row * n + kk] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// acc (16 x 16) += X^T . Y over the 16 rows of a tile: rows row0 .. of X's nx columns, columns col0 .. of Y's ny columns (both LDS)
__device__ __forceinline__ vae_f4v vae_atb(const float *X, int nx, int row0, const float *Y, int ny, int col0, int m16, int q4, vae_f4v acc) {
  const int row = row0 + m16, col = col0 + m16;
#pragma unroll
  for (int k0 = 0; k0 < 16; k0 += 4) {
    const int kk = k0 + q4;
    const float a = row < nx ? X[kk * kVaeTS + row] : 0.f;
    const float b = col < ny ? Y[kk * kVaeTS + col] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// the logits of 16 rows (Ht: their h2, LDS) x 16 items (Wt: their rows of W_out, LDS), without the bias
__device__ __forceinline__ vae_f4v vae_logits(const float *Ht, const float *Wt, int H, int m16, int q4) {
  vae_f4v acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < H; k0 += 4) {
    const int kk = k0 + q4;
    const float a = kk < H ? Ht[m16 * kVaeTS + kk] : 0.f;
    const float b = kk < H ? Wt[m16 * kVaeTS + kk] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// 16 rows of `ld` floats (ld a multiple of 4, at most 128) from global rows first .. first + 15 into a tile, rows >= n_rows zero;
// `threads` consecutive threads starting at thread `t`
__device__ __forceinline__ void vae_stage(float *T, const float *__restrict__ src, int first, int n_rows, int ld, int t, int threads) {
  const int per = ld >> 2;
  for (int i = t; i < 16 * per; i += threads) {
    const int r = i / per, c4 = i - r * per;
    const int row = first + r;
    const float4 v = row < n_rows ? reinterpret_cast<const float4 *>(src + (size_t)row * ld)[c4] : f4_zero();
    *reinterpret_cast<float4 *>(T + r * kVaeTS + 4 * c4) = v;
  }
}

// acc[c] += the column sums (the 16 rows ascending) of tile A, by threads 0 .. n - 1
__device__ __forceinline__ void vae_colsums(const float *A, float *acc, int n) {
  const int c = threadIdx.x;
  if (c < n) {
    float g = 0.f;
    for (int s = 0; s < 16; ++s) g += A[s * kVaeTS + c];
    acc[c] += g;
  }
}

// ---- the forward pass of one tile of 16 rows -------------------------------------------------------------------------------------------
// ids [16] (LDS): the user of row r of the tile, < 0 = no row.  koff [16] (LDS): where the row's lookups start in keep / keys / scale
// units (see the callers; a lookup past n_keys or past `group` per row is not written).  keep == nullptr: every lookup kept.
// eps == nullptr (or not variational): z = mu.  Fills the tiles H1, ML ([mu | logvar]), Z, H2, cb [16] (c_b of the row) and nu [16] (N_u); columns past the logical width are zero up to the next multiple
// of 4.  keys / scale (both or none): the item of every lookup of the row, and keep ? c_b : 0.  Every thread of the workgroup calls
// it; it ends with the workgroup's barrier.
__device__ __forceinline__ void vae_forward(const DrxVaeDims &D, const float *__restrict__ W_in, const float *__restrict__ sw,
                                            const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const int *ids,
                                            const int *koff, const int *soff, int row0, int n_keys, int group,
                                            const uint8_t *__restrict__ keep,
                                            const float *__restrict__ eps, float dropout, int32_t *__restrict__ keys,
                                            float *__restrict__ scale, float *H1, float *ML, float *Z, float *H2, float *cbv, int *nuv) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m16 = lane & 15, q4 = lane >> 4;
  const int ts = threadIdx.x >> 4, tj = threadIdx.x & 15;
  const int H = D.h, L = D.latent, E = D.e;
  // the bag of row r: the 16 groups of 16 lanes take the lookups g, g + 16, ..; their partial sums are added in group order (H2 holds
  // them until the decoder writes it)
#pragma unroll 1
  for (int r = 0; r < 16; ++r) {
    const int u = ids[r];
    float4 acc0 = f4_zero(), acc1 = f4_zero();
    float cb = 0.f;
    int n = 0;
    if (u >= 0) {
      const int64_t p0 = indptr[u];
      n = (int)(indptr[u + 1] - p0);
      cb = n > 0 ? 1.0f / (sqrtf((float)n) * (1.0f - dropout)) : 0.f;
      const int ko = koff[r], so = soff[r];
      const bool c0 = 4 * tj < D.ldh, c1 = 64 + 4 * tj < D.ldh;
#pragma unroll 2
      for (int j = ts; j < n; j += 16) {
        const int item = indices[p0 + j];
        const bool kept = keep ? keep[ko + j] != 0 : true;
        if (keys && tj == 0 && ko + j < n_keys && j < group) {
          keys[ko + j] = item;
          scale[so + j] = kept ? cb : 0.f;
        }
        if (kept) {
          const float4 *w = reinterpret_cast<const float4 *>(W_in + (size_t)item * D.ldh);
          if (c0) f4_add(acc0, w[tj]);
          if (c1) f4_add(acc1, w[16 + tj]);
        }
      }
    }
    *reinterpret_cast<float4 *>(H2 + ts * kVaeTS + 4 * tj) = acc0;
    *reinterpret_cast<float4 *>(H2 + ts * kVaeTS + 64 + 4 * tj) = acc1;
    if (threadIdx.x == 0) {
      cbv[r] = cb;
      nuv[r] = n;
    }
    __syncthreads();
    if (threadIdx.x < 128) {
      const int c = threadIdx.x;
      float sum = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) sum += H2[g * kVaeTS + c];
      H1[r * kVaeTS + c] = (u >= 0 && c < H) ? tanhf(fmaf(cb, sum, sw[D.off_vec + c])) : 0.f;
    }
    __syncthreads();
  }
  for (int ct = wv; ct * 16 < E; ct += 4) {
    const vae_f4v y = vae_xw(H1, sw + D.off_we, H, E, ct * 16, m16, q4);
    const int col = ct * 16 + m16;
    const float be = col < E ? sw[D.off_vec + H + col] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) ML[(4 * q4 + r) * kVaeTS + col] = (col < E && ids[4 * q4 + r] >= 0) ? y[r] + be : 0.f;
  }
  __syncthreads();
  for (int c = tj; c < 64; c += 16) {
    float z = 0.f;
    if (c < L && ids[ts] >= 0) {
      z = ML[ts * kVaeTS + c];
      if (D.variational && eps) z = fmaf(eps[(size_t)(row0 + ts) * L + c], expf(0.5f * ML[ts * kVaeTS + L + c]), z);
    }
    Z[ts * kVaeTS + c] = z;
  }
  __syncthreads();
  for (int ct = wv; ct * 16 < 128; ct += 4) {
    const int col = ct * 16 + m16;
    vae_f4v y = {0.f, 0.f, 0.f, 0.f};
    if (ct * 16 < H) y = vae_xw(Z, sw + D.off_wd, L, H, ct * 16, m16, q4);
    const float bd = col < H ? sw[D.off_vec + H + E + col] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) H2[(4 * q4 + r) * kVaeTS + col] = (col < H && ids[4 * q4 + r] >= 0) ? tanhf(y[r] + bd) : 0.f;
  }
  __syncthreads();
}

// rows first .. of a tile (ld floats each) to global rows, those < n_rows
__device__ __forceinline__ void vae_unstage(const float *T, float *__restrict__ dst, int first, int n_rows, int ld) {
  const int per = ld >> 2;
  for (int i = threadIdx.x; i < 16 * per; i += 256) {
    const int r = i / per, c4 = i - r * per;
    if (first + r < n_rows) reinterpret_cast<float4 *>(dst + (size_t)(first + r) * ld)[c4] = *reinterpret_cast<const float4 *>(T + r * kVaeTS + 4 * c4);
  }
}

struct VaeActs {
  float *H2, *H1, *ML, *Z;     // [B, ldh], [B, ldh], [B, lde], [B, ldz]
  int lde, ldz;
};

__global__ __launch_bounds__(256) void k_vae_encode(DrxVaeDims D, const float *__restrict__ W_in, const float *__restrict__ sw,
                                                    const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                    const int32_t *__restrict__ uid, const int32_t *__restrict__ boff, int B, int T, int group,
                                                    const uint8_t *__restrict__ keep, const float *__restrict__ eps, float dropout,
                                                    VaeActs A, int32_t *__restrict__ keys, float *__restrict__ scale,
                                                    float *__restrict__ nrow, double *__restrict__ kl_part) {
  __shared__ __align__(16) float tiles[4 * kVaeTile];
  __shared__ float cbv[16];
  __shared__ float klrow[16];
  __shared__ int ids[16], koff[16], soff[16], nuv[16];
  float *const H1 = tiles, *const ML = H1 + kVaeTile, *const Z = ML + kVaeTile, *const H2 = Z + kVaeTile;
  const int ts = threadIdx.x >> 4, tj = threadIdx.x & 15;
  const int L = D.latent;
  double kl = 0.0;
  const int n_tiles = (B + 15) / 16;
#pragma unroll 1
  for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    __syncthreads();
    if (threadIdx.x < 16) {
      const int row = t * 16 + (int)threadIdx.x;
      ids[threadIdx.x] = row < B ? uid[row] : -1;
      koff[threadIdx.x] = row < B ? boff[row] : 0;
      soff[threadIdx.x] = row < B ? row * group : 0;
    }
    __syncthreads();
    vae_forward(D, W_in, sw, indptr, indices, ids, koff, soff, t * 16, T, group, keep, eps, dropout, keys, scale, H1, ML, Z, H2, cbv, nuv);
    vae_unstage(H2, A.H2, t * 16, B, D.ldh);
    vae_unstage(H1, A.H1, t * 16, B, D.ldh);
    vae_unstage(ML, A.ML, t * 16, B, A.lde);
    vae_unstage(Z, A.Z, t * 16, B, A.ldz);
    if (threadIdx.x < 16 && t * 16 + (int)threadIdx.x < B) nrow[t * 16 + threadIdx.x] = (float)nuv[threadIdx.x];
    // KL of a row = -1/2 sum (1 + logvar - mu^2 - exp(logvar)), 16 lanes a row, then the rows ascending
    float s = 0.f;
    if (D.variational && ids[ts] >= 0) {
      for (int c = tj; c < L; c += 16) {
        const float mu = ML[ts * kVaeTS + c], lv = ML[ts * kVaeTS + L + c];
        s += (1.0f + lv) - mu * mu - expf(lv);
      }
    }
    s = group_sum<16>(s);
    if (tj == 0) klrow[ts] = -0.5f * s;
    __syncthreads();
    if (threadIdx.x == 0)
      for (int r = 0; r < 16; ++r) kl += (double)klrow[r];
  }
  if (threadIdx.x == 0) kl_part[blockIdx.x] = kl;
}

// ---- pass 1: (max, sum exp(logit - max)) of every row over the item tiles of a workgroup ---------------------------------------------
// Workgroup g walks the item tiles g, g + grid, ...; its waves take the row tiles wv, wv + 4, ...; part[g][row] is its own.
__device__ __forceinline__ void vae_stage_items(float *Wt, float *bt, const float *__restrict__ W_out, const float *__restrict__ b_out,
                                                int item0, const DrxVaeDims &D) {
  vae_stage(Wt, W_out, item0, D.n_items, D.ldh, threadIdx.x, 256);
  if (threadIdx.x < 16) bt[threadIdx.x] = item0 + (int)threadIdx.x < D.n_items ? b_out[item0 + threadIdx.x] : 0.f;
}

__global__ __launch_bounds__(256) void k_vae_lse(DrxVaeDims D, const float *__restrict__ H2g, const float *__restrict__ W_out,
                                                 const float *__restrict__ b_out, int B, float2 *__restrict__ part) {
  __shared__ __align__(16) float Wt[kVaeTile];
  __shared__ __align__(16) float Ht[4 * kVaeTile];
  __shared__ float bt[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m16 = lane & 15, q4 = lane >> 4;
  const int n_it = (D.n_items + 15) / 16, n_rt = (B + 15) / 16;
  float2 *const mine = part + (size_t)blockIdx.x * B;
  float *const Hw = Ht + wv * kVaeTile;
#pragma unroll 1
  for (int it = blockIdx.x; it < n_it; it += gridDim.x) {
    const bool first = it == (int)blockIdx.x;
    __syncthreads();
    vae_stage_items(Wt, bt, W_out, b_out, it * 16, D);
#pragma unroll 1
    for (int rt0 = 0; rt0 < n_rt; rt0 += 4) {
      const int rt = rt0 + wv;
      __syncthreads();
      vae_stage(Hw, H2g, rt * 16, B, D.ldh, lane, 64);
      __syncthreads();
      const vae_f4v acc = vae_logits(Hw, Wt, D.h, m16, q4);
      const bool item_ok = it * 16 + m16 < D.n_items;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rt * 16 + 4 * q4 + r;
        const float v = item_ok ? acc[r] + bt[m16] : -3.0e38f;
        float top = v;
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) top = fmaxf(top, __shfl_xor(top, m, kWave));
        const float sum = group_sum<16>(item_ok ? expf(v - top) : 0.f);
        if (m16 == 0 && row < B) {
          float2 ms = make_float2(top, sum);
          if (!first) {
            const float2 old = mine[row];
            const float nm = fmaxf(old.x, top);
            ms = make_float2(nm, fmaf(old.y, expf(old.x - nm), sum * expf(top - nm)));
          }
          mine[row] = ms;
        }
      }
    }
  }
}

// lse[row] = the n_parts partials of the row combined in workgroup order
__global__ __launch_bounds__(256) void k_vae_lse_combine(const float2 *__restrict__ part, int n_parts, int B, float2 *__restrict__ lse) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= B) return;
  float2 ms = part[row];
  for (int g = 1; g < n_parts; ++g) {
    const float2 p = part[(size_t)g * B + row];
    const float nm = fmaxf(ms.x, p.x);
    ms = make_float2(nm, fmaf(ms.y, expf(ms.x - nm), p.y * expf(p.x - nm)));
  }
  lse[row] = ms;
}

// ---- pass 2 ------------------------------------------------------------------------------------------------------------------------------
struct VaeOutOpt {
  int kind;
  float alpha, b1, b2, eps, reg;
  float *w_s1, *w_s2, *b_s1, *b_s2;
};

__global__ __launch_bounds__(256) void k_vae_out(DrxVaeDims D, const float *__restrict__ H2g, float *W_out, float *b_out, VaeOutOpt O,
                                                 const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                 const int32_t *__restrict__ uid, const float2 *__restrict__ lse, int B,
                                                 float *__restrict__ slab, double *__restrict__ loss_part) {
  __shared__ __align__(16) float Wt[kVaeTile];
  __shared__ __align__(16) float Ht[4 * kVaeTile];                  // after the row tiles of an item tile: the four waves' dW_out
  __shared__ float DL[4 * 16 * kVaeDS];
  __shared__ float bt[16], dbp[4 * 16], rm[kVaeChunk], rs[kVaeChunk];
  __shared__ int msk[kVaeChunk], nu[kVaeChunk];
  __shared__ double lossw[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m16 = lane & 15, q4 = lane >> 4;
  const int H = D.h;
  const int n_it = (D.n_items + 15) / 16, n_rt = (B + 15) / 16;
  const float inv_b = 1.0f / (float)B;
  float *const mine = slab + (size_t)blockIdx.x * B * D.ldh;
  float *const Hw = Ht + wv * kVaeTile;
  float *const DLw = DL + wv * 16 * kVaeDS;
  double loss = 0.0;
#pragma unroll 1
  for (int it = blockIdx.x; it < n_it; it += gridDim.x) {
    const bool first = it == (int)blockIdx.x;
    const int item0 = it * 16;
    __syncthreads();
    vae_stage_items(Wt, bt, W_out, b_out, item0, D);
    vae_f4v dw[8];
#pragma unroll
    for (int ct = 0; ct < 8; ++ct) dw[ct] = vae_f4v{0.f, 0.f, 0.f, 0.f};
    float db = 0.f;
    const bool item_ok = item0 + m16 < D.n_items;
#pragma unroll 1
    for (int c0 = 0; c0 < B; c0 += kVaeChunk) {
    // a chunk of rows: each row's members among the tile's items, from its ascending CSR row, its N_u and its (max, sum)
    __syncthreads();
    for (int i = threadIdx.x; i < kVaeChunk; i += 256) {
      const int row = c0 + i;
      int mask = 0, n = 0;
      float2 ms = make_float2(0.f, 1.f);
      if (row < B) {
        const int u = uid[row];
        const int64_t p0 = indptr[u], p1 = indptr[u + 1];
        n = (int)(p1 - p0);
        int64_t lo = p0, hi = p1;
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (indices[mid] < item0) lo = mid + 1;
          else hi = mid;
        }
        for (; lo < p1; ++lo) {
          const int d = indices[lo] - item0;
          if (d >= 16) break;
          mask |= 1 << d;
        }
        ms = lse[row];
      }
      msk[i] = mask;
      nu[i] = n;
      rm[i] = ms.x;
      rs[i] = ms.y;
    }
    const int rt_end = min(n_rt, (c0 + kVaeChunk) / 16);
#pragma unroll 1
    for (int rt0 = c0 / 16; rt0 < rt_end; rt0 += 4) {
      const int rt = rt0 + wv;
      __syncthreads();
      vae_stage(Hw, H2g, rt * 16, B, D.ldh, lane, 64);
      __syncthreads();
      const vae_f4v acc = vae_logits(Hw, Wt, H, m16, q4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = 4 * q4 + r, row = rt * 16 + lr, li = row - c0;
        float dl = 0.f;
        if (item_ok && row < B) {
          const float logit = acc[r] + bt[m16];
          const float m = rm[li], s = rs[li];
          const bool member = (msk[li] >> m16) & 1;
          const float p = expf(fminf(logit - m, 0.f)) / s;
          dl = ((float)nu[li] * p - (member ? 1.0f : 0.f)) * inv_b;
          if (member) loss += (double)((m - logit) + logf(s));
        }
        DLw[lr * kVaeDS + m16] = dl;
        db += dl;
      }
      __syncthreads();
      // dW_out tile += dlogit^T h2 (items x hidden); the slab's rows (+)= dlogit W_out tile (rows x hidden)
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) {
        if (ct * 16 < H) {
          const int col = ct * 16 + m16;
          vae_f4v dh = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int k0 = 0; k0 < 16; k0 += 4) {
            const int kk = k0 + q4;
            dw[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(DLw[kk * kVaeDS + m16], col < H ? Hw[kk * kVaeTS + col] : 0.f, dw[ct], 0, 0, 0);
            dh = __builtin_amdgcn_mfma_f32_16x16x4f32(DLw[m16 * kVaeDS + kk], col < H ? Wt[kk * kVaeTS + col] : 0.f, dh, 0, 0, 0);
          }
          if (col < H) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = rt * 16 + 4 * q4 + r;
              if (row < B) {
                float *at = mine + (size_t)row * D.ldh + col;
                *at = first ? dh[r] : *at + dh[r];
              }
            }
          }
        }
      }
    }
    }
    __syncthreads();
    // the four waves' partial sums of the tile's dW_out and db_out, added in wave order; the dense rule in place
#pragma unroll
    for (int ct = 0; ct < 8; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) Hw[(4 * q4 + r) * kVaeTS + ct * 16 + m16] = dw[ct][r];
    db += __shfl_xor(db, 16, kWave);
    db += __shfl_xor(db, 32, kWave);
    if (lane < 16) dbp[wv * 16 + lane] = db;
    __syncthreads();
    {
      const int r = threadIdx.x >> 4, tj = threadIdx.x & 15;
      const int item = item0 + r;
      if (item < D.n_items) {
        const bool h1 = opt_has_s1(O.kind), h2 = opt_has_s2(O.kind);
        const OptScalars o{O.kind, O.alpha, 0.f, O.b1, O.b2, O.eps, O.alpha};
        for (int c = tj; c < H; c += 16) {
          const int at = r * kVaeTS + c;
          const float g = ((Ht[at] + Ht[kVaeTile + at]) + Ht[2 * kVaeTile + at]) + Ht[3 * kVaeTile + at];
          const size_t e = (size_t)item * D.ldh + c;
          float pp = Wt[at], mm = h1 ? O.w_s1[e] : 0.f, vv = h2 ? O.w_s2[e] : 0.f;
          opt_update_dense<-1>(o, fmaf(O.reg, pp, g), pp, mm, vv);
          W_out[e] = pp;
          if (h1) O.w_s1[e] = mm;
          if (h2) O.w_s2[e] = vv;
        }
        if (tj == 0) {
          const float g = ((dbp[r] + dbp[16 + r]) + dbp[32 + r]) + dbp[48 + r];
          float pp = bt[r], mm = h1 ? O.b_s1[item] : 0.f, vv = h2 ? O.b_s2[item] : 0.f;
          opt_update_dense<-1>(o, g, pp, mm, vv);
          b_out[item] = pp;
          if (h1) O.b_s1[item] = mm;
          if (h2) O.b_s2[item] = vv;
        }
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) loss += __shfl_xor(loss, m, kWave);
  if (lane == 0) lossw[wv] = loss;
  __syncthreads();
  if (threadIdx.x == 0) loss_part[blockIdx.x] = ((lossw[0] + lossw[1]) + lossw[2]) + lossw[3];
}

// ---- the backward pass of the small layers, a tile of 16 rows at a time -------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vae_back(DrxVaeDims D, const float *__restrict__ sw, VaeActs A, const float *__restrict__ eps,
                                                  const float *__restrict__ slab, int n_slabs, int B, float kl_weight,
                                                  float *__restrict__ DX1, float *__restrict__ gsw_part, const double *__restrict__ data_part,
                                                  const double *__restrict__ kl_part, int n_kl, double *__restrict__ loss_part) {
  __shared__ __align__(16) float tiles[7 * kVaeTile];
  __shared__ float vacc[2 * kVaeMaxH + 2 * kVaeMaxL];               // b_in [h] | b_e [e] | b_d [h]
  float *const H1 = tiles, *const ML = H1 + kVaeTile, *const Z = ML + kVaeTile, *const H2 = Z + kVaeTile;
  float *const G2 = H2 + kVaeTile, *const GE = G2 + kVaeTile, *const G1 = GE + kVaeTile;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m16 = lane & 15, q4 = lane >> 4;
  const int ts = threadIdx.x >> 4, tj = threadIdx.x & 15;
  const int H = D.h, L = D.latent, E = D.e;
  const int n_vec = 2 * H + E;
  const float inv_b = 1.0f / (float)B;
  for (int i = threadIdx.x; i < n_vec; i += 256) vacc[i] = 0.f;
  vae_f4v gwe[8][2], gwd[4][2];                                     // this wave's column tiles wv, wv + 4 of dW_e [h, e] and dW_d [latent, h]
#pragma unroll
  for (int mi = 0; mi < 8; ++mi)
#pragma unroll
    for (int cj = 0; cj < 2; ++cj) gwe[mi][cj] = vae_f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int cj = 0; cj < 2; ++cj) gwd[mi][cj] = vae_f4v{0.f, 0.f, 0.f, 0.f};
  const int n_tiles = (B + 15) / 16;
#pragma unroll 1
  for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    __syncthreads();
    vae_stage(H1, A.H1, t * 16, B, D.ldh, threadIdx.x, 256);
    vae_stage(ML, A.ML, t * 16, B, A.lde, threadIdx.x, 256);
    vae_stage(Z, A.Z, t * 16, B, A.ldz, threadIdx.x, 256);
    vae_stage(H2, A.H2, t * 16, B, D.ldh, threadIdx.x, 256);
    __syncthreads();
    // G2 <- da2 = (the slabs of dh2 summed in slab order) (1 - h2^2)
    {
      const int row = t * 16 + ts;
      for (int c = tj; c < 128; c += 16) {
        float s = 0.f;
        if (row < B && c < H) {
          for (int g = 0; g < n_slabs; ++g) s += slab[((size_t)g * B + row) * D.ldh + c];
          const float h2 = H2[ts * kVaeTS + c];
          s *= 1.0f - h2 * h2;
        }
        G2[ts * kVaeTS + c] = s;
      }
    }
    __syncthreads();
    vae_colsums(G2, vacc + H + E, H);
    // dW_d += z^T da2;  dz = da2 W_d^T;  GE <- [dmu | dlogvar]
#pragma unroll
    for (int cj = 0; cj < 2; ++cj) {
      const int col0 = (wv + 4 * cj) * 16;
      if (col0 < H) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
          if (mi * 16 < L) gwd[mi][cj] = vae_atb(Z, L, mi * 16, G2, H, col0, m16, q4, gwd[mi][cj]);
      }
    }
    if (wv * 16 < L) {
      const vae_f4v dz = vae_gwt(G2, sw + D.off_wd, L, H, wv * 16, m16, q4);
      const int col = wv * 16 + m16;
      if (col < L) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int lr = 4 * q4 + r, row = t * 16 + lr;
          float dmu = 0.f, dlv = 0.f;
          if (row < B) {
            dmu = dz[r];
            if (D.variational) {
              const float mu = ML[lr * kVaeTS + col], lv = ML[lr * kVaeTS + L + col];
              dmu = fmaf(kl_weight * inv_b, mu, dmu);
              dlv = (kl_weight * inv_b) * (0.5f * (expf(lv) - 1.0f));
              if (eps) dlv = fmaf(dz[r] * eps[(size_t)row * L + col], 0.5f * expf(0.5f * lv), dlv);
            }
          }
          GE[lr * kVaeTS + col] = dmu;
          if (D.variational) GE[lr * kVaeTS + L + col] = dlv;
        }
      }
    }
    __syncthreads();
    vae_colsums(GE, vacc + H, E);
    // dW_e += h1^T dE;  dx1 = (dE W_e^T) (1 - h1^2)
#pragma unroll
    for (int cj = 0; cj < 2; ++cj) {
      const int col0 = (wv + 4 * cj) * 16;
      if (col0 < E) {
#pragma unroll
        for (int mi = 0; mi < 8; ++mi)
          if (mi * 16 < H) gwe[mi][cj] = vae_atb(H1, H, mi * 16, GE, E, col0, m16, q4, gwe[mi][cj]);
      }
    }
#pragma unroll
    for (int cj = 0; cj < 2; ++cj) {
      const int col0 = (wv + 4 * cj) * 16;
      const int col = col0 + m16;
      vae_f4v dh = {0.f, 0.f, 0.f, 0.f};
      if (col0 < H) dh = vae_gwt(GE, sw + D.off_we, H, E, col0, m16, q4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = 4 * q4 + r;
        const float h1 = H1[lr * kVaeTS + col];
        G1[lr * kVaeTS + col] = col < H ? dh[r] * (1.0f - h1 * h1) : 0.f;
      }
    }
    __syncthreads();
    vae_colsums(G1, vacc, H);
    vae_unstage(G1, DX1, t * 16, B, D.ldh);
  }
  // ---- the workgroup's row of partial sums: every entry of it is written
  float *const part = gsw_part + (size_t)blockIdx.x * D.n_small;
#pragma unroll
  for (int cj = 0; cj < 2; ++cj) {
    const int col = (wv + 4 * cj) * 16 + m16;
#pragma unroll
    for (int mi = 0; mi < 8; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = mi * 16 + 4 * q4 + r;
        if (row < H && col < E) part[D.off_we + row * E + col] = gwe[mi][cj][r];
      }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = mi * 16 + 4 * q4 + r;
        if (row < L && col < H) part[D.off_wd + row * H + col] = gwd[mi][cj][r];
      }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_vec; i += 256) part[D.off_vec + i] = vacc[i];
  if (threadIdx.x == 0) {
    double s = 0.0;
    if (blockIdx.x == 0) {
      double kl = 0.0;
      for (int g = 0; g < n_slabs; ++g) s += data_part[g];
      for (int g = 0; g < n_kl; ++g) kl += kl_part[g];
      s += (double)kl_weight * kl;
    }
    loss_part[blockIdx.x] = s;
  }
}

// order[q]: a lookup's place t in the batch's list -> b * group + j, the index of its scale; o / group = b names its row of dx1
__global__ __launch_bounds__(256) void k_vae_remap(int32_t *__restrict__ order, int T, const int32_t *__restrict__ boff, int B, int group) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= T) return;
  const int t = order[q];
  int lo = 0, hi = B - 1;                                             // the last b with boff[b] <= t
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (boff[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  order[q] = lo * group + (t - boff[lo]);
}

// ---- noise -------------------------------------------------------------------------------------------------------------------------------
// threads 0 .. T - 1: the keep byte of a lookup; threads T .. T + B latent - 1: the two words and the Box-Muller value of (b, column)
__global__ __launch_bounds__(256) void k_vae_noise(uint64_t seed, const int32_t *__restrict__ boff, int B, int T, int latent, uint32_t qthr,
                                                   float *__restrict__ eps, uint8_t *__restrict__ keep, uint32_t *__restrict__ words) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < T) {
    if (!keep) return;
    const int t = (int)i;
    int lo = 0, hi = B - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (boff[mid] <= t) lo = mid;
      else hi = mid - 1;
    }
    keep[t] = hash_u32(seed * 2, (uint32_t)lo, (uint32_t)(t - boff[lo])) >= qthr ? 1 : 0;
    return;
  }
  const int64_t e = i - T;
  if (e >= (int64_t)B * latent || (!eps && !words)) return;
  const uint32_t b = (uint32_t)(e / latent), c = (uint32_t)(e % latent);
  const uint32_t w1 = hash_u32(seed * 2 + 1, b, 2 * c), w2 = hash_u32(seed * 2 + 1, b, 2 * c + 1);
  if (words) {
    words[2 * e] = w1;
    words[2 * e + 1] = w2;
  }
  if (eps) {
    const float u1 = ((float)w1 + 1.0f) * 2.3283064365386963e-10f, u2 = (float)w2 * 2.3283064365386963e-10f;
    eps[e] = sqrtf(-2.0f * logf(u1)) * cosf(6.2831855f * u2);
  }
}

// ---- serving -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vae_query_rows(DrxVaeDims D, const float *__restrict__ W_in, const float *__restrict__ sw,
                                                        const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                        const int32_t *__restrict__ uid, int n, float *__restrict__ out) {
  __shared__ __align__(16) float tiles[4 * kVaeTile];
  __shared__ float cbv[16];
  __shared__ int ids[16], zero[16], nuv[16];
  float *const H1 = tiles, *const ML = H1 + kVaeTile, *const Z = ML + kVaeTile, *const H2 = Z + kVaeTile;
  const int n_tiles = (n + 15) / 16;
#pragma unroll 1
  for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    __syncthreads();
    if (threadIdx.x < 16) {
      ids[threadIdx.x] = t * 16 + (int)threadIdx.x < n ? uid[t * 16 + threadIdx.x] : -1;
      zero[threadIdx.x] = 0;
    }
    __syncthreads();
    vae_forward(D, W_in, sw, indptr, indices, ids, zero, zero, t * 16, 0, 0, nullptr, nullptr, 0.f, nullptr, nullptr, H1, ML, Z, H2, cbv, nuv);
    vae_unstage(H2, out, t * 16, n, D.ldh);
  }
}

struct VaeScratch {
  VaeActs A;
  float *DX1, *scale, *nrow, *slab, *gsw_part, *sink;
  float2 *lse_part, *lse;
  double *loss_part, *data_part, *kl_part;
  int32_t *keys, *rp, *ord;
  void *csr;
  size_t csr_bytes;
  int row_grid, item_grid;
};

static bool vae_shape_ok(const DrxVaeDims *D, int64_t B, int64_t T, int64_t max_len) {
  return vae_dims_ok(D) && B >= 1 && B <= kVaeMaxB && T >= 1 && T < (1 << 30) && max_len >= 1 && max_len <= D->n_items &&
         B * max_len < ((int64_t)1 << 31) && T <= B * max_len;
}

static bool vae_carve(Carver &cv, const DrxVaeDims *D, int B, int T, int max_len, VaeScratch &S) {
  if (!vae_shape_ok(D, B, T, max_len)) return false;
  S.row_grid = step_tile_grid(B, kVaeRowGrid);
  S.item_grid = vae_item_grid(D);
  S.A.lde = vae_round4(D->e);
  S.A.ldz = vae_round4(D->latent);
  // h2 first: engine_vae.py VaeEngine.step_hidden reads it at this place (tests/test_gpu_vae.py holds serving's rows to its bits)
  S.A.H2 = cv.take<float>((size_t)B * D->ldh);
  S.A.H1 = cv.take<float>((size_t)B * D->ldh);
  S.A.ML = cv.take<float>((size_t)B * S.A.lde);
  S.A.Z = cv.take<float>((size_t)B * S.A.ldz);
  S.DX1 = cv.take<float>((size_t)B * D->ldh);
  S.scale = cv.take<float>((size_t)B * max_len);
  S.nrow = cv.take<float>((size_t)B);
  S.lse_part = cv.take<float2>((size_t)S.item_grid * B);
  S.lse = cv.take<float2>((size_t)B);
  S.slab = cv.take<float>((size_t)S.item_grid * B * D->ldh);
  S.gsw_part = cv.take<float>((size_t)S.row_grid * D->n_small);
  S.sink = cv.take<float>((size_t)D->n_items);
  S.loss_part = cv.take<double>((size_t)S.row_grid);
  S.data_part = cv.take<double>((size_t)S.item_grid);
  S.kl_part = cv.take<double>((size_t)S.row_grid);
  S.keys = cv.take<int32_t>((size_t)T);
  S.rp = cv.take<int32_t>((size_t)D->n_items + 1);
  S.ord = cv.take<int32_t>((size_t)T);
  const DrxCsrList ls = {S.keys, T, D->n_items, S.rp, S.ord};
  S.csr_bytes = drx_batch_csr_device_bytes(&ls, 1);
  if (!S.csr_bytes) return false;
  S.csr = cv.take<char>(S.csr_bytes);
  return true;
}

}  // namespace drx

extern "C" {

size_t drx_vae_step_scratch_bytes(const DrxVaeDims *D, int32_t B, int32_t T, int32_t max_len) {
  using namespace drx;
  Carver cv = step_dry_carver();
  VaeScratch S;
  return vae_carve(cv, D, B, T, max_len, S) ? step_scratch_total(cv) : 0;
}

int drx_vae_step(const DrxVaeDims *D, float *W_in, float *sw, float *W_out, float *b_out, float *W_in_s1, float *W_in_s2, float *sw_s1,
                 float *sw_s2, float *W_out_s1, float *W_out_s2, float *b_out_s1, float *b_out_s2, const DrxHistory *Hst,
                 const int32_t *uid, const int32_t *boff, int32_t B, int32_t T, int32_t max_len, const float *eps, const uint8_t *keep,
                 float dropout, float kl_weight, const DrxOptRule *rule, const float *alphas, float reg, double *loss_out, void *scratch,
                 size_t scratch_bytes, void *stream) {
  using namespace drx;
  if (!D || !W_in || !sw || !W_out || !b_out || !Hst || !Hst->indptr || !Hst->indices || !uid || !boff || !rule || !alphas || !scratch ||
      !vae_shape_ok(D, B, T, max_len) || !(dropout >= 0.f && dropout < 1.f) || !(kl_weight >= 0.f))
    return DRX_EINVAL;
  const int kind = rule->kind;
  StepTensor t[4] = {{W_in, W_in_s1, W_in_s2}, {W_out, W_out_s1, W_out_s2}, {sw, sw_s1, sw_s2}, {b_out, b_out_s1, b_out_s2}};
  if (!step_tensors_ok(kind, t, 4, 2)) return DRX_EINVAL;
  Carver cv(nullptr, 0);
  if (int rc = step_carver(scratch, scratch_bytes, cv)) return rc;
  VaeScratch S;
  if (!vae_carve(cv, D, B, T, max_len, S)) return DRX_EINVAL;
  if (!cv.ok()) return DRX_ESCRATCH;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_vae_encode, dim3(S.row_grid), dim3(256), 0, st, *D, W_in, sw, Hst->indptr, Hst->indices, uid, boff, B, T, max_len, keep,
                     eps, dropout, S.A, S.keys, S.scale, S.nrow, S.kl_part);
  DRX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_vae_lse, dim3(S.item_grid), dim3(256), 0, st, *D, S.A.H2, W_out, b_out, B, S.lse_part);
  DRX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_vae_lse_combine, dim3((B + 255) / 256), dim3(256), 0, st, S.lse_part, S.item_grid, B, S.lse);
  DRX_LAUNCH_CHECK();
  const VaeOutOpt O{kind, alphas[2], rule->mu, rule->mu2, rule->eps, reg, t[1].s1, t[1].s2, t[3].s1, t[3].s2};
  hipLaunchKernelGGL(k_vae_out, dim3(S.item_grid), dim3(256), 0, st, *D, S.A.H2, W_out, b_out, O, Hst->indptr, Hst->indices, uid, S.lse, B,
                     S.slab, S.data_part);
  DRX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_vae_back, dim3(S.row_grid), dim3(256), 0, st, *D, sw, S.A, D->variational ? eps : nullptr, S.slab, S.item_grid, B,
                     kl_weight, S.DX1, S.gsw_part, S.data_part, S.kl_part, S.row_grid, S.loss_part);
  DRX_LAUNCH_CHECK();
  DrxAdamSegments sg;
  memset(&sg, 0, sizeof(sg));
  sg.n = 2;                                                           // [W_e | W_d] regularised, the biases not
  sg.start[0] = 0; sg.len[0] = D->off_vec; sg.alpha[0] = alphas[1]; sg.l2_coef[0] = reg;
  sg.start[1] = D->off_vec; sg.len[1] = D->n_small - D->off_vec; sg.alpha[1] = alphas[1]; sg.l2_coef[1] = 0.f;
  hipLaunchKernelGGL(k_small_opt<>, dim3((D->n_small + 255) / 256), dim3(256), 0, st, S.gsw_part, S.row_grid, D->n_small, sw, t[2].s1, t[2].s2,
                     sg, kind, rule->mu, rule->mu2, rule->eps, S.loss_part, (double)B, loss_out);
  DRX_LAUNCH_CHECK();
  const DrxCsrList ls = {S.keys, T, D->n_items, S.rp, S.ord};
  if (int rc = drx_batch_csr_device(&ls, 1, S.csr, S.csr_bytes, stream)) return rc;
  hipLaunchKernelGGL(k_vae_remap, dim3((T + 255) / 256), dim3(256), 0, st, S.ord, T, boff, B, max_len);
  DRX_LAUNCH_CHECK();
  // the outer-product form of the CSR update has a scalar per row beside the table: W_in has none, so the lookups' scales add up in a
  // sink in scratch that nobody reads (one array stands for the scalar and both of its slots: a row's lane reads and writes all three)
  const StepTensor sink{S.sink, S.sink, S.sink};
  const DrxCsrAdamTable tab = step_table_outer(S.rp, S.ord, S.DX1, S.scale, max_len, D->ldh, D->n_items, t[0], sink, alphas[0], alphas[0], reg);
  return drx_rows_csr_opt_multi(&tab, 1, rule, stream);
}

int drx_vae_noise(uint64_t seed, const int32_t *boff, int32_t B, int32_t T, int32_t latent, float dropout, float *eps, uint8_t *keep,
                  uint32_t *words, void *stream) {
  using namespace drx;
  if (!boff || B < 1 || B > kVaeMaxB || T < 0 || latent < 1 || latent > kVaeMaxL || !(dropout >= 0.f && dropout < 1.f)) return DRX_EINVAL;
  const int64_t n = (int64_t)T + (int64_t)B * latent;
  hipLaunchKernelGGL(k_vae_noise, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed, boff, B, T, latent,
                     q_threshold(dropout), eps, keep, words);
  DRX_LAUNCH_CHECK();
  return DRX_OK;
}

int drx_vae_query_rows(const float *W_in, const float *sw, const DrxVaeDims *D, const DrxHistory *Hst, const int32_t *uid, int32_t n,
                       float *out, void *stream) {
  using namespace drx;
  if (!W_in || !sw || !D || !Hst || !Hst->indptr || !Hst->indices || !uid || !out || n < 1 || !vae_dims_ok(D) ||
      (((uintptr_t)W_in | (uintptr_t)out) & 15))
    return DRX_EINVAL;
  const int tiles = (n + 15) / 16;
  hipLaunchKernelGGL(k_vae_query_rows, dim3(tiles < 4096 ? tiles : 4096), dim3(256), 0, (hipStream_t)stream, *D, W_in, sw, Hst->indptr,
                     Hst->indices, uid, n, out);
  DRX_LAUNCH_CHECK();
  return DRX_OK;
}

}  // extern "C"
