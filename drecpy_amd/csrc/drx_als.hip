// ALS for implicit-feedback WMF (Hu, Koren, Volinsky 2008; include/drx.h "ALS / WMF").
//   drx_als_gram       : G = T^T T.  Workgroups take row strips and accumulate 16 x 16 tiles of the lower triangle with
//                        v_mfma_f32_16x16x4_f32; a second launch adds the strips' tiles in ascending order and mirrors them.  No atomics.
//   drx_als_solve_rows : one half-sweep, one workgroup per row: A = G + lambda I in LDS, the row's entries in rounds of 32 gathered rows
//                        (the next round's loads in flight while this one is multiplied), A += sum_j (w_j y_j) y_j^T on fp32 MFMA with
//                        the accumulators in registers for the whole row, b on the vector units, then a right-looking column Cholesky
//                        of [A; b^T] in LDS (its last row comes out as L^-1 b), the back substitution in one wave, x by float4 stores.
//                        One step of iterative refinement follows, its residual summed in double from the definition.
//   drx_als_loss       : <Gx, Gy>_F + sum over positives of c (1 - s)^2 - s^2 + lambda (tr Gx + tr Gy); scores fp32, sums double.
// Only the lower triangle of a system is formed and read: tile t = m (m + 1) / 2 + n, n <= m, belongs to wave t % 4.
#include "drx_common.hpp"

namespace drx {

typedef float als_f4 __attribute__((ext_vector_type(4)));

constexpr int kAlsChunk = 32;          // entries of a round
constexpr int kAlsGramStrip = 64;      // rows of a Gram strip at the least
constexpr int kAlsGramBlocks = 256;    // strips at the most
constexpr int kAlsLossBlocks = 1024;

__host__ __device__ inline int als_tri_m(int t) {
  int m = 0;
  while ((m + 1) * (m + 2) / 2 <= t) ++m;
  return m;
}

// floats between two staged rows: Kp and a shift of 16 banks, so that the four rows a k-step reads lie in four quarters of the banks
__host__ __device__ constexpr int als_stage_stride(int Kp) { return (Kp + 47) / 64 * 64 + 16; }

// the solve's LDS in floats: [A: Kp + 1 rows of Kp + 1][stage: 2 x 32 rows][ws: 2 x 32][col: Kp + 4][dg: Kp][xs: Kp]
__host__ __device__ constexpr int als_a_floats(int Kp) { return ((Kp + 1) * (Kp + 1) + 3) & ~3; }
__host__ __device__ constexpr int als_solve_lds_floats(int Kp) {
  return als_a_floats(Kp) + 2 * kAlsChunk * als_stage_stride(Kp) + 2 * kAlsChunk + (Kp + 4) + 2 * Kp;
}

// ---- G = T^T T -------------------------------------------------------------------------------------------------------------------
// part[(strip * NTT + t) * 64 + lane] = the lane's four accumulators of tile t over the strip's rows (C/D map: col = lane & 15,
// row = 4 (lane >> 4) + reg).  A operand: T[k][16 m + (lane & 15)], B operand: T[k][16 n + (lane & 15)], k = row quad + (lane >> 4).
template <int NT>
__global__ __launch_bounds__(kBlock) void k_als_gram(const float *__restrict__ T, int n_rows, int ld, int strip, als_f4 *__restrict__ part) {
  constexpr int NTT = NT * (NT + 1) / 2, TPW = (NTT + 3) / 4;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, kq = lane >> 4;
  int tm[TPW], tn[TPW];
  als_f4 acc[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int t = wave + 4 * i;
    tm[i] = als_tri_m(t < NTT ? t : 0);
    tn[i] = (t < NTT ? t : 0) - tm[i] * (tm[i] + 1) / 2;
    acc[i] = als_f4{0.f, 0.f, 0.f, 0.f};
  }
  const int r0 = blockIdx.x * strip;
  const int r1 = r0 + strip < n_rows ? r0 + strip : n_rows;
  for (int r = r0; r < r1; r += 4) {
    const int row = r + kq;
    const float *src = T + (size_t)(row < r1 ? row : r0) * ld;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      if (wave + 4 * i >= NTT) continue;
      const int ca = 16 * tm[i] + c, cb = 16 * tn[i] + c;
      const float a = row < r1 && ca < ld ? src[ca] : 0.f;
      const float b = row < r1 && cb < ld ? src[cb] : 0.f;
      acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[i], 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < TPW; ++i)
    if (wave + 4 * i < NTT) part[((size_t)blockIdx.x * NTT + wave + 4 * i) * 64 + lane] = acc[i];
}

// one thread per (tile, lane): the strips' accumulators added in ascending order, written at (row, col) and, off the diagonal tiles,
// at (col, row)
__global__ __launch_bounds__(kBlock) void k_als_gram_sum(const als_f4 *__restrict__ part, int strips, int ntt, int ld, float *__restrict__ G) {
  const int id = blockIdx.x * kBlock + threadIdx.x;
  if (id >= ntt * 64) return;
  const int t = id >> 6, lane = id & 63;
  als_f4 s = part[id];
  for (int b = 1; b < strips; ++b) {
    const als_f4 v = part[(size_t)b * ntt * 64 + id];
    s += v;
  }
  const int m = als_tri_m(t), n = t - m * (m + 1) / 2;
  const int col = 16 * n + (lane & 15);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * m + 4 * (lane >> 4) + r;
    if (row < ld && col < ld) {
      G[(size_t)row * ld + col] = s[r];
      if (m != n) G[(size_t)col * ld + row] = s[r];
    }
  }
}

// ---- one half-sweep ----------------------------------------------------------------------------------------------------------------
struct AlsSolveArgs {
  float *out;
  const float *other, *G;
  const int64_t *indptr;
  const int32_t *indices;
  const float *weights;
  const int32_t *order;
  int n_rows, n_other, ld;
  float lambda;
  int32_t *fail_count;
};

// PARTS: 3 everywhere but in scripts/als_bench.py's own build of this file (DRX_ALS_BENCH_PARTS), which also instantiates 1 (the
// accumulation over the entries alone; out = b) and 2 (the factorisation and the two substitutions alone) to time the two against each other
template <int NT, int PARTS>
__global__ __launch_bounds__(kBlock) void k_als_solve(AlsSolveArgs a) {
  extern __shared__ __align__(16) float als_lds[];
  constexpr int Kp = 16 * NT, AS = Kp + 1, SS = als_stage_stride(Kp), C = kAlsChunk;
  constexpr int NTT = NT * (NT + 1) / 2, TPW = (NTT + 3) / 4, PF = (C * NT * 4 + kBlock - 1) / kBlock;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ld = a.ld, q4 = ld >> 2;
  const int row = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
  if ((unsigned)row >= (unsigned)a.n_rows) return;
  const int64_t e0 = a.indptr[row], e1 = a.indptr[row + 1];
  float *out = a.out + (size_t)row * ld;
  if (e1 <= e0) {                                       // no entries: b = 0, so x = 0
    if (tid < q4) reinterpret_cast<float4 *>(out)[tid] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  float *A = als_lds;
  float *stage = A + als_a_floats(Kp);
  float *ws = stage + 2 * C * SS;
  float *col = ws + 2 * C;
  float *dg = col + Kp + 4;
  float *xs = dg + Kp;

  // (a) the lower triangle of A = G + lambda I; the stage's padding columns and idle rows are zero from here on
  for (int m = wave; m < ld; m += 4)
    for (int n = lane; n <= m; n += 64) A[m * AS + n] = a.G[(size_t)m * ld + n] + (m == n ? a.lambda : 0.f);
  for (int i = tid; i < 2 * C * SS; i += kBlock) stage[i] = 0.f;
  __syncthreads();

  int tm[TPW], tn[TPW];
  als_f4 acc[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int t = wave + 4 * i;
    tm[i] = als_tri_m(t < NTT ? t : 0);
    tn[i] = (t < NTT ? t : 0) - tm[i] * (tm[i] + 1) / 2;
    acc[i] = als_f4{0.f, 0.f, 0.f, 0.f};
  }
  float bacc = 0.f;

  if (PARTS & 1) {
    // (b) slot s = tid + 256 f of a round is float4 q of entry j: s = j q4 + q; an entry past the row's end, or an id outside the
    // table, is a zero row with weight zero
    float4 v[PF];
    float wreg;
    auto fetch = [&](int64_t eb) {
#pragma unroll
      for (int f = 0; f < PF; ++f) {
        const int s = tid + kBlock * f;
        v[f] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (s < C * q4) {
          const int j = s / q4, q = s - j * q4;
          if (eb + j < e1) {
            const int id = a.indices[eb + j];
            if ((unsigned)id < (unsigned)a.n_other) v[f] = reinterpret_cast<const float4 *>(a.other + (size_t)id * ld)[q];
          }
        }
      }
      wreg = tid < C && eb + tid < e1 ? a.weights[eb + tid] : 0.f;
    };
    auto commit = [&](int buf) {
#pragma unroll
      for (int f = 0; f < PF; ++f) {
        const int s = tid + kBlock * f;
        if (s < C * q4) {
          const int j = s / q4, q = s - j * q4;
          *reinterpret_cast<float4 *>(stage + (buf * C + j) * SS + 4 * q) = v[f];
        }
      }
      if (tid < C) ws[buf * C + tid] = wreg;
    };
    fetch(e0);
    commit(0);
    __syncthreads();
    int buf = 0;
    for (int64_t eb = e0; eb < e1; eb += C, buf ^= 1) {
      const bool more = eb + C < e1;
      if (more) fetch(eb + C);
      const float *st = stage + buf * C * SS;
      const float *w = ws + buf * C;
      if (tid < ld) {
#pragma unroll 8
        for (int j = 0; j < C; ++j) bacc = fmaf(1.f + w[j], st[j * SS + tid], bacc);
      }
#pragma unroll 2
      for (int kk = 0; kk < C / 4; ++kk) {
        const int j = 4 * kk + (lane >> 4);
        const float wj = w[j];
        const float *y = st + j * SS + (lane & 15);
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
          if (wave + 4 * i >= NTT) continue;
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wj * y[16 * tm[i]], y[16 * tn[i]], acc[i], 0, 0, 0);
        }
      }
      if (more) commit(buf ^ 1);
      __syncthreads();
    }
  }

  // (c) the accumulators into A (every element of the triangle has one owner), b as row ld
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    if (wave + 4 * i >= NTT) continue;
    const int cc = 16 * tn[i] + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = 16 * tm[i] + 4 * (lane >> 4) + r;
      if (rr < ld && cc <= rr) A[rr * AS + cc] += acc[i][r];
    }
  }
  if (tid < ld) A[ld * AS + tid] = bacc;
  __syncthreads();

  bool fail = false;
  if (PARTS & 2) {
    // right-looking column Cholesky of rows 0 .. ld (row ld is b: it leaves as z = L^-1 b).  A[j][j] keeps the pivot, dg[j] its root.
    const int n = ld;
    for (int j = 0; j < n; ++j) {
      const float d = A[j * AS + j];
      if (!(d > 0.f) || !(d < INFINITY)) {            // (every thread reads the same pivot)
        fail = true;
        break;
      }
      const float s = sqrtf(d);
      if (tid > j && tid <= n) {
        const float l = A[tid * AS + j] / s;
        col[tid] = l;
        A[tid * AS + j] = l;
      }
      if (tid == j) dg[j] = s;
      __syncthreads();
      for (int i = j + 1 + (tid >> 4); i <= n; i += 16) {
        const float li = col[i];
        for (int k = j + 1 + (tid & 15); k <= i && k < n; k += 16) A[i * AS + k] = fmaf(-li, col[k], A[i * AS + k]);
      }
      __syncthreads();
    }
    // L^T x = z in one wave: lane l holds z[l] and z[l + 64]; step j takes x[j] and row j of L, read one step ahead.  add: xs += x
    auto back = [&](float z0, float z1, bool add) {
      float l0 = lane < n - 1 ? A[(n - 1) * AS + lane] : 0.f;
      float l1 = lane + 64 < n - 1 ? A[(n - 1) * AS + lane + 64] : 0.f;
      float dj = dg[n - 1];
      for (int j = n - 1; j >= 0; --j) {
        const float c0 = l0, c1 = l1, cd = dj;
        if (j > 0) {
          l0 = lane < j - 1 ? A[(j - 1) * AS + lane] : 0.f;
          l1 = lane + 64 < j - 1 ? A[(j - 1) * AS + lane + 64] : 0.f;
          dj = dg[j - 1];
        }
        const float xj = __shfl(j < 64 ? z0 : z1, j & 63, 64) / cd;
        if (lane < j) z0 = fmaf(-c0, xj, z0);
        if (lane + 64 < j) z1 = fmaf(-c1, xj, z1);
        if (lane == 0) xs[j] = add ? xs[j] + xj : xj;
      }
    };
    if (!fail && wave == 0) back(lane < n ? A[n * AS + lane] : 0.f, lane + 64 < n ? A[n * AS + lane + 64] : 0.f, false);
    if (!fail && PARTS == 3) {
      // ONE step of iterative refinement.  The residual comes from the definition, in double, not from the rounded A:
      //   r = sum_j [(1 + w_j) - w_j (y_j . x)] y_j - G x - lambda x
      // (wave w takes the entries w, w + 4, ...; lane l the columns l and l + 64; a fixed shuffle tree per entry, the four waves
      // added in order), then L L^T d = r in fp32 and x += d.  What is left is the rounding of G and of x itself.
      __syncthreads();
      double *rw = reinterpret_cast<double *>(stage);   // (the stages are free: 4 Kp doubles of their 64 rows)
      const double x0 = lane < ld ? (double)xs[lane] : 0.0, x1 = lane + 64 < ld ? (double)xs[lane + 64] : 0.0;
      double r0 = 0.0, r1 = 0.0;
      for (int64_t e = e0 + wave; e < e1; e += 4) {
        const int id = a.indices[e];
        if ((unsigned)id >= (unsigned)a.n_other) continue;
        const float *yr = a.other + (size_t)id * ld;
        const double y0 = lane < ld ? (double)yr[lane] : 0.0, y1 = lane + 64 < ld ? (double)yr[lane + 64] : 0.0;
        double sc = y0 * x0 + y1 * x1;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) sc += __shfl_xor(sc, m, 64);
        const double wj = (double)a.weights[e], c = (1.0 + wj) - wj * sc;
        r0 += c * y0;
        r1 += c * y1;
      }
      if (lane < Kp) rw[wave * Kp + lane] = r0;
      if (lane + 64 < Kp) rw[wave * Kp + lane + 64] = r1;
      __syncthreads();
      if (tid < ld) {
        double g = (double)a.lambda * (double)xs[tid];
        for (int m = 0; m < ld; ++m) g += (double)a.G[(size_t)m * ld + tid] * (double)xs[m];      // (G is symmetric bit for bit)
        col[tid] = (float)((((rw[tid] + rw[Kp + tid]) + rw[2 * Kp + tid]) + rw[3 * Kp + tid]) - g);
      }
      __syncthreads();
      if (wave == 0) {
        // L z = r by columns: lane l holds r[l] and r[l + 64] and, once step l has passed, z[l]
        float z0 = lane < n ? col[lane] : 0.f, z1 = lane + 64 < n ? col[lane + 64] : 0.f;
        for (int j = 0; j < n; ++j) {
          const float zj = __shfl(j < 64 ? z0 : z1, j & 63, 64) / dg[j];
          if (lane > j && lane < n) z0 = fmaf(-A[lane * AS + j], zj, z0);
          if (lane + 64 > j && lane + 64 < n) z1 = fmaf(-A[(lane + 64) * AS + j], zj, z1);
          if (lane == (j & 63)) {
            if (j < 64) z0 = zj; else z1 = zj;
          }
        }
        back(z0, z1, true);
      }
    }
  } else if (tid < ld) {
    xs[tid] = A[ld * AS + tid];
  }
  __syncthreads();
  if (tid < q4) reinterpret_cast<float4 *>(out)[tid] = fail ? make_float4(0.f, 0.f, 0.f, 0.f) : reinterpret_cast<const float4 *>(xs)[tid];
  if (fail && tid == 0) atomicAdd(a.fail_count, 1);
}

// ---- the loss ------------------------------------------------------------------------------------------------------------------------
// workgroup b takes users b, b + grid, ...; wave w the entries w, w + 4, ... of a user; part[b] = the workgroup's sum of
// c (1 - s)^2 - s^2, s = x_u . y_i as an fp32 fmaf chain per lane and a fixed shuffle tree
__global__ __launch_bounds__(kBlock) void k_als_loss_rows(const float *__restrict__ X, const float *__restrict__ Y, const int64_t *__restrict__ indptr,
                                                          const int32_t *__restrict__ indices, const float *__restrict__ weights, int n_users,
                                                          int n_items, int ld, double *__restrict__ part) {
  __shared__ double wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double sum = 0.0;
  for (int u = blockIdx.x; u < n_users; u += gridDim.x) {
    const float x0 = lane < ld ? X[(size_t)u * ld + lane] : 0.f;
    const float x1 = lane + 64 < ld ? X[(size_t)u * ld + lane + 64] : 0.f;
    const int64_t e1 = indptr[u + 1];
    for (int64_t e = indptr[u] + wave; e < e1; e += 4) {
      const int i = indices[e];
      if ((unsigned)i >= (unsigned)n_items) continue;
      float s = lane < ld ? x0 * Y[(size_t)i * ld + lane] : 0.f;
      if (lane + 64 < ld) s = fmaf(x1, Y[(size_t)i * ld + lane + 64], s);
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
      const double sd = (double)s, c = 1.0 + (double)weights[e];
      sum += c * (1.0 - sd) * (1.0 - sd) - sd * sd;
    }
  }
  if (lane == 0) wsum[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// out[0] = sum_kl Gx[k][l] Gy[k][l] + lambda (tr Gx + tr Gy) + the n partials: thread t adds elements t, t + 256, ... ascending, then a
// fixed tree
__global__ __launch_bounds__(kBlock) void k_als_loss_sum(const float *__restrict__ Gx, const float *__restrict__ Gy, int ld, float lambda,
                                                         const double *__restrict__ part, int n, double *__restrict__ out) {
  __shared__ double red[kBlock];
  double s = 0.0;
  for (int k = threadIdx.x; k < ld * ld; k += kBlock) s += (double)Gx[k] * (double)Gy[k];
  for (int k = threadIdx.x; k < ld; k += kBlock) s += (double)lambda * ((double)Gx[k * ld + k] + (double)Gy[k * ld + k]);
  for (int k = threadIdx.x; k < n; k += kBlock) s += part[k];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int m = kBlock / 2; m >= 1; m >>= 1) {
    if (threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

static bool als_ld_ok(int ld) { return ld >= 4 && ld <= 128 && !(ld & 3); }
static bool als_lambda_ok(float lambda) { return lambda >= 0.f && lambda < INFINITY; }
static bool als_aligned(const void *p) { return !((uintptr_t)p & 15); }

// the tile counts the kernels are built for; the smallest that holds ld
template <class F>
static int als_dispatch(int ld, F &&f) {
  const int nt = (ld + 15) / 16;
  if (nt <= 1) return f(std::integral_constant<int, 1>{});
  if (nt <= 2) return f(std::integral_constant<int, 2>{});
  if (nt <= 3) return f(std::integral_constant<int, 3>{});
  if (nt <= 4) return f(std::integral_constant<int, 4>{});
  if (nt <= 6) return f(std::integral_constant<int, 6>{});
  return f(std::integral_constant<int, 8>{});
}

static int als_gram_strips(int n_rows, int *strip) {
  int s = (n_rows + kAlsGramBlocks - 1) / kAlsGramBlocks;
  if (s < kAlsGramStrip) s = kAlsGramStrip;
  s = (s + 3) & ~3;
  *strip = s;
  return (n_rows + s - 1) / s;
}

static int als_loss_blocks(int n_users) { return n_users < kAlsLossBlocks ? n_users : kAlsLossBlocks; }

template <int PARTS>
static int als_solve(const AlsSolveArgs &a, hipStream_t st) {
  return als_dispatch(a.ld, [&](auto nt) -> int {
    constexpr int NT = decltype(nt)::value;
    constexpr size_t lds = (size_t)als_solve_lds_floats(16 * NT) * 4;
    if (lds > 48 * 1024) DRX_HIP(hipFuncSetAttribute((const void *)(k_als_solve<NT, PARTS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_als_solve<NT, PARTS>), dim3(a.n_rows), dim3(kBlock), lds, st, a);
    DRX_LAUNCH_CHECK();
    return DRX_OK;
  });
}

}  // namespace drx

extern "C" {

size_t drx_als_gram_scratch_bytes(int32_t n_rows, int32_t ld) {
  using namespace drx;
  if (n_rows < 1 || !als_ld_ok(ld)) return 0;
  int strip;
  const int strips = als_gram_strips(n_rows, &strip);
  const int nt = als_dispatch(ld, [](auto t) -> int { return decltype(t)::value; });
  return (size_t)strips * (nt * (nt + 1) / 2) * 64 * sizeof(als_f4) + 256;          // (+ 256: the call aligns the base it is given)
}

int drx_als_gram(const float *table, int32_t n_rows, int32_t ld, float *out_G, void *scratch, size_t scratch_bytes, void *stream) {
  using namespace drx;
  if (!table || !out_G || !scratch || n_rows < 1 || !als_ld_ok(ld) || !als_aligned(table) || !als_aligned(out_G)) return DRX_EINVAL;
  if (scratch_bytes < drx_als_gram_scratch_bytes(n_rows, ld)) return DRX_ESCRATCH;
  als_f4 *part = (als_f4 *)(((uintptr_t)scratch + 255) & ~uintptr_t(255));
  int strip;
  const int strips = als_gram_strips(n_rows, &strip);
  hipStream_t st = (hipStream_t)stream;
  return als_dispatch(ld, [&](auto nt) -> int {
    constexpr int NT = decltype(nt)::value, NTT = NT * (NT + 1) / 2;
    hipLaunchKernelGGL(k_als_gram<NT>, dim3(strips), dim3(kBlock), 0, st, table, n_rows, ld, strip, part);
    hipLaunchKernelGGL(k_als_gram_sum, dim3((NTT * 64 + kBlock - 1) / kBlock), dim3(kBlock), 0, st, part, strips, NTT, ld, out_G);
    DRX_LAUNCH_CHECK();
    return DRX_OK;
  });
}

size_t drx_als_solve_rows_scratch_bytes(int32_t n_rows, int32_t n_other, int32_t ld) {
  using namespace drx;
  if (n_rows < 1 || n_other < 1 || !als_ld_ok(ld)) return 0;
  return 256;                                           // (a row's system lives in its workgroup's LDS: nothing is carved)
}

// the validated half-sweep with the kernel's PARTS
extern "C++" template <int PARTS>
static int als_solve_rows(float *out, const float *other, const float *G, const int64_t *indptr, const int32_t *indices, const float *weights,
                          const int32_t *order, int32_t n_rows, int32_t n_other, int32_t ld, float lambda, int32_t *fail_count, void *scratch,
                          size_t scratch_bytes, void *stream) {
  using namespace drx;
  if (!out || !other || !G || !indptr || !indices || !weights || !fail_count || !scratch || n_rows < 1 || n_other < 1 || !als_ld_ok(ld) ||
      !als_lambda_ok(lambda) || !als_aligned(out) || !als_aligned(other) || !als_aligned(G))
    return DRX_EINVAL;
  if (scratch_bytes < drx_als_solve_rows_scratch_bytes(n_rows, n_other, ld)) return DRX_ESCRATCH;
  AlsSolveArgs a{out, other, G, indptr, indices, weights, order, n_rows, n_other, ld, lambda, fail_count};
  return als_solve<PARTS>(a, (hipStream_t)stream);
}

int drx_als_solve_rows(float *out, const float *other, const float *G, const int64_t *indptr, const int32_t *indices, const float *weights,
                       const int32_t *order, int32_t n_rows, int32_t n_other, int32_t ld, float lambda, int32_t *fail_count, void *scratch,
                       size_t scratch_bytes, void *stream) {
  return als_solve_rows<3>(out, other, G, indptr, indices, weights, order, n_rows, n_other, ld, lambda, fail_count, scratch, scratch_bytes, stream);
}

#ifdef DRX_ALS_BENCH_PARTS
// not part of libdrx.so or include/drx.h: scripts/als_bench.py compiles this file alone with the macro and loads the result beside it
int drx_als_bench_solve_rows_parts(float *out, const float *other, const float *G, const int64_t *indptr, const int32_t *indices,
                                   const float *weights, const int32_t *order, int32_t n_rows, int32_t n_other, int32_t ld, float lambda,
                                   int32_t *fail_count, int32_t parts, void *scratch, size_t scratch_bytes, void *stream) {
  if (parts == 1)
    return als_solve_rows<1>(out, other, G, indptr, indices, weights, order, n_rows, n_other, ld, lambda, fail_count, scratch, scratch_bytes, stream);
  if (parts == 2)
    return als_solve_rows<2>(out, other, G, indptr, indices, weights, order, n_rows, n_other, ld, lambda, fail_count, scratch, scratch_bytes, stream);
  if (parts == 3)
    return als_solve_rows<3>(out, other, G, indptr, indices, weights, order, n_rows, n_other, ld, lambda, fail_count, scratch, scratch_bytes, stream);
  return DRX_EINVAL;
}
#endif

size_t drx_als_loss_scratch_bytes(int32_t n_users, int32_t ld) {
  using namespace drx;
  if (n_users < 1 || !als_ld_ok(ld)) return 0;
  return (size_t)als_loss_blocks(n_users) * sizeof(double) + 256;
}

int drx_als_loss(const float *X, const float *Y, const float *Gx, const float *Gy, const int64_t *indptr, const int32_t *indices,
                 const float *weights, int32_t n_users, int32_t n_items, int32_t ld, float lambda, double *out_loss, void *scratch,
                 size_t scratch_bytes, void *stream) {
  using namespace drx;
  if (!X || !Y || !Gx || !Gy || !indptr || !indices || !weights || !out_loss || !scratch || n_users < 1 || n_items < 1 || !als_ld_ok(ld) ||
      !als_lambda_ok(lambda) || !als_aligned(X) || !als_aligned(Y) || !als_aligned(Gx) || !als_aligned(Gy))
    return DRX_EINVAL;
  if (scratch_bytes < drx_als_loss_scratch_bytes(n_users, ld)) return DRX_ESCRATCH;
  double *part = (double *)(((uintptr_t)scratch + 255) & ~uintptr_t(255));
  const int blocks = als_loss_blocks(n_users);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_als_loss_rows, dim3(blocks), dim3(kBlock), 0, st, X, Y, indptr, indices, weights, n_users, n_items, ld, part);
  hipLaunchKernelGGL(k_als_loss_sum, dim3(1), dim3(kBlock), 0, st, Gx, Gy, ld, lambda, part, blocks, out_loss);
  DRX_LAUNCH_CHECK();
  return DRX_OK;
}

}  // extern "C"
