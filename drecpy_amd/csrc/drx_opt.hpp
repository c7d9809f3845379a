// The update rules of the DENSE steps (drx.h DrxOptRule): Adam and Adagrad as drx_rows.hpp has them, and SGD, momentum, Nesterov momentum,
// RMSprop with and without momentum on top.  The sampled step's kernels stay on drx_rows.hpp's opt_update1 / row_update (Adam and Adagrad
// only) and include nothing of this file.
#pragma once
#include <type_traits>
#include "drx_rows.hpp"

namespace drx {

// the slots a rule has: one it lacks is a NULL pointer that no kernel may touch
__host__ __device__ constexpr bool opt_has_s1(int kind) { return kind != DRX_OPT_SGD; }
__host__ __device__ constexpr bool opt_has_s2(int kind) { return kind == DRX_OPT_ADAM || kind == DRX_OPT_RMSPROP_MOMENTUM; }
// the kinds of the dense entry points (every DRX_OPT_* but the row-wise Adagrad of the sampled step)
inline bool opt_dense_kind(int kind) { return kind >= DRX_OPT_ADAM && kind <= DRX_OPT_RMSPROP_MOMENTUM && kind != DRX_OPT_ROWWISE_ADAGRAD; }
// the rule's slots are there (what it lacks may be anything: it is not passed on)
inline bool opt_slots_ok(int kind, const void *s1, const void *s2) { return (!opt_has_s1(kind) || s1) && (!opt_has_s2(kind) || s2); }

// One element under rule `kind` (KIND >= 0: known at compile time; KIND < 0: o.kind decides).  fp32, one operation at a time, in TF's
// order; momentum rides in o.b1, rho in o.b2, the step size in o.lr (Adam: its lr_t in o.alpha).  Adam and Adagrad are opt_update1's.
template <int KIND = -1>
__device__ __forceinline__ void opt_update_dense(const OptScalars &o, float g, float &p, float &s1, float &s2) {
  const int kind = KIND >= 0 ? KIND : o.kind;
  if (kind == DRX_OPT_ADAM) {
    opt_update1<DRX_OPT_ADAM>(o, g, p, s1, s2);
  } else if (kind == DRX_OPT_SGD) {
    p = p - o.lr * g;
  } else if (kind == DRX_OPT_MOMENTUM || kind == DRX_OPT_NESTEROV) {
    // Keras SGD's dense apply: the accumulator holds the (negative) step
    s1 = s1 * o.b1 - g * o.lr;
    p = kind == DRX_OPT_NESTEROV ? p + (s1 * o.b1 - g * o.lr) : p + s1;
  } else if (kind == DRX_OPT_RMSPROP) {
    // Keras RMSprop without momentum: epsilon OUTSIDE the root
    s1 = s1 + (g * g - s1) * (1.0f - o.b2);
    p = p - o.lr * g / (sqrtf(s1) + o.eps);
  } else if (kind == DRX_OPT_RMSPROP_MOMENTUM) {
    // TF's ApplyRMSProp functor: epsilon INSIDE the root
    s1 = s1 + (g * g - s1) * (1.0f - o.b2);
    s2 = s2 * o.b1 + (g * o.lr) / sqrtf(s1 + o.eps);
    p = p - s2;
  } else {
    opt_update1<DRX_OPT_ADAGRAD>(o, g, p, s1, s2);
  }
}

// row_update (drx_rows.hpp) for the dense rules: g (data gradient, already complete) + rb * p applied to one row of `tab`; s1 / s2 of a
// rule without that slot are NULL and are neither read nor written.  Returns the lane's partial |row|^2 (pre-update).
template <int G, int J, int KIND = -1>
__device__ __forceinline__ float row_update_dense(const OptScalars &o, float *tab, float *s1, float *s2, size_t row, int ld, int lane,
                                                  const float4 (&w)[J], const float4 (&g)[J]) {
  float sq = 0.f;
  const int kind = KIND >= 0 ? KIND : o.kind;
  float4 *pr = reinterpret_cast<float4 *>(tab + row * (size_t)ld);
  float4 *a1 = opt_has_s1(kind) ? reinterpret_cast<float4 *>(s1 + row * (size_t)ld) : nullptr;
  float4 *a2 = opt_has_s2(kind) ? reinterpret_cast<float4 *>(s2 + row * (size_t)ld) : nullptr;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int c = lane + j * G;
    if (4 * c < ld) {
      float4 p = w[j];
      float4 m = a1 ? a1[c] : f4_zero();
      float4 v = a2 ? a2[c] : f4_zero();
      sq += f4_dot(p, p);
      opt_update_dense<KIND>(o, fmaf(o.rb, p.x, g[j].x), p.x, m.x, v.x);
      opt_update_dense<KIND>(o, fmaf(o.rb, p.y, g[j].y), p.y, m.y, v.y);
      opt_update_dense<KIND>(o, fmaf(o.rb, p.z, g[j].z), p.z, m.z, v.z);
      opt_update_dense<KIND>(o, fmaf(o.rb, p.w, g[j].w), p.w, m.w, v.w);
      pr[c] = p;
      if (a1) a1[c] = m;
      if (a2) a2[c] = v;
    }
  }
  return sq;
}

// The same three for kernels that keep their run-time Adam / Adagrad form (KIND < 0: drx_rows.hpp's opt_update1 / row_update with o.kind,
// the code they had before the other rules came) and take the new rules at compile time (KIND >= 0).
template <int KIND>
__device__ __forceinline__ bool rule_has_s1(const OptScalars &o) { return KIND < 0 ? true : opt_has_s1(KIND); }
template <int KIND>
__device__ __forceinline__ bool rule_has_s2(const OptScalars &o) { return KIND < 0 ? o.kind == DRX_OPT_ADAM : opt_has_s2(KIND); }
template <int KIND>
__device__ __forceinline__ void opt_update_rule(const OptScalars &o, float g, float &p, float &s1, float &s2) {
  if constexpr (KIND < 0) opt_update1(o, g, p, s1, s2);
  else opt_update_dense<KIND>(o, g, p, s1, s2);
}
template <int G, int J, int KIND>
__device__ __forceinline__ float row_update_rule(const OptScalars &o, float *tab, float *s1, float *s2, size_t row, int ld, int lane,
                                                 const float4 (&w)[J], const float4 (&g)[J]) {
  if constexpr (KIND < 0) return row_update<G, J>(o, tab, s1, s2, row, ld, lane, w, g);
  else return row_update_dense<G, J, KIND>(o, tab, s1, s2, row, ld, lane, w, g);
}

// f(std::integral_constant<int, kind>) for a dense kind: the rule as a template argument of a step's big kernels
template <class F>
inline int dispatch_opt_kind(int kind, F &&f) {
  switch (kind) {
    case DRX_OPT_ADAM: return f(std::integral_constant<int, DRX_OPT_ADAM>{});
    case DRX_OPT_ADAGRAD: return f(std::integral_constant<int, DRX_OPT_ADAGRAD>{});
    case DRX_OPT_SGD: return f(std::integral_constant<int, DRX_OPT_SGD>{});
    case DRX_OPT_MOMENTUM: return f(std::integral_constant<int, DRX_OPT_MOMENTUM>{});
    case DRX_OPT_NESTEROV: return f(std::integral_constant<int, DRX_OPT_NESTEROV>{});
    case DRX_OPT_RMSPROP: return f(std::integral_constant<int, DRX_OPT_RMSPROP>{});
    case DRX_OPT_RMSPROP_MOMENTUM: return f(std::integral_constant<int, DRX_OPT_RMSPROP_MOMENTUM>{});
    default: return DRX_EINVAL;
  }
}

// ... with Adam and Adagrad left to the run-time form (std::integral_constant<int, -1>): reference-mode CDAE, whose Adam kernels stay as they were
template <class F>
inline int dispatch_opt_kind_keep_adam(int kind, F &&f) {
  switch (kind) {
    case DRX_OPT_ADAM:
    case DRX_OPT_ADAGRAD: return f(std::integral_constant<int, -1>{});
    case DRX_OPT_SGD: return f(std::integral_constant<int, DRX_OPT_SGD>{});
    case DRX_OPT_MOMENTUM: return f(std::integral_constant<int, DRX_OPT_MOMENTUM>{});
    case DRX_OPT_NESTEROV: return f(std::integral_constant<int, DRX_OPT_NESTEROV>{});
    case DRX_OPT_RMSPROP: return f(std::integral_constant<int, DRX_OPT_RMSPROP>{});
    case DRX_OPT_RMSPROP_MOMENTUM: return f(std::integral_constant<int, DRX_OPT_RMSPROP_MOMENTUM>{});
    default: return DRX_EINVAL;
  }
}

}  // namespace drx
