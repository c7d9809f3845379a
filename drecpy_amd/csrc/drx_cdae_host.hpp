// Host-only helpers shared by the CDAE translation units (drx_cdae.hip: the sampled step; drx_cdae_dense.hip: reference mode and
// inference; drx_cdae_parts.hip: the touch list prepared in parts): argument checks and the one size the sampled unit asks of the
// dense one.  No device code lives here.
#pragma once
#include "drx_common.hpp"

namespace drx {

inline int check_params(const DrxCdaeParams *p) {
  if (!p || !p->W || !p->W2T || !p->V || !p->b || !p->b2) return DRX_EINVAL;
  if (p->k < 1 || p->k > DRX_MAX_K || p->ld < p->k || (p->ld & 3) || p->ld > DRX_MAX_K) return DRX_EINVAL;
  if (p->n_users < 1 || p->n_items < 1) return DRX_EINVAL;
  return DRX_OK;
}

inline int check_batch(const DrxHistory *h, const DrxBatch *bt) {
  if (!h || !h->indptr || !h->indices || !bt || !bt->uid) return DRX_EINVAL;
  if (bt->keep && !bt->keep_off) return DRX_EINVAL;
  if (bt->B < 1 || bt->q < 0.f || bt->q >= 1.f) return DRX_EINVAL;
  return DRX_OK;
}

// Bytes the dense step's scratch layout takes for a batch of B rows (drx_cdae_dense.hip: dense_layout), before the closing
// alignment drx_cdae_scratch_bytes adds for both modes.
size_t dense_layout_bytes(const DrxCdaeParams &P, int B);

}  // namespace drx
