"""Device-side state of one BPR-MF model (Rendle et al. 2009) and the calls into libdrx.so (drx_bpr_*; include/drx.h "BPR-MF",
DESIGN.md section 3.7).

Score x(u, i) = P[u] . Q[i] + bq[i] — DRX_REC_BIAS of the fused scorer, with Q as the table, bq as the bias and rows of P as the query
rows: recommend / rank_items / rank_lists / pair_scores are RowsRecommender's.  One training step = drx_bpr_step on T (user, positive,
negative) triples, drawn on the device by drx_bpr_sample or given.  torch is the allocator / stream provider only.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .engine_dense import DenseEngine
from .engine_rows import _round_up

MAX_FACTORS = 256


class BprEngine(DenseEngine):
    EPILOGUE = _lib.DRX_REC_BIAS
    ALPHA_OF = (0, 1, 1)                   # P with the user handle; Q and bq with the item handle

    def __init__(self, n_users, n_items, factors=64, device='cuda:0'):
        self._require_gpu()
        if not (isinstance(factors, (int, np.integer)) and 1 <= factors <= MAX_FACTORS):
            raise _lib.DrxError(f'BPR engine: factors must be an integer in 1..{MAX_FACTORS} (a row is one float4 per lane of a wavefront), '
                                f'got factors={factors!r}')
        z = self._open(n_users, n_items, device)
        self.K = int(factors)
        self.ld = _round_up(self.K, 4)
        self.P = torch.zeros(self.n_users, self.ld, **z)
        self.Q = torch.zeros(self.n_items, self.ld, **z)
        self.bq = torch.zeros(self.n_items, **z)
        self._init_step_state()
        # what BPR._pre_fit registers, in this order: one apply_gradients per handle and step (the item factors with their biases)
        self.user_emb = self._handle('user_factors', 'P')
        self.item_emb = self._handle('item_factors', 'Q', 'bq')

    def tensors(self):
        return {'P': self.P, 'Q': self.Q, 'bq': self.bq}

    def views(self):
        """{'P': [n_users, K], 'Q': [n_items, K], 'bq': [n_items]}"""
        return {'P': self.P[:, :self.K], 'Q': self.Q[:, :self.K], 'bq': self.bq}

    # ---- the triple stream (include/drx.h drx_bpr_sample) --------------------------------------------------------------------------
    def set_sampler_frame(self, positives, recorded, eligible):
        """positives / recorded: DenseEngine._upload_frame's; eligible: the users with a positive and fewer than n_items recorded items."""
        eligible = np.ascontiguousarray(eligible, dtype=np.int32)
        if len(eligible) == 0:
            raise _lib.DrxError('BPR engine: no eligible user (one with a positive and an item it has not recorded)')
        self._upload_frame(positives, recorded)
        self._eligible = torch.as_tensor(eligible).to(self.device)

    def sample(self, T, neg_ratio, seed):
        """(uid, pos, neg) int32 [T] device tensors: the T triples of `seed` (drx_bpr_sample)"""
        T = int(T)
        out = torch.empty(3, max(T, 1), dtype=torch.int32, device=self.device)
        check(lib().drx_bpr_sample(C.byref(self._H), C.byref(self._R) if self._R is not None else None, ptr(self._eligible),
                                   int(self._eligible.numel()), self.n_items, T, int(neg_ratio), int(seed) & ((1 << 64) - 1), ptr(out[0]),
                                   ptr(out[1]), ptr(out[2]), stream_ptr(self.device)), 'drx_bpr_sample')
        return out[0], out[1], out[2]

    # ---- the step (include/drx.h drx_bpr_step) -------------------------------------------------------------------------------------
    def step(self, step_idx, uid, pos, neg, want_loss=False, applies=None):
        """One step on the triples (arrays or device tensors).  applies = (n, j_user, j_item): the number of apply_gradients calls per
        step and the positions of the user and the item factors among them (the registration order); default (2, 0, 1).  Returns the
        mean softplus(-(x(u, i) - x(u, j))) of the batch before the update when want_loss, else None."""
        applies = tuple(applies) if applies is not None else (2, 0, 1)
        uid, pos, neg = self._dev_i32(uid), self._dev_i32(pos), self._dev_i32(neg)
        T = int(uid.numel())
        assert pos.numel() == T and neg.numel() == T, 'step takes parallel users, positives and negatives'
        L_ = lib()
        scratch = self._step_scratch(int(L_.drx_bpr_step_scratch_bytes(T, self.ld, self.n_users, self.n_items)),
                                     lambda: f'drx_bpr_step: a batch of {T} triples at rows of {self.ld} floats is outside its domain')
        alphas, slots, loss = self._step_args(step_idx, applies, want_loss)
        check(L_.drx_bpr_step(ptr(self.P), ptr(self.Q), ptr(self.bq), *slots, self.ld, self.n_users, self.n_items, ptr(uid), ptr(pos),
                              ptr(neg), T, C.byref(self._rule()), alphas, float(self.reg), loss, ptr(scratch), scratch.numel(),
                              stream_ptr(self.device)), 'drx_bpr_step')
        return self._read_loss(want_loss)

    # what the four calls of RowsRecommender and its score_matrix score against: the item factors and biases themselves, and rows of P
    def rank_ld(self):
        return self.ld

    def _score_table(self, items=None):
        return self.Q, self.bq

    def _query_rows(self, uid):
        return self._gather_rows(self.P, uid)
