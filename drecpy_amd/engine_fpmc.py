"""Device-side state of one FPMC model (Rendle, Freudenthaler, Schmidt-Thieme 2010) and the calls into libdrx.so (drx_fpmc_*;
include/drx.h "FPMC").

Score x(u, S, i) = P[u] . Q[i] + mean_{l in S} M[l] . N[i] + b[i] = c(u, S) . QN[i] + b[i] — DRX_REC_BIAS of the fused scorer at rows of
2 ld floats, with QN = [Q | N] as the table, b as the bias and c = [P[u] | mean M] (drx_fpmc_query_rows over the user's basket) as the
query rows: recommend / rank_items / rank_lists / pair_scores are RowsRecommender's.  One training step = drx_fpmc_step on B windows
(uid [B], before [B, L], after [B, 1 + r]) as ListSampler.sample_device returns them.  torch is the allocator / stream provider only.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .engine_dense import DenseEngine
from .engine_rows import _round_up

MAX_FACTORS = 128
MAX_L = 8
MAX_NEG_RATIO = 16


class FpmcEngine(DenseEngine):
    EPILOGUE = _lib.DRX_REC_BIAS
    ALPHA_OF = (0, 1, 2, 2)                # P, M, then QN and b with the item handle

    def __init__(self, n_users, n_items, factors=64, L=1, device='cuda:0'):
        self._require_gpu()
        if not (isinstance(factors, (int, np.integer)) and 1 <= factors <= MAX_FACTORS):
            raise _lib.DrxError(f'FPMC engine: factors must be an integer in 1..{MAX_FACTORS} (a row [Q | N] of the fused scorer holds at most '
                                f'256 floats), got factors={factors!r}')
        if not (isinstance(L, (int, np.integer)) and 1 <= L <= MAX_L):
            raise _lib.DrxError(f'FPMC engine: L must be an integer in 1..{MAX_L}, got L={L!r}')
        z = self._open(n_users, n_items, device)
        self.K, self.L = int(factors), int(L)
        self.ld = _round_up(self.K, 4)
        self.P = torch.zeros(self.n_users, self.ld, **z)
        self.M = torch.zeros(self.n_items, self.ld, **z)
        self.QN = torch.zeros(self.n_items, 2 * self.ld, **z)
        self.b = torch.zeros(self.n_items, **z)
        self.baskets = torch.full((self.n_users, self.L), -1, dtype=torch.int32, device=self.device)
        self._init_step_state()
        # what FPMC._pre_fit registers, in this order: one apply_gradients per handle and step (the item side with its biases)
        self.user_emb = self._handle('user_factors', 'P')
        self.trans_emb = self._handle('transition_factors', 'M')
        self.item_emb = self._handle('item_factors', 'Q', 'N', 'b')

    def tensors(self):
        return {'P': self.P, 'M': self.M, 'QN': self.QN, 'b': self.b}

    def views(self):
        """{'P': [n_users, K], 'Q', 'M', 'N': [n_items, K], 'b': [n_items]}: Q and N are the two halves of a row of QN"""
        K, ld = self.K, self.ld
        return {'P': self.P[:, :K], 'Q': self.QN[:, :K], 'M': self.M[:, :K], 'N': self.QN[:, ld:ld + K], 'b': self.b}

    def set_baskets(self, baskets):
        """baskets [n_users, L] int: the items the transition term of serving averages over, in sequence order; -1 = an absent position"""
        a = np.ascontiguousarray(baskets, dtype=np.int32)
        if a.shape != (self.n_users, self.L) or a.max(initial=-1) >= self.n_items or a.min(initial=0) < -1:
            raise _lib.DrxError(f'FPMC engine: baskets must be [{self.n_users}, {self.L}] item ids in -1..{self.n_items - 1}')
        self.baskets.copy_(torch.as_tensor(a))

    # ---- the step (include/drx.h drx_fpmc_step) ------------------------------------------------------------------------------------
    def step(self, step_idx, uid, before, after, want_loss=False, applies=None):
        """One step on B windows (arrays or device tensors): uid [B], before [B, L], after [B, 1 + r] (the target first).
        applies = (n, j_user, j_transition, j_item): the number of apply_gradients calls per step and the positions of the three
        handles among them (the registration order); default (3, 0, 1, 2).  Returns the mean softplus(-(x(u, S, i) - x(u, S, j))) of the
        batch before the update when want_loss, else None."""
        applies = tuple(applies) if applies is not None else (3, 0, 1, 2)
        uid, before, after = self._dev_i32(uid).reshape(-1), self._dev_i32(before), self._dev_i32(after)
        B = int(uid.numel())
        assert before.dim() == 2 and after.dim() == 2 and before.shape[0] == B and after.shape[0] == B, 'step takes B windows'
        assert before.shape[1] == self.L, f'a window holds L = {self.L} previous items'
        r = int(after.shape[1]) - 1
        L_ = lib()
        scratch = self._step_scratch(int(L_.drx_fpmc_step_scratch_bytes(B, self.L, r, self.ld, self.n_users, self.n_items)),
                                     lambda: f'drx_fpmc_step: a batch of {B} windows of {self.L} + 1 + {r} items at {self.ld} factors is outside its '
                                     f'domain (1..{MAX_NEG_RATIO} negatives per window)')
        alphas, slots, loss = self._step_args(step_idx, applies, want_loss)
        check(L_.drx_fpmc_step(ptr(self.P), ptr(self.M), ptr(self.QN), ptr(self.b), *slots, self.ld, self.n_users, self.n_items, ptr(uid),
                               ptr(before), ptr(after), B, self.L, r, C.byref(self._rule()), alphas, float(self.reg), loss, ptr(scratch),
                               scratch.numel(), stream_ptr(self.device)), 'drx_fpmc_step')
        return self._read_loss(want_loss)

    # what the four calls of RowsRecommender and its score_matrix (at 2 ld) score against: [Q | N] and b themselves, and the context
    # rows of the users' baskets
    def rank_ld(self):
        return 2 * self.ld

    def _score_table(self, items=None):
        return self.QN, self.b

    def _query_rows(self, uid):
        """[len(uid), 2 ld] rows [P[u] | mean of M over the basket of u] (drx_fpmc_query_rows): they depend on the user alone"""
        n = int(uid.numel())
        out = torch.empty(n, 2 * self.ld, dtype=torch.float32, device=self.device)
        if n:
            check(lib().drx_fpmc_query_rows(ptr(self.P), ptr(self.M), self.ld, ptr(self.baskets), self.L, ptr(uid), n, ptr(out),
                                            stream_ptr(self.device)), 'drx_fpmc_query_rows')
        return out
