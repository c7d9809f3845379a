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
from ._lib import History, check, lib, ptr, stream_ptr
from .engine_dense import DenseEngine
from .engine_rows import _round_up

MAX_FACTORS = 256


class BprEngine(DenseEngine):
    EPILOGUE = _lib.DRX_REC_BIAS

    def __init__(self, n_users, n_items, factors=64, device='cuda:0'):
        if not torch.cuda.is_available():
            raise _lib.DrxError('drecpy_amd needs a ROCm GPU (MI355X); there is no CPU fallback.')
        if not (isinstance(factors, (int, np.integer)) and 1 <= factors <= MAX_FACTORS):
            raise _lib.DrxError(f'BPR engine: factors must be an integer in 1..{MAX_FACTORS} (a row is one float4 per lane of a wavefront), '
                                f'got factors={factors!r}')
        lib()
        self.device = torch.device(device)
        self.n_users, self.n_items, self.K = int(n_users), int(n_items), int(factors)
        self.ld = _round_up(self.K, 4)
        z = dict(dtype=torch.float32, device=self.device)
        self.P = torch.zeros(self.n_users, self.ld, **z)
        self.Q = torch.zeros(self.n_items, self.ld, **z)
        self.bq = torch.zeros(self.n_items, **z)
        self._init_optimizer_state()
        self.lr, self.reg = 1e-3, 1e-3
        self._scratch = None
        self._loss = torch.zeros(1, dtype=torch.float64, device=self.device)
        from .Recommender.trainables import TrainableModel
        # what BPR._pre_fit registers, in this order: one apply_gradients per handle and step (the item factors with their biases)
        self.user_emb = TrainableModel('user_factors', lambda: [self.P[:, :self.K]])
        self.item_emb = TrainableModel('item_factors', lambda: [self.Q[:, :self.K], self.bq])

    def tensors(self):
        return {'P': self.P, 'Q': self.Q, 'bq': self.bq}

    def set_params(self, p):
        """p: {'P': [n_users, K], 'Q': [n_items, K], 'bq': [n_items]} (unpadded); the padding columns are zeroed"""
        t = lambda a, shape: torch.as_tensor(np.asarray(a, dtype=np.float32).reshape(shape)).to(self.device)
        for x in self.tensors().values():
            x.zero_()
        self.P[:, :self.K] = t(p['P'], (self.n_users, self.K))
        self.Q[:, :self.K] = t(p['Q'], (self.n_items, self.K))
        self.bq.copy_(t(p['bq'], (self.n_items,)))

    def get_params(self):
        c = lambda x: x.detach().cpu().numpy().copy()
        return {'P': c(self.P[:, :self.K]), 'Q': c(self.Q[:, :self.K]), 'bq': c(self.bq)}

    # ---- the triple stream (include/drx.h drx_bpr_sample) --------------------------------------------------------------------------
    def set_sampler_frame(self, positives, recorded, eligible):
        """positives = (indptr, indices) of the pairs with interaction >= threshold; recorded = (indptr, indices) of every pair of the
        frame, or None where all of them are positives; eligible: the users with a positive and fewer than n_items recorded items."""
        d = self.device
        up = lambda csr: (torch.as_tensor(np.asarray(csr[0], np.int64)).to(d),
                          torch.as_tensor(np.asarray(csr[1], np.int32) if len(csr[1]) else np.zeros(1, np.int32)).to(d))
        eligible = np.ascontiguousarray(eligible, dtype=np.int32)
        if len(eligible) == 0:
            raise _lib.DrxError('BPR engine: no eligible user (one with a positive and an item it has not recorded)')
        self._pos = up(positives)
        self._rec = up(recorded) if recorded is not None else None
        self._eligible = torch.as_tensor(eligible).to(d)
        self._H = History(ptr(self._pos[0]), ptr(self._pos[1]))
        self._R = History(ptr(self._rec[0]), ptr(self._rec[1])) if self._rec is not None else None

    def sample(self, T, neg_ratio, seed):
        """(uid, pos, neg) int32 [T] device tensors: the T triples of `seed` (drx_bpr_sample)"""
        T = int(T)
        out = torch.empty(3, max(T, 1), dtype=torch.int32, device=self.device)
        check(lib().drx_bpr_sample(C.byref(self._H), C.byref(self._R) if self._R is not None else None, ptr(self._eligible),
                                   int(self._eligible.numel()), self.n_items, T, int(neg_ratio), int(seed) & ((1 << 64) - 1), ptr(out[0]),
                                   ptr(out[1]), ptr(out[2]), stream_ptr(self.device)), 'drx_bpr_sample')
        return out[0], out[1], out[2]

    # ---- the step (include/drx.h drx_bpr_step) -------------------------------------------------------------------------------------
    def _step_sizes(self, step_idx, applies):
        """(alpha_P, alpha_Q, alpha_bq): Keras Adam's lr_t of each apply's counter; the learning rate under every other rule"""
        n, j_user, j_item = applies
        if self.opt_kind != 'adam':
            return self.lr, self.lr, self.lr
        a = [self.adam_alpha(self.lr, n * step_idx + j + 1, self.beta1, self.beta2) for j in (j_user, j_item)]
        return a[0], a[1], a[1]

    def step(self, step_idx, uid, pos, neg, want_loss=False, applies=None):
        """One step on the triples (arrays or device tensors).  applies = (n, j_user, j_item): the number of apply_gradients calls per
        step and the positions of the user and the item factors among them (the registration order); default (2, 0, 1).  Returns the
        mean softplus(-(x(u, i) - x(u, j))) of the batch before the update when want_loss, else None."""
        applies = tuple(applies) if applies is not None else (2, 0, 1)
        uid, pos, neg = self._dev_i32(uid), self._dev_i32(pos), self._dev_i32(neg)
        T = int(uid.numel())
        assert pos.numel() == T and neg.numel() == T, 'step takes parallel users, positives and negatives'
        L_ = lib()
        need = int(L_.drx_bpr_step_scratch_bytes(T, self.ld, self.n_users, self.n_items))
        if need == 0:
            raise _lib.DrxError(f'drx_bpr_step: a batch of {T} triples at rows of {self.ld} floats is outside its domain')
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = None
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        alphas = (C.c_float * 3)(*self._step_sizes(step_idx, applies))
        slots = [s for name in ('P', 'Q', 'bq') for s in self.state[name]]
        check(L_.drx_bpr_step(ptr(self.P), ptr(self.Q), ptr(self.bq), *[ptr(s) for s in slots], self.ld, self.n_users, self.n_items, ptr(uid),
                              ptr(pos), ptr(neg), T, C.byref(self._rule()), alphas, float(self.reg), ptr(self._loss) if want_loss else None,
                              ptr(self._scratch), self._scratch.numel(), stream_ptr(self.device)), 'drx_bpr_step')
        return float(self._loss.cpu().numpy()[0]) if want_loss else None

    # ---- scores ----------------------------------------------------------------------------------------------------------------------
    def _rows(self, table, ids):
        """[len(ids), ld] rows of `table` by device id (drx_bpr_gather_rows)"""
        n = int(ids.numel())
        out = torch.empty(n, self.ld, dtype=torch.float32, device=self.device)
        if n:
            check(lib().drx_bpr_gather_rows(ptr(table), self.ld, ptr(ids), n, ptr(out), stream_ptr(self.device)), 'drx_bpr_gather_rows')
        return out

    def score_matrix(self, uids):
        """[len(uids), n_items] scores of the given users against all items (drx_rows_dot): the score-matrix route of _rank_rows"""
        uid = self._dev_i32(uids).reshape(-1)
        B = int(uid.numel())
        out = torch.empty(B, self.n_items, dtype=torch.float32, device=self.device)
        if B:
            q = self._rows(self.P, uid)
            check(lib().drx_rows_dot(ptr(q), B, ptr(self.Q), self.n_items, self.ld, ptr(self.bq), ptr(out), stream_ptr(self.device)),
                  'drx_rows_dot')
        return out

    # what the four calls of RowsRecommender score against: the item factors and biases themselves, and rows of P
    def rank_ld(self):
        return self.ld

    def _score_table(self, items=None):
        return self.Q, self.bq

    def _query_rows(self, uid):
        return self._rows(self.P, uid)
