"""Device-side state of one ALS / WMF model (Hu, Koren, Volinsky 2008) and the calls into libdrx.so (drx_als_*; include/drx.h
"ALS / WMF").

Score x(u, i) = X[u] . Y[i] — DRX_REC_BIAS of the fused scorer with Y as the table, a zero vector as the bias and rows of X as the query
rows: recommend / rank_items / rank_lists / pair_scores are RowsRecommender's.  One sweep = gram(Y), the user half, gram(X), the item
half (drx_als_gram, drx_als_solve_rows), and drx_als_loss when asked.  There is no sampler, no learning rate and no optimizer state.
torch is the allocator / stream provider only.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .engine_rows import RowsRecommender, _round_up

MAX_FACTORS = 128


class AlsEngine(RowsRecommender):
    EPILOGUE = _lib.DRX_REC_BIAS

    def __init__(self, n_users, n_items, factors=64, device='cuda:0'):
        self._require_gpu()
        if not (isinstance(factors, (int, np.integer)) and 1 <= factors <= MAX_FACTORS):
            raise _lib.DrxError(f'ALS engine: factors must be an integer in 1..{MAX_FACTORS} (a row\'s K x K system lives in one '
                                f'workgroup\'s LDS), got factors={factors!r}')
        z = self._open(n_users, n_items, device)
        self.K = int(factors)
        self.ld = _round_up(self.K, 4)
        self.X = torch.zeros(self.n_users, self.ld, **z)
        self.Y = torch.zeros(self.n_items, self.ld, **z)
        self.bias = torch.zeros(self.n_items, **z)                # stays zero: the scorer's epilogue adds it
        self.Gx = torch.zeros(self.ld, self.ld, **z)
        self.Gy = torch.zeros(self.ld, self.ld, **z)
        self.reg = 0.1
        self._fail = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._loss = torch.zeros(1, dtype=torch.float64, device=self.device)
        self._frame = None
        self._als_scratch = torch.empty(self.scratch_need(self.n_users, self.n_items, self.ld), dtype=torch.uint8, device=self.device)
        self.user_emb = self._handle('user_factors', 'X')
        self.item_emb = self._handle('item_factors', 'Y')

    @staticmethod
    def scratch_need(n_users, n_items, ld):
        """bytes that hold the scratch of every call of a sweep: the Gram of EACH table (its companion is not monotone in the row
        count: the strips grow past 16 384 rows), both halves and the loss"""
        L_ = lib()
        return max(int(L_.drx_als_gram_scratch_bytes(n_users, ld)), int(L_.drx_als_gram_scratch_bytes(n_items, ld)),
                   int(L_.drx_als_solve_rows_scratch_bytes(n_users, n_items, ld)), int(L_.drx_als_solve_rows_scratch_bytes(n_items, n_users, ld)),
                   int(L_.drx_als_loss_scratch_bytes(n_users, ld)))

    def tensors(self):
        return {'X': self.X, 'Y': self.Y}

    def views(self):
        """{'X': [n_users, K], 'Y': [n_items, K]}"""
        return {'X': self.X[:, :self.K], 'Y': self.Y[:, :self.K]}

    def snapshot(self):
        return {'p': {n: t.clone() for n, t in self.tensors().items()}}

    def restore(self, snap, with_optimizer=False):
        for n, t in self.tensors().items():
            t.copy_(snap['p'][n])

    # ---- the frame ---------------------------------------------------------------------------------------------------------------------
    def set_frame(self, csr, csr_t, weights, weights_t):
        """csr = (indptr, indices) of the positives, user-major, and csr_t item-major; weights / weights_t: w = c - 1 >= 0 per entry of
        each.  The rows of each orientation are ordered by descending degree once: the CSR never changes during a fit."""
        d = self.device
        halves = []
        for (indptr, indices), w, n_rows in ((csr, weights, self.n_users), (csr_t, weights_t, self.n_items)):
            indptr = np.ascontiguousarray(indptr, dtype=np.int64)
            assert len(indptr) == n_rows + 1 and len(indices) == len(w) == indptr[-1], 'a CSR of the wrong shape'
            w = np.ascontiguousarray(w, dtype=np.float32)
            if len(w) and not (w >= 0).all():
                raise _lib.DrxError('ALS engine: a negative weight (confidence below 1)')
            order = np.argsort(-np.diff(indptr), kind='stable').astype(np.int32)
            pad = lambda a, t: torch.as_tensor(a if len(a) else np.zeros(1, t)).to(d)
            halves.append((torch.as_tensor(indptr).to(d), pad(np.ascontiguousarray(indices, dtype=np.int32), np.int32), pad(w, np.float32),
                           torch.as_tensor(order).to(d)))
        self._frame = halves

    def gram(self, table, out):
        """out [ld, ld] = table^T table (drx_als_gram)"""
        check(lib().drx_als_gram(ptr(table), int(table.shape[0]), self.ld, ptr(out), ptr(self._als_scratch), self._als_scratch.numel(),
                                 stream_ptr(self.device)), 'drx_als_gram')
        return out

    def solve_half(self, half, ordered=True):
        """half 0: X from Y over the user-major CSR; half 1: Y from X over the item-major one.  Raises DrxError when a factorisation
        failed (those rows are zero)."""
        out, other, G = (self.X, self.Y, self.Gy) if half == 0 else (self.Y, self.X, self.Gx)
        indptr, indices, w, order = self._frame[half]
        self._fail.zero_()
        check(lib().drx_als_solve_rows(ptr(out), ptr(other), ptr(G), ptr(indptr), ptr(indices), ptr(w), ptr(order) if ordered else None,
                                       int(out.shape[0]), int(other.shape[0]), self.ld, float(self.reg), ptr(self._fail),
                                       ptr(self._als_scratch), self._als_scratch.numel(), stream_ptr(self.device)), 'drx_als_solve_rows')
        failed = int(self._fail.cpu().numpy()[0])
        if failed:
            raise _lib.DrxError(f'drx_als_solve_rows: the {("user", "item")[half]} half met {failed} row(s) whose system is not positive '
                                f'definite in fp32 (lambda = {self.reg}); they were set to zero')

    def loss(self):
        """L of the current X, Y; Gx must be X^T X (the item half's Gram); Y^T Y is computed here"""
        self.gram(self.Y, self.Gy)
        indptr, indices, w, _ = self._frame[0]
        check(lib().drx_als_loss(ptr(self.X), ptr(self.Y), ptr(self.Gx), ptr(self.Gy), ptr(indptr), ptr(indices), ptr(w), self.n_users,
                                 self.n_items, self.ld, float(self.reg), ptr(self._loss), ptr(self._als_scratch),
                                 self._als_scratch.numel(), stream_ptr(self.device)), 'drx_als_loss')
        return float(self._loss.cpu().numpy()[0])

    def sweep(self, want_loss=False):
        """gram(Y), the user half, gram(X), the item half; the loss after the item half when asked (one more gram, of the new Y)"""
        assert self._frame is not None, 'set_frame first'
        self.gram(self.Y, self.Gy)
        self.solve_half(0)
        self.gram(self.X, self.Gx)
        self.solve_half(1)
        return self.loss() if want_loss else None

    # ---- scores ----------------------------------------------------------------------------------------------------------------------
    def rank_ld(self):
        return self.ld

    def _score_table(self, items=None):
        return self.Y, self.bias

    def _query_rows(self, uid):
        return self._gather_rows(self.X, uid)
