"""Device-side state of one GRU4Rec model (Hidasi, Karatzoglou, Baltrunas, Tikk 2016) and the calls into libdrx.so (drx_gru_*;
include/drx.h "GRU4Rec").

Score x(S, i) = h_L(S) . Q[i] + b[i] — DRX_REC_BIAS of the fused scorer at rows of ldh floats, with Q as the table, b as the bias and
h after the cell has run over the user's basket (drx_gru_query_rows) as the query row: recommend / rank_items / rank_lists /
pair_scores are RowsRecommender's.  There is no user table.  One training step = drx_gru_step on B windows (uid [B], before [B, L],
after [B, 1 + r]) as ListSampler.sample_device returns them; uid plays no part in it.  torch is the allocator / stream provider only.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .engine_dense import DenseEngine
from .engine_rows import _round_up

MAX_FACTORS = 64
MAX_HIDDEN = 64
MAX_L = 8
MAX_NEG_RATIO = 16


def check_shape(factors, hidden, L, who='GRU4Rec engine'):
    """the domain of csrc/drx_gru.hip, refused by name"""
    integer = lambda x: isinstance(x, (int, np.integer)) and not isinstance(x, bool)
    if not (integer(factors) and 1 <= factors <= MAX_FACTORS):
        raise _lib.DrxError(f'{who}: factors must be an integer in 1..{MAX_FACTORS}, got factors={factors!r}')
    if not (integer(hidden) and 1 <= hidden <= MAX_HIDDEN):
        raise _lib.DrxError(f'{who}: hidden must be an integer in 1..{MAX_HIDDEN}, got hidden={hidden!r}')
    if not (integer(L) and 1 <= L <= MAX_L):
        raise _lib.DrxError(f'{who}: L must be an integer in 1..{MAX_L}, got L={L!r}')
    return int(factors), int(hidden), int(L)


class GruEngine(DenseEngine):
    EPILOGUE = _lib.DRX_REC_BIAS
    ALPHA_OF = (0, 1, 2)                   # E, the small weights, Q with b: a handle each

    def __init__(self, n_users, n_items, factors=64, hidden=64, L=5, device='cuda:0'):
        self._require_gpu()
        self.K, self.H, self.L = check_shape(factors, hidden, L)
        z = self._open(n_users, n_items, device)
        K, H = self.K, self.H
        self.ldk, self.ldh = _round_up(K, 4), _round_up(H, 4)
        # the flat array of small weights: Wx [K, 3 H], Wh [H, 3 H], bx [3 H], bhn [H], no padding (include/drx.h DrxGruDims)
        off_wh, off_bx = 3 * K * H, 3 * (K + H) * H
        self.dims = _lib.GruDims(n_items=self.n_items, k=K, h=H, ldk=self.ldk, ldh=self.ldh, off_wx=0, off_wh=off_wh, off_bx=off_bx,
                                 off_bhn=off_bx + 3 * H, n_small=off_bx + 4 * H)
        self.slices = {'Wx': (0, (K, 3 * H)), 'Wh': (off_wh, (H, 3 * H)), 'bx': (off_bx, (3 * H,)), 'bhn': (off_bx + 3 * H, (H,))}
        self.n_small = int(self.dims.n_small)
        self.E = torch.zeros(self.n_items, self.ldk, **z)
        self.sw = torch.zeros(self.n_small, **z)
        self.Q = torch.zeros(self.n_items, self.ldh, **z)
        self.b = torch.zeros(self.n_items, **z)
        self.baskets = torch.full((self.n_users, self.L), -1, dtype=torch.int32, device=self.device)
        self._init_step_state()
        # what GRU4Rec._pre_fit registers, in this order: one apply_gradients per handle and step (the item side with its biases)
        self.input_emb = self._handle('input_embeddings', 'E')
        self.small = self._handle('small_weights', *self.slices)
        self.item_emb = self._handle('item_factors', 'Q', 'b')

    def tensors(self):
        return {'E': self.E, 'sw': self.sw, 'Q': self.Q, 'b': self.b}

    def _small(self, name):
        off, shape = self.slices[name]
        return self.sw[off:off + int(np.prod(shape))].view(*shape)

    def views(self):
        """{'E': [n_items, K], 'Wx': [K, 3 H], 'Wh': [H, 3 H], 'bx': [3 H], 'bhn': [H], 'Q': [n_items, H], 'b': [n_items]}; the gate
        columns are z | r | n"""
        v = {'E': self.E[:, :self.K]}
        v.update({name: self._small(name) for name in self.slices})
        v.update({'Q': self.Q[:, :self.H], 'b': self.b})
        return v

    def set_baskets(self, baskets):
        """baskets [n_users, L] int: the items the cell runs over at serving, in sequence order; -1 = an absent position (no step)"""
        a = np.ascontiguousarray(baskets, dtype=np.int32)
        if a.shape != (self.n_users, self.L) or a.max(initial=-1) >= self.n_items or a.min(initial=0) < -1:
            raise _lib.DrxError(f'GRU4Rec engine: baskets must be [{self.n_users}, {self.L}] item ids in -1..{self.n_items - 1}')
        self.baskets.copy_(torch.as_tensor(a))

    # ---- the step (include/drx.h drx_gru_step) ---------------------------------------------------------------------------------------
    def step(self, step_idx, uid, before, after, want_loss=False, applies=None):
        """One step on B windows (arrays or device tensors): uid [B] (the sampler's; not used: the sequence is the session),
        before [B, L], after [B, 1 + r] (the target first).  applies = (n, j_input, j_small, j_item): the number of apply_gradients
        calls per step and the positions of the three handles among them (the registration order); default (3, 0, 1, 2).  Returns
        the mean softplus(-(x(S, i) - x(S, j))) of the batch before the update when want_loss, else None."""
        applies = tuple(applies) if applies is not None else (3, 0, 1, 2)
        before, after = self._dev_i32(before), self._dev_i32(after)
        assert before.dim() == 2 and after.dim() == 2 and before.shape[0] == after.shape[0], 'step takes B windows'
        assert before.shape[1] == self.L, f'a window holds L = {self.L} previous items'
        B, r = int(before.shape[0]), int(after.shape[1]) - 1
        L_ = lib()
        scratch = self._step_scratch(int(L_.drx_gru_step_scratch_bytes(C.byref(self.dims), B, self.L, r)),
                                     lambda: f'drx_gru_step: a batch of {B} windows of {self.L} + 1 + {r} items is outside its domain '
                                     f'(1..{MAX_NEG_RATIO} negatives per window)')
        alphas, slots, loss = self._step_args(step_idx, applies, want_loss)
        check(L_.drx_gru_step(C.byref(self.dims), ptr(self.E), ptr(self.sw), ptr(self.Q), ptr(self.b), *slots, ptr(before), ptr(after), B,
                              self.L, r, C.byref(self._rule()), alphas, float(self.reg), loss, ptr(scratch), scratch.numel(),
                              stream_ptr(self.device)), 'drx_gru_step')
        return self._read_loss(want_loss)

    # what the four calls of RowsRecommender and its score_matrix score against: Q and b themselves, and h of the users' baskets
    def rank_ld(self):
        return self.ldh

    def _score_table(self, items=None):
        return self.Q, self.b

    def _query_rows(self, uid):
        """[len(uid), ldh] rows h(basket of u) (drx_gru_query_rows): they depend on the user alone"""
        n = int(uid.numel())
        out = torch.empty(n, self.ldh, dtype=torch.float32, device=self.device)
        if n:
            check(lib().drx_gru_query_rows(ptr(self.E), ptr(self.sw), C.byref(self.dims), ptr(self.baskets), self.L, ptr(uid), n, ptr(out),
                                           stream_ptr(self.device)), 'drx_gru_query_rows')
        return out
