"""Device-side state of one SASRec model (Kang & McAuley 2018) and the calls into libdrx.so (drx_sas_*; include/drx.h "SASRec",
DESIGN.md section 3.12).

Score x(S, i) = h(S) . Q[i] + b[i] — DRX_REC_BIAS of the fused scorer at rows of ldh floats, with Q as the table, b as the bias and h of
the user's basket (drx_sas_query_rows) as the query row: recommend / rank_items / rank_lists / pair_scores are RowsRecommender's.  There
is no user table.  One training step = drx_sas_step on B windows (uid [B], before [B, L], after [B, 1 + r]) as
ListSampler.sample_device returns them; uid plays no part in it.  torch is the allocator / stream provider only.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .engine_dense import DenseEngine
from .engine_rows import _round_up

MAX_HIDDEN = 64
MAX_L = 16
MAX_BLOCKS = 2
MAX_NEG_RATIO = 16
MATRICES = ('Wq', 'Wk', 'Wv', 'W1', 'W2')
VECTORS = ('b1', 'b2', 'ln1_g', 'ln1_b', 'ln2_g', 'ln2_b')


def check_shape(hidden, L, blocks, who='SASRec engine'):
    """the domain of csrc/drx_sas.hip, refused by name"""
    integer = lambda x: isinstance(x, (int, np.integer)) and not isinstance(x, bool)
    if not (integer(hidden) and 1 <= hidden <= MAX_HIDDEN):
        raise _lib.DrxError(f'{who}: hidden must be an integer in 1..{MAX_HIDDEN}, got hidden={hidden!r}')
    if not (integer(L) and 1 <= L <= MAX_L):
        raise _lib.DrxError(f'{who}: L must be an integer in 1..{MAX_L}, got L={L!r}')
    if not (integer(blocks) and 1 <= blocks <= MAX_BLOCKS):
        raise _lib.DrxError(f'{who}: blocks must be an integer in 1..{MAX_BLOCKS}, got blocks={blocks!r}')
    return int(hidden), int(L), int(blocks)


class SasEngine(DenseEngine):
    EPILOGUE = _lib.DRX_REC_BIAS
    ALPHA_OF = (0, 1, 2)                   # E, the small weights, Q with b: a handle each

    def __init__(self, n_users, n_items, hidden=64, L=10, blocks=2, device='cuda:0'):
        self._require_gpu()
        self.H, self.L, self.blocks = check_shape(hidden, L, blocks)
        z = self._open(n_users, n_items, device)
        H, nb = self.H, self.blocks
        self.ldh = _round_up(H, 4)
        # the flat array of small weights, no padding, the regularised entries first (include/drx.h DrxSasDims):
        # Pos [L, H] | per block Wq Wk Wv W1 W2 [H, H] || per block b1 b2 ln1_g ln1_b ln2_g ln2_b [H] | lnf_g lnf_b [H]
        off_blk = self.L * H
        off_vec = off_blk + 5 * H * H * nb
        off_lnf = off_vec + len(VECTORS) * H * nb
        self.dims = _lib.SasDims(n_items=self.n_items, h=H, ldh=self.ldh, L=self.L, blocks=nb, off_pos=0, off_blk=off_blk, off_vec=off_vec,
                                 off_lnf=off_lnf, n_small=off_lnf + 2 * H)
        self.slices = {'Pos': (0, (self.L, H))}
        self.slices.update({f'{m}{b}': (off_blk + (5 * b + j) * H * H, (H, H)) for b in range(nb) for j, m in enumerate(MATRICES)})
        self.slices.update({f'{v}{b}': (off_vec + (len(VECTORS) * b + j) * H, (H,)) for b in range(nb) for j, v in enumerate(VECTORS)})
        self.slices.update({'lnf_g': (off_lnf, (H,)), 'lnf_b': (off_lnf + H, (H,))})
        self.n_small = int(self.dims.n_small)
        self.E = torch.zeros(self.n_items, self.ldh, **z)
        self.sw = torch.zeros(self.n_small, **z)
        self.Q = torch.zeros(self.n_items, self.ldh, **z)
        self.b = torch.zeros(self.n_items, **z)
        self.baskets = torch.full((self.n_users, self.L), -1, dtype=torch.int32, device=self.device)
        self._init_step_state()
        # what SASRec._pre_fit registers, in this order: one apply_gradients per handle and step (the item side with its biases)
        self.input_emb = self._handle('input_embeddings', 'E')
        self.small = self._handle('small_weights', *self.slices)
        self.item_emb = self._handle('item_factors', 'Q', 'b')

    def tensors(self):
        return {'E': self.E, 'sw': self.sw, 'Q': self.Q, 'b': self.b}

    def _small(self, name):
        off, shape = self.slices[name]
        return self.sw[off:off + int(np.prod(shape))].view(*shape)

    def views(self):
        """{'E': [n_items, H], 'Pos': [L, H], 'Wq0' .. 'W20': [H, H], ('Wq1' ..,) 'b10' .. 'ln2_b0': [H], (..,) 'lnf_g', 'lnf_b': [H],
        'Q': [n_items, H], 'b': [n_items]}: the small weights in the order of the flat array"""
        v = {'E': self.E[:, :self.H]}
        v.update({name: self._small(name) for name in self.slices})
        v.update({'Q': self.Q[:, :self.H], 'b': self.b})
        return v

    def set_baskets(self, baskets):
        """baskets [n_users, L] int: the items of a user's sequence at serving, in sequence order, left-aligned; -1 = an absent position
        (the kernel shifts a basket so that its newest item stands at position L - 1)"""
        a = np.ascontiguousarray(baskets, dtype=np.int32)
        if a.shape != (self.n_users, self.L) or a.max(initial=-1) >= self.n_items or a.min(initial=0) < -1:
            raise _lib.DrxError(f'SASRec engine: baskets must be [{self.n_users}, {self.L}] item ids in -1..{self.n_items - 1}')
        self.baskets.copy_(torch.as_tensor(a))

    # ---- the step (include/drx.h drx_sas_step) ---------------------------------------------------------------------------------------
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
        scratch = self._step_scratch(int(L_.drx_sas_step_scratch_bytes(C.byref(self.dims), B, r)),
                                     lambda: f'drx_sas_step: a batch of {B} windows of {self.L} + 1 + {r} items is outside its domain '
                                     f'(1..{MAX_NEG_RATIO} negatives per window)')
        alphas, slots, loss = self._step_args(step_idx, applies, want_loss)
        check(L_.drx_sas_step(C.byref(self.dims), ptr(self.E), ptr(self.sw), ptr(self.Q), ptr(self.b), *slots, ptr(before), ptr(after), B,
                              r, C.byref(self._rule()), alphas, float(self.reg), loss, ptr(scratch), scratch.numel(),
                              stream_ptr(self.device)), 'drx_sas_step')
        return self._read_loss(want_loss)

    def step_hidden(self, B):
        """[B, ldh]: the h the last step wrote for its B windows — the second array of its scratch (drx_sas_step's carve: the gradient
        rows of E [B L, ldh] first, every array at the next 256-byte boundary).  For tests: serving's rows are held to these bits."""
        base = (-self._scratch.data_ptr()) % 256
        off = base + _round_up(4 * B * self.L * self.ldh, 256)
        return self._scratch[off:off + 4 * B * self.ldh].view(torch.float32).view(B, self.ldh).clone()

    # what the four calls of RowsRecommender and its score_matrix score against: Q and b themselves, and h of the users' baskets
    def rank_ld(self):
        return self.ldh

    def _score_table(self, items=None):
        return self.Q, self.b

    def _query_rows(self, uid):
        """[len(uid), ldh] rows h(basket of u) (drx_sas_query_rows): they depend on the user alone"""
        n = int(uid.numel())
        out = torch.empty(n, self.ldh, dtype=torch.float32, device=self.device)
        if n:
            check(lib().drx_sas_query_rows(ptr(self.E), ptr(self.sw), C.byref(self.dims), ptr(self.baskets), ptr(uid), n, ptr(out),
                                           stream_ptr(self.device)), 'drx_sas_query_rows')
        return out
