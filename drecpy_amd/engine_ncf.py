"""Device-side state of one NeuMF model (He et al. 2017) and the calls into libdrx.so (drx_ncf_*; include/drx.h "NeuMF", DESIGN.md
section 3.10).

Logit x(u, i) = sum_k hg[k] Pg[u, k] Qg[i, k] + hm . MLP([Pm[u] ; Qm[i]]) + b0 — not a dot product, so the fused scorer of
RowsRecommender cannot serve it: score_matrix / pair_scores go through the model's own scorer (half rows per side, then
drx_ncf_score_rows / drx_ncf_pair_scores) and the four calls of RowsRecommender are refused by name.  The device always produces
LOGITS; the public class turns them into probabilities at its boundary.  One training step = drx_ncf_step on B point samples
(uid, iid, y), drawn on the device by drx_point_sample_recorded or given.  torch is the allocator / stream provider only.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .engine_dense import DenseEngine
from .engine_rows import _round_up

MAX_FACTORS = 64
MAX_LAYERS = 4
MAX_WIDTH = 64


def check_shape(factors, mlp_factors, layers, who='NeuMF engine'):
    """the domain of csrc/drx_ncf.hip, refused by name"""
    integer = lambda x: isinstance(x, (int, np.integer)) and not isinstance(x, bool)
    if not (integer(factors) and 1 <= factors <= MAX_FACTORS):
        raise _lib.DrxError(f'{who}: factors must be an integer in 1..{MAX_FACTORS}, got factors={factors!r}')
    if not (integer(mlp_factors) and 1 <= mlp_factors <= MAX_FACTORS):
        raise _lib.DrxError(f'{who}: mlp_factors must be an integer in 1..{MAX_FACTORS}, got mlp_factors={mlp_factors!r}')
    try:
        layers = tuple(layers)
    except TypeError:
        layers = None
    if layers is None or not 1 <= len(layers) <= MAX_LAYERS or not all(integer(f) and 1 <= f <= MAX_WIDTH for f in layers):
        raise _lib.DrxError(f'{who}: layers must be 1..{MAX_LAYERS} hidden widths, each an integer in 1..{MAX_WIDTH}, got layers={layers!r}')
    return int(factors), int(mlp_factors), tuple(int(f) for f in layers)


class NcfEngine(DenseEngine):
    ALPHA_OF = (0, 1, 2)                   # U, V and the small weights, a handle each

    def __init__(self, n_users, n_items, factors=8, mlp_factors=32, layers=(32, 16, 8), device='cuda:0'):
        self._require_gpu()
        self.Kg, self.Km, self.layers = check_shape(factors, mlp_factors, layers)
        z = self._open(n_users, n_items, device)
        self.ldg, self.ldm = _round_up(self.Kg, 4), _round_up(self.Km, 4)
        self.ld = self.ldg + self.ldm
        # the flat array of small weights: W_1, b_1, ..., W_n, b_n, h = [hg | hm], b0 (include/drx.h DrxNcfDims)
        self.slices, off, fin = {}, 0, 2 * self.Km
        d = self.dims = _lib.NcfDims(n_users=self.n_users, n_items=self.n_items, kg=self.Kg, km=self.Km, ldg=self.ldg, ldm=self.ldm,
                                     n_layers=len(self.layers))
        for l, fo in enumerate(self.layers):
            d.f[l], d.off_w[l], d.off_b[l] = fo, off, off + fin * fo
            self.slices[f'W{l + 1}'], self.slices[f'b{l + 1}'] = (off, (fin, fo)), (off + fin * fo, (fo,))
            off += fin * fo + fo
            fin = fo
        d.off_h, d.off_b0, d.n_small = off, off + self.Kg + fin, off + self.Kg + fin + 1
        self.slices['hg'], self.slices['hm'], self.slices['b0'] = (off, (self.Kg,)), (off + self.Kg, (fin,)), (off + self.Kg + fin, (1,))
        self.n_small = int(d.n_small)
        self.hw = int(lib().drx_ncf_half_width(C.byref(d)))
        self.U = torch.zeros(self.n_users, self.ld, **z)
        self.V = torch.zeros(self.n_items, self.ld, **z)
        self.sw = torch.zeros(self.n_small, **z)
        self._init_step_state()
        # what NeuMF._pre_fit registers, in this order: one apply_gradients per handle and step
        self.user_emb = self._handle('user_embeddings', 'Pg', 'Pm')
        self.item_emb = self._handle('item_embeddings', 'Qg', 'Qm')
        self.small = self._handle('small_weights', *self.slices)

    def tensors(self):
        return {'U': self.U, 'V': self.V, 'sw': self.sw}

    def _small(self, name):
        off, shape = self.slices[name]
        return self.sw[off:off + int(np.prod(shape))].view(*shape)

    def views(self):
        """{'Pg': [n_users, Kg], 'Pm': [n_users, Km], 'Qg', 'Qm', 'W1' [2 Km, f_1], 'b1' [f_1], ..., 'hg' [Kg], 'hm' [f_n], 'b0' [1]}"""
        Kg, Km, ldg = self.Kg, self.Km, self.ldg
        v = {'Pg': self.U[:, :Kg], 'Pm': self.U[:, ldg:ldg + Km], 'Qg': self.V[:, :Kg], 'Qm': self.V[:, ldg:ldg + Km]}
        v.update({name: self._small(name) for name in self.slices})
        return v

    def set_params(self, p):
        missing = [n for n in ['Pg', 'Pm', 'Qg', 'Qm'] + list(self.slices) if n not in p]
        if missing:
            raise _lib.DrxError(f'NeuMF engine: set_params lacks {missing}')
        super().set_params(p)

    # ---- the point stream (include/drx.h drx_point_sample_recorded) ------------------------------------------------------------------
    def set_sampler_frame(self, positives, recorded):
        """DenseEngine._upload_frame's (columns ascending)"""
        self._upload_frame(positives, recorded)

    def sample(self, B, neg_ratio, seed):
        """(uid int32, iid int32, y float32) [B] device tensors: the B point samples of `seed` (drx_point_sample_recorded)"""
        B = int(B)
        L_ = lib()
        uid, iid = (torch.empty(max(B, 1), dtype=torch.int32, device=self.device) for _ in range(2))
        y = torch.empty(max(B, 1), dtype=torch.float32, device=self.device)
        keep_off = torch.empty(max(B, 1) + 1, dtype=torch.int32, device=self.device)
        need = int(L_.drx_point_sample_scratch_bytes(max(B, 1)))
        sc = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        check(L_.drx_point_sample_recorded(C.byref(self._H), C.byref(self._R) if self._R is not None else None, self.n_users, self.n_items,
                                           B, int(neg_ratio), int(seed) & ((1 << 64) - 1), ptr(uid), ptr(iid), ptr(y), ptr(keep_off),
                                           ptr(sc), need, None, 0, stream_ptr(self.device)), 'drx_point_sample_recorded')
        return uid, iid, y

    # ---- the step (include/drx.h drx_ncf_step) -----------------------------------------------------------------------------------------
    def step(self, step_idx, uid, iid, y, want_loss=False, applies=None):
        """One step on B point samples (arrays or device tensors): uid, iid [B] ids, y [B] in {0, 1}.  applies = (n, j_user, j_item,
        j_small): the number of apply_gradients calls per step and the positions of the three handles among them (the registration
        order); default (3, 0, 1, 2).  Returns the mean BCE of the batch before the update when want_loss, else None."""
        applies = tuple(applies) if applies is not None else (3, 0, 1, 2)
        uid, iid = self._dev_i32(uid).reshape(-1), self._dev_i32(iid).reshape(-1)
        y = (y.to(self.device, torch.float32) if torch.is_tensor(y) else torch.as_tensor(np.ascontiguousarray(y, np.float32)).to(self.device))
        y = y.contiguous().reshape(-1)
        B = int(uid.numel())
        assert iid.numel() == B and y.numel() == B, 'step takes parallel users, items and targets'
        L_ = lib()
        scratch = self._step_scratch(int(L_.drx_ncf_step_scratch_bytes(C.byref(self.dims), B)),
                                     lambda: f'drx_ncf_step: a batch of {B} samples is outside its domain (1 .. 2^24 - 1)')
        alphas, slots, loss = self._step_args(step_idx, applies, want_loss)
        check(L_.drx_ncf_step(C.byref(self.dims), ptr(self.U), ptr(self.V), ptr(self.sw), *slots, ptr(uid), ptr(iid), ptr(y), B,
                              C.byref(self._rule()), alphas, float(self.reg), loss, ptr(scratch), scratch.numel(), stream_ptr(self.device)),
              'drx_ncf_step')
        return self._read_loss(want_loss)

    # ---- logits --------------------------------------------------------------------------------------------------------------------------
    def half_rows(self, side, ids=None):
        """[n, hw] half rows of the device ids (None: every row) of the users (side 0) or the items (side 1) (drx_ncf_half_rows)"""
        table = self.U if side == 0 else self.V
        n = int(ids.numel()) if ids is not None else int(table.shape[0])
        out = torch.empty(n, self.hw, dtype=torch.float32, device=self.device)
        if n:
            check(lib().drx_ncf_half_rows(C.byref(self.dims), ptr(table), ptr(self.sw), ptr(ids), n, side, ptr(out), stream_ptr(self.device)),
                  'drx_ncf_half_rows')
        return out

    def score_matrix(self, uids):
        """[len(uids), n_items] LOGITS of the given users against all items: the item half rows once per call, the users', then
        drx_ncf_score_rows — the score-matrix route of every ranking call"""
        uid = self._dev_i32(uids).reshape(-1)
        R = int(uid.numel())
        out = torch.empty(R, self.n_items, dtype=torch.float32, device=self.device)
        if R:
            ih, uh = self.half_rows(1), self.half_rows(0, uid)
            check(lib().drx_ncf_score_rows(C.byref(self.dims), ptr(self.sw), ptr(uh), ptr(ih), R, ptr(out), stream_ptr(self.device)),
                  'drx_ncf_score_rows')
        return out

    def pair_scores(self, uids, iids):
        """float32 [P] LOGITS of the parallel (user, item) ids, -inf for an item outside the catalogue: half rows of the request's
        distinct users and items, then drx_ncf_pair_scores — the bits of the matching cells of score_matrix"""
        uid, iid = self._pairs_request(uids, iids, 'pair_scores')
        P = int(uid.numel())
        out = torch.empty(P, dtype=torch.float32, device=self.device)
        if P == 0:
            return out
        inside = (iid >= 0) & (iid < self.n_items)
        du, urow = torch.unique(uid, return_inverse=True)
        di, irow = torch.unique(torch.where(inside, iid, torch.zeros_like(iid)), return_inverse=True)
        uh, ih = self.half_rows(0, du.to(torch.int32).contiguous()), self.half_rows(1, di.to(torch.int32).contiguous())
        urow, irow = urow.to(torch.int32).contiguous(), irow.to(torch.int32).contiguous()
        check(lib().drx_ncf_pair_scores(C.byref(self.dims), ptr(self.sw), ptr(uh), ptr(ih), ptr(urow), ptr(irow), P, ptr(out),
                                        stream_ptr(self.device)), 'drx_ncf_pair_scores')
        return torch.where(inside, out, torch.full_like(out, float('-inf')))

    # ---- the fused scorer of RowsRecommender takes query row . item row: NeuMF's logit is none -------------------------------------------
    def _refuse(self, call):
        raise _lib.DrxError(f'NcfEngine.{call}: NeuMF\'s logit is not a dot product and the fused scorer does not serve it; '
                            f'use score_matrix + topk, or pair_scores')

    def recommend(self, *a, **k):
        self._refuse('recommend')

    def rank_items(self, *a, **k):
        self._refuse('rank_items')

    def rank_lists(self, *a, **k):
        self._refuse('rank_lists')
