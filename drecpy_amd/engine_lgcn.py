"""Device-side state of one LightGCN model (He et al. 2020) and the calls into libdrx.so (drx_lgcn_*; include/drx.h "LightGCN",
DESIGN.md section 3.14).

Nodes are the users, then the items; E0 = [P ; Q] is ONE allocation with P and Q as views of it.  Final embeddings
Ebar = (1 / (layers + 1)) sum_l A^l E0 over the symmetric normalised adjacency A of the positives; score x(u, i) = Ebar[u] . Ebar[n_users
+ i] — DRX_REC_BIAS of the fused scorer with a zero bias, the item rows of a cached Ebar as the table and its user rows as the query
rows: recommend / rank_items / rank_lists / pair_scores are RowsRecommender's.  One training step = drx_lgcn_step on T (user, positive,
negative) triples, BPR's stream.  torch is the allocator / stream provider only.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .engine_bpr import BprEngine
from .engine_rows import _round_up

MAX_FACTORS = 256
MAX_LAYERS = 4


class LgcnGraph:
    """include/drx.h DrxLgcnGraph on the device: the CSR of a symmetric adjacency (indptr int64 [N + 1], indices [nnz2], columns of a
    row in the order they are summed in), the node weights w [N] and the cut of rows longer than drx_lgcn_row_split()."""

    def __init__(self, indptr, indices, w, device='cuda:0'):
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        w = np.ascontiguousarray(w, dtype=np.float32)
        N = len(indptr) - 1
        if N < 1 or len(w) != N or indptr[0] != 0 or indptr[-1] != len(indices) or (np.diff(indptr) < 0).any():
            raise _lib.DrxError('LightGCN graph: indptr, indices and w do not describe one CSR')
        if len(indices) and (indices.min() < 0 or indices.max() >= N):
            raise _lib.DrxError('LightGCN graph: a column outside [0, N)')
        S = int(lib().drx_lgcn_row_split())
        length = np.diff(indptr)
        n_seg = np.maximum(1, (length + S - 1) // S) if S > 0 else np.ones(N, np.int64)
        seg_ptr = np.zeros(N + 1, np.int64)
        seg_ptr[1:] = np.cumsum(n_seg)
        if seg_ptr[-1] >= 1 << 30:
            raise _lib.DrxError('LightGCN graph: too many row segments')
        cut = np.flatnonzero(n_seg > 1)
        self.N, self.nnz2, self.n_seg, self.n_cut = N, int(len(indices)), int(seg_ptr[-1]), int(len(cut))
        d = torch.device(device)
        up = lambda a, t: torch.as_tensor(np.ascontiguousarray(a if len(a) else np.zeros(1, t), dtype=t)).to(d)
        self._arrays = [up(indptr, np.int64), up(indices, np.int32), up(w, np.float32), up(np.repeat(np.arange(N), n_seg), np.int32),
                        up(seg_ptr, np.int32), up(cut, np.int32)]
        self.w = self._arrays[2]
        self.struct = _lib.LgcnGraph(*[ptr(a) for a in self._arrays[:5]], ptr(self._arrays[5]) if self.n_cut else None, N, self.n_seg,
                                     self.n_cut)

    @classmethod
    def from_positives(cls, positives, n_users, n_items, device='cuda:0'):
        """The bipartite graph of the positives CSR (indptr [n_users + 1], item ids): duplicates merged, a user row lists n_users + iid
        ascending, an item row lists uids ascending, w = degree^(-1/2) (0 for a node without edges) rounded to fp32."""
        indptr, cols = np.asarray(positives[0], np.int64), np.asarray(positives[1], np.int64)
        u = np.repeat(np.arange(n_users, dtype=np.int64), np.diff(indptr))
        pairs = np.unique(u * n_items + cols)                       # ascending by (user, item), duplicates merged
        u, i = pairs // n_items, pairs % n_items
        by_item = np.lexsort((u, i))
        deg = np.concatenate([np.bincount(u, minlength=n_users), np.bincount(i, minlength=n_items)]).astype(np.int64)
        ip = np.zeros(n_users + n_items + 1, np.int64)
        ip[1:] = np.cumsum(deg)
        w = np.zeros(len(deg), np.float64)
        w[deg > 0] = 1.0 / np.sqrt(deg[deg > 0])
        return cls(ip, np.concatenate([n_users + i, u[by_item]]), w, device)


def propagate(graph, inp, base=None, scale=1.0, out=None):
    """scale (base + A inp) for [N, ld] device tensors (drx_lgcn_propagate): what the tests and the benchmark call by itself"""
    N, ld = inp.shape
    out = torch.empty_like(inp) if out is None else out
    need = int(lib().drx_lgcn_part_bytes(C.byref(graph.struct), ld))
    if need == 0:
        raise _lib.DrxError(f'drx_lgcn_propagate: rows of {ld} floats are outside its domain')
    part = torch.empty(need, dtype=torch.uint8, device=inp.device)
    check(lib().drx_lgcn_propagate(C.byref(graph.struct), ptr(base), ptr(inp), ptr(out), ld, float(scale), ptr(part), need,
                                   stream_ptr(inp.device)), 'drx_lgcn_propagate')
    return out


class LgcnEngine(BprEngine):
    """(BprEngine's triple stream — set_sampler_frame, sample — is inherited; its tables, step and serving are replaced.)"""
    EPILOGUE = _lib.DRX_REC_BIAS
    ALPHA_OF = (0, 1)                      # P with the user handle, Q with the item handle

    def __init__(self, n_users, n_items, factors=64, layers=3, device='cuda:0'):
        self._require_gpu()
        if not (isinstance(factors, (int, np.integer)) and 1 <= factors <= MAX_FACTORS):
            raise _lib.DrxError(f'LightGCN engine: factors must be an integer in 1..{MAX_FACTORS} (a row is one float4 per lane of a '
                                f'wavefront), got factors={factors!r}')
        if not (isinstance(layers, (int, np.integer)) and 0 <= layers <= MAX_LAYERS):
            raise _lib.DrxError(f'LightGCN engine: layers must be an integer in 0..{MAX_LAYERS}, got layers={layers!r}')
        z = self._open(n_users, n_items, device)
        self.K, self.layers = int(factors), int(layers)
        self.ld = _round_up(self.K, 4)
        self.N = self.n_users + self.n_items
        self.E0 = torch.zeros(self.N, self.ld, **z)
        self.P, self.Q = self.E0[:self.n_users], self.E0[self.n_users:]
        self.bias = torch.zeros(self.n_items, **z)                # stays zero: the scorer's epilogue adds it
        self._graph = None
        self._ebar = None
        self._init_step_state()
        self.user_emb = self._handle('user_factors', 'P')
        self.item_emb = self._handle('item_factors', 'Q')

    def tensors(self):
        return {'P': self.P, 'Q': self.Q}

    def views(self):
        """{'P': [n_users, K], 'Q': [n_items, K]}"""
        return {'P': self.P[:, :self.K], 'Q': self.Q[:, :self.K]}

    def set_params(self, p):
        self._ebar = None
        super().set_params(p)

    def restore(self, snap, with_optimizer=False):
        self._ebar = None
        super().restore(snap, with_optimizer)

    # ---- the graph ------------------------------------------------------------------------------------------------------------------
    def set_graph(self, positives):
        """positives: (indptr, item ids) of the pairs with interaction >= threshold — the frame the sampler draws from"""
        self._graph = LgcnGraph.from_positives(positives, self.n_users, self.n_items, self.device)
        self._ebar = None

    def _need_graph(self):
        if self._graph is None:
            raise _lib.DrxError('LightGCN engine: set_graph(positives) first')
        return C.byref(self._graph.struct)

    # ---- the step (include/drx.h drx_lgcn_step) -------------------------------------------------------------------------------------
    def step(self, step_idx, uid, pos, neg, want_loss=False, applies=None):
        """BprEngine.step's contract: one step on the triples; applies = (n, j_user, j_item), default (2, 0, 1)."""
        applies = tuple(applies) if applies is not None else (2, 0, 1)
        uid, pos, neg = self._dev_i32(uid), self._dev_i32(pos), self._dev_i32(neg)
        T = int(uid.numel())
        assert pos.numel() == T and neg.numel() == T, 'step takes parallel users, positives and negatives'
        L_, g = lib(), self._need_graph()
        scratch = self._step_scratch(int(L_.drx_lgcn_step_scratch_bytes(g, T, self.ld, self.n_users)),
                                     lambda: f'drx_lgcn_step: a batch of {T} triples at rows of {self.ld} floats is outside its domain')
        alphas, slots, loss = self._step_args(step_idx, applies, want_loss)
        self._ebar = None
        check(L_.drx_lgcn_step(ptr(self.E0), *slots, self.ld, self.n_users, g, ptr(uid), ptr(pos), ptr(neg), T, self.layers,
                               C.byref(self._rule()), alphas, float(self.reg), loss, ptr(scratch), scratch.numel(),
                               stream_ptr(self.device)), 'drx_lgcn_step')
        return self._read_loss(want_loss)

    def step_ebar(self):
        """[N, ld]: the final embeddings the LAST step's forward pass left in its scratch (layers >= 1; include/drx.h drx_lgcn_step)"""
        assert self.layers >= 1 and self._scratch is not None
        lead = (-self._scratch.data_ptr()) % 256
        return self._scratch[lead:lead + self.N * self.ld * 4].view(torch.float32).view(self.N, self.ld).clone()

    # ---- serving: the cached final embeddings (drx_lgcn_final), dropped by step, set_params, restore and set_graph --------------------
    def final_embeddings(self):
        if self._ebar is None:
            L_, g = lib(), self._need_graph()
            need = int(L_.drx_lgcn_final_scratch_bytes(g, self.ld))
            scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
            out = torch.empty_like(self.E0)
            check(L_.drx_lgcn_final(ptr(self.E0), g, self.layers, self.ld, ptr(out), ptr(scratch), need, stream_ptr(self.device)),
                  'drx_lgcn_final')
            self._ebar = out
        return self._ebar

    def rank_ld(self):
        return self.ld

    def _score_table(self, items=None):
        return self.final_embeddings()[self.n_users:], self.bias

    def _query_rows(self, uid):
        return self._gather_rows(self.final_embeddings()[:self.n_users], uid)
