"""What the engines of all models share: the exclusion CSR on the device, the four calls into the fused scorer (include/drx.h
drx_rows_recommend / drx_rows_rank_items / drx_rows_rank_lists / drx_rows_pair_scores) and the selection of the
score-matrix route (drx_topk under a host candidate mask).  torch is the allocator / stream provider only.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr

ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-7  # tf.keras.optimizers.Adam defaults


def _round_up(x, m):
    return (x + m - 1) // m * m


def pack_mask_bits(mask_bool):
    """bool [R,n] (numpy) -> uint32 words; bit (i & 31) of word (i >> 5) is flat element i."""
    flat = np.asarray(mask_bool, dtype=bool).ravel()
    pad = (-len(flat)) % 32
    if pad:
        flat = np.concatenate([flat, np.zeros(pad, bool)])
    return np.packbits(flat, bitorder='little').view(np.uint32).copy()


class RowsRecommender:
    """The base of every engine.  An engine brings n_users, n_items and device, and says in ONE place what it scores against:

      EPILOGUE            the DRX_REC_* of its scores, and rank_ld() the width of a row in floats
      _score_table(items) -> (table [n, ld], bias [n] or None), float32 contiguous: the rows of the catalogue (items None) or of the
                          device ids `items`.  TABLE_IS_COMPUTED False: the weights themselves, whatever `items`.  True (DMF's item
                          tower): computed when asked — once per call, and in pair_scores over the request's distinct items only
      _query_rows(uid, *query) -> [r, ld] float32 contiguous rows, padding columns ZERO (the scorer multiplies them)
      QUERY_BY_ROW        False: a query row is its user's alone (CDAE, DMF).  True: it belongs to the request row (uid, *query) —
                          Caser's (user, last L items); `query` are per-row arrays, uploaded once per call as int32 [R, -1]

    recommend / rank_items / rank_lists / pair_scores below then answer for it, `chunk` rows at a time, from one kept scratch.
    Calling convention: (uids, *query, <the call's own arrays>, keywords); an engine with QUERY_BY_ROW False takes no `query`.
    KnnEngine scores with kernels of its own and overrides the calls; it shares the request and scratch helpers."""
    EPILOGUE = None
    TABLE_IS_COMPUTED = False
    QUERY_BY_ROW = False
    RECOMMEND_CHUNK_USERS = 16384          # rows per launch of recommend / rank_items / rank_lists: bounds the scratch (candidate keys only)
    PAIR_CHUNK_PAIRS = 1 << 20             # pairs per launch of pair_scores: bounds the query rows of a chunk's distinct users
    # pairs are grouped per user when there are at least this many per distinct user (RecommenderABC._catalogue_ranks_fused;
    # DESIGN.md section 3.5 has the measurement behind the value)
    RANK_LISTS_MIN_MEAN = 2.0

    @staticmethod
    def adam_alpha(lr, t, beta1=ADAM_B1, beta2=ADAM_B2):
        """Keras-Adam lr_t for the 1-based step t, in fp32 like optimizer_v2/adam.py."""
        f = np.float32
        return float(f(lr) * np.sqrt(f(1.0) - np.power(f(beta2), f(t))) / (f(1.0) - np.power(f(beta1), f(t))))

    def _dev_i32(self, a):
        if torch.is_tensor(a):
            return a.to(self.device, torch.int32).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)

    # ---- what the constructors of the factor baselines open with, and their parameters by name ----------------------------------------
    @staticmethod
    def _require_gpu():
        if not torch.cuda.is_available():
            raise _lib.DrxError('drecpy_amd needs a ROCm GPU (MI355X); there is no CPU fallback.')

    def _open(self, n_users, n_items, device):
        """After the engine's own domain checks: the library, the device and the sizes.  Returns the keywords of a float32 device tensor."""
        lib()
        self.device = torch.device(device)
        self.n_users, self.n_items = int(n_users), int(n_items)
        return dict(dtype=torch.float32, device=self.device)

    def views(self):
        """name -> the UNPADDED view of a parameter inside tensors(), in get_params()'s order: what an engine of a factor baseline
        declares once; set_params, get_params and its TrainableModel handles read it"""
        raise NotImplementedError(f'{type(self).__name__} names its parameters itself')

    def set_params(self, p):
        """p: name -> array of the shape of views()[name] (unpadded); the padding columns are zeroed"""
        for x in self.tensors().values():
            x.zero_()
        for name, v in self.views().items():
            v.copy_(torch.as_tensor(np.asarray(p[name], dtype=np.float32).reshape(tuple(v.shape))).to(self.device))

    def get_params(self):
        return {name: v.detach().cpu().numpy().copy() for name, v in self.views().items()}

    def _handle(self, name, *params):
        """the TrainableModel a model registers for the parameters `params` of views(): one apply_gradients per handle and step"""
        from .Recommender.trainables import TrainableModel
        return TrainableModel(name, lambda: [self.views()[n] for n in params])

    def _gather_rows(self, table, ids):
        """[len(ids), ld] rows of `table` [n, ld] by device id (drx_bpr_gather_rows: a plain row gather)"""
        n, ld = int(ids.numel()), int(table.shape[1])
        out = torch.empty(n, ld, dtype=torch.float32, device=self.device)
        if n:
            check(lib().drx_bpr_gather_rows(ptr(table), ld, ptr(ids), n, ptr(out), stream_ptr(self.device)), 'drx_bpr_gather_rows')
        return out

    # ---- the score-matrix route: rank(), ranking_evaluation and requests outside the fused domain ------------------------------------
    def score_matrix(self, uids):
        """[len(uids), n_items] scores of the given users against all items, from what the engine declares below (_query_rows,
        _score_table, rank_ld) through drx_rows_dot: the score-matrix route of _rank_rows.  An engine whose score is no dot product
        (NeuMF) or whose table is computed (DMF) has its own."""
        uid = self._dev_i32(uids).reshape(-1)
        B = int(uid.numel())
        out = torch.empty(B, self.n_items, dtype=torch.float32, device=self.device)
        if B:
            q, (table, bias) = self._query_rows(uid), self._score_table()
            check(lib().drx_rows_dot(ptr(q), B, ptr(table), self.n_items, self.rank_ld(), ptr(bias), ptr(out), stream_ptr(self.device)),
                  'drx_rows_dot')
        return out

    def topk(self, scores, k, cand_mask=None):
        """Row-wise top-k with heapq.nlargest((score, iid)) ordering (cdae.py:103)."""
        scores = scores.contiguous()
        R, n = scores.shape
        out_idx = torch.empty(R, k, dtype=torch.int32, device=self.device)
        out_val = torch.empty(R, k, dtype=torch.float32, device=self.device)
        sb = lib().drx_topk_scratch_bytes_k(R, n, k)
        sc = torch.empty(sb, dtype=torch.uint8, device=self.device) if sb else None
        check(lib().drx_topk(ptr(scores), ptr(cand_mask), R, n, k, ptr(out_idx), ptr(out_val), ptr(sc), sb,
                             stream_ptr(self.device)), 'drx_topk')
        return out_idx, out_val

    def masked_topk(self, scores, cand, k):
        """topk among the candidates `cand`, a host bool array [R, n_items]: -1 / -inf behind a row's last candidate."""
        return self.topk(scores, k, torch.as_tensor(pack_mask_bits(cand).view(np.int32)).to(self.device))

    @staticmethod
    def matrix_chunk_users(n_items, budget_bytes):
        """Users per chunk of the score-matrix route: their fp32 [R, n_items] matrix within `budget_bytes`, and R * n_items < 2^31
        (the index range of drx_topk's long rows)."""
        return max(1, min(budget_bytes // (4 * n_items), ((1 << 31) - 1) // n_items))

    # ---- exclusions ------------------------------------------------------------------------------------------------------------------
    def set_exclusions(self, indptr, indices):
        """CSR over users (columns ascending and unique) of the items recommend() never returns for a user; None = none."""
        if indptr is None:
            self._excl = None
            return
        ip = np.ascontiguousarray(indptr, dtype=np.int64)
        ix = np.ascontiguousarray(indices, dtype=np.int32)
        assert len(ip) == self.n_users + 1 and int(ip[-1]) == len(ix)
        d_ip = torch.as_tensor(ip).to(self.device)
        d_ix = torch.as_tensor(ix if len(ix) else np.zeros(1, np.int32)).to(self.device)
        self._excl = (d_ip, d_ix, ip, ix)

    def _exclusion_mask(self, host_uids):
        """The rows of set_exclusions() as a host candidate mask, bool [len(host_uids), n_items]: False at a user's excluded items."""
        _, _, ip, ix = self._excl
        cand = np.ones((len(host_uids), self.n_items), dtype=bool)
        for j, x in enumerate(host_uids):
            cand[j, ix[ip[x]:ip[x + 1]]] = False
        return cand

    def _exclusions(self, exclude, call):
        """The CSR of set_exclusions() that `call` excludes by, or None.  exclude: None = where one was given, True = there must be
        one, False = nothing excluded."""
        excl = getattr(self, '_excl', None) if exclude is None or exclude is True else None
        assert not (exclude is True and excl is None), f'{call}(exclude=True) needs set_exclusions()'
        return excl

    @staticmethod
    def _excl_ptrs(excl):
        return (ptr(excl[0]), ptr(excl[1])) if excl else (None, None)

    # ---- what a request is, where its answer goes, what a launch works in -------------------------------------------------------------
    def _recommend_request(self, uids, n, exclude):
        """(uid int32 on the device, n, the exclusion CSR or None, out_idx int32 [R, n], out_val float32 [R, n])"""
        uid = self._dev_i32(uids).reshape(-1)
        n = int(n)
        assert n >= 1
        return (uid, n, self._exclusions(exclude, 'recommend')) + self._outputs(int(uid.numel()), n)

    def _pairs_request(self, uids, items, call):
        """(uid int32 [P], item int32 [P]) on the device"""
        uid, item = self._dev_i32(uids).reshape(-1), self._dev_i32(items).reshape(-1)
        assert uid.numel() == item.numel(), f'{call} takes parallel users and items'
        return uid, item

    def _rank_lists_request(self, uids, indptr, items, exclude):
        """(uid int32 [R] on the device, the offsets int64 [R + 1] on the host and on the device, targets int32 [P] on the device,
        the exclusion CSR or None)"""
        uid, targets = self._dev_i32(uids).reshape(-1), self._dev_i32(items).reshape(-1)
        ip = indptr.cpu().numpy() if torch.is_tensor(indptr) else np.asarray(indptr)
        ip = np.ascontiguousarray(ip, dtype=np.int64).reshape(-1)
        assert len(ip) == uid.numel() + 1 and ip[0] == 0 and ip[-1] == targets.numel() and (np.diff(ip) >= 0).all(), \
            'rank_lists takes CSR offsets [R + 1] over the items: 0 first, ascending, len(items) last'
        return uid, ip, torch.as_tensor(ip).to(self.device), targets, self._exclusions(exclude, 'rank_lists')

    def _outputs(self, *shape):
        """(int32, float32) device tensors of `shape`: ids and values, or ranks and scores.  A request whose outputs are EMPTY returns
        them as they are, before a table or a query row is computed."""
        return torch.empty(*shape, dtype=torch.int32, device=self.device), torch.empty(*shape, dtype=torch.float32, device=self.device)

    def _rows_scratch(self, need):
        """At least `need` bytes on the device (None for 0), kept between the calls and grown when a launch needs more."""
        sc = getattr(self, '_rows_sc', None)
        if need and (sc is None or sc.numel() < need):
            self._rows_sc = None
            sc = self._rows_sc = torch.empty(need, dtype=torch.uint8, device=self.device)
        return sc if need else None

    # ---- what an engine declares ------------------------------------------------------------------------------------------------------
    def rank_ld(self):
        """The width of this engine's query rows in the fused scorer (what rank_is_fused / rank_lists_group are asked about)."""
        raise NotImplementedError(f'{type(self).__name__} does not score through the fused scorer')

    def _score_table(self, items=None):
        raise NotImplementedError(f'{type(self).__name__} does not score through the fused scorer')

    def _query_rows(self, uid, *query):
        raise NotImplementedError(f'{type(self).__name__} does not score through the fused scorer')

    def recommend_is_fused(self, ld, n):
        """Whether rows of `ld` floats and lists of n lie in the fused domain (else drx_rows_recommend answers DRX_ENOTIMPL)."""
        return int(lib().drx_rows_recommend_scratch_bytes(1, self.n_items, int(ld), int(n))) > 0

    def rank_is_fused(self, ld):
        """Whether rows of `ld` floats lie in the fused domain of drx_rows_rank_items (else it answers DRX_ENOTIMPL)."""
        return int(lib().drx_rows_rank_items_scratch_bytes(1, self.n_items, int(ld))) > 0

    def rank_lists_group(self, ld):
        """G: the targets of one row that drx_rows_rank_lists counts in ONE walk at rows of `ld` floats (a longer row walks again for
        every further G); 0 outside the fused domain."""
        return int(lib().drx_rows_rank_lists_group(int(ld)))

    def _recommend_fused(self, R, n):
        """Whether recommend() answers R rows and lists of n from the fused scorer-selector.  An engine that may say no has a
        _recommend_by_matrix(uid, n, excl, out_idx, out_val); for the others the library refuses a request outside the fused domain."""
        return True

    # ---- the chunk loop and the query rows of a chunk ---------------------------------------------------------------------------------
    def _catalogue_table(self):
        """(table [n_items, ld], bias, ld, stream): what recommend, rank_items and rank_lists score against, once per call"""
        table, bias = self._score_table()
        ld = self.rank_ld()
        assert table.is_contiguous() and tuple(table.shape) == (self.n_items, ld)
        return table, bias, ld, stream_ptr(self.device)

    def _query_arrays(self, query, R):
        assert self.QUERY_BY_ROW or not query, f'{type(self).__name__} makes its query rows from the users alone'
        return [self._dev_i32(x).reshape(R, -1) for x in query]

    @staticmethod
    def _chunks(total, chunk):
        """(lo, hi) of `chunk` rows of a request at a time"""
        for lo in range(0, total, chunk):
            yield lo, min(lo + chunk, total)

    def _chunk_rows(self, uid, query, lo, hi, per_distinct):
        """(q, inverse): the query rows of request rows [lo, hi).  By request row, or per_distinct False: q [hi - lo, ld] as given,
        inverse None.  Else the rows of the chunk's DISTINCT users, made once, and each request row's position among them."""
        u, inverse = uid[lo:hi], None
        if per_distinct and not self.QUERY_BY_ROW:
            u, inverse = torch.unique(u, return_inverse=True)
            u = u.to(torch.int32).contiguous()
        q = self._query_rows(u, *[x[lo:hi] for x in query])
        assert q.is_contiguous() and tuple(q.shape) == (int(u.numel()), self.rank_ld()) and q.dtype == torch.float32
        return q, inverse

    def _gathered_rows(self, uid, query, lo, hi):
        """one query row per request row of [lo, hi), made once per distinct user where a row is its user's alone"""
        q, inverse = self._chunk_rows(uid, query, lo, hi, True)
        return q if inverse is None else q[inverse].contiguous()

    # ---- the four calls ---------------------------------------------------------------------------------------------------------------
    def recommend(self, uids, *query_n, exclude=None, chunk_users=None):
        """recommend(uids, *query, n): (idx int32 [R, n], val float32 [R, n]) device tensors — the n best items of every request row by
        (score, item) descending, -1 / -inf behind the last eligible one.  exclude: None = the rows of set_exclusions() where one was
        given, True = they must have been, False = nothing excluded.  The table once per call, the query rows of every row as given,
        scores and selection from the fused scorer-selector `chunk_users` rows at a time.  Outside its domain (n > 128, rows wider
        than 256 floats): DrxError (recommend_is_fused tells) — unless the engine has another route (_recommend_fused)."""
        *query, n = query_n
        uid, n, excl, out_idx, out_val = self._recommend_request(uids, n, exclude)
        R = int(uid.numel())
        if R == 0:
            return out_idx, out_val
        if not self._recommend_fused(R, n):
            return self._recommend_by_matrix(uid, n, excl, out_idx, out_val)
        L, query = lib(), self._query_arrays(query, R)
        table, bias, ld, stream = self._catalogue_table()
        for lo, hi in self._chunks(R, int(chunk_users or self.RECOMMEND_CHUNK_USERS)):
            q, _ = self._chunk_rows(uid, query, lo, hi, False)
            sc = self._rows_scratch(int(L.drx_rows_recommend_scratch_bytes(hi - lo, self.n_items, ld, n)))
            check(L.drx_rows_recommend(ptr(table), ptr(bias), self.n_items, ld, self.EPILOGUE, ptr(q), ptr(uid[lo:hi]), hi - lo, n,
                                       *self._excl_ptrs(excl), ptr(out_idx[lo:hi]), ptr(out_val[lo:hi]), ptr(sc),
                                       sc.numel() if sc is not None else 0, stream), 'drx_rows_recommend')
        return out_idx, out_val

    def rank_items(self, uids, *query_items, exclude=None, chunk_rows=None):
        """rank_items(uids, *query, items): (rank int32 [P], score float32 [P]) device tensors for the parallel rows / items — the
        position of items[p] in the list recommend(row p, n = unbounded, exclude) would give, whatever the item's own exclusion: the
        number of eligible items ahead of it —, and its score; -1 / -inf for an item outside the catalogue.  One row and one catalogue
        walk per pair: a user with T items costs T rows (rank_lists takes them as one).  The same table, bias and epilogue as
        recommend().  Rows wider than 256 floats: DrxError (rank_is_fused tells)."""
        *query, items = query_items
        uid, target = self._pairs_request(uids, items, 'rank_items')
        excl = self._exclusions(exclude, 'rank_items')
        P = int(uid.numel())
        out_rank, out_score = self._outputs(P)
        if P == 0:
            return out_rank, out_score
        L, query = lib(), self._query_arrays(query, P)
        table, bias, ld, stream = self._catalogue_table()
        for lo, hi in self._chunks(P, int(chunk_rows or self.RECOMMEND_CHUNK_USERS)):
            q = self._gathered_rows(uid, query, lo, hi)
            sc = self._rows_scratch(int(L.drx_rows_rank_items_scratch_bytes(hi - lo, self.n_items, ld)))
            check(L.drx_rows_rank_items(ptr(table), ptr(bias), self.n_items, ld, self.EPILOGUE, ptr(q), ptr(uid[lo:hi]), ptr(target[lo:hi]),
                                        hi - lo, *self._excl_ptrs(excl), ptr(out_rank[lo:hi]), ptr(out_score[lo:hi]), ptr(sc),
                                        sc.numel() if sc is not None else 0, stream), 'drx_rows_rank_items')
        return out_rank, out_score

    def rank_lists(self, uids, *query_indptr_items, exclude=None, chunk_rows=None):
        """rank_lists(uids, *query, indptr, items): rank_items for rows that own several items — row r with the ASCENDING
        items[indptr[r]:indptr[r + 1]] (CSR offsets [R + 1]; a row may be empty, a user may own several rows).  (rank int32 [P], score
        float32 [P]) device tensors parallel to `items`, bit for bit what rank_items gives for the pairs — at one catalogue walk and
        one query row per rank_lists_group(ld) items of a row instead of one per item.  A chunk without items is skipped; the offsets
        are absolute, so a launch gets them from its first row on and writes the outputs in place."""
        *query, indptr, items = query_indptr_items
        uid, ip, d_ip, targets, excl = self._rank_lists_request(uids, indptr, items, exclude)
        R = int(uid.numel())
        out_rank, out_score = self._outputs(int(targets.numel()))
        if targets.numel() == 0:
            return out_rank, out_score
        L, query = lib(), self._query_arrays(query, R)
        table, bias, ld, stream = self._catalogue_table()
        for lo, hi in self._chunks(R, int(chunk_rows or self.RECOMMEND_CHUNK_USERS)):
            p = int(ip[hi] - ip[lo])
            if p == 0:
                continue
            q = self._gathered_rows(uid, query, lo, hi)
            sc = self._rows_scratch(int(L.drx_rows_rank_lists_scratch_bytes(hi - lo, p, self.n_items, ld)))
            if sc is None:
                raise _lib.DrxError(f'drx_rows_rank_lists: rows of {ld} floats lie outside the fused domain (rank_is_fused tells)')
            check(L.drx_rows_rank_lists(ptr(table), ptr(bias), self.n_items, ld, self.EPILOGUE, ptr(q), ptr(uid[lo:hi]), hi - lo,
                                        ptr(d_ip[lo:]), ptr(targets), *self._excl_ptrs(excl), ptr(out_rank), ptr(out_score), ptr(sc),
                                        sc.numel(), stream), 'drx_rows_rank_lists')
        return out_rank, out_score

    def pair_scores(self, uids, *query_items, chunk_pairs=None):
        """pair_scores(uids, *query, items): float32 [P] device tensor — the score of items[p] for request row p and nothing else, two
        rows per pair, no catalogue walk and no scratch —, -inf for an item outside the catalogue.  The same table, bias and epilogue
        as rank_items and, for rows of up to 256 floats, its values; wider rows are answered too.  A computed table (TABLE_IS_COMPUTED)
        holds the request's DISTINCT in-catalogue items alone, a pair's table row being its item's position among them.  Query rows:
        once per distinct user of a chunk, or the chunk's own rows (QUERY_BY_ROW).  Any pair order; sorted by user the query rows are
        read from the L1."""
        *query, items = query_items
        uid, t_row = self._pairs_request(uids, items, 'pair_scores')
        P = int(uid.numel())
        out = torch.empty(P, dtype=torch.float32, device=self.device)
        if P == 0:
            return out
        distinct = None
        if self.TABLE_IS_COMPUTED:
            inside = (t_row >= 0) & (t_row < self.n_items)
            distinct, t_row = torch.unique(torch.where(inside, t_row, torch.full_like(t_row, -1)), return_inverse=True)   # ascending: -1 first
            outside = int(distinct[0].item() < 0)
            distinct, t_row = distinct[outside:].to(torch.int32).contiguous(), (t_row - outside).to(torch.int32).contiguous()  # (-1: no row)
            if int(distinct.numel()) == 0:
                return out.fill_(float('-inf'))
        L, query = lib(), self._query_arrays(query, P)
        (table, bias), ld, stream = self._score_table(distinct), self.rank_ld(), stream_ptr(self.device)
        assert table.is_contiguous() and table.dim() == 2 and table.shape[1] == ld
        chunk = int(chunk_pairs or self.PAIR_CHUNK_PAIRS)
        own_row = torch.arange(min(chunk, P), dtype=torch.int32, device=self.device) if self.QUERY_BY_ROW else None
        for lo, hi in self._chunks(P, chunk):
            q, inverse = self._chunk_rows(uid, query, lo, hi, True)
            q_row = own_row[:hi - lo] if inverse is None else inverse.to(torch.int32).contiguous()
            check(L.drx_rows_pair_scores(ptr(table), ptr(bias), int(table.shape[0]), ld, self.EPILOGUE, ptr(q), int(q.shape[0]), ptr(q_row),
                                         ptr(t_row[lo:hi]), hi - lo, ptr(out[lo:hi]), stream), 'drx_rows_pair_scores')
        return out
