"""The chunk paths of RowsRecommender's four calls for the engines whose table is computed (DMF: the item tower) or whose query rows
belong to the request row (Caser: one hidden row per (user, last L items)) — what tests/test_gpu_rank_items.py, test_gpu_rank_lists.py
and test_gpu_pair_scores.py exercise through the CDAE engine.  Every comparison is torch.equal: a chunking, an order or a form of the
request changes no bit."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U, N = 120, 3000
KINDS = ['dmf', 'caser']


class _Problem:
    """a small engine of test_gpu_recommend_models' making, exclusions set, and the query arrays of a request's rows (Caser: the same
    `before` for every row of a user, so that equal users are equal rows)"""

    def __init__(self, kind):
        import test_gpu_recommend_models as tm
        rng = np.random.default_rng({'dmf': 41, 'caser': 42}[kind])
        if kind == 'dmf':
            factors = (64, 32)
            dense = tm._dmf_dense(rng, U, N, 20, 60)
            self.eng = tm._dmf_engine(tm._dmf_spread(rng, U, N, factors), dense, factors, True)
            self.before = None
        else:
            L, d = 5, 64
            rows = [np.unique(rng.choice(N, int(rng.integers(5, 61)))) for _ in range(U)]
            self.eng = tm._caser_engine(tm._caser_spread(rng, U, N, L, d), U, N, L, d, tm._csr_of_rows(rows))
            self.before = rng.integers(0, N, (U, L)).astype(np.int32)

    def query(self, uids):
        return () if self.before is None else (self.before[np.asarray(uids)],)


@functools.lru_cache(maxsize=None)
def _problem(kind):
    return _Problem(kind)


@pytest.mark.parametrize('kind', KINDS)
def test_rank_items_in_chunks_of_permuted_pairs(kind):
    import torch
    pb = _problem(kind)
    rng = np.random.default_rng(1)
    P = 150
    uid, items = rng.integers(0, U, P).astype(np.int32), rng.integers(0, N, P).astype(np.int32)
    items[[5, 77]] = [-1, N]
    rank, score = pb.eng.rank_items(uid, *pb.query(uid), items)
    assert rank.dtype == torch.int32 and score.dtype == torch.float32 and tuple(rank.shape) == tuple(score.shape) == (P,)
    assert (rank[[5, 77]] == -1).all() and torch.isneginf(score[[5, 77]]).all() and (rank >= 0).sum() == P - 2
    perm = rng.permutation(P)
    c_rank, c_score = pb.eng.rank_items(uid[perm], *pb.query(uid[perm]), items[perm], chunk_rows=7)
    at = torch.as_tensor(perm).to(rank.device)
    assert torch.equal(c_rank, rank[at]) and torch.equal(c_score, score[at])


@pytest.mark.parametrize('kind', KINDS)
def test_rank_lists_in_chunks_with_empty_chunks(kind):
    import torch
    pb = _problem(kind)
    rng = np.random.default_rng(2)
    R = 321                                                           # a last chunk of ONE row at chunks of 5 and of 64
    row_uid = rng.integers(0, U, R).astype(np.int32)
    row_uid[[0, 1, 200]] = 17                                         # a user owning several rows, in different chunks too
    lists = [np.sort(rng.integers(0, N, int(rng.integers(0, 9)))) for _ in range(R)]
    for r in range(10, 17):                                           # rows 10 .. 14 are a whole chunk of 5 without a target
        lists[r] = lists[r][:0]
    lists[R - 1] = np.sort(rng.integers(0, N, 3))
    indptr = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.int64)
    items = np.concatenate(lists).astype(np.int32)
    assert indptr[15] == indptr[10] and indptr[R] > indptr[R - 1] and R % 5 == 1 and R % 64 == 1
    rank, score = pb.eng.rank_lists(row_uid, *pb.query(row_uid), indptr, items)
    assert rank.dtype == torch.int32 and score.dtype == torch.float32 and tuple(rank.shape) == tuple(score.shape) == (len(items),)
    for chunk in (5, 64):
        c_rank, c_score = pb.eng.rank_lists(row_uid, *pb.query(row_uid), indptr, items, chunk_rows=chunk)
        assert torch.equal(c_rank, rank) and torch.equal(c_score, score), chunk
    pair_uid = np.repeat(row_uid, np.diff(indptr))
    p_rank, p_score = pb.eng.rank_items(pair_uid, *pb.query(pair_uid), items)
    assert torch.equal(p_rank, rank) and torch.equal(p_score, score) and (rank >= 0).all()
    # no target at all, with rows and without
    for uids, ip in ((row_uid[:2], np.zeros(3, np.int64)), (row_uid[:0], np.zeros(1, np.int64))):
        e_rank, e_score = pb.eng.rank_lists(uids, *pb.query(uids), ip, np.zeros(0, np.int32))
        assert (e_rank.dtype, e_score.dtype, tuple(e_rank.shape), tuple(e_score.shape)) == (torch.int32, torch.float32, (0,), (0,))


@pytest.mark.parametrize('kind', KINDS)
def test_pair_scores_in_chunks_are_rank_items_scores(kind):
    import torch
    pb = _problem(kind)
    rng = np.random.default_rng(3)
    P = 300
    uid, items = rng.integers(0, U, P).astype(np.int32), rng.integers(0, N, P).astype(np.int32)
    got = pb.eng.pair_scores(uid, *pb.query(uid), items)
    _, want = pb.eng.rank_items(uid, *pb.query(uid), items, exclude=False)
    assert got.dtype == torch.float32 and tuple(got.shape) == (P,) and torch.isfinite(got).all()
    assert torch.equal(got, want)
    assert torch.equal(pb.eng.pair_scores(uid, *pb.query(uid), items, chunk_pairs=33), got)
    none = np.zeros(0, np.int32)
    empty = pb.eng.pair_scores(none, *pb.query(none), none)
    assert empty.dtype == torch.float32 and tuple(empty.shape) == (0,)


def test_dmf_pair_scores_with_items_outside_the_catalogue():
    import torch
    pb = _problem('dmf')
    rng = np.random.default_rng(4)
    P = 200
    uid, items = rng.integers(0, U, P).astype(np.int32), rng.integers(0, N, P).astype(np.int32)
    clean = pb.eng.pair_scores(uid, items)
    out = rng.choice(P, 20, replace=False)
    mixed = items.copy()
    mixed[out] = np.tile([-1, N], 10)
    inside = torch.ones(P, dtype=torch.bool, device=clean.device)
    inside[torch.as_tensor(out).to(clean.device)] = False
    for chunk in (None, 33):
        got = pb.eng.pair_scores(uid, mixed, chunk_pairs=chunk)
        assert torch.isneginf(got[~inside]).all() and torch.equal(got[inside], clean[inside]), chunk
    allout = pb.eng.pair_scores(uid[:20], mixed[out])
    assert allout.dtype == torch.float32 and tuple(allout.shape) == (20,) and torch.isneginf(allout).all()


def test_dmf_pair_scores_run_the_item_tower_over_the_distinct_items(monkeypatch):
    import torch
    from drecpy_amd import _lib
    pb = _problem('dmf')
    rng = np.random.default_rng(5)
    P = 400
    uid = rng.integers(0, U, P).astype(np.int32)
    items = rng.choice(rng.choice(N, 53, replace=False), P).astype(np.int32)
    items[:3] = [-1, N, N + 7]
    _, want = pb.eng.rank_items(uid, items, exclude=False)
    L, sizes = _lib.lib(), []
    orig = L.drx_dmf_predict

    def counted(D, A, stream):
        sizes.append(int(A._obj.B))
        return orig(D, A, stream)
    monkeypatch.setattr(L, 'drx_dmf_predict', counted)
    got = pb.eng.pair_scores(uid, items)
    n_items, n_users = len(np.unique(items[3:])), len(np.unique(uid))
    assert sizes == [n_items, n_users] and n_items <= 53 < N          # the item tower once, over the distinct items inside — never N
    assert torch.equal(got, want)
    sizes.clear()
    assert torch.equal(pb.eng.pair_scores(uid, items, chunk_pairs=33), want)
    assert sizes[0] == n_items and len(sizes) == 1 + (P + 32) // 33 and N not in sizes
    sizes.clear()
    assert torch.isneginf(pb.eng.pair_scores(uid[:3], items[:3])).all() and sizes == []      # nothing inside: no tower at all


@pytest.mark.parametrize('kind', KINDS)
def test_recommend_in_chunks_of_users_named_twice(kind):
    import torch
    pb = _problem(kind)
    rng = np.random.default_rng(6)
    n = 10
    uids = rng.permutation(np.concatenate([np.arange(U), np.arange(0, U, 3)])).astype(np.int32)       # 160 rows: chunks of 37 end on 12
    idx, val = pb.eng.recommend(uids, *pb.query(uids), n)
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and tuple(idx.shape) == tuple(val.shape) == (len(uids), n)
    c_idx, c_val = pb.eng.recommend(uids, *pb.query(uids), n, chunk_users=37)
    assert torch.equal(c_idx, idx) and torch.equal(c_val, val) and (idx >= 0).all()
    h_idx, h_val, first = c_idx.cpu().numpy(), c_val.cpu().numpy().view(np.uint32), {}
    for r, u in enumerate(uids.tolist()):                             # equal users, equal rows — wherever their chunks put them
        a = first.setdefault(u, r)
        assert np.array_equal(h_idx[r], h_idx[a]) and np.array_equal(h_val[r], h_val[a]), (u, r, a)
    assert len(first) == U
