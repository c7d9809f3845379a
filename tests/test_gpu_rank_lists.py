"""Catalogue ranks of rows that own a LIST of targets: drx_rows_rank_lists (k_rankl_keys / k_rankl_count / k_rankl_finish), the engines'
rank_lists and the routing of RecommenderABC.catalogue_ranks between the list form and the pair form.  Every expected value is exact:
a rank against numpy on test_gpu_rank_items' integer problems (integer logits in [-8, 8], heavy ties) or against the position in a
drx_rows_recommend list, and rank AND score bits against drx_rows_rank_items called with one row per pair.
"""
import os
import sys

import numpy as np
import pytest

import test_gpu_rank_items as base

pytestmark = pytest.mark.gpu

SIGMOID_BIAS, BIAS, CLIP = 0, 1, 2
RANK0, SCORE0 = -7, 7.0                                               # what the outputs hold before a call


def _group(ld):
    from drecpy_amd import _lib
    return int(_lib.lib().drx_rows_rank_lists_group(ld))


def _lists(pb, row_uid, indptr, targets, exclude=True, first_row=0, n_rows=None, scratch_short=0):
    """drx_rows_rank_lists on rows [first_row, first_row + n_rows) of (row_uid, indptr) — launched with indptr + first_row, the offsets
    absolute —; (rank, score) as long as `targets`, RANK0 / SCORE0 where the call wrote nothing; (status, ...) first if scratch_short"""
    import torch
    from drecpy_amd import _lib
    L = _lib.lib()
    row_uid, indptr, targets = np.asarray(row_uid), np.asarray(indptr, np.int64), np.asarray(targets)
    R = len(row_uid) - first_row if n_rows is None else n_rows
    P = int(indptr[first_row + R] - indptr[first_row])
    d_uid, d_ip, d_t = base._dev(row_uid[first_row:first_row + R], np.int32), base._dev(indptr, np.int64), base._dev(targets, np.int32)
    q = pb.q[d_uid.long()].contiguous()
    out_rank = torch.full((len(targets),), RANK0, dtype=torch.int32, device='cuda:0')
    out_score = torch.full((len(targets),), SCORE0, dtype=torch.float32, device='cuda:0')
    sb = int(L.drx_rows_rank_lists_scratch_bytes(R, P, pb.N, pb.ld))
    assert sb > 0
    sc = torch.empty(sb, dtype=torch.uint8, device='cuda:0')
    x = pb.excl if exclude and pb.excl is not None else (None, None)
    rc = L.drx_rows_rank_lists(_lib.ptr(pb.table), _lib.ptr(pb.bias), pb.N, pb.ld, pb.epilogue, _lib.ptr(q), _lib.ptr(d_uid), R,
                               _lib.ptr(d_ip[first_row:]), _lib.ptr(d_t), _lib.ptr(x[0]), _lib.ptr(x[1]), _lib.ptr(out_rank), _lib.ptr(out_score),
                               _lib.ptr(sc), sb - scratch_short, _lib.stream_ptr(torch.device('cuda:0')))
    if scratch_short:
        return rc, out_rank.cpu().numpy(), out_score.cpu().numpy()
    _lib.check(rc, 'drx_rows_rank_lists')
    return out_rank.cpu().numpy(), out_score.cpu().numpy()


def _pairs_of(row_uid, indptr):
    return np.repeat(np.asarray(row_uid), np.diff(indptr))


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


# ---- 1. exact integer problems --------------------------------------------------------------------------------------------------------
def _integer_problem(seed, N, U, ld, epilogue, rows):
    """base._integer_problem's construction with the exclusion rows given by the caller (None: no exclusions)"""
    rng = np.random.default_rng(seed)
    K = 50 if ld == 52 else ld
    table, bias, q = base._integer_parts(rng, N, U, K, ld, epilogue != CLIP)
    z = q.astype(np.float64) @ table.astype(np.float64).T + (0 if bias is None else bias.astype(np.float64))
    score = z if epilogue != CLIP else np.maximum(float(base.FLOOR), z)
    return base._Problem(table, bias, q, rows, epilogue), z, score


def _row_lists(rng, N, R, G):
    """R rows, user r = row r.  Lengths cycle through G, G + 1, 2 G + 3, 0, 1, 2, G - 1 (row 1: G + 1).  Among the targets: items 0 and
    N - 1, two items of one 32-item tile in different halves (33: offset 1, bit 2 clear; 38: offset 6, bit 2 set), several of one
    128-block, duplicates, -1 and N.  Row 1 holds distinct items of the catalogue only (everything else is excluded for it)."""
    lengths = [G, G + 1, 2 * G + 3, 0, 1, 2, G - 1]
    special = [-1, 0, 33, 38, 64, 65, 70, 70, 100, N - 2, N - 1, N]
    rows = []
    for r in range(R):
        n = lengths[r % 7]
        if r == 1:
            t = rng.choice(N, size=n, replace=False)
        else:
            k = min(n, len(special)) if r % 2 == 0 or n > 2 else 0
            t = np.concatenate([rng.permutation(special)[:k], rng.integers(0, N, n - k)])
            if n >= 2:
                t[-1] = t[0]                                          # a duplicate in every row of two or more
        rows.append(np.sort(np.asarray(t, np.int64)))
    indptr = np.concatenate([[0], np.cumsum([len(t) for t in rows])]).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32), rows


@pytest.mark.parametrize('N,ld', [(130, 52), (4097, 128), (257, 256)])       # G = 32, 26 and 4 (three walks for the longest rows)
def test_integer_problems(N, ld):
    R, G = 70, _group(ld)                                             # one tile: the third wave partly filled, the fourth empty
    assert 2 <= G <= 32
    rng = np.random.default_rng(N + ld)
    indptr, targets, lists = _row_lists(rng, N, R, G)
    assert sorted(set(np.diff(indptr).tolist())) == sorted({0, 1, 2, G - 1, G, G + 1, 2 * G + 3})
    row_uid = np.arange(R, dtype=np.int32)
    uid = _pairs_of(row_uid, indptr)
    # two slots in front of the first row and three behind the last belong to no row
    ip2, t2 = indptr + 2, np.concatenate([[5, 6], targets, [7, 8, 9]]).astype(np.int32)
    for epilogue in (SIGMOID_BIAS, BIAS, CLIP):
        for with_rows in (False, True):
            excl = None
            if with_rows:
                excl = [np.sort(rng.choice(N, size=int(rng.integers(0, N // 3 + 1)), replace=False)) for _ in range(R)]
                excl[0] = np.zeros(0, np.int64)
                excl[1] = np.setdiff1d(np.arange(N), lists[1])       # row 1 excludes everything but its targets
            pb, z, score = _integer_problem(N + ld + epilogue, N, R, ld, epilogue, excl)
            rank, val = _lists(pb, row_uid, ip2, t2)
            assert (rank[:2] == RANK0).all() and (rank[-3:] == RANK0).all() and (val[:2] == SCORE0).all() and (val[-3:] == SCORE0).all()
            rank, val = rank[2:-3], val[2:-3]
            want = base._expected_ranks(score, uid, targets, pb.rows)
            bad = np.flatnonzero(rank != want)
            assert len(bad) == 0, (epilogue, with_rows, uid[bad][:5], targets[bad][:5], rank[bad][:5], want[bad][:5])
            outside = (targets < 0) | (targets >= N)
            assert outside.sum() >= 10 and (rank[outside] == -1).all() and np.isneginf(val[outside]).all() and np.isfinite(val[~outside]).all()
            p_rank, p_val = pb.rank(uid, targets)                     # the pair entry point: one row per pair
            assert np.array_equal(rank, p_rank) and _same_bits(val, p_val), (epilogue, with_rows)
            if with_rows:
                r1 = rank[indptr[1]:indptr[2]]
                assert sorted(r1.tolist()) == list(range(len(r1)))    # nothing but row 1's own (distinct) targets is left to count
                assert (rank[uid == 0] == base._expected_ranks(score, uid, targets, None)[uid == 0]).all()
            # a chunk of rows in the middle, launched at its offset: only its slots are written
            c_rank, c_val = _lists(pb, row_uid, indptr, targets, first_row=9, n_rows=40)
            lo, hi = indptr[9], indptr[49]
            assert np.array_equal(c_rank[lo:hi], rank[lo:hi]) and _same_bits(c_val[lo:hi], val[lo:hi])
            assert (c_rank[:lo] == RANK0).all() and (c_rank[hi:] == RANK0).all() and (c_val[:lo] == SCORE0).all() and (c_val[hi:] == SCORE0).all()


def test_integer_problem_whose_splits_span_several_blocks():
    N, ld, R, T = 33_100, 64, 3, 16                                   # 259 blocks for 256 splits: two blocks a split, the last one partial
    rng = np.random.default_rng(2)
    lists = [np.sort(np.concatenate([[0, 255, 256, N - 1], rng.integers(0, N, T - 4)])) for _ in range(R)]
    indptr, targets = np.arange(R + 1, dtype=np.int64) * T, np.concatenate(lists).astype(np.int32)
    row_uid = np.arange(R, dtype=np.int32)
    uid = _pairs_of(row_uid, indptr)
    for epilogue in (SIGMOID_BIAS, BIAS, CLIP):
        excl = [np.sort(rng.choice(N, size=n, replace=False)) for n in (0, 5000, 11)]
        pb, z, score = _integer_problem(7 + epilogue, N, R, ld, epilogue, excl)
        rank, val = _lists(pb, row_uid, indptr, targets)
        assert rank.tolist() == base._expected_ranks(score, uid, targets, pb.rows).tolist(), epilogue
        p_rank, p_val = pb.rank(uid, targets)
        assert np.array_equal(rank, p_rank) and _same_bits(val, p_val), epilogue


# ---- 2. a float problem against the selector ------------------------------------------------------------------------------------------
def _float_problem():
    rng = np.random.default_rng(23)
    N, U, K, ld = 1000, 200, 50, 52
    table, q = np.zeros((N, ld), np.float32), np.zeros((U, ld), np.float32)
    table[:, :K] = rng.normal(0, 2.0 / np.sqrt(K), (N, K))
    q[:, :K] = rng.normal(0, 0.5, (U, K))
    bias = rng.normal(0, 0.3, N).astype(np.float32)
    rows = [np.sort(rng.choice(N, size=int(rng.integers(5, 61)), replace=False)) for _ in range(U)]
    return base._Problem(table, bias, q, rows, SIGMOID_BIAS), rng


def test_the_rank_is_the_position_in_the_selectors_list():
    pb, rng = _float_problem()
    U, n = 200, 128                                                   # two tiles of rows
    users = np.arange(U, dtype=np.int32)
    idx, val = pb.lists(users, n)
    assert (idx >= 0).all()
    where = np.stack([np.sort(rng.choice(n, size=4, replace=False)) for _ in range(U)])      # four listed items per row
    listed = np.take_along_axis(idx, where, axis=1)
    other = rng.integers(0, pb.N, (U, 4))
    both = np.concatenate([listed, other], axis=1)
    order = np.argsort(both, axis=1, kind='stable')
    targets = np.take_along_axis(both, order, axis=1).reshape(-1).astype(np.int32)
    from_list = (order < 4).reshape(-1)
    want_pos = np.take_along_axis(np.concatenate([where, np.full((U, 4), -1)], axis=1), order, axis=1).reshape(-1)
    want_val = np.take_along_axis(np.concatenate([np.take_along_axis(val, where, axis=1), np.zeros((U, 4), np.float32)], axis=1), order,
                                  axis=1).reshape(-1)
    indptr = np.arange(U + 1, dtype=np.int64) * 8
    rank, score = _lists(pb, users, indptr, targets)
    assert rank[from_list].tolist() == want_pos[from_list].tolist()
    assert _same_bits(score[from_list], want_val[from_list])
    p_rank, p_score = pb.rank(np.repeat(users, 8), targets)
    assert np.array_equal(rank, p_rank) and _same_bits(score, p_score)


# ---- 3. a function of the inputs alone ------------------------------------------------------------------------------------------------
def test_rows_permuted_and_rows_cut_in_two_give_the_same():
    N, ld, R = 4097, 128, 70
    G = _group(ld)
    rng = np.random.default_rng(41)
    indptr, targets, lists = _row_lists(rng, N, R, G)
    excl = [np.sort(rng.choice(N, size=int(rng.integers(0, 500)), replace=False)) for _ in range(R)]
    pb, z, score = _integer_problem(3, N, R, ld, SIGMOID_BIAS, excl)
    row_uid = np.arange(R, dtype=np.int32)
    rank, val = _lists(pb, row_uid, indptr, targets)
    again = _lists(pb, row_uid, indptr, targets)
    assert np.array_equal(rank, again[0]) and _same_bits(val, again[1])
    perm = rng.permutation(R)
    p_ip = np.concatenate([[0], np.cumsum([len(lists[r]) for r in perm])]).astype(np.int64)
    p_rank, p_val = _lists(pb, row_uid[perm], p_ip, np.concatenate([lists[r] for r in perm]).astype(np.int32))
    for j, r in enumerate(perm):
        assert np.array_equal(p_rank[p_ip[j]:p_ip[j + 1]], rank[indptr[r]:indptr[r + 1]]), r
        assert _same_bits(p_val[p_ip[j]:p_ip[j + 1]], val[indptr[r]:indptr[r + 1]]), r
    # rows cut into two or three rows of the same user: the same targets, the same slots
    cut_uid, cut_ip = [], [0]
    for r in range(R):
        n = len(lists[r])
        for part in ([n] if n < 2 else [n // 2, n - n // 2] if n < 6 else [n // 3, n // 3, n - 2 * (n // 3)]):
            cut_uid.append(r)
            cut_ip.append(cut_ip[-1] + part)
    assert len(cut_uid) > 128                                         # (and a second tile of rows)
    c_rank, c_val = _lists(pb, np.array(cut_uid, np.int32), np.array(cut_ip, np.int64), targets)
    assert np.array_equal(c_rank, rank) and _same_bits(c_val, val)


def test_engine_chunkings_and_calls_give_the_same():
    import torch
    eng = base._cdae_engine()                                         # 90 users, 6000 items, K = 50
    rng = np.random.default_rng(6)
    row_uid = rng.integers(0, 90, 150).astype(np.int32)
    lists = [np.sort(rng.integers(0, 6000, int(rng.integers(0, 9)))) for _ in row_uid]
    indptr = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.int64)
    items = np.concatenate(lists).astype(np.int32)
    a_rank, a_score = eng.rank_lists(row_uid, indptr, items)
    assert a_rank.dtype == torch.int32 and a_score.dtype == torch.float32 and tuple(a_rank.shape) == tuple(a_score.shape) == (len(items),)
    for chunk in (64, 16_384):
        b_rank, b_score = eng.rank_lists(row_uid, indptr, items, chunk_rows=chunk)
        assert torch.equal(a_rank, b_rank) and torch.equal(a_score, b_score), chunk
    p_rank, p_score = eng.rank_items(_pairs_of(row_uid, indptr), items)
    assert torch.equal(a_rank, p_rank) and torch.equal(a_score, p_score)
    e_rank, e_score = eng.rank_lists(np.zeros(2, np.int32), np.zeros(3, np.int64), np.zeros(0, np.int32))
    assert e_rank.numel() == 0 and e_score.numel() == 0
    assert eng.rank_lists_group(eng.rank_ld()) == _group(eng.ld) and eng.rank_lists_group(260) == 0


# ---- 4. the scratch -------------------------------------------------------------------------------------------------------------------
def test_scratch():
    from drecpy_amd import _lib
    L = _lib.lib()
    need = int(L.drx_rows_rank_lists_scratch_bytes(128, 1280, 100_000, 128))
    assert need > 0 and need == int(L.drx_rows_rank_lists_scratch_bytes(128, 1280, 1_000_000, 128))
    assert int(L.drx_rows_rank_lists_scratch_bytes(128, 1280, 1_000_000, 260)) == 0 and _group(260) == 0
    # per target: two words and the partial counts of the splits, no row of n_items scores
    assert int(L.drx_rows_rank_lists_scratch_bytes(16_384, 163_840, 1_000_000, 128)) < 163_840 * 64
    pb, z, score = _integer_problem(1, 130, 4, 52, BIAS, None)
    indptr, targets = np.array([0, 2, 2, 5, 6], np.int64), np.array([1, 7, 0, 64, 129, 3], np.int32)
    rc, rank, val = _lists(pb, np.arange(4), indptr, targets, scratch_short=1)
    assert rc == -2 and (rank == RANK0).all() and (val == SCORE0).all()      # DRX_ESCRATCH, nothing written
    rank, _ = _lists(pb, np.arange(4), indptr, targets)
    assert rank.tolist() == base._expected_ranks(score, _pairs_of(np.arange(4), indptr), targets, None).tolist()
    rank, val = _lists(pb, np.arange(4), np.full(5, 3, np.int64), targets)   # no target at all: DRX_OK, nothing written
    assert (rank == RANK0).all() and (val == SCORE0).all()


# ---- 5. the public layer on fitted models ---------------------------------------------------------------------------------------------
class _Spy:
    """the two entry points of the library, counted"""

    def __init__(self, monkeypatch):
        from drecpy_amd import _lib
        L = _lib.lib()
        self.calls = {'drx_rows_rank_lists': 0, 'drx_rows_rank_items': 0}
        for name in self.calls:
            monkeypatch.setattr(L, name, self._counted(name, getattr(L, name)))

    def _counted(self, name, fn):
        def call(*args):
            self.calls[name] += 1
            return fn(*args)
        return call

    def take(self):
        got = (self.calls['drx_rows_rank_lists'], self.calls['drx_rows_rank_items'])
        self.calls = dict.fromkeys(self.calls, 0)
        return got


@pytest.mark.parametrize('kind', ['cdae', 'cdae_sampled', 'dmf', 'caser'])
def test_catalogue_ranks_take_the_list_form(kind, monkeypatch):
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Evaluation import recommendation_evaluation
    from drecpy_amd.engine import RowsRecommender
    model, frame = base._fitted(kind)
    eng = model._engine
    G = eng.rank_lists_group(eng.rank_ld())
    assert 2 <= G <= 32
    rng = np.random.default_rng(9)
    raw_users = [int(u) for u in rng.permutation(np.arange(1000, 1060))[:12]] + [1060]       # 1060 has recorded the whole catalogue
    users, items = base._test_pairs(model, frame, raw_users, rng)                             # 40 items and an unknown one per user
    long_user = raw_users[3]
    more = [70000 + int(i) for i in rng.choice(600, size=2 * G + 3 - 41, replace=False)]     # (may repeat a pair: duplicates are allowed)
    users, items = users + [long_user] * len(more), items + more
    assert users.count(long_user) == 2 * G + 3
    spy = _Spy(monkeypatch)
    n = 128
    lists = model.recommend_batch(raw_users, n=n)
    ranks, scores = model.catalogue_ranks(users, items, return_scores=True)
    assert spy.take() == (1, 0)                                       # one launch of the list form, none of the pair form
    base._check_against_lists(model, frame, raw_users, lists, users, items, ranks, scores, n)
    assert (ranks[np.asarray(users) == 1060] == -1).all()
    # one pair per user: the pair form
    one_u, one_i = raw_users[:8], [70000 + int(i) for i in rng.choice(600, size=8, replace=False)]
    one = model.catalogue_ranks(one_u, one_i)
    assert spy.take() == (0, 1)
    # either route forced: equal arrays
    for novelty in (True, False):
        monkeypatch.setattr(RowsRecommender, 'RANK_LISTS_MIN_MEAN', 0.0)
        a = model.catalogue_ranks(users, items, novelty=novelty, return_scores=True)
        a1 = model.catalogue_ranks(one_u, one_i, novelty=novelty)
        assert spy.take() == (2, 0)
        monkeypatch.setattr(RowsRecommender, 'RANK_LISTS_MIN_MEAN', float('inf'))
        b = model.catalogue_ranks(users, items, novelty=novelty, return_scores=True)
        b1 = model.catalogue_ranks(one_u, one_i, novelty=novelty)
        assert spy.take() == (0, 2)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a1, b1)
        if novelty:
            assert np.array_equal(a[0], ranks) and np.array_equal(a[1], scores) and np.array_equal(a1, one)
    monkeypatch.undo()
    # the evaluation rebuilt from ranks (several held-out items per user: the list form) equals the one from lists, dict for dict
    spy = _Spy(monkeypatch)
    tu, ti, tv = [], [], []
    for u, a in zip(raw_users[:12], lists):
        mine = [i for uu, i in zip(frame['user'].tolist(), frame['item'].tolist()) if uu == u]
        held = [a[j][1] for j in rng.permutation(12)[:4]] + (70000 + rng.choice(600, size=4, replace=False)).tolist() + [mine[0], 5]
        for i in dict.fromkeys(int(x) for x in held):
            tu.append(u)
            ti.append(i)
            tv.append(int(rng.integers(1, 6)))
    ds_te = InteractionDataset.read_df({'user': np.array(tu), 'item': np.array(ti), 'interaction': np.array(tv)}, verbose=False)
    for kw in (dict(k=[1, 5, 10]), dict(k=[1, 5, 10], n_pos_interactions=2, seed=4)):
        a = recommendation_evaluation(model, ds_te, novelty=True, verbose=False, batched=True, **kw)
        assert spy.take() == (0, 0)
        b = recommendation_evaluation(model, ds_te, novelty=True, verbose=False, batched='ranks', **kw)
        got = spy.take()
        assert got[0] >= 1 and got[1] == 0, got
        assert a == b and a and any(v > 0 for v in a.values()), (a, b)


def test_caser_short_sequences_and_a_dmf_subclass_keep_the_default(monkeypatch):
    """with several pairs per user (the list form's domain) the default hook still answers a Caser user whose sequence is shorter than
    L and a DMF subclass with its own prediction hooks"""
    import test_gpu_recommend_models as tm
    model, frame = base._fitted('caser')
    short = model.interaction_dataset.user_to_uid(1061)
    assert len(model._user_sequence(short)) == 2 < model.L
    counter = tm._Counter(monkeypatch, skip=(short,))
    spy = _Spy(monkeypatch)
    users = [1003, 1061, 1004, 1061, 1003, 1003, 1004, 1061]
    items = [70010, 70011, 70012, 70013, 70400, 70002, 70300, 70001]
    ranks = model.catalogue_ranks(users, items)
    assert counter.calls == [short] and spy.take() == (1, 0)          # the short user once by the default, the others in one list launch
    counter.calls.clear()
    want = {u: {i: p for p, (_, i) in enumerate(model.recommend_batch([u], n=128)[0])} for u in (1003, 1004)}
    for r, i, u in zip(ranks.tolist(), items, users):
        assert r == -1 if u == 1061 else (r == want[u][i] if i in want[u] else (r >= 128 or r == -1)), (u, i, r)
    counter.calls.clear()

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))
    try:
        from extending_recommender_dmf import ModifiedDMF
    finally:
        sys.path.pop(0)
    modified, frame = base._fitted('dmf', cls=ModifiedDMF, epochs=2)
    few = [1002, 1017, 1002, 1040]
    rng = np.random.default_rng(6)
    users = [u for u in few for _ in range(30)]
    items = [70000 + int(i) for _ in few for i in rng.choice(600, size=30, replace=False)]
    ranks, scores = modified.catalogue_ranks(users, items, return_scores=True)
    assert sorted(counter.calls) == sorted(modified.interaction_dataset.user_to_uid(u) for u in set(few)) and spy.take() == (0, 0)
    own = {u: {i: (p, s) for p, (s, i) in enumerate(modified.recommend(u, n=None))} for u in set(few)}
    for u, i, r, s in zip(users, items, ranks.tolist(), scores.tolist()):
        assert (r, s) == own[u].get(i, (-1, -np.inf)), (u, i, r)
