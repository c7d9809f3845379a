"""Catalogue ranks of given (row, item) pairs: drx_rows_rank_items (k_rank_keys / k_rank_count / k_rank_finish), the engines'
rank_items, RecommenderABC.catalogue_ranks and recommendation_evaluation(batched='ranks').  Every expected value is exact:

  1. integer problems (table in {-1, 0, 1}, six +-1 per query row, integer biases): every logit is an integer in [-8, 8] whatever the
     summation order, so the expected rank is computed in numpy from (z, item); checked here on the CPU: the fp32 sigmoids of
     neighbouring integer logits differ by >= 5.7e-4 relative (the score order is the logit order) and the catalogue holds at most 17
     distinct values (heavy ties, decided by the larger item index);
  2. float problems: the position p of an item in a drx_rows_recommend list IS its rank, and the list's value its score, bit for bit;
     an eligible item outside a list of 128 has a rank >= 128;
  3. the public layer against recommend_batch(n = 128) on fitted models, and the evaluation from ranks against the one from lists.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIGMOID_BIAS, BIAS, CLIP = 0, 1, 2
FLOOR = np.float32(1e-6)


# ---- the two entry points, called directly -------------------------------------------------------------------------------------------
def _dev(a, dtype):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to('cuda:0')


class _Problem:
    """table [N, ld], bias [N] or None, one query row per user q [U, ld] (padding columns zero), excluded items per user or None"""

    def __init__(self, table, bias, q, rows, epilogue):
        self.N, self.ld = table.shape
        self.epilogue, self.rows = epilogue, rows
        self.table, self.bias, self.q = _dev(table, np.float32), (None if bias is None else _dev(bias, np.float32)), _dev(q, np.float32)
        self.excl = None
        if rows is not None:
            ip = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
            ix = np.concatenate([np.asarray(r, np.int32) for r in rows] + [np.zeros(0, np.int32)])
            self.excl = (_dev(ip, np.int64), _dev(ix if len(ix) else np.zeros(1, np.int32), np.int32))

    def rank(self, uid, target, exclude=True):
        import torch
        from drecpy_amd import _lib
        L = _lib.lib()
        uid, target = np.asarray(uid), np.asarray(target)
        P = len(uid)
        d_uid, d_t = _dev(uid, np.int32), _dev(target, np.int32)
        q = self.q[d_uid.long()].contiguous()
        out_rank = torch.full((P,), -7, dtype=torch.int32, device='cuda:0')
        out_score = torch.full((P,), 7.0, dtype=torch.float32, device='cuda:0')
        sb = int(L.drx_rows_rank_items_scratch_bytes(P, self.N, self.ld))
        assert sb > 0
        sc = torch.empty(sb, dtype=torch.uint8, device='cuda:0')
        x = self.excl if exclude and self.excl is not None else (None, None)
        _lib.check(L.drx_rows_rank_items(_lib.ptr(self.table), _lib.ptr(self.bias), self.N, self.ld, self.epilogue, _lib.ptr(q), _lib.ptr(d_uid),
                                         _lib.ptr(d_t), P, _lib.ptr(x[0]), _lib.ptr(x[1]), _lib.ptr(out_rank), _lib.ptr(out_score), _lib.ptr(sc), sb,
                                         _lib.stream_ptr(torch.device('cuda:0'))), 'drx_rows_rank_items')
        return out_rank.cpu().numpy(), out_score.cpu().numpy()

    def lists(self, uid, n, exclude=True):
        import torch
        from drecpy_amd import _lib
        L = _lib.lib()
        R = len(uid)
        d_uid = _dev(uid, np.int32)
        q = self.q[d_uid.long()].contiguous()
        out_idx = torch.empty(R, n, dtype=torch.int32, device='cuda:0')
        out_val = torch.empty(R, n, dtype=torch.float32, device='cuda:0')
        sb = int(L.drx_rows_recommend_scratch_bytes(R, self.N, self.ld, n))
        sc = torch.empty(sb, dtype=torch.uint8, device='cuda:0')
        x = self.excl if exclude and self.excl is not None else (None, None)
        _lib.check(L.drx_rows_recommend(_lib.ptr(self.table), _lib.ptr(self.bias), self.N, self.ld, self.epilogue, _lib.ptr(q), _lib.ptr(d_uid), R, n,
                                        _lib.ptr(x[0]), _lib.ptr(x[1]), _lib.ptr(out_idx), _lib.ptr(out_val), _lib.ptr(sc), sb,
                                        _lib.stream_ptr(torch.device('cuda:0'))), 'drx_rows_recommend')
        return out_idx.cpu().numpy(), out_val.cpu().numpy()


# ---- 1. exact integer problems --------------------------------------------------------------------------------------------------------
def _sigmoid32(z):
    return (np.float32(1) / (np.float32(1) + np.exp(-z.astype(np.float32)))).astype(np.float32)


def test_the_integer_construction_on_the_cpu():
    """what the expectations below rest on (no device involved)"""
    s = _sigmoid32(np.arange(-8, 9)).astype(np.float64)
    gap = float(((s[1:] - s[:-1]) / s[1:]).min())
    print('smallest relative gap between the fp32 sigmoids of neighbouring integer logits:', gap)
    # 5.76e-4, between the logits 7 and 8 (5.8e-4 rounded): 250 times the 2.2e-6 that two roundings of expf (1e-6 relative each,
    # rec_logit_bound's assumption) and of the fp32 quotient could move two scores towards each other
    assert 5.7e-4 <= gap < 5.8e-4
    rng = np.random.default_rng(0)
    table, bias, q = _integer_parts(rng, 4097, 3, 128, 128, True)
    z = q.astype(np.float64) @ table.astype(np.float64).T + bias
    assert (z == np.rint(z)).all() and np.abs(z).max() <= 8 and len(np.unique(z)) <= 17 and len(np.unique(z[0])) >= 9


def _integer_parts(rng, N, U, K, ld, with_bias):
    table = np.zeros((N, ld), np.float32)
    table[:, :K] = rng.integers(-1, 2, (N, K))
    q = np.zeros((U, ld), np.float32)
    for u in range(U):
        q[u, rng.choice(K, 6, replace=False)] = rng.choice([-1.0, 1.0], 6)
    bias = rng.integers(-2, 3, N).astype(np.float32) if with_bias else None
    return table, bias, q


def _integer_problem(seed, N, U, ld, epilogue, with_rows, t1=None):
    """rows (where asked for): user 0 excludes nothing, user 1 everything but its one target t1, the others ordinary rows (which may
    hold a pair's target: the target's own exclusion is ignored)"""
    rng = np.random.default_rng(seed)
    K = 50 if ld == 52 else ld
    table, bias, q = _integer_parts(rng, N, U, K, ld, epilogue != CLIP)
    z = q.astype(np.float64) @ table.astype(np.float64).T + (0 if bias is None else bias.astype(np.float64))
    score = z if epilogue != CLIP else np.maximum(float(FLOOR), z)      # (sigmoid: the logit orders as its fp32 score does)
    rows = None
    if with_rows:
        rows = [np.sort(rng.choice(N, size=int(rng.integers(0, max(1, N // 3) + 1)), replace=False)) for _ in range(U)]
        rows[0] = np.zeros(0, np.int64)
        if U > 1:
            rows[1] = np.setdiff1d(np.arange(N), [t1])
    return _Problem(table, bias, q, rows, epilogue), z, score


def _expected_ranks(score, uid, target, rows):
    N = score.shape[1]
    items = np.arange(N)
    want = np.empty(len(uid), np.int64)
    for p, (u, t) in enumerate(zip(uid, target)):
        if not 0 <= t < N:
            want[p] = -1
            continue
        s = score[u]
        ahead = (s > s[t]) | ((s == s[t]) & (items > t))
        if rows is not None:
            ahead[rows[u]] = False
        want[p] = int(ahead.sum())
    return want


def _expected_scores(z, uid, target, epilogue):
    zt = np.array([z[u, t] if 0 <= t < z.shape[1] else -np.inf for u, t in zip(uid, target)])
    return np.maximum(FLOOR, zt.astype(np.float32)) if epilogue == CLIP else zt.astype(np.float32)


def _pairs(rng, N, U, P, t1):
    """targets: item 0, N - 1, the first and last item of a 128-block, then random ones; user 1 only ever asks for t1"""
    fixed = [0, N - 1, 127, 128, (N - 1) // 128 * 128, N // 2]
    target = np.array([t for t in fixed if 0 <= t < N][:P] + rng.integers(0, N, max(0, P - 6)).tolist())[:P]
    target = np.resize(target, P)
    uid = rng.integers(0, U, P)
    target[uid == 1] = t1
    return uid.astype(np.int32), target.astype(np.int32)


@pytest.mark.parametrize('ld', [52, 128])
@pytest.mark.parametrize('N', [1, 31, 33, 128, 129, 257, 4097])
def test_integer_problems(N, ld):
    U = 9
    rng = np.random.default_rng(N * 1000 + ld)
    t1 = N // 2
    for epilogue in (SIGMOID_BIAS, BIAS, CLIP):
        for with_rows in (False, True):
            pb, z, score = _integer_problem(N + ld + epilogue, N, U, ld, epilogue, with_rows, t1)
            for P in (1, 3, 65, 130):
                uid, target = _pairs(rng, N, U, P, t1)
                rank, val = pb.rank(uid, target)
                want = _expected_ranks(score, uid, target, pb.rows)
                assert rank.tolist() == want.tolist(), (epilogue, with_rows, P, uid[rank != want][:5], target[rank != want][:5])
                if epilogue != SIGMOID_BIAS:
                    assert np.array_equal(val, _expected_scores(z, uid, target, epilogue)), (epilogue, P)
                if with_rows:
                    assert (rank[uid == 0] == _expected_ranks(score, uid, target, None)[uid == 0]).all()      # the empty row excludes nothing
                    assert (rank[uid == 1] == 0).all()                                                       # nothing but the target is left
            if N <= 130:                                              # one user, every item of the catalogue as target
                for u in (2, 1) if with_rows else (2,):
                    uid, target = np.full(N, u, np.int32), np.arange(N, dtype=np.int32)
                    rank, _ = pb.rank(uid, target)
                    assert rank.tolist() == _expected_ranks(score, uid, target, pb.rows).tolist(), (epilogue, with_rows, u)
                    if not with_rows:
                        assert sorted(rank.tolist()) == list(range(N))                                       # a permutation: the keys are unique


def test_integer_problem_whose_splits_span_several_blocks_and_targets_outside_the_catalogue():
    N, U, ld = 76801, 4, 128
    for epilogue in (SIGMOID_BIAS, BIAS, CLIP):
        pb, z, score = _integer_problem(5 + epilogue, N, U, ld, epilogue, True, N // 2)
        uid = np.array([2, 3, 0], np.int32)
        target = np.array([N - 1, 38400, 12345], np.int32)
        rank, _ = pb.rank(uid, target)
        assert rank.tolist() == _expected_ranks(score, uid, target, pb.rows).tolist(), epilogue
        uid = np.array([2, 1, 3, 0, 2], np.int32)
        target = np.array([-1, N // 2, N, 2_000_000_000, 77], np.int32)
        rank, val = pb.rank(uid, target)
        assert rank.tolist() == _expected_ranks(score, uid, target, pb.rows).tolist() and rank[[0, 2, 3]].tolist() == [-1, -1, -1]
        assert np.isneginf(val[[0, 2, 3]]).all() and np.isfinite(val[[1, 4]]).all()


# ---- 2. against the selector on float problems ----------------------------------------------------------------------------------------
def _float_problem(name):
    rng = np.random.default_rng(17)
    N, U = 5000, 65
    rows = [np.sort(rng.choice(N, size=int(rng.integers(5, 61)), replace=False)) for _ in range(U)]
    if name in ('sigmoid', 'saturated'):
        K, ld, epilogue = 50, 52, SIGMOID_BIAS
    elif name in ('bias', 'duplicates'):
        K, ld, epilogue = 128, 128, BIAS
    else:
        K, ld, epilogue = 64, 64, CLIP
    table, q = np.zeros((N, ld), np.float32), np.zeros((U, ld), np.float32)
    table[:, :K] = rng.normal(0, 2.0 / np.sqrt(K), (N, K))
    q[:, :K] = rng.normal(0, 0.5, (U, K))
    bias = rng.normal(0, 0.3, N).astype(np.float32)
    if name == 'saturated':                                           # many scores of exactly 1.0f, tiny ones at the other end
        bias[:] = -40.0
        bias[rng.choice(N, size=500, replace=False)] = 40.0
    if name == 'duplicates':                                          # byte-equal rows (and biases) across tile, block and split boundaries
        for d in [1, 31, 32, 33, 127, 128, 129, 2047, 2048] * 30:
            s = int(rng.integers(0, N - d))
            table[s + d], bias[s + d] = table[s], bias[s]
    if epilogue == CLIP:
        table /= np.linalg.norm(table, axis=1, keepdims=True)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        bias = None
        if name == 'dmf_floor':                                       # 60 live items: every list of 128 reaches down into the floor
            dead = np.setdiff1d(np.arange(N), rng.choice(N, size=60, replace=False))
            table[dead] = 0.0
    return _Problem(table, bias, q, rows, epilogue)


@pytest.mark.parametrize('name', ['sigmoid', 'bias', 'clip', 'saturated', 'duplicates', 'dmf_floor'])
def test_the_rank_is_the_position_in_the_selectors_list(name):
    pb = _float_problem(name)
    U, n = pb.q.shape[0], 128
    users = np.arange(U, dtype=np.int32)
    idx, val = pb.lists(users, n)
    assert (idx >= 0).all()
    uid, target = np.repeat(users, n), idx.reshape(-1)
    rank, score = pb.rank(uid, target)
    assert rank.tolist() == np.tile(np.arange(n), U).tolist(), np.flatnonzero(rank != np.tile(np.arange(n), U))[:10]
    assert np.array_equal(score.view(np.uint32), val.reshape(-1).view(np.uint32))
    if name == 'saturated':
        assert (val == 1.0).sum() > U * 8
    if name == 'duplicates':
        assert (val[:, 1:] == val[:, :-1]).sum() > 20
    if name == 'dmf_floor':
        assert (val[:, -1] == FLOOR).all() and (val[:, 0] > FLOOR).all()
    rng = np.random.default_rng(3)
    uid, target = [], []
    while len(uid) < 200:                                             # unlisted eligible items
        u, t = int(rng.integers(0, U)), int(rng.integers(0, pb.N))
        if t not in pb.rows[u] and t not in idx[u]:
            uid.append(u)
            target.append(t)
    rank, _ = pb.rank(np.array(uid), np.array(target))
    assert (rank >= n).all()
    # without the exclusions: the same against the lists without them
    idx0, val0 = pb.lists(users[:3], n, exclude=False)
    rank, score = pb.rank(np.repeat(users[:3], n), idx0.reshape(-1), exclude=False)
    assert rank.tolist() == np.tile(np.arange(n), 3).tolist() and np.array_equal(score, val0.reshape(-1))


# ---- 3. determinism (through an engine: its chunked launch) ---------------------------------------------------------------------------
def _cdae_engine(U=90, N=6000, K=50, seed=22):
    from test_gpu_recommend import _engine, _histories, _spread_params
    rng = np.random.default_rng(seed)
    p = _spread_params(rng, U, N, K)
    indptr, indices = _histories(rng, U, N)
    return _engine(p, indptr, indices, (indptr, indices))


def test_bit_identical_between_calls_orders_and_chunkings():
    import torch
    eng = _cdae_engine()
    rng = np.random.default_rng(5)
    P = 300
    uid, items = rng.integers(0, 90, P).astype(np.int32), rng.integers(0, 6000, P).astype(np.int32)
    a_rank, a_score = eng.rank_items(uid, items)
    b_rank, b_score = eng.rank_items(uid, items)
    assert a_rank.dtype == torch.int32 and a_score.dtype == torch.float32 and tuple(a_rank.shape) == tuple(a_score.shape) == (P,)
    assert torch.equal(a_rank, b_rank) and torch.equal(a_score, b_score)
    perm = rng.permutation(P)
    c_rank, c_score = eng.rank_items(uid[perm], items[perm], chunk_rows=7)
    inv = torch.as_tensor(np.argsort(perm)).to(eng.device)
    assert torch.equal(a_rank, c_rank[inv]) and torch.equal(a_score, c_score[inv])
    d_rank, d_score = eng.rank_items(uid[:5], items[:5])              # other neighbours in the tile, another split count
    assert torch.equal(a_rank[:5], d_rank) and torch.equal(a_score[:5], d_score)
    # and the engine's answer is the position in its own recommend()
    users = np.arange(20, dtype=np.int32)
    idx, val = eng.recommend(users, 50)
    rank, score = eng.rank_items(np.repeat(users, 50), idx.reshape(-1))
    assert rank.cpu().tolist() == np.tile(np.arange(50), 20).tolist() and torch.equal(score, val.reshape(-1))
    e_rank, e_score = eng.rank_items(np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert e_rank.numel() == 0 and e_score.numel() == 0
    assert eng.rank_is_fused(eng.ld) and eng.rank_is_fused(256) and not eng.rank_is_fused(260)


# ---- 4. a long catalogue --------------------------------------------------------------------------------------------------------------
def test_long_catalogue_and_scratch_does_not_grow_with_it():
    import torch
    from drecpy_amd import _lib
    N, K, P, U = 1_000_000, 128, 128, 12
    L = _lib.lib()
    need = int(L.drx_rows_rank_items_scratch_bytes(P, N, K))
    assert 0 < need < 1_000_000
    assert int(L.drx_rows_rank_items_scratch_bytes(P, 2_000_000_000, K)) <= need
    assert int(L.drx_rows_rank_items_scratch_bytes(P, N, 260)) == 0
    gen = torch.Generator(device='cuda:0')
    gen.manual_seed(11)
    pb = _Problem(np.zeros((1, K), np.float32), np.zeros(1, np.float32), np.random.default_rng(1).normal(0, 0.5, (U, K)),
                  [np.arange(u, N, 1000 + u) for u in range(U)], SIGMOID_BIAS)
    pb.N = N
    pb.table = torch.randn(N, K, generator=gen, device='cuda:0') * (2.0 / np.sqrt(K))
    pb.bias = torch.randn(N, generator=gen, device='cuda:0') * 0.3
    users = np.arange(U, dtype=np.int32)
    idx, val = pb.lists(users, 10)
    extra = np.array([0, N - 1, 999_936, 524_288, 7, 123_456, N, -5], np.int32)
    uid = np.concatenate([np.repeat(users, 10), np.arange(8, dtype=np.int32)])
    target = np.concatenate([idx.reshape(-1), extra])
    assert len(uid) == P
    rank, score = pb.rank(uid, target)
    assert rank[:120].tolist() == np.tile(np.arange(10), U).tolist() and np.array_equal(score[:120], val.reshape(-1))
    assert (rank[120:126] >= 0).all() and (rank[120:126] < N).all() and rank[126:].tolist() == [-1, -1]


# ---- 5. the public layer on fitted models ---------------------------------------------------------------------------------------------
def _fitted(kind, **kw):
    import test_gpu_recommend_models as tm
    if kind in ('dmf', 'caser'):
        return tm._fitted(kind, **kw)
    from test_gpu_recommend import _spread_params
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender import CDAE
    frame = tm._frame(31)                                             # 60 users (+ one with every item, one with two), 600 items
    ds = InteractionDataset.read_df(frame, verbose=False)
    U, N = len(set(frame['user'].tolist())), len(set(frame['item'].tolist()))
    mode = dict(mode='sampled') if kind == 'cdae_sampled' else {}
    model = CDAE(hidden_factors=50, seed=5, verbose=False, interaction_threshold=3, **mode)
    model.fit(ds, epochs=4, batch_size=16 if not mode else 256, learning_rate=1e-3, initial_weights=_spread_params(np.random.default_rng(5), U, N, 50))
    return model, frame


def _test_pairs(model, frame, raw_users, rng, per_user=40):
    """(users, items) raw: per user random items of the catalogue (recorded ones among them) and an unknown item"""
    users, items = [], []
    for u in raw_users:
        for i in rng.choice(600, size=per_user, replace=False):
            users.append(u)
            items.append(70000 + int(i))
        users.append(u)
        items.append(5)
    return users, items


def _check_against_lists(model, frame, raw_users, lists, users, items, ranks, scores, n):
    recorded = {(int(u), int(i)) for u, i in zip(frame['user'], frame['item'])}
    place = [{item: (p, s) for p, (s, item) in enumerate(a)} for a in lists]
    row_of = {u: j for j, u in enumerate(raw_users)}
    seen = {'listed': 0, 'beyond': 0, 'excluded': 0, 'unknown': 0}
    for u, i, r, s in zip(users, items, ranks.tolist(), scores.tolist()):
        hit = place[row_of[u]].get(i)
        if hit is not None:
            assert (r, s) == hit, (u, i, r, hit)
            seen['listed'] += 1
        elif i == 5:
            assert r == -1 and s == -np.inf
            seen['unknown'] += 1
        elif (u, i) in recorded:
            assert r == -1 and s == -np.inf, (u, i, r)
            seen['excluded'] += 1
        else:
            assert r >= n and np.isfinite(s), (u, i, r)
            seen['beyond'] += 1
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize('kind', ['cdae', 'cdae_sampled', 'dmf', 'caser'])
def test_catalogue_ranks_on_a_fitted_model(kind, monkeypatch):
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Evaluation import recommendation_evaluation
    import test_gpu_recommend_models as tm
    model, frame = _fitted(kind)
    rng = np.random.default_rng(8)
    raw_users = [int(u) for u in rng.permutation(np.arange(1000, 1060))[:20]] + [1060]       # 1060 has recorded the whole catalogue
    users, items = _test_pairs(model, frame, raw_users, rng)
    counter = tm._Counter(monkeypatch)
    n = 128
    lists = model.recommend_batch(raw_users, n=n)
    ranks, scores = model.catalogue_ranks(users, items, return_scores=True)
    assert counter.calls == []                                        # the fused path: no per-user ranking
    assert ranks.dtype == np.int64 and scores.dtype == np.float64 and ranks.shape == scores.shape == (len(users),)
    _check_against_lists(model, frame, raw_users, lists, users, items, ranks, scores, n)
    assert (ranks[np.asarray(users) == 1060] == -1).all()
    # without novelty nothing is excluded; pair order does not matter
    free = model.recommend_batch(raw_users, n=n, novelty=False)
    r0 = model.catalogue_ranks(users, items, novelty=False)
    place = [{item: p for p, (s, item) in enumerate(a)} for a in free]
    for u, i, r in zip(users, items, r0.tolist()):
        want = place[raw_users.index(u)].get(i)
        assert (r == want) if want is not None else (r == -1 if i == 5 else r >= n), (u, i, r, want)
    perm = rng.permutation(len(users))
    assert np.array_equal(model.catalogue_ranks([users[j] for j in perm], [items[j] for j in perm]), ranks[perm])
    with pytest.raises(AssertionError, match='was not found'):
        model.catalogue_ranks([raw_users[0], 5], [70000, 70001])
    # the evaluation rebuilt from ranks equals the one from lists, dict for dict
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
        b = recommendation_evaluation(model, ds_te, novelty=True, verbose=False, batched='ranks', **kw)
        assert a == b and a and any(v > 0 for v in a.values()), (a, b)
    assert counter.calls == []


def test_caser_short_sequences_and_a_dmf_subclass_take_the_default(monkeypatch):
    """a Caser user whose sequence is shorter than L, and a DMF subclass with its own prediction hooks, are answered by the default
    hook — one _recommend per distinct user — and agree with their own recommend().  (As in tests/test_gpu_recommend_models.py the
    short user's _rank itself is not run: it hands the device a `before` row of fewer than L items; the counter answers for it.)"""
    import test_gpu_recommend_models as tm
    model, frame = _fitted('caser')
    short = model.interaction_dataset.user_to_uid(1061)
    assert len(model._user_sequence(short)) == 2 < model.L
    counter = tm._Counter(monkeypatch, skip=(short,))
    users = [1003, 1061, 1004, 1061, 1003]
    items = [70010, 70011, 70012, 70013, 70400]
    ranks = model.catalogue_ranks(users, items)
    assert counter.calls == [short]                                   # once per distinct user of the default route
    counter.calls.clear()
    want = [{i: p for p, (_, i) in enumerate(lst)} for lst in ([] if u == 1061 else model.recommend_batch([u], n=128)[0] for u in users)]
    for r, i, w, u in zip(ranks.tolist(), items, want, users):
        assert r == -1 if u == 1061 else (r == w[i] if i in w else (r >= 128 or r == -1)), (u, i, r)
    assert [model.recommend(u, n=None) for u in (1061,)] == [[]]
    counter.calls.clear()

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))
    try:
        from extending_recommender_dmf import ModifiedDMF
    finally:
        sys.path.pop(0)
    modified, frame = _fitted('dmf', cls=ModifiedDMF, epochs=2)
    few = [1002, 1017, 1002, 1040]
    rng = np.random.default_rng(6)
    users = [u for u in few for _ in range(30)]
    items = [70000 + int(i) for _ in few for i in rng.choice(600, size=30, replace=False)]
    ranks, scores = modified.catalogue_ranks(users, items, return_scores=True)
    assert sorted(counter.calls) == sorted(modified.interaction_dataset.user_to_uid(u) for u in set(few))
    own = {u: {i: (p, s) for p, (s, i) in enumerate(modified.recommend(u, n=None))} for u in set(few)}
    for u, i, r, s in zip(users, items, ranks.tolist(), scores.tolist()):
        assert (r, s) == own[u].get(i, (-1, -np.inf)), (u, i, r)
    assert (ranks >= 0).sum() > 60 and (ranks == -1).sum() > 0
