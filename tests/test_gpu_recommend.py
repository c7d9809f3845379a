"""Batched top-n recommendation (drx_cdae_recommend, CdaeEngine.recommend, RecommenderABC.recommend_batch) against the fp64 oracle.

The judge is oracle/cdae_oracle.py::forward in fp64 on fp64 copies of the fp32 parameters, s64[r, i], with REL = 1e-5 (the gate
tests/test_gpu_cdae.py applies to predictions).  Glorot tables put every logit within +-0.05 of the others (every score ~ 0.5: any
ranking passes a tolerance check), so the problems here use SPREAD parameters: W ~ N(0, 0.05), V ~ N(0, 0.5), b ~ N(0, 0.1),
W_ ~ N(0, 0.25 * sqrt(64 / K)), b_ ~ N(0, 0.3), histories of 5 - 60 items.  The logit is a sum of K products, so its spread grows
with sqrt(K): 0.25 at K = 64 gives a logit std of 1.08, and keeping W_'s std at 2 / sqrt(K) keeps it there for every K.  (With 0.25 at
K = 200 the std is 1.9, the best scores sit above 0.9998 where sigmoid's slope s (1 - s) squeezes neighbouring scores together, and fewer
than half of the users have an oracle gap above 2 REL at rank 128: condition 5 below would then be a statement about nothing.)

For every requested user with returned list L = [(v_j, i_j)]:
  1. len(L) == min(n, eligible items); items distinct, in range, not excluded; -1 / -inf only behind the last real entry
  2. |v_j - s64[r, i_j]| <= REL * s64[r, i_j]
  3. L is sorted descending by (v_j, i_j), compared exactly
  4. min_j s64[r, i_j] >= max over eligible non-returned i of s64[r, i] * (1 - 2 REL)          (every user)
  5. at least 0.80 of the users have an oracle gap between ranks n and n + 1 above 2 REL * score (asserted from the oracle alone,
     where the catalogue is large enough for the statement to mean something); for those the item SET equals the oracle's
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL = 1e-5


def _spread_params(rng, U, N, K):
    return {'W': rng.normal(0, 0.05, (N, K)).astype(np.float32), 'W_': rng.normal(0, 2.0 / np.sqrt(K), (K, N)).astype(np.float32),
            'V': rng.normal(0, 0.5, (U, K)).astype(np.float32), 'b': rng.normal(0, 0.1, K).astype(np.float32),
            'b_': rng.normal(0, 0.3, N).astype(np.float32)}


def _histories(rng, U, N, lo=5, hi=60, empty=()):
    indptr, idx = [0], []
    for u in range(U):
        d = 0 if u in empty else min(N, int(rng.integers(lo, hi + 1)))
        idx.append(np.sort(rng.choice(N, size=d, replace=False)).astype(np.int32))
        indptr.append(indptr[-1] + d)
    return np.asarray(indptr, np.int64), np.concatenate(idx).astype(np.int32) if idx else np.zeros(0, np.int32)


def _oracle_scores(p, indptr, indices, uids, block=1 << 16):
    """s64 [R, N]: cdae_oracle.forward in fp64; for long catalogues the same arithmetic in column blocks (x W is a sum over column
    blocks; the output layer is independent per column)."""
    from oracle import cdae_oracle as co
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    N = p['W'].shape[0]
    R = len(uids)
    if N <= block:
        x = np.zeros((R, N))
        for j, u in enumerate(uids):
            x[j, indices[indptr[u]:indptr[u + 1]]] = 1.0
        return co.forward(p64, np.asarray(uids), x)[1]
    z1 = np.zeros((R, p['W'].shape[1]))
    for j, u in enumerate(uids):
        z1[j] = p64['W'][indices[indptr[u]:indptr[u + 1]]].sum(axis=0)
    h = co.sigmoid(z1 + p64['V'][np.asarray(uids)] + p64['b'])
    out = np.empty((R, N))
    for lo in range(0, N, block):
        out[:, lo:lo + block] = co.sigmoid(h @ p64['W_'][:, lo:lo + block] + p64['b_'][lo:lo + block])
    return out


def _engine(p, indptr, indices, excl=None):
    from drecpy_amd.engine import CdaeEngine
    N, K = p['W'].shape
    eng = CdaeEngine(p['V'].shape[0], N, K)
    eng.set_params(**p)
    eng.set_history(indptr, indices, with_transpose=False)
    if excl is not None:
        eng.set_exclusions(*excl)
    return eng


def _check(idx, val, s64, excl_rows, n, min_separated=None):
    """checks 1 - 5 of the module docstring; excl_rows[j] = excluded items of requested user j (or None).  Returns the separated share."""
    R, N = s64.shape
    assert idx.shape == (R, n) and val.shape == (R, n)
    separated = 0
    for j in range(R):
        elig = np.ones(N, bool)
        if excl_rows is not None:
            elig[excl_rows[j]] = False
        want = min(n, int(elig.sum()))
        got = int((idx[j] >= 0).sum())
        assert got == want, (j, got, want)
        assert (idx[j, want:] == -1).all() and np.isneginf(val[j, want:]).all()                  # 1: padding behind the last entry only
        items, vals = idx[j, :want].astype(np.int64), val[j, :want]
        assert len(set(items.tolist())) == want and (items >= 0).all() and (items < N).all() and elig[items].all()
        ref = s64[j, items]
        assert (np.abs(vals.astype(np.float64) - ref) <= REL * ref).all(), (j, np.max(np.abs(vals - ref) / ref))          # 2
        for a in range(want - 1):                                                                # 3: exact (value, item) order
            assert (vals[a], items[a]) > (vals[a + 1], items[a + 1]), (j, a)
        rest = elig.copy()
        rest[items] = False
        if want and rest.any():
            assert ref.min() >= s64[j, rest].max() * (1 - 2 * REL), j                            # 4
        se = np.where(elig, s64[j], -np.inf)
        order = np.argsort(-se, kind='stable')
        if int(elig.sum()) > n:
            a, b = se[order[n - 1]], se[order[n]]
            if a - b > 2 * REL * a:
                separated += 1
                assert set(items.tolist()) == set(order[:n].tolist()), j                         # 5: the oracle's item set
        else:
            separated += 1
            assert set(items.tolist()) == set(np.flatnonzero(elig).tolist()), j
    share = separated / R
    if min_separated is not None:
        assert share >= min_separated, share
    return share


_PROBLEMS = {}


def _problem(K, U=400, N=50000, R=256, seed=7):
    key = (K, U, N, R, seed)
    if key not in _PROBLEMS:
        rng = np.random.default_rng(seed)
        p = _spread_params(rng, U, N, K)
        indptr, indices = _histories(rng, U, N)
        uids = rng.choice(U, size=R, replace=False).astype(np.int32)
        s64 = _oracle_scores(p, indptr, indices, uids)
        _PROBLEMS.clear()                                   # (one resident problem: 100 MB of oracle scores each)
        _PROBLEMS[key] = (p, indptr, indices, uids, s64)
    return _PROBLEMS[key]


def _rows(indptr, indices, uids):
    return [indices[indptr[u]:indptr[u + 1]] for u in uids]


@pytest.mark.parametrize('K', [50, 128, 200])
def test_fused_lists_match_the_oracle(K):
    p, indptr, indices, uids, s64 = _problem(K)
    eng = _engine(p, indptr, indices, (indptr, indices))
    for n in (1, 10, 64, 128):
        idx, val = eng.recommend(uids, n)
        _check(idx.cpu().numpy(), val.cpu().numpy(), s64, _rows(indptr, indices, uids), n, min_separated=0.80)


def test_without_exclusions():
    p, indptr, indices, uids, s64 = _problem(128)
    eng = _engine(p, indptr, indices, (indptr, indices))
    idx, val = eng.recommend(uids, 10, exclude=False)
    _check(idx.cpu().numpy(), val.cpu().numpy(), s64, None, 10, min_separated=0.80)
    eng2 = _engine(p, indptr, indices)                      # no exclusion CSR at all
    idx2, val2 = eng2.recommend(uids, 10)
    import torch
    assert torch.equal(idx, idx2) and torch.equal(val, val2)


@pytest.mark.parametrize('N', [1, 31, 33, 150, 4097])
@pytest.mark.parametrize('R', [1, 3, 65])
def test_shapes_that_do_not_fill_a_tile(N, R):
    """n beyond the eligible items, a user whose whole catalogue is excluded (the first requested), one with an empty history (the second)"""
    rng = np.random.default_rng(1000 * N + R)
    U, K = 80, 50
    p = _spread_params(rng, U, N, K)
    indptr, indices = _histories(rng, U, N, empty=(1,))
    uids = np.concatenate([[0, 1, 2][:R], rng.choice(np.arange(3, U), size=max(R - 3, 0), replace=False)]).astype(np.int32)
    rows = [indices[indptr[u]:indptr[u + 1]] for u in range(U)]
    rows[0] = np.arange(N, dtype=np.int32)                  # user 0: everything excluded
    xptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    xidx = np.concatenate(rows).astype(np.int32)
    s64 = _oracle_scores(p, indptr, indices, uids)
    eng = _engine(p, indptr, indices, (xptr, xidx))
    for n in (10, 128):
        idx, val = eng.recommend(uids, n)
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        _check(idx, val, s64, [rows[u] for u in uids], n)
        assert (idx[0] == -1).all()
        if R > 1:
            assert (idx[1] >= 0).sum() == min(n, N)         # the empty history excludes nothing


def test_long_catalogue_and_scratch_is_not_a_score_matrix():
    from drecpy_amd import _lib
    U, N, K, R, n = 300, 1_000_000, 128, 128, 10
    rng = np.random.default_rng(11)
    p = _spread_params(rng, U, N, K)
    indptr, indices = _histories(rng, U, N)
    uids = rng.choice(U, size=R, replace=False).astype(np.int32)
    need = int(_lib.lib().drx_cdae_recommend_scratch_bytes(R, N, 128, n))
    assert 0 < need < R * N // 4, need                      # a sixteenth of the fp32 score matrix
    assert int(_lib.lib().drx_cdae_recommend_scratch_bytes(R, 2_000_000_000, 128, n)) < R * N // 4     # ... and does not grow with n_items
    eng = _engine(p, indptr, indices, (indptr, indices))
    idx, val = eng.recommend(uids, n)
    assert eng._rows_sc.numel() < R * N // 4
    s64 = _oracle_scores(p, indptr, indices, uids)
    _check(idx.cpu().numpy(), val.cpu().numpy(), s64, _rows(indptr, indices, uids), n, min_separated=0.80)


@pytest.mark.parametrize('case', ['n300', 'ld260'])
def test_outside_the_fused_domain_takes_the_score_matrix_route(case):
    from drecpy_amd import _lib
    rng = np.random.default_rng(5)
    U, N, R = 60, 4097, 40
    K, n = (50, 300) if case == 'n300' else (260, 10)
    p = _spread_params(rng, U, N, K)
    indptr, indices = _histories(rng, U, N)
    uids = rng.choice(U, size=R, replace=False).astype(np.int32)
    eng = _engine(p, indptr, indices, (indptr, indices))
    L = _lib.lib()
    assert L.drx_cdae_recommend_scratch_bytes(R, N, eng.ld, n) == 0
    import torch
    h = eng._hidden_rows(torch.as_tensor(uids).to(eng.device))
    oi = torch.empty(R, n, dtype=torch.int32, device=eng.device)
    ov = torch.empty(R, n, dtype=torch.float32, device=eng.device)
    sc = torch.empty(1 << 20, dtype=torch.uint8, device=eng.device)
    rc = L.drx_cdae_recommend(C.byref(eng._params), _lib.ptr(h), _lib.ptr(torch.as_tensor(uids).to(eng.device)), R, n, None, None,
                              _lib.ptr(oi), _lib.ptr(ov), _lib.ptr(sc), sc.numel(), None)
    assert rc == -3                                         # DRX_ENOTIMPL
    idx, val = eng.recommend(uids, n)
    s64 = _oracle_scores(p, indptr, indices, uids)
    _check(idx.cpu().numpy(), val.cpu().numpy(), s64, _rows(indptr, indices, uids), n)


def test_small_requests_may_be_routed_to_the_score_matrix_path():
    """RECOMMEND_MIN_FUSED_USERS routes requests below it through forward + drx_topk: same contract"""
    p, indptr, indices, uids, s64 = _problem(128)
    eng = _engine(p, indptr, indices, (indptr, indices))
    eng.RECOMMEND_MIN_FUSED_USERS = 1 << 30
    idx, val = eng.recommend(uids[:8], 10)
    _check(idx.cpu().numpy(), val.cpu().numpy(), s64[:8], _rows(indptr, indices, uids[:8]), 10)


def _tie_order_ok(idx, val):
    for j in range(idx.shape[0]):
        k = int((idx[j] >= 0).sum())
        for a in range(k - 1):
            if val[j, a] == val[j, a + 1]:
                assert idx[j, a] > idx[j, a + 1], (j, a)
            else:
                assert val[j, a] > val[j, a + 1], (j, a)


def test_exact_ties_duplicate_rows():
    """40 item rows are byte copies of other rows, pairs straddling tile (32), block (128) and split boundaries: equal scores, the
    larger index first, and of a tied pair at the cut the larger index is the one kept"""
    rng = np.random.default_rng(21)
    U, N, K, R = 120, 50000, 64, 96
    p = _spread_params(rng, U, N, K)
    src, dst, used = [], [], set()
    for d in [1, 31, 32, 33, 127, 128, 129, 4095, 4096, 25000] * 4:
        while True:
            s = int(rng.integers(0, N))
            if s not in used and (s + d) % N not in used:
                break
        used.update((s, (s + d) % N))
        src.append(s)
        dst.append((s + d) % N)
    src, dst = np.array(src), np.array(dst)
    assert len(src) == 40
    # push the copied rows' scores up so that the pairs show up in the lists (and at their cuts)
    p['W_'][:, src] *= 3.0
    p['W_'][:, dst] = p['W_'][:, src]
    p['b_'][dst] = p['b_'][src]
    indptr, indices = _histories(rng, U, N)
    uids = rng.choice(U, size=R, replace=False).astype(np.int32)
    eng = _engine(p, indptr, indices)
    s64 = _oracle_scores(p, indptr, indices, uids)
    pair_of = {int(a): int(b) for a, b in zip(src, dst)}
    pair_of.update({int(b): int(a) for a, b in zip(src, dst)})
    seen_pairs = cut_pairs = 0
    for n in (1, 5, 10, 33):
        idx, val = eng.recommend(uids, n, exclude=False)
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        _check(idx, val, s64, None, n)
        _tie_order_ok(idx, val)
        for j in range(R):
            got = idx[j].tolist()
            for pos, i in enumerate(got):
                o = pair_of.get(i)
                if o is None:
                    continue
                if o in got:
                    seen_pairs += 1
                    assert val[j, pos] == val[j, got.index(o)]                  # byte-equal rows: bit-equal scores
                    assert abs(got.index(o) - pos) == 1
                elif pos == n - 1:
                    cut_pairs += 1
                    assert i > o, (j, i, o)                                     # the tied pair at the cut: the larger index stays
    assert seen_pairs > 0 and cut_pairs > 0, (seen_pairs, cut_pairs)


def test_exact_ties_saturated_scores():
    """b_ pushed to +-40: many scores are exactly 1.0f (and tiny ones at the other end): ties by larger index"""
    rng = np.random.default_rng(22)
    U, N, K, R = 90, 6000, 50, 70
    p = _spread_params(rng, U, N, K)
    up = rng.choice(N, size=500, replace=False)
    p['b_'][:] = -40.0
    p['b_'][up] = 40.0
    indptr, indices = _histories(rng, U, N)
    uids = rng.choice(U, size=R, replace=False).astype(np.int32)
    eng = _engine(p, indptr, indices, (indptr, indices))
    s64 = _oracle_scores(p, indptr, indices, uids)
    rows = _rows(indptr, indices, uids)
    for n in (10, 128):
        idx, val = eng.recommend(uids, n)
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        _check(idx, val, s64, rows, n)
        _tie_order_ok(idx, val)
        assert (val[:, 0] == 1.0).all()
        for j in range(R):                                  # all ones: the n largest eligible indices among the saturated items
            ones = np.setdiff1d(up, rows[j])
            fwd = eng.forward(uids[j:j + 1])[1][0].cpu().numpy()
            ones = ones[fwd[ones] == 1.0]
            if len(ones) >= n and (val[j] == 1.0).all():
                assert idx[j].tolist() == np.sort(ones)[::-1][:n].tolist(), j


def test_bit_identical_between_calls_orders_and_chunkings():
    import torch
    p, indptr, indices, uids, s64 = _problem(128)
    eng = _engine(p, indptr, indices, (indptr, indices))
    for n in (10, 100):
        a_idx, a_val = eng.recommend(uids, n)
        b_idx, b_val = eng.recommend(uids, n)
        assert torch.equal(a_idx, b_idx) and torch.equal(a_val, b_val)
        perm = np.random.default_rng(3).permutation(len(uids))
        c_idx, c_val = eng.recommend(uids[perm], n, chunk_users=37)
        inv = torch.as_tensor(np.argsort(perm)).to(eng.device)
        assert torch.equal(a_idx, c_idx[inv]) and torch.equal(a_val, c_val[inv])
        d_idx, d_val = eng.recommend(uids[:5], n)            # other neighbours in the tile, another split count
        assert torch.equal(a_idx[:5], d_idx) and torch.equal(a_val[:5], d_val)


# ---- the public layer: CDAE.recommend_batch / recommendation_evaluation(batched=True) ----------------------------------------------
def _frame(seed, U=48, N=3000, lo=5, hi=60):
    """raw ids are offset from the internal ones; values 1 - 5 (pairs below a threshold of 3 are recorded too)"""
    rng = np.random.default_rng(seed)
    users, items, vals = [], [], []
    for u in range(U):
        d = int(rng.integers(lo, hi + 1))
        users += [1000 + u] * d
        items += (70000 + rng.choice(N, size=d, replace=False)).tolist()
        vals += rng.integers(1, 6, size=d).tolist()
    users += [1000] * N                                      # every item appears (user 1000 has recorded the whole catalogue, value 1)
    items += (70000 + np.arange(N)).tolist()
    vals += [1] * N
    return {'user': np.array(users), 'item': np.array(items), 'interaction': np.array(vals)}


def _fitted(mode, seed=5, K=50, threshold=3, frame_seed=31, spread=True):
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender import CDAE
    frame = _frame(frame_seed)
    ds = InteractionDataset.read_df(frame, verbose=False)
    U, N = len(set(frame['user'].tolist())), len(set(frame['item'].tolist()))
    w = _spread_params(np.random.default_rng(seed), U, N, K) if spread else None
    kw = dict(mode='sampled') if mode == 'sampled' else {}
    model = CDAE(hidden_factors=K, seed=seed, verbose=False, interaction_threshold=threshold, **kw)
    model.fit(ds, epochs=5, batch_size=16 if mode == 'reference' else 256, learning_rate=1e-3, initial_weights=w)
    return model, frame


def _model_scores(model, raw_users):
    """fp64 oracle scores of the fitted model for the raw users, and their recorded (excluded) internal items"""
    ds = model.interaction_dataset
    p = model._engine.get_params()
    indptr, indices = ds.positives_csr(model.interaction_threshold)
    uids = np.array([ds.user_to_uid(u) for u in raw_users])
    s64 = _oracle_scores(p, np.asarray(indptr), np.asarray(indices), uids)
    ip, cols, _ = ds.interaction_csr()
    return s64, [np.asarray(cols[ip[u]:ip[u + 1]], dtype=np.int64) for u in uids], uids


@pytest.mark.parametrize('mode', ['reference', 'sampled'])
def test_recommend_batch_on_a_fitted_model(mode, tmp_path):
    model, frame = _fitted(mode)
    ds = model.interaction_dataset
    raw_users = [int(u) for u in np.random.default_rng(2).permutation(np.unique(frame['user']))[:20]] + [1000]
    n = 5
    got = model.recommend_batch(raw_users, n=n)
    one = [model.recommend(u, n=n) for u in raw_users]
    assert len(got) == len(one) == len(raw_users)
    raw_items = set(frame['item'].tolist())
    for a, b in zip(got, one):                               # length, tuple shape and raw ids of recommend()
        assert len(a) == len(b)
        assert all(type(x) is tuple and len(x) == 2 and type(x[0]) is type(y[0]) is float and type(x[1]) is type(y[1]) and x[1] in raw_items
                   for x, y in zip(a, b))
    assert got[-1] == [] and one[-1] == []                   # user 1000 has recorded every item
    # each path against the oracle; where the oracle separates rank n from n + 1 the two paths return the same item SET
    s64, recorded, uids = _model_scores(model, raw_users)
    idx = np.array([[ds.item_to_iid(i) for _, i in a] + [-1] * (n - len(a)) for a in got])
    val = np.array([[s for s, _ in a] + [-np.inf] * (n - len(a)) for a in got], dtype=np.float32)
    _check(idx, val, s64, recorded, n, min_separated=0.80)
    sep = 0
    for j, (a, b) in enumerate(zip(got, one)):
        se = s64[j].copy()
        se[recorded[j]] = -np.inf
        top = np.sort(se)[::-1][:n + 1]
        if len(a) == n and top[n - 1] - top[n] > 2 * REL * top[n - 1]:
            sep += 1
            assert {i for _, i in a} == {i for _, i in b}, j
    assert sep >= 0.8 * (len(raw_users) - 1)
    # pairs recorded BELOW the interaction threshold are excluded too (what _all_user_items does), and are not without novelty
    low = {(int(u), int(i)) for u, i, v in zip(frame['user'], frame['item'], frame['interaction']) if v < 3}
    assert low
    for u, a in zip(raw_users, got):
        mine = {i for uu, i in zip(frame['user'].tolist(), frame['item'].tolist()) if uu == u}
        assert not mine & {i for _, i in a}
    everything = model.recommend_batch([1000], n=n, novelty=False)[0]
    assert len(everything) == n
    # request order, repeated users
    again = model.recommend_batch(raw_users[::-1] + raw_users[:3], n=n)
    assert again == got[::-1] + got[:3]
    # interaction_threshold cuts the tail; as_arrays carries the same content
    cut = float(np.median([a[2][0] for a in got if len(a) == n]))
    kept = model.recommend_batch(raw_users, n=n, interaction_threshold=cut)
    assert kept == [[x for x in a if x[0] >= cut] for a in got] and any(len(a) < len(b) for a, b in zip(kept, got))
    scores, items, counts = model.recommend_batch(raw_users, n=n, interaction_threshold=cut, as_arrays=True)
    assert scores.dtype == np.float32 and scores.shape == items.shape == (len(raw_users), n)
    for r, a in enumerate(kept):
        assert counts[r] == len(a) and [(float(s), i) for s, i in zip(scores[r, :counts[r]], items[r, :counts[r]])] == a
        assert np.isneginf(scores[r, counts[r]:]).all()
    # save / load: bit-identical (the exclusion CSR is rebuilt for the restored engine)
    path = str(tmp_path / 'cdae.bin')
    model.save(path)
    from drecpy_amd.Recommender.recommender_abc import RecommenderABC
    back = RecommenderABC.load(path)
    assert getattr(back._engine, '_excl', None) is None
    assert back.recommend_batch(raw_users, n=n) == got
    with pytest.raises(AssertionError, match='was not found'):
        model.recommend_batch([raw_users[0], 5], n=n)


def test_batched_recommendation_evaluation_equals_the_loop_on_the_gpu():
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Evaluation import recommendation_evaluation
    n = 5
    for frame_seed in range(40, 60):                         # re-seeded until the oracle separates every evaluated user's ranks 1 .. n + 1
        model, frame = _fitted('reference', frame_seed=frame_seed)
        rng = np.random.default_rng(frame_seed)
        raw_users = [int(u) for u in rng.permutation(np.arange(1001, 1048))[:12]]
        s64, recorded, uids = _model_scores(model, raw_users)
        ok = True
        for j in range(len(raw_users)):
            se = s64[j].copy()
            se[recorded[j]] = -np.inf
            top = np.sort(se)[::-1][:n + 1]
            ok &= bool((top[:-1] - top[1:] > 2 * REL * top[:-1]).all())
        if ok:
            break
    assert ok, 'no seed separates the oracle ranks of every evaluated user'
    # the held-out positives: for every evaluated user a few items it has not recorded, some of them among its best
    tu, ti, tv = [], [], []
    for j, u in enumerate(raw_users):
        se = s64[j].copy()
        se[recorded[j]] = -np.inf
        best = np.argsort(-se)[:8]
        for iid in list(best[rng.permutation(8)[:3]]) + rng.choice(np.setdiff1d(np.arange(3000), recorded[j]), size=3, replace=False).tolist():
            tu.append(u)
            ti.append(model.interaction_dataset.iid_to_item(int(iid)))
            tv.append(int(rng.integers(3, 6)))
    ds_te = InteractionDataset.read_df({'user': np.array(tu), 'item': np.array(ti), 'interaction': np.array(tv)}, verbose=False)
    for kw in (dict(k=[1, 3, 5], novelty=True), dict(k=5, novelty=True, n_pos_interactions=2, seed=4)):
        a = recommendation_evaluation(model, ds_te, verbose=False, **kw)
        b = recommendation_evaluation(model, ds_te, verbose=False, batched=True, **kw)
        assert a == b and a and any(v > 0 for v in a.values()), (a, b)
