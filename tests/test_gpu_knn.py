"""The KNN baselines on the device: drx_knn_neighbours against the NumPy oracle (tests/knn_oracle.py) bit for bit on integer ratings
(sums of integers are exact in fp32 below 2^24; the epilogue is a fixed sequence of correctly rounded double operations), within a
derived tolerance on non-integer ratings; drx_knn_score_rows / drx_knn_pair_scores on the oracle's table; the public classes against
what the reference computed (tests/golden/knn.json) by the rules of tests/test_knn_oracle.py; evaluation; save / load."""
import os

import numpy as np
import pytest

import knn_oracle as ko
from test_knn_oracle import TOL, csr32, golden_dataset, load_golden, reference_matrix

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.as_tensor(a if len(a) else np.zeros(1, a.dtype)).to('cuda:0')


def dev_neighbours(csr, R, C, metric, k, m, shrinkage, max_diff=None, splits=0):
    from drecpy_amd import _lib
    L = _lib.lib()
    ip, ix, v = _dev(csr[0]), _dev(csr[1]), _dev(csr[2])
    md = ko.max_diff_of(csr, R, C) if max_diff is None else max_diff
    need = int(L.drx_knn_neighbours_scratch_bytes(R, C, k, splits))
    assert need > 0
    sc = torch.empty(need, dtype=torch.uint8, device='cuda:0')
    idx = torch.full((R, k), -7, dtype=torch.int32, device='cuda:0')
    sim = torch.full((R, k), -7.0, dtype=torch.float32, device='cuda:0')
    _lib.check(L.drx_knn_neighbours(_lib.ptr(ip), _lib.ptr(ix), _lib.ptr(v), len(csr[1]), R, C, _lib.KNN_METRICS[metric], k, m,
                                    -1.0 if shrinkage is None else float(shrinkage), float(md) or 1.0, splits, _lib.ptr(idx), _lib.ptr(sim),
                                    _lib.ptr(sc), need, _lib.stream_ptr(torch.device('cuda:0'))), 'drx_knn_neighbours')
    return idx.cpu().numpy(), sim.cpu().numpy()


def random_csr(seed, R, C, density, scale=1.0):
    rng = np.random.default_rng(seed)
    mask = rng.random((R, C)) < density
    rows, cols = np.nonzero(mask)
    vals = rng.integers(1, 6, size=len(rows)).astype(np.float32) * np.float32(scale)
    return ko.csr_of(rows, cols, vals, R)


def assert_bit_equal(csr, R, C, metric, k, m, shrinkage, splits=0):
    idx, sim = dev_neighbours(csr, R, C, metric, k, m, shrinkage, splits=splits)
    want_idx, want_sim = ko.neighbours(ko.similarities(csr, R, C, metric, m, shrinkage), k)
    assert np.array_equal(idx, want_idx), (metric, np.argwhere(idx != want_idx)[:5])
    assert np.array_equal(sim.view(np.uint32), want_sim.view(np.uint32)), (metric, np.argwhere(sim != want_sim)[:5])
    return idx, sim


# ---- 1. neighbours against the oracle, integer ratings: bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize('metric', ko.METRICS)
def test_every_metric_partial_tiles(metric):
    """R = 70, C = 37: a partial row tile, a partial column step"""
    assert_bit_equal(random_csr(1, 70, 37, 0.35), 70, 37, metric, 5, 2, 10)


@pytest.mark.parametrize('R,C,k,m,shrinkage,splits,metric', [
    (130, 50, 7, 2, 10, 3, 'pearson'),              # two row tiles, a forced split count: the merge
    (130, 50, 7, 2, 10, 3, 'adjusted_cosine'),
    (1, 9, 4, 0, None, 0, 'cosine'),                # no neighbours at all
    (200, 64, 128, 1, 100, 0, 'cosine'),            # the longest list
    (200, 64, 128, 1, 100, 2, 'jaccard'),           # ... full of ties
    (70, 37, 1, 2, 10, 0, 'msd'),                   # k = 1
    (70, 37, 5, 0, 10, 0, 'cosine_cf'),             # m = 0
    (70, 37, 5, 1000, 10, 0, 'cosine'),             # m above every co-count: all lists empty
    (70, 37, 5, 2, None, 0, 'pearson'),             # no shrinkage
    (70, 37, 20, 5, 100, 0, 'adjusted_cosine'),     # the reference's defaults
])
def test_shapes(R, C, k, m, shrinkage, splits, metric):
    idx, sim = assert_bit_equal(random_csr(R + C + k, R, C, 0.3), R, C, metric, k, m, shrinkage, splits)
    if R == 1 or m == 1000:
        assert (idx == -1).all() and (sim == 0).all()
    if k == 128:
        assert (idx[:, -1] >= 0).any()              # some lists are full at k = 128


def test_ties_dropped_pairs_and_an_empty_row():
    """rows 0 and 1 identical, 2 and 3 identical to them in pattern; rows 4 and 5 share no column; row 6 is empty (ABI level)"""
    C = 12
    rows = {0: {0: 3, 1: 4, 2: 5, 3: 1}, 1: {0: 3, 1: 4, 2: 5, 3: 1}, 2: {0: 3, 1: 4, 2: 5, 3: 1}, 3: {0: 1, 1: 2, 2: 2, 3: 5},
            4: {4: 2, 5: 3, 6: 4}, 5: {7: 2, 8: 3, 9: 5}, 6: {}, 7: {0: 3, 1: 4, 5: 1, 8: 2}}
    r, c, v = zip(*[(i, j, x) for i, row in rows.items() for j, x in row.items()])
    csr = ko.csr_of(r, c, v, 8)
    for metric in ko.METRICS:
        idx, sim = assert_bit_equal(csr, 8, C, metric, 3, 0, None)
        assert (idx[6] == -1).all() and 6 not in idx
        assert 5 not in idx[4] and 4 not in idx[5]                  # no common column: dropped
        if metric == 'cosine':
            assert idx[0, 0] == 2 and idx[0, 1] == 1 and sim[0, 0] == sim[0, 1]     # a tie goes to the larger id
            assert idx[2, 0] == 1 and idx[2, 1] == 0
        if metric == 'jaccard':                                      # rows 0..3 share one pattern: a three-way tie
            assert idx[0].tolist() == [3, 2, 1] and idx[3].tolist() == [2, 1, 0] and (sim[0] == 1.0).all()


def test_bit_reproducible_between_calls_and_split_counts():
    csr = random_csr(5, 300, 90, 0.25)
    for metric in ('pearson', 'jaccard'):
        first = dev_neighbours(csr, 300, 90, metric, 10, 2, 10)
        for splits in (0, 1, 2, 5, 64):
            again = dev_neighbours(csr, 300, 90, metric, 10, 2, 10, splits=splits)
            assert np.array_equal(first[0], again[0]) and np.array_equal(first[1].view(np.uint32), again[1].view(np.uint32)), (metric, splits)


def test_argument_errors_and_empty_requests():
    from drecpy_amd import _lib
    L = _lib.lib()
    csr = random_csr(2, 20, 10, 0.4)
    ip, ix, v = _dev(csr[0]), _dev(csr[1]), _dev(csr[2])
    out_i, out_s = torch.full((20, 4), -7, dtype=torch.int32, device='cuda:0'), torch.zeros(20, 4, device='cuda:0')
    sc = torch.empty(1 << 20, dtype=torch.uint8, device='cuda:0')
    st = _lib.stream_ptr(torch.device('cuda:0'))

    def call(R=20, C=10, metric=0, k=4, m=0, shr=-1.0, md=5.0, scratch=sc, nbytes=1 << 20):
        return L.drx_knn_neighbours(_lib.ptr(ip), _lib.ptr(ix), _lib.ptr(v), len(csr[1]), R, C, metric, k, m, shr, md, 0, _lib.ptr(out_i),
                                    _lib.ptr(out_s), _lib.ptr(scratch), nbytes, st)
    einval = call(metric=9)
    assert einval != 0 and call(k=0) == call(k=129) == call(m=-1) == call(C=0) == call(metric=4, md=0.0) == einval
    assert call(nbytes=64) not in (0, einval) and call(scratch=None) not in (0, einval)       # DRX_ESCRATCH
    assert call(R=0) == 0 and int(out_i.min()) == -7                                          # nothing written
    assert call() == 0
    assert L.drx_knn_neighbours_scratch_bytes(20, 10, 129, 0) == 0


# ---- 2. non-integer ratings: against the float64 oracle within a derived tolerance ---------------------------------------------------
@pytest.mark.parametrize('metric', ko.METRICS)
def test_non_integer_ratings(metric):
    """Ratings drawn from [0.5, 5) as float32: every product and sum rounds in fp32.  Gate: max(1e-5, 4 x the error of the oracle's
    own float32-accumulated variant).  (m = 5: pearson's radicand Sxx - Sx^2 / n cancels; with two or three common ratings that lie
    close together it amplifies the fp32 rounding of the sums without bound, on the device and in the float32 oracle alike —
    DESIGN.md section 3.6 has the figures.)"""
    R, C, k, m, shr = 150, 80, 10, 5, 10
    csr = random_csr(11, R, C, 0.3)
    csr = (csr[0], csr[1], np.random.default_rng(12).uniform(0.5, 5.0, len(csr[2])).astype(np.float32))
    S64 = ko.similarities(csr, R, C, metric, m, shr, acc=np.float64, raw=True)
    S32 = ko.similarities(csr, R, C, metric, m, shr, raw=True)
    own = float(np.max(np.abs(S32 - S64)))
    tol = max(1e-5, 4 * own)
    idx, sim = dev_neighbours(csr, R, C, metric, k, m, shr)
    listed = idx >= 0
    err = float(np.max(np.abs(sim[listed] - S64[np.nonzero(listed)[0], idx[listed]]))) if listed.any() else 0.0
    print(f'{metric}: device vs float64 oracle {err:.3e}; float32-accumulated oracle vs float64 {own:.3e}; gate {tol:.3e}')
    assert err <= tol
    ko.check_neighbours_against(S64, idx, sim, tol)


# ---- 3. score_rows / pair_scores on the oracle's table -----------------------------------------------------------------------------
def dev_score_rows(kind, agg, ucsr, U, N, nb_idx, nb_sim, uids, cand, fallback):
    from drecpy_amd import _lib
    from drecpy_amd.engine import pack_mask_bits
    L = _lib.lib()
    ip, ix, v = _dev(ucsr[0]), _dev(ucsr[1]), _dev(ucsr[2])
    d_idx, d_sim, d_uid = _dev(nb_idx), _dev(nb_sim), _dev(np.asarray(uids, np.int32))
    R = len(uids)
    out = torch.full((R, N), -7.0, dtype=torch.float32, device='cuda:0')
    mask = _dev(pack_mask_bits(cand).view(np.int32))
    fb = _dev(np.asarray(fallback, np.float64)) if fallback is not None else None
    t = _lib.KNN_USER if kind == 'user' else _lib.KNN_ITEM
    need = int(L.drx_knn_score_rows_scratch_bytes(t, R, N))
    sc = torch.empty(need, dtype=torch.uint8, device='cuda:0') if need else None
    _lib.check(L.drx_knn_score_rows(t, _lib.KNN_AGGREGATIONS[agg], _lib.ptr(ip), _lib.ptr(ix), _lib.ptr(v), len(ucsr[1]), U, N, _lib.ptr(d_idx),
                                    _lib.ptr(d_sim), nb_idx.shape[1], _lib.ptr(d_uid), R, _lib.ptr(fb), _lib.ptr(out), _lib.ptr(mask),
                                    _lib.ptr(sc), need, _lib.stream_ptr(torch.device('cuda:0'))), 'drx_knn_score_rows')
    bits = np.unpackbits(mask.cpu().numpy().view(np.uint8), bitorder='little')[:R * N].astype(bool).reshape(R, N)
    return out.cpu().numpy(), bits, need


def dev_pair_scores(kind, agg, ucsr, U, N, nb_idx, nb_sim, uids, iids, fallback):
    from drecpy_amd import _lib
    L = _lib.lib()
    ip, ix, v = _dev(ucsr[0]), _dev(ucsr[1]), _dev(ucsr[2])
    d_idx, d_sim = _dev(nb_idx), _dev(nb_sim)
    P = len(uids)
    out = torch.full((max(P, 1),), -7.0, dtype=torch.float64, device='cuda:0')
    none = torch.full((max(P, 1),), 9, dtype=torch.uint8, device='cuda:0')
    fb = _dev(np.asarray(fallback, np.float64)) if fallback is not None else None
    d_uid, d_iid = _dev(np.asarray(uids, np.int32)), _dev(np.asarray(iids, np.int32))     # (named: they must outlive the launch)
    rc = L.drx_knn_pair_scores(_lib.KNN_USER if kind == 'user' else _lib.KNN_ITEM, _lib.KNN_AGGREGATIONS[agg], _lib.ptr(ip), _lib.ptr(ix),
                               _lib.ptr(v), len(ucsr[1]), U, N, _lib.ptr(d_idx), _lib.ptr(d_sim), nb_idx.shape[1],
                               _lib.ptr(d_uid), _lib.ptr(d_iid), P, _lib.ptr(fb),
                               _lib.ptr(out), _lib.ptr(none), _lib.stream_ptr(torch.device('cuda:0')))
    assert rc == 0
    return out.cpu().numpy(), none.cpu().numpy()


@pytest.fixture(scope='module')
def small_model():
    """U = 60 users x N = 37 items (ratings / 2: non-integer products), the oracle's tables of both types"""
    U, N = 60, 37
    ucsr = random_csr(21, U, N, 0.3, scale=0.5)
    icsr = ko.transpose_csr(ucsr, U, N)
    tables = {'user': ko.neighbours(ko.similarities(ucsr, U, N, 'cosine', 2, 10), 6),
              'item': ko.neighbours(ko.similarities(icsr, N, U, 'adjusted_cosine', 2, 10), 6)}
    return U, N, ucsr, icsr, tables


@pytest.mark.parametrize('kind', ['user', 'item'])
@pytest.mark.parametrize('agg', ['mean', 'weighted_mean'])
@pytest.mark.parametrize('averages', [False, True])
def test_scores_against_the_oracle(small_model, kind, agg, averages):
    U, N, ucsr, icsr, tables = small_model
    nb_idx, nb_sim = tables[kind]
    rng = np.random.default_rng(3)
    uids = np.array([0, 59, 17, 17, 33], np.int32)
    cand = rng.random((len(uids), N)) < 0.8
    row_fb = ko.row_means(ucsr, U) if averages and kind == 'item' else None
    out, bits, need = dev_score_rows(kind, agg, ucsr, U, N, nb_idx, nb_sim, uids, cand, row_fb)
    want, has = ko.score_rows(kind, agg, ucsr, N, nb_idx, nb_sim, uids, row_fb)
    assert need == 0
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(bits, cand & has)
    assert row_fb is not None or not has.all()                       # some item without a prediction: a cleared bit
    # pairs: doubles, bit for bit; the fallback of both types
    pair_fb = (ko.row_means(ucsr, U) if kind == 'item' else ko.row_means(icsr, N)) if averages else None
    pu, pi = rng.integers(0, U, 300), rng.integers(0, N, 300)
    got, none = dev_pair_scores(kind, agg, ucsr, U, N, nb_idx, nb_sim, pu, pi, pair_fb)
    for p in range(300):
        w = ko.pair_score(kind, agg, ucsr, nb_idx, nb_sim, int(pu[p]), int(pi[p]), pair_fb)
        assert (w is None) == bool(none[p]), (p, w, none[p])
        assert w is None or np.float64(w).view(np.uint64) == got[p].view(np.uint64), (p, w, got[p])
    assert averages or none.any()
    got, none = dev_pair_scores(kind, agg, ucsr, U, N, nb_idx, nb_sim, [], [], pair_fb)        # P = 0: nothing written
    assert got[0] == -7.0 and none[0] == 9


@pytest.mark.parametrize('kind,N', [('item', 41000), ('user', 10300)])
def test_scores_past_the_lds_row(kind, N):
    """n_items beyond what a workgroup's LDS holds: the row lives in the scratch"""
    U = 24
    rng = np.random.default_rng(8)
    live = np.sort(rng.choice(N, 40, replace=False))                 # the items anybody rated
    mask = rng.random((U, 40)) < 0.4
    rows, cols = np.nonzero(mask)
    ucsr = ko.csr_of(rows, live[cols], rng.integers(1, 6, len(rows)), U)
    csr, R, C = (ucsr, U, N) if kind == 'user' else (ko.transpose_csr(ucsr, U, N), N, U)
    nb_idx, nb_sim = dev_neighbours(csr, R, C, 'cosine', 4, 1, 10)
    if kind == 'user':                                               # (the item-side oracle table at N = 41000 takes too long in Python)
        want_idx, want_sim = ko.neighbours(ko.similarities(csr, R, C, 'cosine', 1, 10), 4)
        assert np.array_equal(nb_idx, want_idx) and np.array_equal(nb_sim.view(np.uint32), want_sim.view(np.uint32))
    uids = np.array([3, 20], np.int32)
    cand = np.ones((2, N), bool)
    out, bits, need = dev_score_rows(kind, 'weighted_mean', ucsr, U, N, nb_idx, nb_sim, uids, cand, None)
    want, has = ko.score_rows(kind, 'weighted_mean', ucsr, N, nb_idx, nb_sim, uids, None)
    assert need > 0 and has.any()
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32)) and np.array_equal(bits, has)


# ---- 4. the public classes on the fixture frame, against the reference ---------------------------------------------------------------
@pytest.fixture(scope='module')
def golden():
    g = load_golden()
    return g, golden_dataset(g)


def _fit(cls_name, ds, **kw):
    from drecpy_amd.Recommender import Baseline
    model = getattr(Baseline, cls_name)(verbose=False, **kw)
    model.fit(ds)
    return model


def test_fitted_tables_against_the_reference(golden):
    g, ds = golden
    for c in g['similarities']:
        if c['k'] != 5 and c['metric'] not in ('adjusted_cosine', 'pearson'):
            continue                                                 # (every metric at one setting, two metrics at all three)
        model = _fit('UserKNN' if c['type'] == 'user' else 'ItemKNN', ds, k=c['k'], m=c['m'], sim_metric=c['metric'], shrinkage=c['shrinkage'])
        R = model.n_users if c['type'] == 'user' else model.n_items
        idx, sim = np.full((R, c['k']), -1, np.int32), np.zeros((R, c['k']), np.float32)
        for i in range(R):
            for t, (s, j) in enumerate(model._neighbours[i]):
                idx[i, t], sim[i, t] = j, s
        ko.check_neighbours_against(reference_matrix(c['lower'], R), idx, sim, TOL)


def test_public_methods_against_the_reference(golden):
    g, ds = golden
    bound = TOL * float(max(g['frame']['interaction']))
    for p in g['predictions']:
        model = _fit('UserKNN' if p['type'] == 'user' else 'ItemKNN', ds, k=p['k'], m=p['m'], sim_metric=p['metric'], shrinkage=p['shrinkage'],
                     aggregation=p['aggregation'], use_averages=p['use_averages'])
        users, items = [u for u, _ in g['pairs']], [i for _, i in g['pairs']]
        got = [model.predict(u, i, skip_errors=True) for u, i in g['pairs']]
        batch = model.predict_pairs(users, items, skip_errors=True)
        for want, one, many in zip(p['predict'], got, batch):
            assert (want is None) == (one is None) == bool(np.isnan(many))
            assert want is None or (abs(one - want) <= bound and one == many)           # predict_pairs equals predict pair for pair
        for user, ref in p['rank'].items():
            ko.check_list_against(ref, model.rank(int(user), g['rank_items'], novelty=False), bound)
            for novelty, ref5 in p['recommend'][user].items():
                mine = model.recommend(int(user), n=5, novelty=novelty == 'True')
                ko.check_list_against(ref5, mine, bound)
                assert model.recommend_batch([int(user)], n=5, novelty=novelty == 'True')[0] == mine
        some = [int(u) for u in list(p['rank'])]
        assert model.recommend_batch(some, n=7) == [model.recommend(u, n=7) for u in some]


def test_evaluation_and_save_load(golden, tmp_path):
    from drecpy_amd.Evaluation import predictive_evaluation, ranking_evaluation
    from drecpy_amd.Recommender import RecommenderABC
    g, ds = golden
    for cls_name in ('ItemKNN', 'UserKNN'):
        model = _fit(cls_name, ds, k=5, m=2, sim_metric='cosine', shrinkage=10)
        kw = dict(n_test_users=20, k=[1, 5], n_pos_interactions=None, n_neg_interactions=None, novelty=False, seed=3, verbose=False)
        fused = ranking_evaluation(model, batched=True, **kw)
        assert fused == ranking_evaluation(model, batched=False, **kw) and fused
        res = predictive_evaluation(model, n_test_predictions=100, skip_errors=True, verbose=False)
        assert set(res) == {'RMSE', 'MSE'} and all(np.isfinite(v) for v in res.values())
        path = os.path.join(tmp_path, cls_name + '.pkl')
        model.save(path)
        again = RecommenderABC.load(path)
        users, items = g['frame']['user'][:200], g['frame']['item'][200:400]
        a, b = model.predict_pairs(users, items, skip_errors=True), again.predict_pairs(users, items, skip_errors=True)
        assert np.array_equal(a, b, equal_nan=True) and again._neighbours == model._neighbours
        assert again.recommend(users[0], n=5) == model.recommend(users[0], n=5)
        assert [again.predict(u, i, skip_errors=True) for u, i in zip(users[:20], items[:20])] == \
               [model.predict(u, i, skip_errors=True) for u, i in zip(users[:20], items[:20])]
