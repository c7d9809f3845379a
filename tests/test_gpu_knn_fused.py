"""The KNN baselines' fused top-n and catalogue ranks on the device: drx_knn_recommend / drx_knn_rank_lists through the C ABI on
hand-made tables and CSRs against tests/knn_rank_oracle.py (on knn_oracle.score_rows) and against the route they replace
(drx_knn_score_rows + drx_topk); then KnnEngine and the public classes.  The predictions are double sums rounded to float32 once, in a
fixed order: every comparison here is exact, ids and float32 bits."""
import os
import types

import numpy as np
import pytest

import knn_oracle as ko
import knn_rank_oracle as kro

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

EINVAL, ESCRATCH, ENOTIMPL = -1, -2, -3
LDS_WIDTH = {'item': 20472, 'user': 10236}        # the widest catalogue whose working row (8 / 16 bytes an item + 64) fits 160 KiB


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.as_tensor(a if len(a) else np.zeros(1, a.dtype)).to('cuda:0')


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_csr(seed, R, C, density, scale=1.0):
    rng = np.random.default_rng(seed)
    mask = rng.random((R, C)) < density
    rows, cols = np.nonzero(mask)
    vals = rng.integers(1, 6, size=len(rows)).astype(np.float32) * np.float32(scale)
    return ko.csr_of(rows, cols, vals, R)


def dev_neighbours(csr, R, C, metric, k, m, shrinkage):
    from drecpy_amd import _lib
    L = _lib.lib()
    ip, ix, v = _dev(csr[0]), _dev(csr[1]), _dev(csr[2])
    need = int(L.drx_knn_neighbours_scratch_bytes(R, C, k, 0))
    sc = torch.empty(need, dtype=torch.uint8, device='cuda:0')
    idx = torch.empty((R, k), dtype=torch.int32, device='cuda:0')
    sim = torch.empty((R, k), dtype=torch.float32, device='cuda:0')
    _lib.check(L.drx_knn_neighbours(_lib.ptr(ip), _lib.ptr(ix), _lib.ptr(v), len(csr[1]), R, C, _lib.KNN_METRICS[metric], k, m, float(shrinkage),
                                    float(ko.max_diff_of(csr, R, C)) or 1.0, 0, _lib.ptr(idx), _lib.ptr(sim), _lib.ptr(sc), need,
                                    _lib.stream_ptr(torch.device('cuda:0'))), 'drx_knn_neighbours')
    return idx.cpu().numpy(), sim.cpu().numpy()


class Dev:
    """a model on the device and the calls into libdrx.so"""

    def __init__(self, kind, ucsr, U, N, nb_idx, nb_sim):
        from drecpy_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.kind, self.ucsr, self.U, self.N, self.nb_idx, self.nb_sim = kind, ucsr, U, N, nb_idx, nb_sim
        self.type = _lib.KNN_USER if kind == 'user' else _lib.KNN_ITEM
        self.d = [_dev(ucsr[0]), _dev(ucsr[1]), _dev(ucsr[2]), _dev(nb_idx), _dev(nb_sim)]
        self.st = _lib.stream_ptr(torch.device('cuda:0'))

    def args(self, agg, type_=None):
        p = self.lib.ptr
        return (self.type if type_ is None else type_, self.lib.KNN_AGGREGATIONS[agg], p(self.d[0]), p(self.d[1]), p(self.d[2]), len(self.ucsr[1]),
                self.U, self.N, p(self.d[3]), p(self.d[4]), self.nb_idx.shape[1])

    def _opt(self, fallback, excl):
        fb = _dev(np.asarray(fallback, np.float64)) if fallback is not None else None
        xp, xi = (_dev(np.asarray(excl[0], np.int64)), _dev(np.asarray(excl[1], np.int32))) if excl is not None else (None, None)
        return fb, xp, xi

    def recommend(self, agg, uids, n, fallback=None, excl=None):
        p = self.lib.ptr
        R = len(uids)
        uid = _dev(np.asarray(uids, np.int32))
        fb, xp, xi = self._opt(fallback, excl)
        need = int(self.L.drx_knn_recommend_scratch_bytes(self.type, R, self.N, n))
        sc = torch.empty(need, dtype=torch.uint8, device='cuda:0') if need else None
        idx = torch.full((R, n), -7, dtype=torch.int32, device='cuda:0')
        val = torch.full((R, n), -7.0, dtype=torch.float32, device='cuda:0')
        self.lib.check(self.L.drx_knn_recommend(*self.args(agg), p(uid), R, n, p(fb), p(xp), p(xi), p(idx), p(val), p(sc), need, self.st),
                       'drx_knn_recommend')
        return idx.cpu().numpy(), val.cpu().numpy(), need

    def rank_lists(self, agg, uids, indptr, targets, fallback=None, excl=None, slack=3):
        p = self.lib.ptr
        R, P = len(uids), len(targets)
        uid, ip, tg = _dev(np.asarray(uids, np.int32)), _dev(np.asarray(indptr, np.int64)), _dev(np.asarray(targets, np.int32))
        fb, xp, xi = self._opt(fallback, excl)
        need = int(self.L.drx_knn_rank_lists_scratch_bytes(self.type, R, P, self.N))
        sc = torch.empty(need, dtype=torch.uint8, device='cuda:0') if need else None
        rank = torch.full((P + slack,), -7, dtype=torch.int32, device='cuda:0')
        score = torch.full((P + slack,), -7.0, dtype=torch.float32, device='cuda:0')
        self.lib.check(self.L.drx_knn_rank_lists(*self.args(agg), p(uid), R, p(ip), p(tg), P, p(fb), p(xp), p(xi), p(rank), p(score), p(sc), need,
                                                 self.st), 'drx_knn_rank_lists')
        rank, score = rank.cpu().numpy(), score.cpu().numpy()
        assert (rank[P:] == -7).all() and (score[P:] == -7.0).all()         # slots from P on are never written
        return rank[:P], score[:P], need

    def by_matrix(self, agg, uids, n, fallback=None, excl=None):
        """the route the fused call replaces: drx_knn_score_rows under a host candidate mask, then drx_topk"""
        from drecpy_amd.engine import pack_mask_bits
        p = self.lib.ptr
        R, N = len(uids), self.N
        cand = np.ones((R, N), bool)
        if excl is not None:
            for r, u in enumerate(uids):
                cand[r, excl[1][excl[0][u]:excl[0][u + 1]]] = False
        uid, mask = _dev(np.asarray(uids, np.int32)), _dev(pack_mask_bits(cand).view(np.int32))
        fb, _, _ = self._opt(fallback, None)
        out = torch.empty((R, N), dtype=torch.float32, device='cuda:0')
        need = int(self.L.drx_knn_score_rows_scratch_bytes(self.type, R, N))
        sc = torch.empty(need, dtype=torch.uint8, device='cuda:0') if need else None
        self.lib.check(self.L.drx_knn_score_rows(*self.args(agg), p(uid), R, p(fb), p(out), p(mask), p(sc), need, self.st), 'drx_knn_score_rows')
        k = min(n, N)
        idx = torch.empty((R, k), dtype=torch.int32, device='cuda:0')
        val = torch.empty((R, k), dtype=torch.float32, device='cuda:0')
        sb = int(self.L.drx_topk_scratch_bytes_k(R, N, k))
        sc2 = torch.empty(sb, dtype=torch.uint8, device='cuda:0') if sb else None
        self.lib.check(self.L.drx_topk(p(out), p(mask), R, N, k, p(idx), p(val), p(sc2), sb, self.st), 'drx_topk')
        idx = np.concatenate([idx.cpu().numpy(), np.full((R, n - k), -1, np.int32)], axis=1)
        val = np.concatenate([val.cpu().numpy(), np.full((R, n - k), -np.inf, np.float32)], axis=1)
        return idx, val

    # ---- the oracle's answers ----
    def scores(self, agg, uids, fallback=None):
        return ko.score_rows(self.kind, agg, self.ucsr, self.N, self.nb_idx, self.nb_sim, np.asarray(uids), fallback)

    def want_topn(self, agg, uids, n, fallback=None, excl=None, scored=None):
        out, has = scored if scored is not None else self.scores(agg, uids, fallback)
        rows = [kro.topn(out[r], has[r], None if excl is None else excl[1][excl[0][u]:excl[0][u + 1]], n) for r, u in enumerate(uids)]
        return np.stack([a for a, _ in rows]), np.stack([b for _, b in rows])

    def want_ranks(self, agg, uids, indptr, targets, fallback=None, excl=None, scored=None):
        out, has = scored if scored is not None else self.scores(agg, uids, fallback)
        rank, score = np.empty(len(targets), np.int32), np.empty(len(targets), np.float32)
        for r, u in enumerate(uids):
            lo, hi = int(indptr[r]), int(indptr[r + 1])
            rank[lo:hi], score[lo:hi] = kro.ranks(out[r], has[r], None if excl is None else excl[1][excl[0][u]:excl[0][u + 1]], targets[lo:hi])
        return rank, score


def assert_same(got, want, what=''):
    assert np.array_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:5], got[0][:2], want[0][:2])
    assert np.array_equal(_bits(got[1]), _bits(want[1])), (what, np.argwhere(_bits(got[1]) != _bits(want[1]))[:5])


def model_of(kind, ucsr, U, N, metric='cosine', k=6, m=2, shrinkage=10):
    csr, R, C = (ucsr, U, N) if kind == 'user' else (ko.transpose_csr(ucsr, U, N), N, U)
    nb_idx, nb_sim = ko.neighbours(ko.similarities(csr, R, C, metric, m, shrinkage), k)
    return Dev(kind, ucsr, U, N, nb_idx, nb_sim)


def random_excl(seed, U, N, density=0.3):
    rng = np.random.default_rng(seed)
    rows, cols = np.nonzero(rng.random((U, N)) < density)
    ip, ix, _ = ko.csr_of(rows, cols, np.ones(len(rows)), U)
    return ip, ix


# ---- 1. the 60 x 37 fixture: against the oracle and against the score-matrix route ---------------------------------------------------
@pytest.fixture(scope='module')
def small():
    """U = 60 users x N = 37 items (ratings / 2: non-integer products), the oracle's tables of both types, as test_gpu_knn.py builds them"""
    U, N = 60, 37
    ucsr = random_csr(21, U, N, 0.3, scale=0.5)
    models = {'user': model_of('user', ucsr, U, N, 'cosine'), 'item': model_of('item', ucsr, U, N, 'adjusted_cosine')}
    return U, N, ucsr, models, random_excl(31, U, N)


UIDS = np.array([0, 59, 17, 17, 33], np.int32)              # a repeated user


@pytest.mark.parametrize('kind,averages', [('user', False), ('item', False), ('item', True)])
@pytest.mark.parametrize('agg', ['mean', 'weighted_mean'])
def test_recommend_against_the_oracle_and_the_old_route(small, kind, agg, averages):
    U, N, ucsr, models, excl = small
    mo = models[kind]
    fb = ko.row_means(ucsr, U) if averages else None
    scored = mo.scores(agg, UIDS, fb)
    assert averages or not scored[1].all()                           # some item without a prediction
    for x in (None, excl):
        for n in (1, 7, N, 128):                                     # n above the eligible count and above n_items: -1 / -inf behind
            got = mo.recommend(agg, UIDS, n, fb, x)
            assert got[2] == 0
            assert_same(got, mo.want_topn(agg, UIDS, n, fb, x, scored), (kind, agg, averages, n))
            assert_same(got, mo.by_matrix(agg, UIDS, n, fb, x), ('old route', kind, agg, averages, n))
            assert np.array_equal(got[0][2], got[0][3]) and np.array_equal(_bits(got[1][2]), _bits(got[1][3]))
        if x is not None:
            for r, u in enumerate(UIDS):
                assert not set(got[0][r].tolist()) & set(x[1][x[0][u]:x[0][u + 1]].tolist())
    assert (got[0][:, -1] == -1).all() and np.isneginf(got[1][:, -1]).all()


def test_a_user_outside_the_model_and_n_outside_the_domain(small):
    U, N, ucsr, models, excl = small
    for kind in ('user', 'item'):
        mo = models[kind]
        fb = ko.row_means(ucsr, U) if kind == 'item' else None
        idx, val, _ = mo.recommend('mean', [5, U, -1, -2 ** 31], 4, fb, excl)
        assert (idx[0] >= 0).any() and (idx[1:] == -1).all() and np.isneginf(val[1:]).all()
        p = mo.lib.ptr
        uid = _dev(UIDS)
        out_i, out_v = torch.full((5, 129), -7, dtype=torch.int32, device='cuda:0'), torch.full((5, 129), -7.0, device='cuda:0')
        assert mo.L.drx_knn_recommend(*mo.args('mean'), p(uid), 5, 129, None, None, None, p(out_i), p(out_v), None, 0, mo.st) == ENOTIMPL
        assert int(out_i.min()) == -7
        assert mo.L.drx_knn_recommend_scratch_bytes(mo.type, 5, 41000, 129) == 0 < mo.L.drx_knn_recommend_scratch_bytes(mo.type, 5, 41000, 128)


# ---- 2. catalogue widths around the wave and the workgroup, integer ratings and plain means: exact ties ------------------------------
@pytest.mark.parametrize('kind', ['user', 'item'])
@pytest.mark.parametrize('N', [1, 63, 64, 65, 255, 256, 257])
def test_catalogue_widths_full_of_ties(kind, N):
    U = 40
    ucsr = random_csr(100 + N, U, N, 0.3)
    mo = model_of(kind, ucsr, U, N, 'cosine', k=5, m=1, shrinkage=10)
    fb = ko.row_means(ucsr, U) if kind == 'item' and N % 2 else None
    uids = np.array([3, 39, 0, 21], np.int32)
    excl = random_excl(200 + N, U, N, 0.2)
    scored = mo.scores('mean', uids, fb)
    tied = 0
    for n in (1, 10, 128):
        got = mo.recommend('mean', uids, n, fb, excl)
        assert_same(got, mo.want_topn('mean', uids, n, fb, excl, scored), (kind, N, n))
        for r in range(len(uids)):                                   # a tie goes to the larger id
            v, i = got[1][r], got[0][r]
            same = (v[1:] == v[:-1]) & (i[1:] >= 0)
            tied += int(same.sum())
            assert (i[:-1][same] > i[1:][same]).all()
    assert tied > 0 or N == 1
    # every item's rank is its position in the unbounded list
    targets = np.tile(np.arange(N, dtype=np.int32), len(uids))
    indptr = np.arange(len(uids) + 1, dtype=np.int64) * N
    rank, score, _ = mo.rank_lists('mean', uids, indptr, targets, fb, excl)
    assert_same((rank, score), mo.want_ranks('mean', uids, indptr, targets, fb, excl, scored), (kind, N))
    if N <= 128:
        idx, val, _ = mo.recommend('mean', uids, N, fb, None)        # (no exclusions: a target's own exclusion is ignored by rank_lists)
        rank, score, _ = mo.rank_lists('mean', uids, indptr, targets, fb, None)
        for r in range(len(uids)):
            for i in range(N):
                at = np.flatnonzero(idx[r] == i)
                assert rank[r * N + i] == (at[0] if len(at) else -1), (r, i)
                assert len(at) == 0 or _bits(score[r * N + i]) == _bits(val[r, at[0]])


# ---- 3. rank_lists on the fixture: the shapes a list may take ------------------------------------------------------------------------
@pytest.mark.parametrize('kind,averages', [('user', False), ('item', False), ('item', True)])
@pytest.mark.parametrize('agg', ['mean', 'weighted_mean'])
def test_rank_lists_against_the_oracle(small, kind, agg, averages):
    U, N, ucsr, models, excl = small
    mo = models[kind]
    fb = ko.row_means(ucsr, U) if averages else None
    rng = np.random.default_rng(5)
    x17 = excl[1][excl[0][17]:excl[0][17 + 1]]
    lists = [rng.permutation(N)[:9].tolist(),                        # unsorted
             [],                                                     # an empty row
             [4, 4, 30, -1, N, 4, 0, N + 100, -5],                   # duplicated, outside the catalogue
             x17[:3].tolist() + [36, 1],                             # excluded targets: ranked as if listed
             rng.integers(0, N, 11).tolist()]
    indptr = np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.int64)
    targets = np.array([t for a in lists for t in a], np.int32)
    scored = mo.scores(agg, UIDS, fb)
    for x in (None, excl):
        got = mo.rank_lists(agg, UIDS, indptr, targets, fb, x)
        assert got[2] == 0
        assert_same(got[:2], mo.want_ranks(agg, UIDS, indptr, targets, fb, x, scored), (kind, agg, averages))
    rank, score = got[:2]
    out_of_range = (targets < 0) | (targets >= N)
    assert (rank[out_of_range] == -1).all() and np.isneginf(score[out_of_range]).all()
    # an excluded target stands where it would stand if it were listed: one more than the listed items ahead of it
    idx, val, _ = mo.recommend(agg, UIDS[3:4], N, fb, excl)
    lo = int(indptr[3])
    for j, t in enumerate(x17[:3]):
        if rank[lo + j] >= 0:
            ahead = [(v, i) for v, i in zip(val[0], idx[0]) if i >= 0 and (v, i) > (score[lo + j], t)]
            assert rank[lo + j] == len(ahead)
    # a user outside the model: no rank at all
    r2, s2, _ = mo.rank_lists(agg, [U, -3], np.array([0, 3, 5]), np.array([0, 1, 2, 3, 4], np.int32), fb, excl)
    assert (r2 == -1).all() and np.isneginf(s2).all()


# ---- 4. rows past LDS: the working rows in the scratch ---------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=[('item', 41000), ('user', 10300), ('item', LDS_WIDTH['item']), ('item', LDS_WIDTH['item'] + 1),
                                        ('user', LDS_WIDTH['user']), ('user', LDS_WIDTH['user'] + 1)], ids=lambda p: f'{p[0]}-{p[1]}')
def wide(request):
    """as test_scores_past_the_lds_row builds them: 24 users, 40 live items among N, the device's table"""
    kind, N = request.param
    U = 24
    rng = np.random.default_rng(8)
    live = np.sort(rng.choice(N, 40, replace=False))
    rows, cols = np.nonzero(rng.random((U, 40)) < 0.4)
    ucsr = ko.csr_of(rows, live[cols], rng.integers(1, 6, len(rows)), U)
    csr, R, C = (ucsr, U, N) if kind == 'user' else (ko.transpose_csr(ucsr, U, N), N, U)
    nb_idx, nb_sim = dev_neighbours(csr, R, C, 'cosine', 4, 1, 10)
    mo = Dev(kind, ucsr, U, N, nb_idx, nb_sim)
    uids = np.array([3, 20], np.int32)
    excl = (ucsr[0], ucsr[1])                                        # the users' own ratings
    return mo, uids, excl, live, mo.scores('weighted_mean', uids, None)


def test_rows_past_the_lds_row(wide):
    mo, uids, excl, live, scored = wide
    past = mo.N > LDS_WIDTH[mo.kind]
    assert scored[1].any()
    for x in (None, excl):
        for n in (10, 128):
            got = mo.recommend('weighted_mean', uids, n, None, x)
            assert (got[2] > 0) == past
            assert_same(got, mo.want_topn('weighted_mean', uids, n, None, x, scored), (mo.kind, mo.N, n))
    targets = np.concatenate([live[::-1], [mo.N - 1, 0, mo.N, -1], live[:5]]).astype(np.int32)
    targets = np.concatenate([targets, targets[::-1]])
    indptr = np.array([0, len(targets) // 2, len(targets)], np.int64)
    for x in (None, excl):
        got = mo.rank_lists('weighted_mean', uids, indptr, targets, None, x)
        assert (got[2] > 0) == past
        assert_same(got[:2], mo.want_ranks('weighted_mean', uids, indptr, targets, None, x, scored), (mo.kind, mo.N))
    assert (got[0] >= 0).any()
    if mo.kind == 'item' and mo.N == 41000:                          # the fallback fills the whole row: n_items eligible items
        fb = ko.row_means(mo.ucsr, mo.U)
        scored = mo.scores('weighted_mean', uids, fb)
        assert_same(mo.recommend('weighted_mean', uids, 128, fb, excl), mo.want_topn('weighted_mean', uids, 128, fb, excl, scored))
        assert_same(mo.rank_lists('weighted_mean', uids, indptr, targets, fb, excl)[:2],
                    mo.want_ranks('weighted_mean', uids, indptr, targets, fb, excl, scored))


# ---- 5. determinism and argument errors -----------------------------------------------------------------------------------------------
def test_the_same_bits_between_calls_and_row_orders(small):
    U, N, ucsr, models, excl = small
    rng = np.random.default_rng(2)
    uids = rng.integers(0, U, 50).astype(np.int32)
    perm = rng.permutation(50)
    lists = [rng.integers(-1, N + 1, int(rng.integers(0, 7))).tolist() for _ in range(50)]

    def flat(order):
        chosen = [lists[r] for r in order]
        return (np.concatenate([[0], np.cumsum([len(a) for a in chosen])]).astype(np.int64), np.array([t for a in chosen for t in a], np.int32))
    for kind in ('user', 'item'):
        mo = models[kind]
        a = mo.recommend('weighted_mean', uids, 9, None, excl)
        b = mo.recommend('weighted_mean', uids, 9, None, excl)
        c = mo.recommend('weighted_mean', uids[perm], 9, None, excl)
        assert_same(a, b)
        assert_same((a[0][perm], a[1][perm]), c)
        ip, tg = flat(range(50))
        ra = mo.rank_lists('weighted_mean', uids, ip, tg, None, excl)
        assert_same(ra[:2], mo.rank_lists('weighted_mean', uids, ip, tg, None, excl)[:2])
        ip2, tg2 = flat(perm)
        rc = mo.rank_lists('weighted_mean', uids[perm], ip2, tg2, None, excl)
        back = np.concatenate([np.arange(ip[r], ip[r + 1]) for r in perm]).astype(np.int64) if len(tg) else np.zeros(0, np.int64)
        assert_same((ra[0][back], ra[1][back]), rc[:2])


def test_argument_errors_and_empty_requests(small):
    U, N, ucsr, models, excl = small
    mo = models['user']
    p = mo.lib.ptr
    uid, fb = _dev(UIDS), _dev(np.zeros(U, np.float64))
    xp, xi = _dev(excl[0]), _dev(excl[1])
    oi, ov = torch.full((5, 4), -7, dtype=torch.int32, device='cuda:0'), torch.full((5, 4), -7.0, device='cuda:0')
    ip, tg = _dev(np.array([0, 1, 2, 3, 4, 5], np.int64)), _dev(np.arange(5, dtype=np.int32))
    orank, oscore = torch.full((5,), -7, dtype=torch.int32, device='cuda:0'), torch.full((5,), -7.0, device='cuda:0')
    L = mo.L

    def rec(args=None, R=5, n=4, fallback=None, out=(oi, ov), scratch=None, nbytes=0, x=(None, None)):
        return L.drx_knn_recommend(*(args or mo.args('mean')), p(uid), R, n, p(fallback), p(x[0]), p(x[1]), p(out[0]), p(out[1]), p(scratch), nbytes,
                                   mo.st)

    def rnk(args=None, R=5, P=5, fallback=None, out=(orank, oscore), scratch=None, nbytes=0):
        return L.drx_knn_rank_lists(*(args or mo.args('mean')), p(uid), R, p(ip), p(tg), P, p(fallback), None, None, p(out[0]), p(out[1]),
                                    p(scratch), nbytes, mo.st)
    assert rec(fallback=fb) == EINVAL == rnk(fallback=fb)                              # a fallback with DRX_KNN_USER
    assert rec(args=mo.args('mean', type_=2)) == EINVAL == rnk(args=mo.args('mean', type_=2))
    assert rec(out=(None, ov)) == EINVAL == rec(out=(oi, None)) and rnk(out=(None, oscore)) == EINVAL == rnk(out=(orank, None))
    assert rec(n=0) == EINVAL and rec(x=(xp, None)) == EINVAL
    assert int(oi.min()) == -7 and int(orank.min()) == -7
    assert rec(R=0) == 0 and rnk(R=0) == 0 and rnk(P=0) == 0                            # nothing to do: nothing written
    assert int(oi.min()) == -7 and float(ov.max()) == -7.0 and int(orank.min()) == -7 and float(oscore.max()) == -7.0
    assert rec() == 0 and rnk() == 0 and int(oi.max()) >= 0
    # a short scratch, where one is needed
    wide = Dev('user', ucsr, U, LDS_WIDTH['user'] + 1, mo.nb_idx, mo.nb_sim)
    need = int(L.drx_knn_recommend_scratch_bytes(wide.type, 5, wide.N, 4))
    assert need > 0 and need == int(L.drx_knn_rank_lists_scratch_bytes(wide.type, 5, 5, wide.N))
    sc = torch.empty(need, dtype=torch.uint8, device='cuda:0')
    assert rec(args=wide.args('mean'), scratch=sc, nbytes=need - 1) == ESCRATCH == rec(args=wide.args('mean'))
    assert rnk(args=wide.args('mean'), scratch=sc, nbytes=need - 1) == ESCRATCH == rnk(args=wide.args('mean'))
    assert rec(args=wide.args('mean'), scratch=sc, nbytes=need) == 0 and rnk(args=wide.args('mean'), scratch=sc, nbytes=need) == 0
    torch.cuda.synchronize()


# ---- 6. the engine past LDS in chunks, and the public classes --------------------------------------------------------------------------
def test_engine_chunks_rows_past_lds(wide):
    """(at the widths that fit LDS there is no scratch and nothing to chunk: one launch whatever chunk_bytes says)"""
    from drecpy_amd.engine_knn import KnnEngine
    mo, uids, excl, live, scored = wide
    eng = KnnEngine(mo.U, mo.N, mo.kind)
    eng.set_interactions(mo.ucsr, ko.transpose_csr(mo.ucsr, mo.U, mo.N))
    eng.set_table(mo.nb_idx, mo.nb_sim)
    eng.set_exclusions(*excl)
    users = np.array([3, 20, 20, 7, 3], np.int32)
    one = [eng.recommend(users, 6, 'weighted_mean', exclude=True, chunk_bytes=b) for b in (None, 1, 3 * 16 * mo.N)]
    for idx, val in one[1:]:
        assert torch.equal(idx, one[0][0]) and torch.equal(val.view(torch.int32), one[0][1].view(torch.int32))
    assert_same((one[0][0].cpu().numpy()[:2], one[0][1].cpu().numpy()[:2]), mo.want_topn('weighted_mean', uids, 6, None, excl, scored))
    indptr, targets = np.array([0, 3, 3, 8, 9, 12]), np.concatenate([live[:12]]).astype(np.int32)
    two = [eng.rank_lists(users, indptr, targets, 'weighted_mean', exclude=True, chunk_bytes=b) for b in (None, 1, 3 * 16 * mo.N)]
    for rank, score in two[1:]:
        assert torch.equal(rank, two[0][0]) and torch.equal(score.view(torch.int32), two[0][1].view(torch.int32))
    assert_same((two[0][0].cpu().numpy()[:3], two[0][1].cpu().numpy()[:3]),
                mo.want_ranks('weighted_mean', uids[:1], indptr[:2], targets[:3], None, excl, (scored[0][:1], scored[1][:1])))


@pytest.fixture(scope='module')
def frame():
    from drecpy_amd.Dataset import InteractionDataset
    rng = np.random.default_rng(13)
    rows, cols = np.nonzero(rng.random((40, 140)) < 0.12)                   # more than 128 items: n=None is a longer list
    rows, cols = np.concatenate([rows, [0]]), np.concatenate([cols, [139]])          # (the corner exists whatever the draw)
    rows, cols = np.unique(np.stack([rows, cols]), axis=1)
    fr = {'user': 100 + rows, 'item': 500 + cols, 'interaction': rng.integers(1, 6, len(rows)).astype(np.float64)}
    ds = InteractionDataset.read_df(fr, verbose=False)
    return fr, ds


def _spied(model):
    calls = {'recommend': 0, 'rank_lists': 0, 'score_rows': 0}
    eng = model._engine
    for name in calls:
        def wrap(*a, _f=getattr(type(eng), name), _n=name, **k):
            calls[_n] += 1
            return _f(eng, *a, **k)
        setattr(eng, name, wrap)
    return calls


def _check_public(model, fr):
    from drecpy_amd.Evaluation import recommendation_evaluation
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender import RecommenderABC
    calls = _spied(model)
    users = [100, 139, 117, 117, 105, 121]
    for novelty in (True, False):
        got = model.recommend_batch(users, n=7, novelty=novelty)
        assert calls == {'recommend': 1, 'rank_lists': 0, 'score_rows': 0}, calls      # one fused call, no score matrix
        calls['recommend'] = 0
        assert got == [model.recommend(u, n=7, novelty=novelty) for u in users] and any(got)
        calls['score_rows'] = 0
    every = model.recommend_batch(users, n=None)                                       # a longer list: the score-matrix route
    assert calls['recommend'] == 0 and calls['score_rows'] > 0
    assert every == [model.recommend(u, n=None) for u in users]
    model._engine.fused = False
    assert model.recommend_batch(users, n=7) == [a[:7] for a in every]
    model._engine.fused = True
    # pairs: repeated users, an unknown item, an excluded pair (the user's own rating), items without a prediction among the rest
    rng = np.random.default_rng(3)
    pu = [100, 100, 117, 139, 117, 100, 105] + rng.choice(fr['user'], 60).tolist()
    pi = [fr['item'][list(fr['user']).index(100)], 99999, 559, 500, 559, 501, 530] + (500 + rng.integers(0, 140, 60)).tolist()
    for novelty in (True, False):
        calls.update(recommend=0, rank_lists=0, score_rows=0)
        rank, score = model.catalogue_ranks(pu, pi, novelty=novelty, return_scores=True)
        assert calls == {'recommend': 0, 'rank_lists': 1, 'score_rows': 0}, calls
        model._catalogue_ranks = types.MethodType(RecommenderABC._catalogue_ranks, model)     # the base class's per-user loop
        want_rank, want_score = model.catalogue_ranks(pu, pi, novelty=novelty, return_scores=True)
        del model._catalogue_ranks
        assert rank.dtype == np.int64 and score.dtype == np.float64
        assert np.array_equal(rank, want_rank) and np.array_equal(score, want_score), (novelty, rank, want_rank)
        assert rank[1] == -1 and (rank[0] == -1 or not novelty) and (rank >= 0).any()
        assert np.array_equal(model.catalogue_ranks(pu, pi, novelty=novelty), rank)
    with pytest.raises(Exception):
        model.catalogue_ranks([100, 7], [500, 500])
    with pytest.raises(Exception):
        model.recommend_batch([7], n=3)
    test = {'user': np.array(pu), 'item': np.array(pi), 'interaction': np.ones(len(pu))}
    keep = np.unique(np.stack([test['user'], test['item']]), axis=1, return_index=True)[1]
    ds_te = InteractionDataset.read_df({k: v[np.sort(keep)] for k, v in test.items()}, verbose=False)
    for kw in (dict(k=[1, 5, 10]), dict(k=[1, 5, 10], n_pos_interactions=2, seed=4)):
        for novelty in (True, False):
            a = recommendation_evaluation(model, ds_te, novelty=novelty, verbose=False, batched=True, **kw)
            b = recommendation_evaluation(model, ds_te, novelty=novelty, verbose=False, batched='ranks', **kw)
            assert a == b and a
    for name in calls:
        delattr(model._engine, name)


@pytest.mark.parametrize('cls_name', ['ItemKNN', 'UserKNN'])
@pytest.mark.parametrize('averages', [False, True])
def test_public_classes(frame, tmp_path, cls_name, averages):
    from drecpy_amd.Recommender import Baseline, RecommenderABC
    fr, ds = frame
    model = getattr(Baseline, cls_name)(k=5, m=1, sim_metric='cosine', shrinkage=10, use_averages=averages, verbose=False)
    model.fit(ds)
    _check_public(model, fr)
    path = os.path.join(tmp_path, cls_name + '.pkl')
    model.save(path)
    again = RecommenderABC.load(path)
    assert getattr(again._engine, '_excl', None) is None                               # a new engine: the exclusions go up again
    _check_public(again, fr)
    users = [100, 117, 139]
    assert again.recommend_batch(users, n=7) == model.recommend_batch(users, n=7)
