"""ALS / WMF on the device against tests/als_oracle.py, through the C ABI (drx_als_gram, drx_als_solve_rows, drx_als_loss), AlsEngine and
the public class (drecpy_amd.Recommender.Baseline.ALS).

The gate of a solve is NOT the project's fixed 1e-5: the error of an fp32 Cholesky scales with the conditioning of a row's system.  The
oracle is therefore run twice on the same float32 inputs, in float64 (the reference) and in float32 (the replay); with
err(a) = max |a - reference| / max(1, max |reference|) the test asserts

    err(GPU) <= max(1e-5, 4 err(replay))

— both are fp32 solves of the same systems, bounded by the same cond x eps product, and differ only in summation order, which moves
the realised error by a small factor.  (drx_als_solve_rows adds one refinement step on a residual summed in double, so its errors lie
well below the replay's; the gate stays the issue's.)  The loss uses the relative error and the floor 1e-6.  Every (GPU, replay) pair
is printed.

Frames: dense-random, ratings 1..5, alpha = 40, lambda = 0.1.  Each has a user row and an item column without positives and a FULL
user row.  A full row and an empty column cannot meet in one matrix: the full row holds every item but the empty column (degree
n_items - 1); the one-row frame is the row of degree n_items exactly."""
import ctypes as C

import numpy as np
import pytest

import als_oracle as ao

pytestmark = pytest.mark.gpu

F, D = np.float32, np.float64
LAM, ALPHA = 0.1, 40.0
EINVAL, ESCRATCH = -1, -2
SHAPES = [(37, 53, 1), (37, 53, 5), (70, 90, 64), (150, 200, 128)]
DEGREES = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300]


def _dev(a, dtype):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to('cuda:0')


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


def _padded(a, ld):
    out = np.zeros((a.shape[0], ld), F)
    out[:, :a.shape[1]] = a
    return out


def _err(got, want):
    got, want = np.asarray(got, D), np.asarray(want, D)
    return float(np.max(np.abs(got - want))) / max(1.0, float(np.max(np.abs(want))))


def _gate(what, gpu, replay, floor=1e-5):
    bound = max(floor, 4.0 * replay)
    print(f'{what}: GPU error {gpu:.3e}, replay error {replay:.3e} (gate {bound:.3e})')
    assert gpu <= bound, f'{what}: GPU error {gpu:.3e} > {bound:.3e} (replay {replay:.3e})'


def _scratch(n=1 << 20):
    import torch
    return torch.zeros(n, dtype=torch.uint8, device='cuda:0')


def _gram(table, ld):
    """G [ld, ld] of a host [n, K] table through drx_als_gram"""
    import torch
    from drecpy_amd._lib import check, lib, ptr
    t = _dev(_padded(np.asarray(table, F), ld), F)
    need = int(lib().drx_als_gram_scratch_bytes(t.shape[0], ld))
    assert need > 0
    sc = _scratch(need)
    G = torch.full((ld, ld), 7.0, dtype=torch.float32, device='cuda:0')
    check(lib().drx_als_gram(ptr(t), t.shape[0], ld, ptr(G), ptr(sc), need, None), 'drx_als_gram')
    torch.cuda.synchronize()
    return G


def _half(other, csr, lam, order=None, n_rows=None):
    """(out [n_rows, ld] as numpy, fail_count) of one half-step through drx_als_gram + drx_als_solve_rows; order: None or int32 [n_rows]"""
    import torch
    from drecpy_amd._lib import check, lib, ptr
    indptr, indices, w = csr
    K = other.shape[1]
    ld = (K + 3) // 4 * 4
    n_rows = len(indptr) - 1
    G = _gram(other, ld)
    o = _dev(_padded(np.asarray(other, F), ld), F)
    ip, ix, ww = _dev(indptr, np.int64), _dev(indices if len(indices) else [0], np.int32), _dev(w if len(w) else [0], F)
    od = _dev(order, np.int32) if order is not None else None
    out = torch.full((n_rows, ld), 7.0, dtype=torch.float32, device='cuda:0')
    fail = torch.zeros(1, dtype=torch.int32, device='cuda:0')
    need = int(lib().drx_als_solve_rows_scratch_bytes(n_rows, o.shape[0], ld))
    sc = _scratch(need)
    check(lib().drx_als_solve_rows(ptr(out), ptr(o), ptr(G), ptr(ip), ptr(ix), ptr(ww), ptr(od) if od is not None else None, n_rows,
                                   o.shape[0], ld, lam, ptr(fail), ptr(sc), need, None), 'drx_als_solve_rows')
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(fail.cpu().numpy()[0])


# ---- frames and their oracle results, computed once ------------------------------------------------------------------------------------
_CACHE = {}


def _case(U, N, K):
    """frame, fp32-exact start, and the float64 / float32 oracle fits after 1 and 6 sweeps"""
    key = (U, N, K)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 + K)
        frame = ao.random_frame(rng, U, N, density=0.3, alpha=ALPHA, empty_user=1, empty_item=9, full_user=0)
        deg = np.diff(frame.csr[0])
        assert deg[0] == N - 1 and deg[1] == 0 and np.diff(frame.csr_t[0])[9] == 0
        p0 = ao.init_params(rng, U, N, K)
        fits = {}
        for dtype in (D, F):
            p, fits[dtype] = {k: v.astype(dtype) for k, v in p0.items()}, {}
            for s in range(1, 7):
                ao.sweep(p, frame, LAM, dtype)
                if s in (1, 2, 3, 6):
                    fits[dtype][s] = ({k: v.copy() for k, v in p.items()}, ao.loss(p, frame, LAM, dtype))
        _CACHE[key] = (frame, p0, fits)
    return _CACHE[key]


def _engine(frame, K, p0, lam=LAM):
    from drecpy_amd.engine_als import AlsEngine
    e = AlsEngine(frame.n_users, frame.n_items, K)
    e.reg = lam
    e.set_frame(frame.csr[:2], frame.csr_t[:2], frame.csr[2], frame.csr_t[2])
    e.set_params(p0)
    return e


# ---- the Gram matrix ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 5, 64, 128])
@pytest.mark.parametrize('n_rows', [1, 7, 200, 4099])
def test_gram_of_small_integers_is_exact(n_rows, K):
    """every fp32 partial sum is an integer below 2^24 (4099 x 9), so G is the int64 product bit for bit, whatever the order"""
    T = np.random.default_rng(n_rows * 131 + K).integers(-3, 4, size=(n_rows, K))
    ld = (K + 3) // 4 * 4
    G = _gram(T.astype(F), ld).cpu().numpy()
    want = np.zeros((ld, ld), np.int64)
    want[:K, :K] = T.T.astype(np.int64) @ T.astype(np.int64)
    assert np.array_equal(G.astype(np.int64), want) and np.array_equal(G, want.astype(F))
    assert np.array_equal(_bits(G), _bits(G.T))


# ---- one half-step -----------------------------------------------------------------------------------------------------------------------
def _half_step_pair(other, csr, lam, what):
    """GPU against the float64 oracle, gated by the float32 replay; returns the GPU rows"""
    o32 = np.asarray(other, F)
    want = ao.half_step(o32.astype(D), csr, lam, D)
    replay = ao.half_step(o32, csr, lam, F)
    got, failed = _half(o32, csr, lam)
    assert failed == 0
    K = o32.shape[1]
    assert not got[:, K:].any(), 'a padding column is not zero'
    _gate(what, _err(got[:, :K], want), _err(replay, want))
    return got


@pytest.mark.parametrize('U, N, K', SHAPES)
def test_half_step_matches_the_oracle(U, N, K):
    frame, p0, fits = _case(U, N, K)
    # from factors of working size (those after one float64 sweep), both halves
    p1 = fits[D][1][0]
    x = _half_step_pair(p1['Y'], frame.csr, LAM, f'{U} x {N} K {K} user half')
    y = _half_step_pair(p1['X'], frame.csr_t, LAM, f'{U} x {N} K {K} item half')
    assert not x[1].any() and not y[9].any(), 'a row without positives is not exactly zero'
    assert x[0].any() and y[8].any()


def test_half_step_at_a_small_lambda():
    frame, _, fits = _case(70, 90, 64)
    _half_step_pair(fits[D][1][0]['Y'], frame.csr, 1e-3, '70 x 90 K 64 user half, lambda 1e-3')


def _degree_frame():
    rng = np.random.default_rng(5)
    W = np.zeros((len(DEGREES), 300))
    for u, d in enumerate(DEGREES):
        W[u, rng.choice(300, size=d, replace=False)] = ALPHA * rng.integers(1, 6, size=d)
    frame = ao.Frame(W)
    assert np.diff(frame.csr[0]).tolist() == DEGREES
    return frame


@pytest.mark.parametrize('K', [5, 64])
def test_row_degrees_around_every_chunk_border(K):
    frame = _degree_frame()
    Y = ao.init_params(np.random.default_rng(K), 1, 300, K, std=0.3)['Y']
    got = _half_step_pair(Y, frame.csr, LAM, f'degrees 0 .. 300, K {K}')
    assert not got[0].any() and all(got[u].any() for u in range(1, len(DEGREES)))


@pytest.mark.parametrize('K', [1, 5, 64])
def test_a_frame_of_one_full_row(K):
    rng = np.random.default_rng(K)
    frame = ao.Frame(ALPHA * rng.integers(1, 6, size=(1, 53)))
    assert np.diff(frame.csr[0]).tolist() == [53]
    p = ao.init_params(rng, 1, 53, K, std=0.3)
    _half_step_pair(p['Y'], frame.csr, LAM, f'one row, K {K}, user half')
    _half_step_pair(p['X'], frame.csr_t, LAM, f'one row, K {K}, item half')


def test_orders_and_repeated_runs_give_equal_bits():
    frame = _degree_frame()
    Y = ao.init_params(np.random.default_rng(3), 1, 300, 20, std=0.3)['Y']
    n = len(DEGREES)
    runs = [_half(Y, frame.csr, LAM, order)[0] for order in (None, None, np.arange(n), np.argsort(-np.asarray(DEGREES), kind='stable'))]
    assert runs[0][1:].any()
    for r in runs[1:]:
        assert np.array_equal(_bits(r), _bits(runs[0]))
    # an order that names a row outside the table skips it and nothing else
    partial, failed = _half(Y, frame.csr, LAM, np.array([n + 3, -1] + list(range(2, n))))
    assert failed == 0 and np.array_equal(_bits(partial[2:]), _bits(runs[0][2:])) and (partial[:2] == 7.0).all()


def test_a_failed_factorisation_is_counted_and_zeroed():
    import torch
    frame = ao.Frame(np.array([[0, 40.0, 0, 80.0], [0, 0, 0, 0]]))
    got, failed = _half(np.zeros((4, 5), F), frame.csr, 0.0)
    assert failed == 1 and not got.any()
    assert torch.cuda.current_stream().query() and torch.zeros(1, device='cuda:0').cpu().numpy()[0] == 0     # no error is pending
    # the class level: a sweep whose first half fails says which half and how many rows
    from drecpy_amd._lib import DrxError
    e = _engine(frame, 5, {'X': np.zeros((2, 5)), 'Y': np.zeros((4, 5))}, lam=0.0)
    with pytest.raises(DrxError, match=r'user half met 1 row'):
        e.sweep()


# ---- whole fits --------------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _device_fit(U, N, K):
    """{sweeps: (params, loss, padding is zero)} after 1 and 6 sweeps of one engine, and its score matrix after the sixth"""
    key = (U, N, K)
    if key not in _RUNS:
        frame, p0, _ = _case(U, N, K)
        e = _engine(frame, K, p0)
        out = {}
        for s in range(1, 7):
            L = e.sweep(want_loss=True)
            if s in (1, 6):
                out[s] = (e.get_params(), L, not e.X[:, K:].cpu().numpy().any() and not e.Y[:, K:].cpu().numpy().any())
        out['score_matrix'] = e.score_matrix(np.arange(U, dtype=np.int32)).cpu().numpy()
        _RUNS[key] = out
    return _RUNS[key]


@pytest.mark.parametrize('U, N, K', SHAPES)
def test_scores_match_the_oracle_fit_after_1_and_6_sweeps(U, N, K):
    _, _, fits = _case(U, N, K)
    run = _device_fit(U, N, K)
    for s in (1, 6):
        got, _, padding_zero = run[s]
        p64, p32 = fits[D][s][0], fits[F][s][0]
        _gate(f'{U} x {N} K {K} scores after {s} sweep(s)', _err(ao.scores(got), ao.scores(p64)), _err(ao.scores(p32), ao.scores(p64)))
        assert padding_zero, 'a padding column moved'
        assert not got['X'][1].any() and not got['Y'][9].any()
    assert _err(run['score_matrix'], ao.scores(run[6][0])) <= 1e-5


@pytest.mark.parametrize('U, N, K', SHAPES)
def test_loss_matches_the_oracle_fit_after_1_and_6_sweeps(U, N, K):
    """The relative error of the logged loss against the float64 fit, gated by max(1e-6, 4 x the float32 replay's).  Without the
    refinement step of drx_als_solve_rows the case [70-90-64] missed this gate after 6 sweeps (7.0e-4 against a replay of 8.2e-5): the
    loss is ONE number, and two fp32 fits that drift alike from the float64 one need not project that drift alike on it.  With the
    step the device's error is 20 x or more below the replay's wherever that exceeds 1e-6 (2.2e-6 here)."""
    _, _, fits = _case(U, N, K)
    run = _device_fit(U, N, K)
    for s in (1, 6):
        L, L64, L32 = run[s][1], fits[D][s][1], fits[F][s][1]
        _gate(f'{U} x {N} K {K} loss after {s} sweep(s)', abs(L - L64) / abs(L64), abs(L32 - L64) / abs(L64), floor=1e-6)


def test_two_fits_give_equal_bits():
    frame, p0, _ = _case(37, 53, 5)
    runs = []
    for _ in range(2):
        e = _engine(frame, 5, p0)
        losses = [e.sweep(want_loss=True) for _ in range(3)]
        runs.append((e.X.cpu().numpy().copy(), e.Y.cpu().numpy().copy(), np.array(losses)))
    assert all(np.array_equal(a.view(np.int64) if a.dtype == D else _bits(a), b.view(np.int64) if b.dtype == D else _bits(b))
               for a, b in zip(*runs))
    assert runs[0][2][2] < runs[0][2][0]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    import torch
    from drecpy_amd._lib import lib, ptr
    L_ = lib()
    frame, p0, _ = _case(37, 53, 5)
    ld = 8
    X, Y = _dev(_padded(p0['X'].astype(F), ld), F), _dev(_padded(p0['Y'].astype(F), ld), F)
    ip, ix, w = _dev(frame.csr[0], np.int64), _dev(frame.csr[1], np.int32), _dev(frame.csr[2], F)
    G = torch.full((ld, ld), 7.0, dtype=torch.float32, device='cuda:0')
    out = torch.full((37, ld), 7.0, dtype=torch.float32, device='cuda:0')
    fail = torch.zeros(1, dtype=torch.int32, device='cuda:0')
    loss = torch.full((1,), 7.0, dtype=torch.float64, device='cuda:0')
    sc = _scratch(1 << 16)
    off = lambda t: C.c_void_p(t.data_ptr() + 4)
    lds = {'ld 0': 0, 'ld 2': 2, 'ld 6': 6, 'ld 132': 132, 'ld -4': -4}
    lams = {'lambda < 0': -0.1, 'lambda nan': float('nan'), 'lambda inf': float('inf')}

    for bad in ((0, ld), (-1, ld), (5, 0), (5, 6), (5, 132)):
        assert L_.drx_als_gram_scratch_bytes(*bad) == 0, bad
    for bad in ((0, 5, ld), (5, 0, ld), (5, 5, 2), (5, 5, 132)):
        assert L_.drx_als_solve_rows_scratch_bytes(*bad) == 0, bad
    for bad in ((0, ld), (5, 6), (5, 132)):
        assert L_.drx_als_loss_scratch_bytes(*bad) == 0, bad

    good = [ptr(Y), 53, ld, ptr(G), ptr(sc), sc.numel(), None]
    bad = {'table': (0, None), 'out_G': (3, None), 'scratch': (4, None), 'n_rows 0': (1, 0), 'n_rows -2': (1, -2), 'misaligned table': (0, off(Y)),
           'misaligned out_G': (3, off(G)), **{k: (2, v) for k, v in lds.items()}}
    for what, (at, value) in bad.items():
        args = list(good)
        args[at] = value
        assert L_.drx_als_gram(*args) == EINVAL, what
    need = int(L_.drx_als_gram_scratch_bytes(53, ld))
    args = list(good)
    args[5] = need - 1
    assert L_.drx_als_gram(*args) == ESCRATCH
    torch.cuda.synchronize()
    assert (G.cpu().numpy() == 7.0).all() and not sc.cpu().numpy().any(), 'a refused gram call wrote'
    args[5] = need
    assert L_.drx_als_gram(*args) == 0

    good = [ptr(out), ptr(Y), ptr(G), ptr(ip), ptr(ix), ptr(w), None, 37, 53, ld, LAM, ptr(fail), ptr(sc), sc.numel(), None]
    bad = {'out': (0, None), 'other': (1, None), 'G': (2, None), 'indptr': (3, None), 'indices': (4, None), 'weights': (5, None),
           'fail_count': (11, None), 'scratch': (12, None), 'n_rows 0': (7, 0), 'n_other 0': (8, 0), 'misaligned out': (0, off(out)),
           'misaligned other': (1, off(Y)), 'misaligned G': (2, off(G)), **{k: (9, v) for k, v in lds.items()},
           **{k: (10, v) for k, v in lams.items()}}
    for what, (at, value) in bad.items():
        args = list(good)
        args[at] = value
        assert L_.drx_als_solve_rows(*args) == EINVAL, what
    need = int(L_.drx_als_solve_rows_scratch_bytes(37, 53, ld))
    args = list(good)
    args[13] = need - 1
    assert L_.drx_als_solve_rows(*args) == ESCRATCH
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all() and fail.cpu().numpy()[0] == 0, 'a refused solve wrote'
    assert L_.drx_als_solve_rows(*good) == 0
    torch.cuda.synchronize()
    assert not (out.cpu().numpy() == 7.0).any() and fail.cpu().numpy()[0] == 0

    good = [ptr(X), ptr(Y), ptr(G), ptr(G), ptr(ip), ptr(ix), ptr(w), 37, 53, ld, LAM, ptr(loss), ptr(sc), sc.numel(), None]
    bad = {'X': (0, None), 'Y': (1, None), 'Gx': (2, None), 'Gy': (3, None), 'indptr': (4, None), 'indices': (5, None), 'weights': (6, None),
           'out_loss': (11, None), 'scratch': (12, None), 'n_users 0': (7, 0), 'n_items 0': (8, 0), 'misaligned X': (0, off(X)),
           'misaligned Gy': (3, off(G)), **{k: (9, v) for k, v in lds.items()}, **{k: (10, v) for k, v in lams.items()}}
    for what, (at, value) in bad.items():
        args = list(good)
        args[at] = value
        assert L_.drx_als_loss(*args) == EINVAL, what
    need = int(L_.drx_als_loss_scratch_bytes(37, ld))
    args = list(good)
    args[13] = need - 1
    assert L_.drx_als_loss(*args) == ESCRATCH
    torch.cuda.synchronize()
    assert loss.cpu().numpy()[0] == 7.0, 'a refused loss call wrote'
    assert L_.drx_als_loss(*good) == 0
    torch.cuda.synchronize()
    assert loss.cpu().numpy()[0] != 7.0


def test_engine_refuses_factors_outside_its_domain_and_negative_weights():
    from drecpy_amd._lib import DrxError
    from drecpy_amd.engine_als import AlsEngine
    for K in (0, 129, 2.5):
        with pytest.raises(DrxError, match='factors'):
            AlsEngine(37, 53, K)
    frame, _, _ = _case(37, 53, 5)
    e = AlsEngine(37, 53, 5)
    with pytest.raises(DrxError, match='negative weight'):
        e.set_frame(frame.csr[:2], frame.csr_t[:2], -frame.csr[2], frame.csr_t[2])


# ---- the public class --------------------------------------------------------------------------------------------------------------------
CU, CN, CK, THR = 70, 90, 64, 1.0


def _class_pairs():
    """the 70 x 90 frame as (user, item, rating) rows in first-appearance order (internal id == raw id), with entries BELOW the
    threshold that are recorded but no positives: user 0's at the empty item 9, the positive-less user 1's only entry, one of user 5"""
    frame, _, _ = _case(CU, CN, CK)
    R = frame.W / ALPHA
    R[0, 9], R[1, 4] = 0.5, 0.5
    low5 = int(np.flatnonzero(R[5] == 0)[0])
    R[5, low5] = 0.5
    u, i = np.nonzero(R)
    assert np.array_equal(np.unique(u), np.arange(CU)) and np.array_equal(i[u == 0], np.arange(CN))
    return u, i, R[u, i], low5


def _dataset():
    from drecpy_amd.Dataset import InteractionDataset
    u, i, r, _ = _class_pairs()
    return InteractionDataset.from_arrays(u.astype(np.int64), i.astype(np.int64), r.astype(np.float64))


def _class_gate(what, got_scores, sweeps):
    _, _, fits = _case(CU, CN, CK)
    want = ao.scores(fits[D][sweeps][0])
    _gate(what, _err(got_scores, want), _err(ao.scores(fits[F][sweeps][0]), want))
    return want


def _all_scores(model):
    return model._engine.score_matrix(np.arange(CU, dtype=np.int32)).cpu().numpy()


@pytest.fixture(scope='module')
def fitted():
    from drecpy_amd.Recommender.Baseline import ALS
    _, p0, _ = _case(CU, CN, CK)
    model = ALS(factors=CK, alpha=ALPHA, seed=3, interaction_threshold=THR, verbose=False)
    model.fit(_dataset(), epochs=3, reg_rate=LAM, initial_weights=p0, batch_size=7, learning_rate=123.0, neg_ratio=0)
    ds = model.interaction_dataset
    assert all(ds.user_to_uid(u) == u for u in range(CU)) and all(ds.item_to_iid(i) == i for i in range(CN))
    return model


def test_fit_equals_the_oracle_fit_from_the_same_weights(fitted):
    _class_gate('ALS.fit(epochs=3) scores', _all_scores(fitted), 3)
    assert isinstance(fitted.predict(5, 7), float)
    assert fitted.predict(5, 7) == pytest.approx(float(_all_scores(fitted)[5, 7]), abs=1e-5)       # (the pair scorer against drx_rows_dot)
    e = fitted._engine
    assert not e.X[:, CK:].cpu().numpy().any() and not e.X[1].cpu().numpy().any() and not e.Y[9].cpu().numpy().any()


def test_the_logged_loss_is_the_oracle_loss():
    from drecpy_amd.Recommender.Baseline import ALS
    from drecpy_amd.Recommender.early_stopping import MaxValidationValueRule
    _, p0, fits = _case(CU, CN, CK)
    model = ALS(factors=CK, alpha=ALPHA, interaction_threshold=THR, verbose=False)
    model.fit(_dataset(), epochs=2, reg_rate=LAM, initial_weights=p0, early_stopping_rule=MaxValidationValueRule('x'), early_stopping_freq=99)
    got = model._loss_tracker.epoch_losses
    assert len(got) == 2
    for s in (1, 2):
        L64, L32 = fits[D][s][1], fits[F][s][1]
        _gate(f'logged loss of epoch {s}', abs(got[s - 1] - L64) / abs(L64), abs(L32 - L64) / abs(L64), floor=1e-6)


def test_recommend_batch_equals_recommend(fitted):
    """The two calls score on two arithmetics (the fused scorer's k-ordered fmaf chain, drx_rows_dot), so a score may differ in its last
    bits and items whose scores lie closer than that may change places — recommend_batch's documented behaviour.  ALS makes such
    near-ties likely: with K = 64 above a user's ~27 positives every positive is fitted to a score just below 1.  So: the values agree
    position by position, and the items agree wherever their scores are further apart than TIE = 64 x 2^-24 (K products of a score of
    order 1, each rounded once); where lists differ, both items at that position have scores within TIE of each other."""
    _, _, _, low5 = _class_pairs()
    users = [0, 1, 2, 5, 17, 69, 5]
    TIE = 64 * 2.0 ** -24
    S = _all_scores(fitted)
    _, _, fits = _case(CU, CN, CK)
    x64 = ao.scores(fits[D][3][0])
    scale = max(1.0, float(np.max(np.abs(x64))))
    gate = max(1e-5, 4 * _err(ao.scores(fits[F][3][0]), x64))
    for novelty in (True, False):
        lists = fitted.recommend_batch(users, n=10, novelty=novelty)
        for u, got in zip(users, lists):
            one = fitted.recommend(u, n=10, novelty=novelty)
            allowed = [i for i in range(CN) if not (novelty and i in fitted._recorded_items(u))]
            assert len(got) == len(one) == min(10, len(allowed)) and all(i in allowed for _, i in got)
            for (_, a), (_, b) in zip(got, one):
                assert a == b or abs(float(S[u, a]) - float(S[u, b])) <= TIE, (u, novelty, a, b, S[u, a], S[u, b])
            assert np.allclose([s for s, _ in got], [s for s, _ in one], rtol=0, atol=TIE)
            assert np.allclose([s for s, _ in got], [S[u, i] for _, i in got], rtol=0, atol=TIE)
            if not got:
                continue
            # against the float64 oracle fit, as test_gpu_bpr.py does: the values inside the gate, the oracle's order wherever its
            # scores differ by more than twice the gate, and the oracle's set when the list's edge is that clear
            err = float(np.max(np.abs(np.array([s for s, _ in got]) - np.array([x64[u, i] for _, i in got])))) / scale
            assert err <= gate, (u, novelty, err, gate)
            for (_, a), (_, b) in zip(got, got[1:]):
                assert x64[u, a] >= x64[u, b] - 2 * gate * scale, (u, a, b)
            best = sorted(allowed, key=lambda i: -x64[u, i])[:len(got)]
            rest = max([x64[u, i] for i in allowed if i not in best], default=-np.inf)
            if len(allowed) == len(got) or x64[u, best[-1]] - rest > 2 * gate * scale:
                assert sorted(best) == sorted(i for _, i in got), (u, novelty)
    assert fitted.recommend_batch([0], n=5, novelty=True) == [[]]                 # user 0 records the whole catalogue
    # an entry below the threshold is no positive, yet recorded: novelty keeps it out
    assert low5 in fitted._recorded_items(5) and low5 not in [i for _, i in fitted.recommend_batch([5], n=CN, novelty=True)[0]]
    assert low5 in [i for _, i in fitted.recommend_batch([5], n=CN, novelty=False)[0]]


def test_catalogue_ranks_are_positions_in_the_full_list(fitted):
    requests = (([2, 5, 5, 17, 69, 69, 69, 1], [17, 0, 52, 30, 1, 2, 3, 4]), ([5] * 9 + [69] * 9, [(5 * k) % CN for k in range(18)]))
    for (users, items), novelty in ((r, nov) for r in requests for nov in (True, False)):
        ranks, scores = fitted.catalogue_ranks(users, items, novelty=novelty, return_scores=True)
        full = {u: fitted.recommend_batch([u], n=CN, novelty=novelty)[0] for u in set(users)}
        for u, i, r, s in zip(users, items, ranks, scores):
            place = {item: (j, v) for j, (v, item) in enumerate(full[u])}
            if i in place:
                assert r == place[i][0] and s == pytest.approx(place[i][1], abs=1e-5), (u, i, novelty)
            else:
                assert r == -1 and s == -np.inf, (u, i, novelty)


def test_predict_pairs_equals_predict(fitted):
    rng = np.random.default_rng(8)
    users, items = rng.integers(0, CU, size=200), rng.integers(0, CN, size=200)
    got = fitted.predict_pairs(users.tolist(), items.tolist())
    assert got.dtype == np.float64
    assert np.array_equal(got, np.array([fitted.predict(int(u), int(i)) for u, i in zip(users, items)]))
    _, _, fits = _case(CU, CN, CK)
    want = ao.scores(fits[D][3][0])
    assert np.max(np.abs(got - want[users, items])) <= max(1e-5, 4 * _err(ao.scores(fits[F][3][0]), want)) * max(1.0, np.max(np.abs(want)))
    assert np.isnan(fitted.predict_pairs([1, 999], [1, 1], skip_errors=True)[1])


def test_evaluations_in_every_batched_form(fitted):
    from drecpy_amd.Evaluation import ranking_evaluation, recommendation_evaluation
    kw = dict(n_pos_interactions=3, n_neg_interactions=10, generate_negative_pairs=True, k=[1, 5], seed=4, verbose=False)
    keys = [f'{m}@{k}' for m in ('Precision', 'Recall', 'HitRatio', 'NDCG') for k in (1, 5)]
    for batched in (True, False):
        r = ranking_evaluation(fitted, batched=batched, **kw)
        assert sorted(r) == sorted(keys) and all(0.0 <= v <= 1.0 for v in r.values()) and any(v > 0 for v in r.values()), r
    for batched in (False, True, 'ranks'):
        r = recommendation_evaluation(fitted, _dataset(), k=[1, 5], novelty=False, seed=4, verbose=False, batched=batched)
        assert sorted(r) == sorted(keys) and all(0.0 <= v <= 1.0 for v in r.values()) and any(v > 0 for v in r.values()), (batched, r)


def test_save_and_load_round_trip_the_scores_bit_for_bit(fitted, tmp_path):
    from drecpy_amd.Recommender.Baseline import ALS
    path = str(tmp_path / 'als.pkl')
    fitted.save(path)
    other = ALS.load(path)
    assert isinstance(other, ALS)
    assert np.array_equal(_bits(_all_scores(other)), _bits(_all_scores(fitted)))
    users, items = list(range(CU)), [(7 * k) % CN for k in range(CU)]
    assert np.array_equal(other.predict_pairs(users, items), fitted.predict_pairs(users, items))
    assert other.recommend_batch([5, 69], n=7) == fitted.recommend_batch([5, 69], n=7)


def test_early_stopping_reverts_to_the_stored_epoch():
    from drecpy_amd.Recommender.Baseline import ALS
    from drecpy_amd.Recommender.early_stopping import MaxValidationValueRule
    _, p0, _ = _case(CU, CN, CK)
    seen = []
    model = ALS(factors=CK, alpha=ALPHA, interaction_threshold=THR, verbose=False)
    model.fit(_dataset(), epochs=6, reg_rate=LAM, initial_weights=p0,
              epoch_callback_fn=lambda m: seen.append(float(m.predict(5, 7))) or {'score': -len(seen)}, epoch_callback_freq=2,
              early_stopping_rule=MaxValidationValueRule('score'), early_stopping_freq=2)
    assert len(seen) >= 1 and model.fitted
    # the score falls from the first evaluation on: the weights are those of epoch 2
    _class_gate('scores after the revert to epoch 2', _all_scores(model), 2)


@pytest.mark.parametrize('what', ['optimizer', 'factors 0', 'factors 129', 'reg_rate', 'alpha', 'negative weight', 'no positive'])
def test_fit_refuses_by_name(what):
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender.Baseline import ALS
    ds = _dataset()
    kw = dict(interaction_threshold=THR, verbose=False)
    if what == 'optimizer':
        with pytest.raises(Exception, match='optimizer'):
            ALS(factors=4, **kw).fit(ds, epochs=1, optimizer='sgd')
    elif what.startswith('factors'):
        with pytest.raises(Exception, match='factors'):
            ALS(factors=int(what[8:]), **kw).fit(ds, epochs=1)
    elif what == 'reg_rate':
        for reg in (0.0, -1.0):
            with pytest.raises(Exception, match='reg_rate'):
                ALS(factors=4, **kw).fit(ds, epochs=1, reg_rate=reg)
    elif what == 'alpha':
        with pytest.raises(Exception, match='alpha'):
            ALS(factors=4, alpha=-1.0, **kw).fit(ds, epochs=1)
    elif what == 'negative weight':
        neg = InteractionDataset.from_arrays(np.array([0, 0, 1]), np.array([0, 1, 0]), np.array([2.0, -1.0, 1.0]))
        with pytest.raises(Exception, match='negative weight'):
            ALS(factors=4, interaction_threshold=None, verbose=False).fit(neg, epochs=1)
    else:
        low = InteractionDataset.from_arrays(np.array([0, 0, 1]), np.array([0, 1, 0]), np.array([0.5, 0.25, 0.5]))
        with pytest.raises(Exception, match='no positive'):
            ALS(factors=4, **kw).fit(low, epochs=1)
