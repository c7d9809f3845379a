"""tests/dense_update_oracle.py without a GPU: its Adam against the independent statements in oracle/cdae_oracle.py and
oracle/caser_oracle.py; an fp32 NumPy replay of the kernels' operation sequence — the lookups summed forward, backward and in gpb
slices — inside the oracle's bound on every input family tests/test_gpu_dense_update.py uses (the reference alone passes); and the
bound is not vacuous: at most 0.05 alpha on p on the general inputs, 1e-3 alpha on the first-step inputs."""
import numpy as np
import pytest

import dense_update_oracle as du
from oracle import caser_oracle as ca
from oracle import cdae_oracle as co

HP = du.HP
F = np.float32


def test_hyperparameters_as_the_cdae_oracle_states_them():
    assert du.omb(0.9) == co.ADAM_OMB1 and du.omb(0.999) == co.ADAM_OMB2
    assert du.f32(HP['eps']) == pytest.approx(co.ADAM_EPS, rel=1e-7)


def test_flat_adam_equals_the_cdae_oracles_dense_update():
    """two steps of cdae_oracle's Adam lines (params[name] - m a / (sqrt(v) + eps), alpha = adam_alpha(lr, t)) in float64"""
    rng = np.random.default_rng(1)
    p, m, v = rng.standard_normal(37), np.zeros(37), np.zeros(37)
    pp, mm, vv = p.copy(), m.copy(), v.copy()
    for t in (1, 2):
        g = rng.standard_normal(37)
        a = co.adam_alpha(1e-3, t)
        mm = mm + (g - mm) * co.ADAM_OMB1
        vv = vv + (g * g - vv) * co.ADAM_OMB2
        pp = pp - (mm * a) / (np.sqrt(vv) + co.ADAM_EPS)
        r = du.adam_flat(p, m, v, g, a, 0.0, 0.9, 0.999, co.ADAM_EPS)
        p, m, v = r.p, r.m, r.v
        np.testing.assert_allclose(p, pp, rtol=1e-7, atol=0)        # (the oracle rounds alpha and eps to fp32: 6e-8 relative)
        np.testing.assert_allclose(m, mm, rtol=1e-14, atol=0)
        np.testing.assert_allclose(v, vv, rtol=1e-14, atol=0)


def test_rows_adam_equals_the_caser_oracles_step_on_a_small_table():
    """caser_oracle.step on a tiny float64 model: its update of item_emb (gradient of the lookups + 2 reg p, Keras Adam with the
    table's own lr_t) against rows_adam given the data gradient of every looked-up row as one lookup and l2c = 2 reg — the rows no
    window names go through rows_adam's no-lookup path"""
    import copy
    rng = np.random.default_rng(2)
    U_, N, L, T, d, B, lr, reg = 6, 14, 3, 2, 8, 5, 5e-3, 1e-3
    p = ca.init_params(rng, U_, N, L, d, 2, 4, np.float64)
    uids, before, after = rng.integers(0, U_, size=B), rng.integers(0, N - 4, size=(B, L)), rng.integers(0, N, size=(B, 2 * T))
    _, g, _ = ca.loss_and_grads(p, uids, before, after, T, reg)
    data = g['item_emb'] - 2.0 * reg * p['item_emb']
    keys = np.nonzero(np.abs(data).sum(axis=1) > 1e-12)[0]
    assert 0 < len(keys) < N                                              # (the last four rows at least: no lookup)
    p2, state = copy.deepcopy(p), ca.adam_state(p)
    ca.step(p2, state, 0, uids, before, after, T, lr, reg)
    j = [name for name, _ in ca.layer_order(L)].index('item_emb')
    row_ptr, order = du.csr_from_keys(keys, N)
    tab, sc = du.rows_adam(p['item_emb'], np.zeros((N, d)), np.zeros((N, d)), row_ptr, order, data[keys], co.adam_alpha(lr, j + 1), 2.0 * reg,
                           0.9, 0.999, co.ADAM_EPS)
    assert sc is None
    np.testing.assert_allclose(tab.p, p2['item_emb'], rtol=1e-6, atol=1e-10)     # (the oracle rounds alpha, 2 reg and eps to fp32)
    np.testing.assert_allclose(tab.m, state['item_emb'][0], rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(tab.v, state['item_emb'][1], rtol=1e-6, atol=1e-14)
    assert (tab.dp > 0).all()


def test_csr_from_keys_groups_lookups_by_row_in_batch_order():
    keys = np.array([3, 0, 3, 1, 3, 0])
    row_ptr, order = du.csr_from_keys(keys, 5)
    assert row_ptr.tolist() == [0, 2, 3, 3, 6, 6] and order.tolist() == [1, 5, 3, 0, 2, 4]
    assert row_ptr.dtype == np.int32 and order.dtype == np.int32


def test_geometry_ladder_covers_every_g_and_j():
    assert {du.geom(ld) for ld in du.LDS} == {(4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4)}
    for ld in du.LDS:
        g, j = du.geom(ld)
        assert ld <= 4 * g * j
    assert sum(1 for ld in du.LDS if ld % (4 * du.geom(ld)[0])) >= 3          # partial last float4 column for J = 1, 2 and 4
    assert {du.geom(ld)[1] for ld in du.LDS if ld % (4 * du.geom(ld)[0])} == {1, 2, 4}


# ---- the fp32 replay -----------------------------------------------------------------------------------------------------------------
def _adam32(p, m, v, g, alpha, l2c, b1, b2, eps):
    """opt_update1's operations in NumPy fp32 (no fused multiply-add: every operation rounds)"""
    o1, o2 = F(1.0) - F(b1), F(1.0) - F(b2)
    gt = F(l2c) * p + g
    m1 = m + (gt - m) * o1
    v1 = v + (gt * gt - v) * o2
    p1 = p - (m1 * F(alpha)) / (np.sqrt(v1) + F(eps))
    assert p1.dtype == F and m1.dtype == F and v1.dtype == F
    return p1, m1, v1


def _sum32(t, mode):
    """per row: the fp32 sum of the lookups' rows and scalars; mode 'fwd' / 'bwd': one walk in list order / reversed;
    'slices': rows of >= 64 lookups in gpb slices of per = ceil(n / gpb) rounded up to 4, the partial sums added in slice order"""
    n_rows, ld, T, group = t['n_rows'], t['ld'], t['T'], t['group']
    if group:
        rows = (t['scale'][:T, None] * t['src'][np.arange(T) // group]).astype(F)
    else:
        rows = t['src'][:T]
    sc = t['scale'][:T] if t['scale'] is not None else np.zeros(T, F)
    ptr, order, cnt = t['row_ptr'].astype(np.int64), t['order'], t['counts']
    g, gs = np.zeros((n_rows, ld), F), np.zeros(n_rows, F)
    hot = (cnt >= du.SPLIT) if mode == 'slices' else np.zeros(n_rows, bool)
    for k in range(int(cnt[~hot].max()) if (~hot).any() else 0):
        r = np.nonzero(~hot & (cnt > k))[0]
        q = ptr[r] + (k if mode != 'bwd' else cnt[r] - 1 - k)
        g[r] += rows[order[q]]
        gs[r] += sc[order[q]]
    gpb = du.gpb(ld)
    for r in np.nonzero(hot)[0]:
        n = int(cnt[r])
        per = ((n + gpb - 1) // gpb + 3) & ~3
        acc, accs = None, None
        for s in range(gpb):
            a, b = min(s * per, n), min((s + 1) * per, n)
            pg, ps = np.zeros(ld, F), F(0)
            for q in range(ptr[r] + a, ptr[r] + b):
                pg = pg + rows[order[q]]
                ps = F(ps + sc[order[q]])
            acc, accs = (pg, ps) if acc is None else (acc + pg, F(accs + ps))
        g[r], gs[r] = acc, accs
    return g, gs


def _inside(got, want, bound, what):
    err = np.abs(got.astype(np.float64) - want)
    bad = err > bound
    assert not bad.any(), f'{what}: {int(bad.sum())} elements outside the bound, worst error / bound {np.max(err[bad] / bound[bad]):.3g}'
    return float(np.max(err / np.maximum(bound, 1e-300)))


def _replay_table(t, alpha, alpha_s, l2c, name):
    tab, sc = du.expected_table(t, alpha, alpha_s, l2c)
    worst = 0.0
    for mode in ('fwd', 'bwd', 'slices'):
        g, gs = _sum32(t, mode)
        p1, m1, v1 = _adam32(t['p0'], t['m0'], t['v0'], g, alpha, l2c, HP['b1'], HP['b2'], HP['eps'])
        for got, want, bound, w in ((p1, tab.p, tab.dp, 'p'), (m1, tab.m, tab.dm, 'm'), (v1, tab.v, tab.dv, 'v')):
            worst = max(worst, _inside(got, want, bound, f'{name} {mode} {w}'))
        if sc is not None:
            q1, n1, w1 = _adam32(t['ps0'], t['ms0'], t['vs0'], gs, alpha_s, 0.0, HP['b1'], HP['b2'], HP['eps'])
            for got, want, bound, w in ((q1, sc.p, sc.dp, 'p_s'), (n1, sc.m, sc.dm, 'm_s'), (w1, sc.v, sc.dv, 'v_s')):
                worst = max(worst, _inside(got, want, bound, f'{name} {mode} {w}'))
    return tab, sc, worst


@pytest.mark.parametrize('name', [c[0] for c in du.single_cases()])
def test_fp32_replay_inside_the_bound_and_the_bound_not_vacuous(name):
    t = du.single_table(name)
    first = t['first_step']
    tab, sc, _ = _replay_table(t, HP['alpha'], HP['alpha_s'], 0.0 if first else HP['l2c'], name)
    lim = 1e-3 if first else 0.05
    assert tab.dp.max() <= lim * du.f32(HP['alpha']), tab.dp.max() / HP['alpha']
    if sc is not None:
        assert sc.dp.max() <= lim * du.f32(HP['alpha_s']), sc.dp.max() / HP['alpha_s']
    cnt = t['counts']
    assert cnt[0] == 0 and {1, 3, 4, 5, 63, 64, 65} <= set(cnt.tolist()) and cnt[-1] >= 590 and len(cnt) == 2 * du.gpb(t['ld']) + 3
    g = du.gpb(t['ld'])                          # some split row fills its LAST slice, some leaves slices empty
    per = lambda n: ((n + g - 1) // g + 3) & ~3
    hot = [int(n) for n in cnt if n >= du.SPLIT]
    assert any(n > (g - 1) * per(n) for n in hot) and (g == 4 or any(n <= (g - 2) * per(n) for n in hot))


def test_first_step_rows_without_lookups_stay_put_in_the_oracle():
    t = du.single_table('first-step-ld52')
    tab, sc = du.expected_table(t, l2c=0.0)
    idle = t['counts'] == 0
    assert idle.sum() >= 2
    assert (tab.p[idle] == t['p0'][idle]).all() and not tab.m[idle].any() and not tab.v[idle].any()
    assert (sc.p[idle] == t['ps0'][idle]).all() and not sc.m[idle].any() and not sc.v[idle].any()


def test_fp32_replay_capped_table():
    t = du.capped_table()
    g = du.gpb(132)
    assert t['n_rows'] == 8192 * 4 + 5 and t['counts'][8192 * g:].max() >= 300 and t['counts'][:8192 * g].max() >= 200
    tab, sc, _ = _replay_table(t, HP['alpha'], HP['alpha_s'], HP['l2c'], 'capped')
    assert tab.dp.max() <= 0.05 * HP['alpha'] and sc.dp.max() <= 0.05 * HP['alpha_s']


def test_fp32_replay_multi_tables():
    ts = du.multi_tables()
    assert len({du.geom(t['ld'])[0] for t in ts}) == 4 and ts[2]['n_rows'] == 1 and ts[3]['n_rows'] == 4096 * 4 + 5
    for i, (t, (a, a_s, l2c)) in enumerate(zip(ts, du.MULTI_HP)):
        tab, sc, _ = _replay_table(t, a, a_s, l2c, f'multi table {i}')
        assert tab.dp.max() <= 0.05 * a


@pytest.mark.parametrize('n', [1, 5, 1025])
@pytest.mark.parametrize('mode', ['g', 'g+l2', 'decay'])
def test_fp32_replay_flat(n, mode):
    p, m, v, g = du.flat_inputs(n, n, with_g=mode != 'decay')
    l2c = 0.0 if mode == 'g' else HP['l2c']
    want = du.adam_flat(p, m, v, g, HP['alpha'], l2c, HP['b1'], HP['b2'], HP['eps'])
    got = _adam32(p, m, v, g if g is not None else np.zeros(n, F), HP['alpha'], l2c, HP['b1'], HP['b2'], HP['eps'])
    for a, w, b, what in zip(got, want[:3], want[3:], 'pmv'):
        _inside(a, w, b, what)
    assert want.dp.max() <= 0.05 * HP['alpha']


def test_two_flat_steps_carry_the_first_steps_error():
    """adam_flat's `din`: the second step of an fp32 replay, started from the replay's own rounded state, stays inside the bound of the
    second float64 step started from the first one's exact result"""
    p, m, v, g = du.flat_inputs(9, 64)
    m[:], v[:] = 0, 0
    a1, a2 = co.adam_alpha(1e-2, 1), co.adam_alpha(1e-2, 2)
    g2 = du.flat_inputs(10, 64)[3]
    w1 = du.adam_flat(p, m, v, g, a1, 0.0, 0.9, 0.999, 1e-7)
    w2 = du.adam_flat(w1.p, w1.m, w1.v, g2, a2, 0.0, 0.9, 0.999, 1e-7, din=(w1.dp, w1.dm, w1.dv))
    r1 = _adam32(p, m, v, g, a1, 0.0, 0.9, 0.999, 1e-7)
    r2 = _adam32(*r1, g2, a2, 0.0, 0.9, 0.999, 1e-7)
    for a, w, b, what in zip(r2, w2[:3], w2[3:], 'pmv'):
        _inside(a, w, b, what)
    assert (w2.dp >= w1.dp).all()


def test_fp32_replay_segments():
    start, lens, alpha, l2, n = du.segment_layout()
    assert len(lens) == 24 and max(lens) > 64 * 256 and 0 in lens
    p, m, v, g = du.flat_inputs(31, n)
    want, inside = du.adam_segments(p, m, v, g, start, lens, alpha, l2, 0.9, 0.999, 1e-7)
    assert 0 < (~inside).sum() < n and inside.sum() == sum(lens)
    gp, gm, gv = p.copy(), m.copy(), v.copy()
    for s0, k, a, l in zip(start, lens, alpha, l2):
        sl = slice(s0, s0 + k)
        gp[sl], gm[sl], gv[sl] = _adam32(p[sl], m[sl], v[sl], g[sl], a, l, 0.9, 0.999, 1e-7)
    for a, w, b, what in zip((gp, gm, gv), want[:3], want[3:], 'pmv'):
        _inside(a, w, b, what)
    assert (want.p[~inside] == p[~inside]).all() and not want.dp[~inside].any()


@pytest.mark.parametrize('ld', [4, 132, 1024])
def test_fp32_replay_rows_dot_and_sumsq(ld):
    rng = np.random.default_rng(ld)
    x, tab, bias = ((rng.random(s) - 0.5).astype(F) for s in ((3, ld), (9, ld), (9,)))
    want, bound = du.rows_dot(x, tab, bias)
    for got in ((x @ tab.T + bias), (x[:, ::-1] @ tab[:, ::-1].T + bias)):
        assert got.dtype == F
        _inside(got, want, bound, 'rows_dot')
    assert bound.max() <= (ld + 1) * du.U * (0.25 * ld + 0.5)
    y = (np.sign(rng.random(5000) - 0.5) * 10.0 ** rng.uniform(-18, 3, 5000)).astype(F)
    s, b = du.sumsq(y[:1000], y[1000:])
    assert abs(float(np.sum(y.astype(np.float64) ** 2)) - s) <= b and abs(float(np.sum(np.sort(y.astype(np.float64) ** 2))) - s) <= b
    assert du.sumsq() == (0.0, 0.0) and du.sumsq(np.array([3.0], F)) == (9.0, 9.0 * 2.0 ** -52)
