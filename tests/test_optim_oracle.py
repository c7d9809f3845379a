"""tests/optim_oracle.py without a GPU: an fp32 NumPy replay of every rule in two operation orders — every operation rounded, and every
a * b + c a fused multiply-add, the two forms a compiler may choose between — inside the oracle's bound on the input families of
tests/test_gpu_optim_rules.py; the bound is not vacuous (at most 0.05 of the step's own size); the oracle's Adagrad equals
oracle/cdae_oracle.py's on a dense gradient; and optimizers.resolve / the constructors: what they accept, reset(), what they refuse."""
import numpy as np
import pytest

import dense_update_oracle as du
import optim_oracle as oo
from oracle import cdae_oracle as co
from test_dense_update_oracle import _sum32

HP = oo.HP
F = np.float32
D = np.float64


def _rule32(kind, p, s1, s2, g, lr, l2c, mu, rho, eps, fused):
    """the kernels' operations in NumPy fp32.  fused: a * b + c rounds once (the product of two fp32 numbers is exact in float64)"""
    lr, l2c, mu, eps = (np.asarray(x, dtype=F) for x in (lr, l2c, mu, eps))
    o2 = F(1.0) - F(rho)
    if fused:
        fma = lambda a, b, c: (a.astype(D) * b.astype(D) + c.astype(D)).astype(F)
    else:
        fma = lambda a, b, c: a * b + c
    gt = fma(l2c, p, g)
    if kind == 'sgd':
        out = fma(-lr, gt, p), None, None
    elif kind in ('momentum', 'nesterov'):
        a1 = fma(s1, mu, -(gt * lr))
        out = (p + a1 if kind == 'momentum' else p + fma(a1, mu, -(gt * lr))), a1, None
    elif kind == 'adagrad':
        a1 = fma(gt, gt, s1)
        out = p - lr * gt / (np.sqrt(a1) + eps), a1, None
    else:
        r1 = fma(fma(gt, gt, -s1), o2, s1)
        if kind == 'rmsprop':
            out = p - lr * gt / (np.sqrt(r1) + eps), r1, None
        else:
            m1 = fma(s2, mu, (gt * lr) / np.sqrt(r1 + eps))
            out = p - m1, r1, m1
    assert all(a is None or a.dtype == F for a in out)
    return out


def _inside(got, want, bound, what):
    if want is None:
        assert got is None and bound is None, what
        return 0.0
    err = np.abs(got.astype(D) - want)
    bad = ~(err <= bound)
    assert not bad.any(), f'{what}: {int(bad.sum())} elements outside the bound, worst error / bound {np.max(err[bad] / bound[bad]):.3g}'
    return float(np.max(err / np.maximum(bound, 1e-300)))


def _check(got, want, what):
    for a, w, b, n in zip(got, want[:3], want[3:], ('p', 's1', 's2')):
        _inside(a, w, b, f'{what} {n}')


@pytest.mark.parametrize('kind', oo.KINDS)
@pytest.mark.parametrize('n', [1, 5, 1027])
@pytest.mark.parametrize('mode', ['g', 'g+l2', 'decay'])
def test_fp32_replay_flat(kind, n, mode):
    p, m, v, g = du.flat_inputs(n, n, with_g=mode != 'decay')
    s1, s2 = oo.flat_slots(kind, m, v)
    l2c = 0.0 if mode == 'g' else HP['l2c']
    want = oo.rule_flat(kind, p, s1, s2, g, HP['lr'], l2c)
    assert (want.s1 is None) == (oo.N_SLOTS[kind] < 1) and (want.s2 is None) == (oo.N_SLOTS[kind] < 2)
    for fused in (False, True):
        _check(_rule32(kind, p, s1, s2, g if g is not None else np.zeros(n, F), HP['lr'], l2c, HP['mu'], HP['rho'], HP['eps'], fused), want,
               f'{kind} n {n} {mode} fused {fused}')
    if mode != 'decay' and n > 1:
        step = oo.step_size(kind, p, s1, g, HP['lr'], l2c, HP['mu'])
        assert want.dp.max() <= 0.05 * np.median(step), (want.dp.max(), np.median(step))


@pytest.mark.parametrize('kind', oo.KINDS)
def test_three_flat_steps_carry_the_earlier_steps_error(kind):
    """`din`: the third step of an fp32 replay, started from the replay's own rounded state (fresh slots first), stays inside the bound of
    the third float64 step started from the exact results before it"""
    n = 64
    p = du.flat_inputs(9, n)[0]
    init = F(0.1 if kind == 'adagrad' else 0.0)
    s1, s2 = (np.full(n, init, F) if i < oo.N_SLOTS[kind] else None for i in range(2))
    for fused in (False, True):
        w, r, din = (p.astype(D), s1, s2), (p, s1, s2), None
        for step in range(3):
            g = du.flat_inputs(10 + step, n)[3]
            want = oo.rule_flat(kind, *w, g, HP['lr'], HP['l2c'], din=din)
            r = _rule32(kind, *r, g, HP['lr'], HP['l2c'], HP['mu'], HP['rho'], HP['eps'], fused)
            _check(r, want, f'{kind} step {step} fused {fused}')
            w, din = want[:3], want[3:]
        assert want.dp.max() <= 0.05 * np.median(oo.step_size(kind, w[0], w[1], g, HP['lr'], HP['l2c'], HP['mu'])) or kind in ('momentum', 'nesterov')


@pytest.mark.parametrize('kind', oo.KINDS)
@pytest.mark.parametrize('name', ['plain-scalars-ld20', 'plain-scalars-ld260', 'outer-g3-ld100', 'first-step-ld52'])
def test_fp32_replay_tables(kind, name):
    """the lookups summed forward, backward and in gpb slices (test_dense_update_oracle._sum32), then the rule in both forms"""
    t = du.single_table(name)
    first = t['first_step']
    l2c = 0.0 if first else HP['l2c']
    tab, sc = oo.expected_table(kind, t, l2c=l2c, fresh=first)
    s1, s2, s1s, s2s = oo.table_slots(kind, t, fresh=first)
    for mode in ('fwd', 'bwd', 'slices'):
        g, gs = _sum32(t, mode)
        for fused in (False, True):
            _check(_rule32(kind, t['p0'], s1, s2, g, HP['lr'], l2c, HP['mu'], HP['rho'], HP['eps'], fused), tab, f'{kind} {name} {mode} {fused}')
            _check(_rule32(kind, t['ps0'], s1s, s2s, gs, HP['lr_s'], 0.0, HP['mu'], HP['rho'], HP['eps'], fused), sc, f'{kind} {name} {mode} {fused} scalars')
    busy = t['counts'] > 0
    sums = du._row_sums(du.lookup_rows(t), t['row_ptr'], t['order'])
    if not (first and kind in ('momentum', 'nesterov')):                  # (fresh momentum: s1 mu = 0, no step to compare with)
        step = oo.step_size(kind, t['p0'], s1, sums, HP['lr'], l2c, HP['mu'])       # row by row: a row of 600 lookups steps further
        ratio = tab.dp.max(axis=1)[busy] / np.median(step, axis=1)[busy]
        assert ratio.max() <= 0.05, ratio.max()


@pytest.mark.parametrize('kind', oo.KINDS)
def test_rows_without_lookups_in_the_oracle(kind):
    """l2c = 0, fresh slots: sgd keeps p; momentum moves p by mu s1 (0 here) and, from a non-zero accumulator, by mu s1 exactly;
    rmsprop decays s1 by rho"""
    t = du.single_table('first-step-ld52')
    idle = t['counts'] == 0
    assert idle.sum() >= 2
    tab, _ = oo.expected_table(kind, t, l2c=0.0, fresh=True)
    assert (tab.p[idle] == t['p0'][idle]).all()
    t2 = du.single_table('plain-scalars-ld52')
    idle = t2['counts'] == 0
    tab, _ = oo.expected_table(kind, t2, l2c=0.0)
    s1 = oo.table_slots(kind, t2)[0]
    mu, o2 = du.f32(HP['mu']), du.omb(HP['rho'])
    if kind == 'sgd':
        assert (tab.p[idle] == t2['p0'][idle]).all()
    elif kind == 'momentum':
        assert (tab.s1[idle] == s1[idle].astype(D) * mu).all() and (tab.p[idle] == t2['p0'][idle] + s1[idle].astype(D) * mu).all()
    elif kind == 'rmsprop':
        assert (tab.s1[idle] == s1[idle] + (0.0 - s1[idle].astype(D)) * o2).all() and (tab.p[idle] == t2['p0'][idle]).all()


def test_fp32_replay_segments():
    start, lens, alpha, l2, n = du.segment_layout()
    p, m, v, g = du.flat_inputs(31, n)
    for kind in oo.KINDS:
        s1, s2 = oo.flat_slots(kind, m, v)
        want, inside = oo.rule_segments(kind, p, s1, s2, g, start, lens, alpha, l2)
        assert 0 < (~inside).sum() < n and inside.sum() == sum(lens)
        got = [None if a is None else a.copy() for a in (p, s1, s2)]
        for s0, k, a, l in zip(start, lens, alpha, l2):
            sl = slice(s0, s0 + k)
            r = _rule32(kind, p[sl], None if s1 is None else s1[sl], None if s2 is None else s2[sl], g[sl], a, l, HP['mu'], HP['rho'], HP['eps'], True)
            for dst, x in zip(got, r):
                if dst is not None:
                    dst[sl] = x
        _check(got, want, f'{kind} segments')
        assert (want.p[~inside] == p[~inside]).all() and not want.dp[~inside].any()


def test_adagrad_equals_the_cdae_oracles_on_a_dense_gradient():
    """cdae_oracle.sparse_step updates the hidden bias b with a DENSE gradient under Keras Adagrad (accumulator 0.1): two steps of it
    against rule_flat('adagrad') given the gradient formed here from the step's own activations (mse: dp = 2 (p - y) / B)"""
    rng = np.random.default_rng(4)
    U_, N, K, B, lr = 7, 11, 6, 9, 0.05
    prm = co.init_params(rng, U_, N, K, D)
    st = co.sparse_state(prm, 'adagrad')
    p, a = prm['b'].copy(), st['b'].copy()
    for step in range(2):
        uids, iids, y = rng.integers(0, U_, B), rng.integers(0, N, B), (rng.random(B) < 0.4).astype(D)
        kept = [rng.choice(N, size=3, replace=False) for _ in range(B)]
        w2 = prm['W_'][:, iids].T.copy()
        _, (h, pr) = co.sparse_step(prm, st, step, uids, iids, y, kept, 0.2, lr, 0.0, loss='mse')
        g = (((2.0 * (pr - y) / B) * pr * (1 - pr))[:, None] * w2 * h * (1 - h)).sum(axis=0)
        r = oo.rule_flat('adagrad', p, a, None, g, lr, 0.0, eps=co.ADAGRAD_EPS)
        p, a = r.p, r.s1
        np.testing.assert_allclose(a, st['b'], rtol=1e-12, atol=0)
        np.testing.assert_allclose(p, prm['b'], rtol=1e-9, atol=1e-12)       # (the oracle here rounds lr to fp32 as the C ABI does)
    assert oo.table_slots('adagrad', du.single_table('first-step-ld52'), fresh=True)[0][0, 0] == F(co.ADAGRAD_INIT)


# ---- optimizers.py -------------------------------------------------------------------------------------------------------------------
def test_resolve_and_the_constructors():
    from drecpy_amd import optimizers as op
    s = op.resolve('sgd', 0.02)
    assert isinstance(s, op.SGD) and (s.kind, s.learning_rate, s.momentum, s.nesterov, s.n_slots) == ('sgd', 0.02, 0.0, False, 0)
    r = op.resolve('rmsprop', 0.003)
    assert isinstance(r, op.RMSprop) and (r.kind, r.learning_rate, r.rho, r.momentum, r.epsilon, r.n_slots) == ('rmsprop', 0.003, 0.9, 0.0, 1e-7, 1)
    assert (op.SGD().learning_rate, op.RMSprop().learning_rate, op.Adagrad().learning_rate) == (0.01, 0.001, 0.001)
    m = op.SGD(learning_rate=0.1, momentum=0.8)
    nv = op.SGD(0.1, 0.8, True)
    assert (m.kind, m.n_slots, nv.kind, nv.n_slots) == ('momentum', 1, 'nesterov', 1) and op.SGD(0.1, nesterov=True).kind == 'sgd'
    rm = op.RMSprop(learning_rate=0.01, rho=0.95, momentum=0.5, epsilon=1e-6, centered=False)
    assert (rm.kind, rm.n_slots, rm.rho, rm.momentum, rm.epsilon) == ('rmsprop_momentum', 2, 0.95, 0.5, 1e-6)
    ag = op.Adagrad(0.05, initial_accumulator_value=0.2, epsilon=1e-6)
    assert (ag.kind, ag.n_slots, ag.slot_init) == ('adagrad', 1, 0.2)
    for o in (m, nv, rm, ag, s, r, op.Adam(0.1)):
        assert op.resolve(o, 123.0) is o and o.iterations == 0
        assert op.KINDS[o.kind] == oo.CODE[o.kind] and op.N_SLOTS[o.kind] == oo.N_SLOTS[o.kind]
    assert op.resolve('adagrad', 0.1).kind == 'adagrad' and op.resolve('rowwise_adagrad', 0.1).kind == 'rowwise_adagrad'
    assert op.resolve(None, 0.1).kind == 'adam' and op.resolve('adam', 0.1).learning_rate == 0.1
    from decimal import Decimal                                # hyper-parameters: whatever float() takes, as before the new rules
    assert op.Adam('0.01').learning_rate == 0.01 and op.Adagrad(Decimal('0.5')).learning_rate == 0.5 and op.SGD(np.float32(0.25)).learning_rate == 0.25


def test_reset_starts_the_counter_and_the_slots_over():
    from drecpy_amd import optimizers as op
    for o in (op.SGD(0.1, 0.9), op.RMSprop(momentum=0.1), op.Adagrad(), op.Adam()):
        o.iterations, o._slots['x'] = 7, (None, None, None)
        o.reset()
        assert o.iterations == 0 and o._slots == {}


def test_refusals():
    from drecpy_amd import optimizers as op
    with pytest.raises(Exception, match='centered'):
        op.RMSprop(centered=True)
    with pytest.raises(Exception, match='amsgrad'):
        op.Adam(amsgrad=True)
    for cls, kw in ((op.SGD, 'clipnorm'), (op.RMSprop, 'clipvalue'), (op.Adagrad, 'global_clipnorm'), (op.Adam, 'clipnorm'), (op.SGD, 'decay')):
        with pytest.raises(Exception, match=kw):
            cls(**{kw: 1.0})
    with pytest.raises(Exception, match='schedule'):
        op.SGD(learning_rate=lambda step: 0.1)
    with pytest.raises(Exception, match='momentum'):
        op.SGD(momentum=1.5)
    for bad in ('adadelta', 'adamax', 'nadam', 'ftrl', object(), 3):
        with pytest.raises(Exception, match='Unsupported optimizer') as e:
            op.resolve(bad, 0.1)
        assert "'sgd'" in str(e.value) and "'rmsprop'" in str(e.value) and 'RMSprop(' in str(e.value)
