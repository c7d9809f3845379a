"""The dense update rules beside Adam through the C ABI — drx_opt_dense, drx_opt_segments, drx_rows_csr_opt, drx_rows_csr_opt_outer,
drx_rows_csr_opt_multi — against tests/optim_oracle.py (NumPy float64) and its forward error bound, element by element with no extra
factor.  Every array is a view into a larger buffer between guards filled with one NaN pattern; a slot the rule does not have is passed
as NULL or as a buffer full of that NaN: guards and absent slots must come back bit-identical.  Each test prints its largest
error / bound ratio (pytest -s shows them)."""
import ctypes as C
import functools

import numpy as np
import pytest

import dense_update_oracle as du
import optim_oracle as oo

pytestmark = pytest.mark.gpu

HP = oo.HP
F = np.float32
NAN_BITS = np.int32(0x7FC0BEEF)
NAN = NAN_BITS.view(F)
NULL = C.c_void_p(0)
BIG_N = 4 * 256 * 4096 + 4 * 256 + 3          # one grid pass of the flat sweep is 4096 x 256 float4: a second trip and a tail of 3


def _L():
    from drecpy_amd import _lib
    return _lib


def _stream():
    import torch
    return _L().stream_ptr(torch.device('cuda:0'))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rule(kind, lr=HP['lr'], mu=HP['mu'], rho=HP['rho'], eps=HP['eps']):
    """DrxOptRule: mu = momentum (Adam: beta_1), mu2 = rho (Adam: beta_2)"""
    return _L().OptRule(oo.CODE[kind] if isinstance(kind, str) else kind, lr, mu, rho, eps)


class Guarded:
    """`a` on the device between two guards of `pad` NaN floats (a None: a buffer of `n` NaN floats, an absent slot): .t is the view"""

    def __init__(self, a, pad, n=None):
        import torch
        self.absent = a is None
        a = np.full(n, NAN, F) if a is None else np.ascontiguousarray(a, dtype=F)
        self.n, self.pad, self.shape = a.size, pad, a.shape
        self.buf = torch.from_numpy(np.full(a.size + 2 * pad, NAN, F)).cuda()
        self.t = self.buf[pad:pad + a.size]
        self.t.copy_(_dev(a.ravel()))

    def ptr(self, shift=0):
        return C.c_void_p(self.t.data_ptr() + 4 * shift)

    def get(self):
        """the array back on the host, after checking both guards (an absent slot: every float) bit for bit"""
        h = self.buf.cpu().numpy()
        g = h if self.absent else np.concatenate([h[:self.pad], h[self.pad + self.n:]])
        assert (g.view(np.int32) == NAN_BITS).all(), 'an absent slot was written' if self.absent else 'a guard was written'
        return None if self.absent else h[self.pad:self.pad + self.n].reshape(self.shape).copy()


def _slot(a, pad, n, absent):
    """a slot array guarded; for a slot the rule lacks: None (pass NULL) or a NaN buffer (a pointer the kernel must not follow)"""
    if a is not None:
        return Guarded(a, pad)
    return None if absent == 'null' else Guarded(None, pad, n)


def _p(x, shift=0):
    return x.ptr(shift) if x is not None else NULL


def _got(x):
    return x.get() if x is not None else None


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, dtype=F).view(np.int32), np.ascontiguousarray(b, dtype=F).view(np.int32))


def _inside(got, want, bound, what):
    """|got - want| <= bound element by element (a NaN fails); an absent slot: nothing came back.  Returns the largest error / bound"""
    if want is None:
        assert got is None and bound is None, what
        return 0.0
    err = np.abs(got.astype(np.float64) - want)
    bad = ~(err <= bound)
    assert not bad.any(), (f'{what}: {int(bad.sum())} of {bad.size} elements outside the bound, first at {np.argwhere(bad)[0].tolist()}: got '
                           f'{got[bad][0]!r} want {want[bad][0]!r} bound {bound[bad][0]:.3g}; worst error / bound '
                           f'{np.nanmax(err[bad] / np.maximum(bound[bad], 1e-300)):.3g}')
    nz = bound > 0
    return float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0


def _check(got, want, what):
    return max(_inside(a, w, b, f'{what} {n}') for a, w, b, n in zip(got, want[:3], want[3:], ('p', 's1', 's2')))


def _report(kernel, case, ratio):
    print(f'[error/bound] {kernel} {case}: {ratio:.3f}')


# ---- drx_opt_dense -------------------------------------------------------------------------------------------------------------------
def _opt_dense(p, s1, s2, g, n, rule, l2c, shift_p=0):
    return _L().lib().drx_opt_dense(p.ptr(shift_p), _p(s1), _p(s2), _p(g), n, C.byref(rule), l2c, _stream())


@pytest.mark.parametrize('kind', oo.KINDS)
@pytest.mark.parametrize('n,absent', [(1, 'null'), (3, 'nan'), (4, 'null'), (5, 'nan'), (1027, 'null'), (1027, 'nan'), (BIG_N, 'nan')])
def test_opt_dense(kind, n, absent):
    """g == NULL with l2 (pure decay) from old slots; a first step from fresh slots; three chained steps, the third one's bound
    carrying the errors of the two before (the large n: the chained steps alone)"""
    import torch
    p0, m0, v0, g0 = du.flat_inputs(n, n)
    worst = 0.0
    if n != BIG_N:
        s10, s20 = oo.flat_slots(kind, m0, v0)
        want = oo.rule_flat(kind, p0, s10, s20, None, HP['lr'], HP['l2c'])
        p, s1, s2 = Guarded(p0, 4), _slot(s10, 4, n, absent), _slot(s20, 4, n, absent)
        assert _opt_dense(p, s1, s2, None, n, _rule(kind), HP['l2c']) == 0
        torch.cuda.synchronize()
        worst = _check((p.get(), _got(s1), _got(s2)), want, f'{kind} n {n} decay')
    init = F(0.1 if kind == 'adagrad' else 0.0)
    fresh = [np.full(n, init, F) if i < oo.N_SLOTS[kind] else None for i in range(2)]
    p, s1, s2 = Guarded(p0, 4), _slot(fresh[0], 4, n, absent), _slot(fresh[1], 4, n, absent)
    state, din = (p0, fresh[0], fresh[1]), None
    for step in range(3):
        gh = du.flat_inputs(n + 1 + step, n)[3]
        g = Guarded(gh, 4)
        want = oo.rule_flat(kind, *state, gh, HP['lr'], HP['l2c'] if step else 0.0, din=din)
        assert _opt_dense(p, s1, s2, g, n, _rule(kind), HP['l2c'] if step else 0.0) == 0
        torch.cuda.synchronize()
        worst = max(worst, _check((p.get(), _got(s1), _got(s2)), want, f'{kind} n {n} step {step + 1}'))
        assert _same_bits(g.get(), gh)
        state, din = want[:3], want[3:]
    _report('drx_opt_dense', f'{kind} n {n}', worst)


@pytest.mark.parametrize('kind', oo.KINDS)
def test_apply_gradients_keeps_the_slots_of_padded_and_view_keyed_variables(kind):
    """optimizers.*.apply_gradients on variables of 1, 3 and 5 elements, on flat[1:9] (4 bytes off a 16-byte boundary) and on a bare
    tensor handed over as a FRESH view object every step: three steps against three chained float64 steps — the slots must survive
    from one call to the next, Adagrad's start at its accumulator value"""
    import torch
    from drecpy_amd import optimizers as op
    lr = 1e-2
    opt = {'sgd': lambda: op.SGD(lr), 'momentum': lambda: op.SGD(lr, HP['mu']), 'nesterov': lambda: op.SGD(lr, HP['mu'], True),
           'adagrad': lambda: op.Adagrad(lr, 0.1, HP['eps']), 'rmsprop': lambda: op.RMSprop(lr, HP['rho'], 0.0, HP['eps']),
           'rmsprop_momentum': lambda: op.RMSprop(lr, HP['rho'], HP['mu'], HP['eps'])}[kind]()
    assert opt.kind == kind
    rng = np.random.default_rng(8)
    flat0 = (rng.random(12) - 0.5).astype(F)
    flat, base = _dev(flat0), _dev((rng.random(16) - 0.5).astype(F))
    host = [(rng.random(k) - 0.5).astype(F) for k in (1, 3, 5)] + [flat0[1:9].copy(), base.cpu().numpy()[4:12].copy()]
    var = [_dev(h) for h in host[:3]] + [flat[1:9], None]
    init = 0.1 if kind == 'adagrad' else 0.0
    state = [(h.astype(np.float64),) + tuple(np.full(h.size, init) if i < oo.N_SLOTS[kind] else None for i in range(2)) + (None,) for h in host]
    worst = 0.0
    for step in (1, 2, 3):
        var[4] = base[4:12]                                       # (a new view object of the same memory)
        grads = [(rng.random(h.size) - 0.5).astype(F) for h in host]
        opt.apply_gradients([(_dev(g), x) for g, x in zip(grads, var)])
        torch.cuda.synchronize()
        assert opt.iterations == step
        for i, (g, x) in enumerate(zip(grads, var)):
            pp, a, b, din = state[i]
            r = oo.rule_flat(kind, pp, a, b, g, lr, 0.0, din=din)
            state[i] = (r.p, r.s1, r.s2, (r.dp, r.ds1, r.ds2))
            got = [x.cpu().numpy()] + [None if t is None else t.cpu().numpy() for t in opt._moments(x, x)]
            worst = max(worst, _check(got, r, f'{kind} step {step} variable {i}'))
    assert _same_bits(flat.cpu().numpy()[:1], flat0[:1]) and _same_bits(flat.cpu().numpy()[9:], flat0[9:])
    _report('drx_opt_dense', f'{kind} apply_gradients', worst)


# ---- drx_opt_segments ----------------------------------------------------------------------------------------------------------------
def _segments(start, lens, alpha, l2):
    sg = _L().AdamSegments()
    sg.n = len(lens)
    for i, (s, k, a, l) in enumerate(zip(start, lens, alpha, l2)):
        sg.start[i], sg.len[i], sg.alpha[i], sg.l2_coef[i] = s, k, a, l
    return sg


@pytest.mark.parametrize('kind', oo.KINDS)
def test_opt_segments(kind):
    """the 24 segments with gaps of dense_update_oracle.segment_layout(), each with its own step size and l2; what lies in no segment keeps
    its bits"""
    import torch
    start, lens, alpha, l2, n = du.segment_layout()
    p0, m0, v0, g0 = du.flat_inputs(31, n)
    s10, s20 = oo.flat_slots(kind, m0, v0)
    want, inside = oo.rule_segments(kind, p0, s10, s20, g0, start, lens, alpha, l2)
    p, s1, s2, g = Guarded(p0, 4), _slot(s10, 4, n, 'nan'), _slot(s20, 4, n, 'null'), Guarded(g0, 4)
    sg = _segments(start, lens, alpha, l2)
    rule = _rule(kind, lr=123.0)                                  # (the step size comes from the segments)
    assert _L().lib().drx_opt_segments(p.ptr(), _p(s1), _p(s2), g.ptr(), C.byref(sg), C.byref(rule), _stream()) == 0
    torch.cuda.synchronize()
    got = (p.get(), _got(s1), _got(s2))
    worst = _check(got, want, f'{kind} segments')
    for x, x0 in zip(got, (p0, s10, s20)):
        if x0 is not None:
            assert _same_bits(x[~inside], x0[~inside])
    assert (got[0][inside] != p0[inside]).mean() > 0.9 and _same_bits(g.get(), g0)
    _report('drx_opt_segments', kind, worst)


# ---- lookup tables -------------------------------------------------------------------------------------------------------------------
class DeviceTable:
    """a table of dense_update_oracle.make_table on the device under rule `kind`: guarded state with optim_oracle.table_slots' slots"""

    def __init__(self, kind, t, fresh=False, absent='null'):
        self.t, self.kind = t, kind
        self.scalars = t['scale'] is not None
        ld, n = t['ld'], t['n_rows']
        self.s0 = oo.table_slots(kind, t, fresh)
        self.p = Guarded(t['p0'], ld)
        self.s1, self.s2 = (_slot(a, ld, n * ld, absent) for a in self.s0[:2])
        self.ps = Guarded(t['ps0'], 1) if self.scalars else None
        self.s1s, self.s2s = (_slot(a, 1, n, absent) for a in self.s0[2:]) if self.scalars else (None, None)
        self.row_ptr, self.order, self.src = _dev(t['row_ptr']), _dev(t['order']), _dev(t['src'])
        self.scale = _dev(t['scale']) if self.scalars else None

    @staticmethod
    def tptr(x):
        return C.c_void_p(x.data_ptr()) if x is not None else NULL

    def launch(self, rule=None, lr=HP['lr'], lr_s=HP['lr_s'], l2c=HP['l2c'], s1=True):
        t, L = self.t, _L().lib()
        rule = rule if rule is not None else _rule(self.kind)
        state = (self.p.ptr(), _p(self.s1) if s1 else NULL, _p(self.s2), _p(self.ps), _p(self.s1s), _p(self.s2s))
        if t['group']:
            return L.drx_rows_csr_opt_outer(self.tptr(self.row_ptr), self.tptr(self.order), self.tptr(self.scale), self.tptr(self.src), t['group'],
                                            t['ld'], t['n_rows'], *state, lr, lr_s, l2c, C.byref(rule), _stream())
        return L.drx_rows_csr_opt(self.tptr(self.row_ptr), self.tptr(self.order), self.tptr(self.src), self.tptr(self.scale), t['ld'],
                                  t['n_rows'], *state, lr, lr_s, l2c, C.byref(rule), _stream())

    def fill(self, tab, lr, lr_s, l2c):
        """this table's entry of a drx_rows_csr_opt_multi call"""
        t = self.t
        tab.row_ptr, tab.order, tab.src, tab.scale = (x.data_ptr() if x is not None else None for x in (self.row_ptr, self.order, self.src, self.scale))
        tab.group, tab.ld, tab.n_rows = t['group'], t['ld'], t['n_rows']
        tab.p, tab.m, tab.v, tab.p_s, tab.m_s, tab.v_s = (x.t.data_ptr() if x is not None else None
                                                          for x in (self.p, self.s1, self.s2, self.ps, self.s1s, self.s2s))
        tab.alpha, tab.alpha_s, tab.l2_coef = lr, lr_s, l2c

    def results(self):
        """(p, s1, s2), (p_s, s1_s, s2_s) or None — after checking guards, absent slots and that the inputs came back bit-identical"""
        import torch
        torch.cuda.synchronize()
        t = self.t
        for dev, host in ((self.row_ptr, t['row_ptr']), (self.order, t['order']), (self.src, t['src'])) + \
                         (((self.scale, t['scale']),) if self.scalars else ()):
            assert np.array_equal(dev.cpu().numpy().view(np.int32), np.ascontiguousarray(host).view(np.int32)), 'an input was written'
        return (self.p.get(), _got(self.s1), _got(self.s2)), ((self.ps.get(), _got(self.s1s), _got(self.s2s)) if self.scalars else None)

    def unchanged(self):
        tab, sc = self.results()
        t = self.t
        ok = all(a is None or _same_bits(a, b) for a, b in zip(tab, (t['p0'],) + self.s0[:2]))
        return ok and (sc is None or all(a is None or _same_bits(a, b) for a, b in zip(sc, (t['ps0'],) + self.s0[2:])))


def _check_table(got, want, what, kernel):
    (tab, sc), (wtab, wsc) = got, want
    worst = _check(tab, wtab, what)
    assert (sc is None) == (wsc is None)
    if sc is not None:
        worst = max(worst, _check(sc, wsc, what + ' scalars'))
    _report(kernel, what, worst)


@functools.lru_cache(maxsize=None)
def _table(name):
    t = du.single_table(name)
    return dict(t, scale=None, ps0=None, ms0=None, vs0=None) if name.startswith('plain-ld') else t


# every (G, J) of pick_geom with the scalar channel — ld 20, 52, 100, 132, 260, 516 leave a partial last float4 column, count_profile has
# rows of 0, 1, 63, 64, 65 and ~600 lookups (across kCsrSplit) — one table without the channel, and the outer form at three group sizes
CSR_CASES = [c[0] for c in du.single_cases() if c[0].startswith('plain-scalars')] + ['plain-ld52', 'outer-g1-ld16', 'outer-g3-ld100',
                                                                                     'outer-g12-ld260']


@pytest.mark.parametrize('kind', oo.KINDS)
@pytest.mark.parametrize('name', CSR_CASES)
def test_rows_csr_opt(kind, name):
    t = _table(name)
    cnt = t['counts']
    assert {0, 1, 63, 64, 65} <= set(cnt.tolist()) and cnt.max() >= 590
    absent = 'nan' if t['ld'] in (20, 260) else 'null'
    d = DeviceTable(kind, t, absent=absent)
    assert d.launch() == 0
    _check_table(d.results(), oo.expected_table(kind, t), f'{kind} {name}', 'drx_rows_csr_opt_outer' if t['group'] else 'drx_rows_csr_opt')


@pytest.mark.parametrize('kind', oo.KINDS)
def test_rows_csr_opt_first_step_and_rows_without_lookups(kind):
    """fresh slots, l2c = 0, gradients multiples of 1/256 (exact sums: dg = 0 in the bound); then rows that no lookup names, exactly:
    under sgd they keep p bit for bit; under momentum (old accumulators) s1 becomes mu s1 and p moves by it; under rmsprop s1 decays
    by (1 - rho) s1 — the fused or the unfused fp32 form — and p keeps its bits"""
    t = _table('first-step-ld52')
    idle = t['counts'] == 0
    assert idle.sum() >= 2
    d = DeviceTable(kind, t, fresh=True, absent='nan')
    assert d.launch(l2c=0.0) == 0
    got = d.results()
    _check_table(got, oo.expected_table(kind, t, l2c=0.0, fresh=True), f'{kind} first step', 'drx_rows_csr_opt')
    assert _same_bits(got[0][0][idle], t['p0'][idle]) and _same_bits(got[1][0][idle], t['ps0'][idle])
    if kind == 'adagrad':
        assert (got[0][1][idle] == F(0.1)).all()
    elif kind != 'sgd':
        assert not got[0][1][idle].any() and (got[0][2] is None or not got[0][2][idle].any())
    t = _table('plain-scalars-ld52')
    idle = t['counts'] == 0
    d = DeviceTable(kind, t)
    assert d.launch(l2c=0.0) == 0
    (p, s1, s2), _ = d.results()
    s10 = d.s0[0]
    mu, o2 = F(HP['mu']), F(1.0) - F(HP['rho'])
    if kind == 'sgd':
        assert _same_bits(p[idle], t['p0'][idle])
    elif kind == 'momentum':
        assert _same_bits(s1[idle], s10[idle] * mu) and _same_bits(p[idle], t['p0'][idle] + s10[idle] * mu)
    elif kind == 'rmsprop':
        a = s10[idle]
        unfused = a + (F(0.0) - a) * o2
        fused = (a.astype(np.float64) + (-a.astype(np.float64)) * np.float64(o2)).astype(F)
        assert ((s1[idle] == unfused) | (s1[idle] == fused)).all() and (s1[idle] < a).all() and _same_bits(p[idle], t['p0'][idle])


@pytest.mark.parametrize('kind', ['nesterov', 'rmsprop_momentum'])
def test_rows_csr_opt_past_the_grid_cap(kind):
    """8192 * 4 + 5 rows of ld 132: the workgroups' row loop makes a second trip, with rows of 300 lookups in it"""
    t = du.capped_table()
    assert t['n_rows'] == 8192 * 4 + 5
    d = DeviceTable(kind, t)
    assert d.launch() == 0
    _check_table(d.results(), oo.expected_table(kind, t), f'{kind} capped-ld132', 'drx_rows_csr_opt')


@functools.lru_cache(maxsize=None)
def _multi_tables():
    return du.multi_tables()


MULTI_RULES = (dict(mu=0.9, rho=0.9, eps=1e-7), dict(mu=0.5, rho=0.99, eps=1e-5))


def _launch_multi(devs, hps, rule):
    L = _L()
    tabs = (L.CsrAdamTable * len(devs))()
    for tab, d, (a, a_s, l2c) in zip(tabs, devs, hps):
        d.fill(tab, a, a_s, l2c)
    return L.lib().drx_rows_csr_opt_multi(tabs, len(devs), C.byref(rule), _stream())


@pytest.mark.parametrize('kind', oo.KINDS)
@pytest.mark.parametrize('call', [0, 1])
def test_rows_csr_opt_multi(kind, call):
    """four tables of four G in one launch — plain and outer, with and without scalars, one of a single row, one past the per-table cap of
    4096 workgroups, each with its own step sizes and l2 — under two sets of the rule's hyper-parameters, in two table orders"""
    ts, hp = _multi_tables(), MULTI_RULES[call]
    order = (0, 1, 2, 3) if call == 0 else (3, 2, 1, 0)
    devs = [DeviceTable(kind, ts[i], absent='nan' if call else 'null') for i in order]
    assert _launch_multi(devs, [du.MULTI_HP[i] for i in order], _rule(kind, lr=99.0, **hp)) == 0
    for d, i in zip(devs, order):
        a, a_s, l2c = du.MULTI_HP[i]
        _check_table(d.results(), oo.expected_table(kind, ts[i], a, a_s, l2c, **hp), f'{kind} table {i} call {call}', 'drx_rows_csr_opt_multi')


def test_same_call_same_bits():
    t = _table('plain-scalars-ld52')
    flat = lambda r: [a for part in r if part is not None for a in part if a is not None]
    for kind in ('momentum', 'rmsprop_momentum'):
        runs = []
        for _ in range(2):
            d = DeviceTable(kind, t)
            assert d.launch() == 0
            runs.append(d.results())
        assert all(_same_bits(a, b) for a, b in zip(flat(runs[0]), flat(runs[1])))
        mruns = []
        for _ in range(2):
            devs = [DeviceTable(kind, x) for x in _multi_tables()[:3]]
            assert _launch_multi(devs, du.MULTI_HP[:3], _rule(kind)) == 0
            mruns.append([d.results() for d in devs])
        for r0, r1 in zip(*mruns):
            assert all(_same_bits(a, b) for a, b in zip(flat(r0), flat(r1)))


# ---- the _adam entry points are their twins with the Adam rule ----------------------------------------------------------------------
def test_adam_entries_equal_their_twins_bit_for_bit():
    import torch
    L = _L()
    lib = L.lib()
    A = du.HP
    adam = L.OptRule(0, A['alpha'], A['b1'], A['b2'], A['eps'])
    st = _stream()
    # flat
    n = 1027
    p0, m0, v0, g0 = du.flat_inputs(5, n)
    out = []
    for twin in (False, True):
        p, m, v, g = (Guarded(a, 4) for a in (p0, m0, v0, g0))
        if twin:
            assert lib.drx_opt_dense(p.ptr(), m.ptr(), v.ptr(), g.ptr(), n, C.byref(adam), A['l2c'], st) == 0
        else:
            assert lib.drx_adam_dense(p.ptr(), m.ptr(), v.ptr(), g.ptr(), n, A['alpha'], A['l2c'], A['b1'], A['b2'], A['eps'], st) == 0
        torch.cuda.synchronize()
        out.append([x.get() for x in (p, m, v)])
    assert all(_same_bits(a, b) for a, b in zip(*out)) and not _same_bits(out[0][0], p0)
    # segments
    start, lens, alpha, l2, n = du.segment_layout()
    p0, m0, v0, g0 = du.flat_inputs(31, n)
    sg = _segments(start, lens, alpha, l2)
    out = []
    for twin in (False, True):
        p, m, v, g = (Guarded(a, 4) for a in (p0, m0, v0, g0))
        if twin:
            assert lib.drx_opt_segments(p.ptr(), m.ptr(), v.ptr(), g.ptr(), C.byref(sg), C.byref(adam), st) == 0
        else:
            assert lib.drx_adam_segments(p.ptr(), m.ptr(), v.ptr(), g.ptr(), C.byref(sg), A['b1'], A['b2'], A['eps'], st) == 0
        torch.cuda.synchronize()
        out.append([x.get() for x in (p, m, v)])
    assert all(_same_bits(a, b) for a, b in zip(*out)) and not _same_bits(out[0][0], p0)
    # lookup tables: plain, outer, multi ('rmsprop_momentum' has Adam's two slots: v0 as s1, m0 as s2 — the same arrays both times)
    flat = lambda r: [a for part in r if part is not None for a in part]
    for name in ('plain-scalars-ld100', 'outer-g3-ld100'):
        t = _table(name)
        out = []
        for twin in (False, True):
            d = DeviceTable('rmsprop_momentum', t)
            state = (d.p.ptr(), d.s1.ptr(), d.s2.ptr(), d.ps.ptr(), d.s1s.ptr(), d.s2s.ptr())
            head = (d.tptr(d.row_ptr), d.tptr(d.order)) + ((d.tptr(d.scale), d.tptr(d.src), t['group']) if t['group'] else (d.tptr(d.src), d.tptr(d.scale)))
            f = {(0, False): lib.drx_rows_csr_adam, (0, True): lib.drx_rows_csr_opt, (1, False): lib.drx_rows_csr_adam_outer,
                 (1, True): lib.drx_rows_csr_opt_outer}[(int(t['group'] > 0), twin)]
            tail = (C.byref(adam),) if twin else (A['b1'], A['b2'], A['eps'])
            assert f(*head, t['ld'], t['n_rows'], *state, A['alpha'], A['alpha_s'], A['l2c'], *tail, st) == 0
            out.append(flat(d.results()))
        assert all(_same_bits(a, b) for a, b in zip(*out)) and not _same_bits(out[0][0], t['p0'])
    out = []
    for twin in (False, True):
        devs = [DeviceTable('rmsprop_momentum', x) for x in _multi_tables()[:3]]
        tabs = (L.CsrAdamTable * 3)()
        for tab, d, hp in zip(tabs, devs, du.MULTI_HP):
            d.fill(tab, *hp)
        if twin:
            assert lib.drx_rows_csr_opt_multi(tabs, 3, C.byref(adam), st) == 0
        else:
            assert lib.drx_rows_csr_adam_multi(tabs, 3, A['b1'], A['b2'], A['eps'], st) == 0
        out.append([a for d in devs for a in flat(d.results())])
    assert all(_same_bits(a, b) for a, b in zip(*out))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """an unknown kind, the row-wise Adagrad of the sampled step, a missing rule, a missing required slot: a status, and the state as it was"""
    import torch
    L = _L()
    lib = L.lib()
    st = _stream()
    n = 16
    p0, m0, v0, g0 = du.flat_inputs(3, n)
    p, m, v, g = (Guarded(a, 4) for a in (p0, m0, v0, g0))
    start, lens, alpha, l2, ns = du.segment_layout()
    sp0, sm0, sv0, sg0 = du.flat_inputs(31, ns)
    sp, sm, sv, sgr = (Guarded(a, 4) for a in (sp0, sm0, sv0, sg0))
    sg = _segments(start, lens, alpha, l2)
    t = du.make_table(5, 8, np.array([2, 0, 1]), 0, True)
    for code in (2, 8, -1, 100):
        rule = _rule(code)
        assert lib.drx_opt_dense(p.ptr(), m.ptr(), v.ptr(), g.ptr(), n, C.byref(rule), 0.0, st) != 0
        assert lib.drx_opt_segments(sp.ptr(), sm.ptr(), sv.ptr(), sgr.ptr(), C.byref(sg), C.byref(rule), st) != 0
    assert lib.drx_opt_dense(p.ptr(), m.ptr(), v.ptr(), g.ptr(), n, None, 0.0, st) != 0
    assert lib.drx_opt_segments(sp.ptr(), sm.ptr(), sv.ptr(), sgr.ptr(), C.byref(sg), None, st) != 0
    for kind in oo.KINDS + ('adam',):
        rule = _rule(kind)
        if oo.N_SLOTS[kind] >= 1:
            assert lib.drx_opt_dense(p.ptr(), NULL, v.ptr(), g.ptr(), n, C.byref(rule), 0.0, st) != 0, kind
            assert lib.drx_opt_segments(sp.ptr(), NULL, sv.ptr(), sgr.ptr(), C.byref(sg), C.byref(rule), st) != 0, kind
        if oo.N_SLOTS[kind] >= 2:
            assert lib.drx_opt_dense(p.ptr(), m.ptr(), NULL, g.ptr(), n, C.byref(rule), 0.0, st) != 0, kind
            assert lib.drx_opt_segments(sp.ptr(), sm.ptr(), NULL, sgr.ptr(), C.byref(sg), C.byref(rule), st) != 0, kind
        assert lib.drx_opt_dense(p.ptr(1), m.ptr(), v.ptr(), g.ptr(), 8, C.byref(rule), 0.0, st) != 0       # p misaligned by one float
    torch.cuda.synchronize()
    assert all(_same_bits(x.get(), a) for x, a in zip((p, m, v, g, sp, sm, sv, sgr), (p0, m0, v0, g0, sp0, sm0, sv0, sg0)))
    tables = []
    for kind in ('momentum', 'rmsprop_momentum'):
        d = DeviceTable(kind, t, absent='nan')
        tables.append(d)
        for code in (2, 8, -1):
            assert d.launch(rule=_rule(code)) != 0
            assert _launch_multi([d], du.MULTI_HP[:1], _rule(code)) != 0
        assert d.launch(s1=False) != 0                                       # the rule's s1 missing
        one = (L.CsrAdamTable * 1)()
        for field in ('m', 'm_s') + (('v', 'v_s') if kind == 'rmsprop_momentum' else ()):
            d.fill(one[0], *du.MULTI_HP[0])
            setattr(one[0], field, None)
            assert lib.drx_rows_csr_opt_multi(one, 1, C.byref(_rule(kind)), st) != 0, field
        d.fill(one[0], *du.MULTI_HP[0])
        assert lib.drx_rows_csr_opt_multi(one, 1, None, st) != 0
        assert d.unchanged()
    for d in tables:                                                         # ... and the same tables are accepted as they are
        assert d.launch() == 0 and not d.unchanged()


def test_sparse_entry_points_refuse_the_dense_kinds():
    """drx_cdae_step_sparse (and through it _timed, _prepared, _hot and drx_cdae_kshard_step: one validation, csrc/drx_cdae.hip
    step_sparse_impl) given DRX_OPT_SGD .. DRX_OPT_RMSPROP_MOMENTUM: DRX_EINVAL (-1), the return code only — parameters and slots keep their bits"""
    import torch
    from drecpy_amd.engine import CdaeEngine
    from oracle import cdae_oracle as co
    from helpers import batch_rows, synth_history
    L = _L()
    rng = np.random.default_rng(0)
    U_, N, K, B = 16, 40, 8, 8
    eng = CdaeEngine(U_, N, K)
    eng.set_params(**co.init_params(rng, U_, N, K, np.float64))
    indptr, indices = synth_history(rng, U_, N, 5)
    eng.set_history(indptr, indices)
    eng.init_optimizer('adagrad', 0.05, 1e-3)
    uids = rng.integers(0, U_, size=B)
    _, keep_off, _ = batch_rows(indptr, indices, uids, N)
    bt, alive = eng.make_batch(uids, rng.integers(0, N, size=B), (rng.random(B) < 0.3).astype(F), keep_off=keep_off, q=0.2, mask_seed=3)
    before = [x.clone() for x in eng.tables() + eng.s1]
    sc = eng._ensure_scratch(bt.B, bt.n_touch_slots)
    ev = (C.c_void_p * 8)()
    hot = L.HotHead()
    for code in (3, 4, 5, 6, 7, 8):
        o = eng._optim([0.05] * 5)
        o.kind = code
        args = (C.byref(eng._params), C.byref(o), C.byref(eng._hist), C.byref(bt), 0)
        assert L.lib().drx_cdae_step_sparse(*args, L.ptr(sc), sc.numel(), None, _stream()) == -1
        assert L.lib().drx_cdae_step_sparse_timed(*args, L.ptr(sc), sc.numel(), None, ev, _stream()) == -1
        assert L.lib().drx_cdae_step_sparse_prepared(*args, L.ptr(sc), sc.numel(), L.ptr(sc), sc.numel(), None, ev, _stream()) == -1
        assert L.lib().drx_cdae_step_sparse_hot(C.byref(eng._params), C.byref(o), C.byref(eng._hist), C.byref(bt), C.byref(hot), 0, L.ptr(sc),
                                                sc.numel(), L.ptr(sc), sc.numel(), None, ev, _stream()) == -1
    eng._optim_struct = None
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, eng.tables() + eng.s1))
    eng.step_sparse(0, bt)                                                   # (the same batch is accepted under its own kind)
    torch.cuda.synchronize()
    assert not torch.equal(before[0], eng.tables()[0])
