"""The dense (Keras-Adam) update kernels through the C ABI against tests/dense_update_oracle.py (NumPy float64) and its forward error
bound, element by element with no extra factor: drx_rows_csr_adam, drx_rows_csr_adam_outer, drx_rows_csr_adam_multi, drx_adam_dense
(and optimizers.Adam.apply_gradients over it), drx_adam_segments, drx_rows_dot, drx_sumsq / _lib.sumsq.  Every table is a view into a
larger buffer with a guard row of a sentinel before and after it; guards and inputs must come back bit-identical.  Each test prints
its largest error / bound ratio (pytest -s shows them)."""
import ctypes as C
import functools

import numpy as np
import pytest

import dense_update_oracle as du
from oracle import cdae_oracle as co

pytestmark = pytest.mark.gpu

HP = du.HP
B1, B2, EPS = HP['b1'], HP['b2'], HP['eps']
SENTINEL = -777.25
F = np.float32


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """`a` on the device between two guards of `pad` sentinel floats: .t is the view the kernels get"""

    def __init__(self, a, pad):
        import torch
        a = np.ascontiguousarray(a)
        self.n, self.pad, self.shape = a.size, pad, a.shape
        self.buf = torch.full((a.size + 2 * pad,), SENTINEL, dtype=torch.float32, device='cuda')
        self.t = self.buf[pad:pad + a.size]
        self.t.copy_(_dev(a.ravel()))

    def ptr(self, shift=0):
        return C.c_void_p(self.t.data_ptr() + 4 * shift)

    def get(self):
        """the array back on the host, after checking both guards bit for bit"""
        h = self.buf.cpu().numpy()
        g = np.concatenate([h[:self.pad], h[self.pad + self.n:]])
        assert g.size == 2 * self.pad and (g.view(np.int32) == np.array(SENTINEL, F).view(np.int32)).all(), 'a guard was written'
        return h[self.pad:self.pad + self.n].reshape(self.shape).copy()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


def _inside(got, want, bound, what):
    """|got - want| <= bound element by element (a NaN fails); returns the largest error / bound"""
    err = np.abs(got.astype(np.float64) - want)
    bad = ~(err <= bound)
    assert not bad.any(), (f'{what}: {int(bad.sum())} of {bad.size} elements outside the bound, first at {np.argwhere(bad)[0].tolist()}: got '
                           f'{got[bad][0]!r} want {want[bad][0]!r} bound {bound[bad][0]:.3g}; worst error / bound '
                           f'{np.nanmax(err[bad] / np.maximum(bound[bad], 1e-300)):.3g}')
    nz = bound > 0
    return float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0


def _report(kernel, case, ratio):
    print(f'[error/bound] {kernel} {case}: {ratio:.3f}')


def _lib():
    from drecpy_amd import _lib as L
    return L


def _stream():
    import torch
    return _lib().stream_ptr(torch.device('cuda:0'))


# ---- lookup tables -------------------------------------------------------------------------------------------------------------------
class DeviceTable:
    """a table of dense_update_oracle.make_table on the device: guarded state, the inputs, and what the ABI takes"""

    def __init__(self, t, scalars=None):
        self.t = t
        self.scalars = (t['scale'] is not None) if scalars is None else scalars
        ld = t['ld']
        self.p, self.m, self.v = (Guarded(t[k], ld) for k in ('p0', 'm0', 'v0'))
        self.ps, self.ms, self.vs = (Guarded(t[k], 1) for k in ('ps0', 'ms0', 'vs0')) if self.scalars else (None, None, None)
        self.row_ptr, self.order, self.src = _dev(t['row_ptr']), _dev(t['order']), _dev(t['src'])
        self.scale = _dev(t['scale']) if self.scalars else None

    def sptr(self, x):
        return x.ptr() if x is not None else C.c_void_p(0)

    def tptr(self, x):
        return C.c_void_p(x.data_ptr()) if x is not None else C.c_void_p(0)

    def launch(self, alpha=HP['alpha'], alpha_s=HP['alpha_s'], l2c=HP['l2c']):
        t, L = self.t, _lib().lib()
        state = (self.p.ptr(), self.m.ptr(), self.v.ptr(), self.sptr(self.ps), self.sptr(self.ms), self.sptr(self.vs))
        if t['group']:
            return L.drx_rows_csr_adam_outer(self.tptr(self.row_ptr), self.tptr(self.order), self.tptr(self.scale), self.tptr(self.src), t['group'],
                                             t['ld'], t['n_rows'], *state, alpha, alpha_s, l2c, B1, B2, EPS, _stream())
        return L.drx_rows_csr_adam(self.tptr(self.row_ptr), self.tptr(self.order), self.tptr(self.src), self.tptr(self.scale), t['ld'],
                                   t['n_rows'], *state, alpha, alpha_s, l2c, B1, B2, EPS, _stream())

    def fill(self, tab, alpha, alpha_s, l2c):
        """this table's entry of a drx_rows_csr_adam_multi call"""
        t = self.t
        tab.row_ptr, tab.order, tab.src, tab.scale = (x.data_ptr() if x is not None else None for x in (self.row_ptr, self.order, self.src, self.scale))
        tab.group, tab.ld, tab.n_rows = t['group'], t['ld'], t['n_rows']
        tab.p, tab.m, tab.v = (x.t.data_ptr() for x in (self.p, self.m, self.v))
        tab.p_s, tab.m_s, tab.v_s = (x.t.data_ptr() if x is not None else None for x in (self.ps, self.ms, self.vs))
        tab.alpha, tab.alpha_s, tab.l2_coef = alpha, alpha_s, l2c

    def results(self):
        """(p, m, v), (p_s, m_s, v_s) or None — after checking the guards and that the inputs came back bit-identical"""
        import torch
        torch.cuda.synchronize()
        t = self.t
        for dev, host in ((self.row_ptr, t['row_ptr']), (self.order, t['order']), (self.src, t['src'])) + \
                         (((self.scale, t['scale']),) if self.scalars else ()):
            assert _same_bits(dev.cpu().numpy(), np.ascontiguousarray(host)), 'an input was written'
        tab = tuple(x.get() for x in (self.p, self.m, self.v))
        return tab, (tuple(x.get() for x in (self.ps, self.ms, self.vs)) if self.scalars else None)

    def unchanged(self):
        tab, sc = self.results()
        t = self.t
        ok = all(_same_bits(a, t[k]) for a, k in zip(tab, ('p0', 'm0', 'v0')))
        return ok and (sc is None or all(_same_bits(a, t[k]) for a, k in zip(sc, ('ps0', 'ms0', 'vs0'))))


def _strip_scalars(t):
    return dict(t, scale=None, ps0=None, ms0=None, vs0=None)


@functools.lru_cache(maxsize=None)
def _single(name):
    """(table, its float64 result) of a single-launch case; 'plain-ld*' cases carry no scalar channel.  Computed once, read-only."""
    t = du.single_table(name)
    if name.startswith('plain-ld'):
        t = _strip_scalars(t)
    want = du.expected_table(t, l2c=0.0 if t['first_step'] else HP['l2c'])
    return t, want


def _check_table(got, want, what, kernel):
    (tab, sc), (wtab, wsc) = got, want
    worst = 0.0
    for a, w, b, n in zip(tab, wtab[:3], wtab[3:], 'pmv'):
        worst = max(worst, _inside(a, w, b, f'{what} {n}'))
    assert (sc is None) == (wsc is None)
    if sc is not None:
        for a, w, b, n in zip(sc, wsc[:3], wsc[3:], ('p_s', 'm_s', 'v_s')):
            worst = max(worst, _inside(a, w, b, f'{what} {n}'))
    _report(kernel, what, worst)
    return worst


@pytest.mark.parametrize('name', [c[0] for c in du.single_cases() if c[0].startswith('plain')])
def test_rows_csr_adam_plain(name):
    t, want = _single(name)
    d = DeviceTable(t)
    assert d.launch() == 0
    _check_table(d.results(), want, name, 'drx_rows_csr_adam')


@pytest.mark.parametrize('name', [c[0] for c in du.single_cases() if c[0].startswith('first-step')])
def test_rows_csr_adam_first_step(name):
    """m0 = v0 = 0, l2c = 0, gradients multiples of 1/256: the sums are exact in any order (dg = 0 in the bound), and a row that no lookup
    names keeps p bit for bit and m = v = 0 exactly"""
    t, want = _single(name)
    d = DeviceTable(t)
    assert d.launch(l2c=0.0) == 0
    got = d.results()
    _check_table(got, want, name, 'drx_rows_csr_adam')
    idle = t['counts'] == 0
    assert idle.sum() >= 2
    (p, m, v), (ps, ms, vs) = got
    assert _same_bits(p[idle], t['p0'][idle]) and not m[idle].any() and not v[idle].any()
    assert _same_bits(ps[idle], t['ps0'][idle]) and not ms[idle].any() and not vs[idle].any()
    assert not np.signbit(m[idle]).any() and not np.signbit(v[idle]).any()


@functools.lru_cache(maxsize=None)
def _capped():
    t = du.capped_table()
    return t, du.expected_table(t)


def test_rows_csr_adam_past_the_grid_cap():
    """8192 * 4 + 5 rows of ld 132: the workgroups' row loop makes a second trip, with rows of 300 lookups in it"""
    t, want = _capped()
    assert t['n_rows'] == 8192 * 4 + 5 and (np.nonzero(t['counts'] >= du.SPLIT)[0] >= 32768).sum() == 2
    d = DeviceTable(t)
    assert d.launch() == 0
    _check_table(d.results(), want, 'capped-ld132', 'drx_rows_csr_adam')


@pytest.mark.parametrize('name', [c[0] for c in du.single_cases() if c[0].startswith('outer')])
def test_rows_csr_adam_outer(name):
    t, want = _single(name)
    assert t['group'] > 0
    d = DeviceTable(t)
    assert d.launch() == 0
    _check_table(d.results(), want, name, 'drx_rows_csr_adam_outer')


@functools.lru_cache(maxsize=None)
def _multi():
    ts = du.multi_tables()
    return ts, [du.expected_table(t, a, a_s, l2c) for t, (a, a_s, l2c) in zip(ts, du.MULTI_HP)]


def _launch_multi(devs, hps):
    L = _lib()
    tabs = (L.CsrAdamTable * len(devs))()
    for tab, d, (a, a_s, l2c) in zip(tabs, devs, hps):
        d.fill(tab, a, a_s, l2c)
    return L.lib().drx_rows_csr_adam_multi(tabs, len(devs), B1, B2, EPS, _stream())


@pytest.mark.parametrize('order', [(0, 1, 2, 3), (3, 2, 1, 0)])
def test_rows_csr_adam_multi_against_the_oracle(order):
    """four tables of four G in one launch — plain and outer, with and without scalars, one of a single row, one past the per-table cap
    of 4096 workgroups, each with its own alpha, alpha_s and l2c — in both orders"""
    ts, wants = _multi()
    devs = [DeviceTable(ts[i]) for i in order]
    assert _launch_multi(devs, [du.MULTI_HP[i] for i in order]) == 0
    for d, i in zip(devs, order):
        _check_table(d.results(), wants[i], f'table {i} of order {order}', 'drx_rows_csr_adam_multi')


def test_same_call_same_bits():
    t, _ = _single('plain-scalars-ld52')
    runs = []
    for _ in range(2):
        d = DeviceTable(t)
        assert d.launch() == 0
        runs.append(d.results())
    ts, _ = _multi()
    mruns = []
    for _ in range(2):
        devs = [DeviceTable(x) for x in ts]
        assert _launch_multi(devs, du.MULTI_HP) == 0
        mruns.append([d.results() for d in devs])
    flat = lambda r: [a for part in r if part is not None for a in part]
    assert all(_same_bits(a, b) for a, b in zip(flat(runs[0]), flat(runs[1])))
    for r0, r1 in zip(*mruns):
        assert all(_same_bits(a, b) for a, b in zip(flat(r0), flat(r1)))


def test_rows_csr_adam_refusals():
    """invalid descriptions return a status and launch nothing: the state stays as it was"""
    L = _lib()
    lib = L.lib()
    null = C.c_void_p(0)
    mk = lambda ld, n_rows=3, group=0, scalars=True: DeviceTable(du.make_table(5, ld, np.array([2, 0, 1][:n_rows]), group, scalars))
    st = _stream()

    def plain(d, ld=None, n_rows=None, p=None, p_s='own', src_s='own'):
        t = d.t
        return lib.drx_rows_csr_adam(d.tptr(d.row_ptr), d.tptr(d.order), d.tptr(d.src), d.tptr(d.scale) if src_s == 'own' else src_s,
                                     t['ld'] if ld is None else ld, t['n_rows'] if n_rows is None else n_rows, p or d.p.ptr(), d.m.ptr(),
                                     d.v.ptr(), d.sptr(d.ps) if p_s == 'own' else p_s, d.sptr(d.ms), d.sptr(d.vs), HP['alpha'], HP['alpha_s'],
                                     HP['l2c'], B1, B2, EPS, st)

    def outer(d, group=None, p_s='own'):
        t = d.t
        return lib.drx_rows_csr_adam_outer(d.tptr(d.row_ptr), d.tptr(d.order), d.tptr(d.scale), d.tptr(d.src), t['group'] if group is None else group,
                                           t['ld'], t['n_rows'], d.p.ptr(), d.m.ptr(), d.v.ptr(), d.sptr(d.ps) if p_s == 'own' else p_s,
                                           d.sptr(d.ms), d.sptr(d.vs), HP['alpha'], HP['alpha_s'], HP['l2c'], B1, B2, EPS, st)

    big = mk(1032)                                       # (room for a row of 1028 floats)
    d8, d260, o8 = mk(8), mk(260), mk(8, group=2)
    assert plain(d8, ld=6) != 0
    assert plain(big, ld=1028) != 0
    assert plain(d8, n_rows=0) != 0
    assert plain(d8, src_s=null) != 0                    # p_s without src_s
    assert plain(d8, p_s=null) != 0                      # src_s without p_s
    assert plain(d8, p=d8.p.ptr(1)) != 0                 # p misaligned by one float
    assert outer(o8, group=0) != 0
    assert outer(o8, p_s=null) != 0
    # the multi launch: ld 260, 5 tables, and the same refusals per table
    assert _launch_multi([d8, d260], du.MULTI_HP[:2]) != 0
    tabs = (L.CsrAdamTable * 5)()
    for tab in tabs:
        d8.fill(tab, *du.MULTI_HP[0])
    assert lib.drx_rows_csr_adam_multi(tabs, 5, B1, B2, EPS, st) != 0
    assert lib.drx_rows_csr_adam_multi(tabs, 0, B1, B2, EPS, st) != 0
    for field, value in (('ld', 6), ('n_rows', 0), ('p_s', None), ('scale', None), ('p', d8.p.t.data_ptr() + 4)):
        one = (L.CsrAdamTable * 1)()
        d8.fill(one[0], *du.MULTI_HP[0])
        setattr(one[0], field, value)
        assert lib.drx_rows_csr_adam_multi(one, 1, B1, B2, EPS, st) != 0, field
    one = (L.CsrAdamTable * 1)()
    o8.fill(one[0], *du.MULTI_HP[0])
    one[0].scale, one[0].p_s, one[0].m_s, one[0].v_s = None, None, None, None      # outer without its scalars
    assert lib.drx_rows_csr_adam_multi(one, 1, B1, B2, EPS, st) != 0
    for d in (big, d8, d260, o8):
        assert d.unchanged()
    # ... and the same tables are accepted as they are
    assert plain(d8) == 0 and outer(o8) == 0
    assert not d8.unchanged() and not o8.unchanged()


# ---- drx_adam_dense ------------------------------------------------------------------------------------------------------------------
DENSE_N = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4 * 256 * 4096 + 4 * 256 + 3)


def _adam_dense(p, m, v, g, n, alpha, l2c, shift_p=0, shift_g=0):
    return _lib().lib().drx_adam_dense(p.ptr(shift_p), m.ptr(), v.ptr(), g.ptr(shift_g) if g is not None else C.c_void_p(0), n, alpha, l2c, B1, B2,
                                       EPS, _stream())


@pytest.mark.parametrize('n', DENSE_N)
def test_adam_dense(n):
    """g with l2c 0, g with l2c 1e-3, g == NULL with l2c 1e-3 (pure decay): one grid pass is 4096 x 256 float4, the last n leaves a second
    pass of one workgroup's worth and a tail of 3 next to it"""
    import torch
    p0, m0, v0, g0 = du.flat_inputs(n, n)
    worst = 0.0
    for mode, l2c in (('g', 0.0), ('g+l2', HP['l2c']), ('decay', HP['l2c'])):
        gh = None if mode == 'decay' else g0
        want = du.adam_flat(p0, m0, v0, gh, HP['alpha'], l2c, B1, B2, EPS)
        p, m, v = (Guarded(a, 4) for a in (p0, m0, v0))
        g = Guarded(g0, 4) if gh is not None else None
        assert _adam_dense(p, m, v, g, n, HP['alpha'], l2c) == 0
        torch.cuda.synchronize()
        for x, w, b, what in zip((p, m, v), want[:3], want[3:], 'pmv'):
            worst = max(worst, _inside(x.get(), w, b, f'n {n} {mode} {what}'))
        if g is not None:
            assert _same_bits(g.get(), g0)
    _report('drx_adam_dense', f'n {n}', worst)


def test_adam_dense_refusals():
    import torch
    p0, m0, v0, g0 = du.flat_inputs(3, 16)
    p, m, v, g = (Guarded(a, 4) for a in (p0, m0, v0, g0))
    assert _adam_dense(p, m, v, g, 0, HP['alpha'], 0.0) != 0
    assert _adam_dense(p, m, v, g, 8, HP['alpha'], 0.0, shift_p=1) != 0
    assert _adam_dense(p, m, v, g, 8, HP['alpha'], 0.0, shift_g=1) != 0
    torch.cuda.synchronize()
    assert all(_same_bits(x.get(), a) for x, a in zip((p, m, v, g), (p0, m0, v0, g0)))


def test_apply_gradients_pads_small_and_misaligned_variables():
    """optimizers.Adam.apply_gradients on variables of 1, 3 and 5 elements and on flat[1:9] (8 floats, 4 bytes off a 16-byte boundary),
    two steps: p against two chained float64 steps (the second one's bound carries the first one's), so the moments of the padded
    path must survive from one call to the next"""
    import torch
    from drecpy_amd.optimizers import Adam
    lr = 1e-2
    rng = np.random.default_rng(8)
    flat0 = (rng.random(12) - 0.5).astype(F)
    flat = _dev(flat0)
    host = [(rng.random(k) - 0.5).astype(F) for k in (1, 3, 5)] + [flat0[1:9].copy()]
    var = [_dev(h) for h in host[:3]] + [flat[1:9]]
    assert var[3].data_ptr() % 16 == 4
    grads = [[(rng.random(h.size) - 0.5).astype(F) for h in host] for _ in range(2)]
    opt = Adam(lr)
    state = [(h.astype(np.float64), np.zeros(h.size), np.zeros(h.size), None) for h in host]
    worst = 0.0
    for step in (1, 2):
        opt.apply_gradients([(_dev(g), x) for g, x in zip(grads[step - 1], var)])
        torch.cuda.synchronize()
        a = co.adam_alpha(lr, step)
        assert opt.iterations == step and opt.lr_t(step) == pytest.approx(a, rel=1e-7)
        for i, (g, x) in enumerate(zip(grads[step - 1], var)):
            p, m, v, din = state[i]
            r = du.adam_flat(p, m, v, g, a, 0.0, B1, B2, EPS, din=din)
            state[i] = (r.p, r.m, r.v, (r.dp, r.dm, r.dv))
            worst = max(worst, _inside(x.cpu().numpy(), r.p, r.dp, f'step {step} variable {i} p'))
            mm, vv = opt._moments(x, x)
            worst = max(worst, _inside(mm.cpu().numpy(), r.m, r.dm, f'step {step} variable {i} m'))
            worst = max(worst, _inside(vv.cpu().numpy(), r.v, r.dv, f'step {step} variable {i} v'))
    back = flat.cpu().numpy()
    assert _same_bits(back[:1], flat0[:1]) and _same_bits(back[9:], flat0[9:])
    _report('drx_adam_dense', 'apply_gradients', worst)


# ---- drx_adam_segments ---------------------------------------------------------------------------------------------------------------
def _segments(start, lens, alpha, l2):
    sg = _lib().AdamSegments()
    sg.n = len(lens)
    for i, (s, k, a, l) in enumerate(zip(start, lens, alpha, l2)):
        sg.start[i], sg.len[i], sg.alpha[i], sg.l2_coef[i] = s, k, a, l
    return sg


@pytest.mark.parametrize('n_seg', [24, 1])
def test_adam_segments(n_seg):
    """24 segments (empty, 1, around 64, around 64 x 256: more than the launch's 64 workgroups cover in one pass) with gaps between
    them, each with its own alpha and l2; what lies in no segment keeps its bits.  n = 1: the first non-empty segment alone."""
    import torch
    start, lens, alpha, l2, n = du.segment_layout()
    if n_seg == 1:
        start, lens, alpha, l2 = start[4:5], lens[4:5], alpha[4:5], l2[4:5]
    p0, m0, v0, g0 = du.flat_inputs(31, n)
    want, inside = du.adam_segments(p0, m0, v0, g0, start, lens, alpha, l2, B1, B2, EPS)
    p, m, v, g = (Guarded(a, 4) for a in (p0, m0, v0, g0))
    sg = _segments(start, lens, alpha, l2)
    assert _lib().lib().drx_adam_segments(p.ptr(), m.ptr(), v.ptr(), g.ptr(), C.byref(sg), B1, B2, EPS, _stream()) == 0
    torch.cuda.synchronize()
    worst = 0.0
    for x, x0, w, b, what in zip((p, m, v), (p0, m0, v0), want[:3], want[3:], 'pmv'):
        got = x.get()
        worst = max(worst, _inside(got, w, b, f'{n_seg} segments {what}'))
        assert _same_bits(got[~inside], x0[~inside])
        assert (got[inside] != x0[inside]).mean() > 0.9
    assert _same_bits(g.get(), g0)
    _report('drx_adam_segments', f'{n_seg} segments', worst)


def test_adam_segments_refusals():
    import torch
    start, lens, alpha, l2, n = du.segment_layout()
    p0, m0, v0, g0 = du.flat_inputs(31, n)
    p, m, v, g = (Guarded(a, 4) for a in (p0, m0, v0, g0))
    sg = _segments(start, lens, alpha, l2)
    for bad in (0, 25):
        sg.n = bad
        assert _lib().lib().drx_adam_segments(p.ptr(), m.ptr(), v.ptr(), g.ptr(), C.byref(sg), B1, B2, EPS, _stream()) != 0
    torch.cuda.synchronize()
    assert all(_same_bits(x.get(), a) for x, a in zip((p, m, v, g), (p0, m0, v0, g0)))


# ---- drx_rows_dot --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ld', du.LDS)
def test_rows_dot(ld):
    """B 1 and 3, with and without bias, tables of 1 row and of gpb + 1 rows (ld 132: also 2048 * 4 + 5, past the launch's 2048 workgroups)"""
    import torch
    rng = np.random.default_rng(ld)
    worst = 0.0
    for n_rows in (1, du.gpb(ld) + 1) + ((2048 * 4 + 5,) if ld == 132 else ()):
        tab0, bias0 = (rng.random((n_rows, ld)) - 0.5).astype(F), (rng.random(n_rows) - 0.5).astype(F)
        tab, bias = Guarded(tab0, ld), Guarded(bias0, 1)
        for B in (1, 3):
            x0 = (rng.random((B, ld)) - 0.5).astype(F)
            x = Guarded(x0, ld)
            for with_bias in (True, False):
                want, bound = du.rows_dot(x0, tab0, bias0 if with_bias else None)
                out = Guarded(np.full((B, n_rows), 5.5, F), 4)
                assert _lib().lib().drx_rows_dot(x.ptr(), B, tab.ptr(), n_rows, ld, bias.ptr() if with_bias else C.c_void_p(0), out.ptr(),
                                                 _stream()) == 0
                torch.cuda.synchronize()
                worst = max(worst, _inside(out.get(), want, bound, f'ld {ld} n_rows {n_rows} B {B} bias {with_bias}'))
            assert _same_bits(x.get(), x0)
        assert _same_bits(tab.get(), tab0) and _same_bits(bias.get(), bias0)
    _report('drx_rows_dot', f'ld {ld}', worst)


# ---- drx_sumsq -----------------------------------------------------------------------------------------------------------------------
def _spread(seed, n):
    rng = np.random.default_rng(seed)
    return (np.sign(rng.random(n) - 0.5) * 10.0 ** rng.uniform(-18, 3, n)).astype(F)


OUT_GUARD = -3.0


def _sumsq_out(first):
    import torch
    out = torch.full((1 + 1024 + 1,), OUT_GUARD, dtype=torch.float64, device='cuda')
    out[0] = first
    return out


@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, 262144, 262145, 3000001])
def test_sumsq(n):
    """magnitudes from 1e-18 to 1e3; accumulate 0 overwrites out[0], accumulate 1 adds to it (n = 0: 0, and out[0] as it was)"""
    import torch
    lib = _lib().lib()
    x0, y0 = _spread(n, max(n, 1)), _spread(n + 1, 300)
    x, y = Guarded(x0, 4), Guarded(y0, 4)
    out = _sumsq_out(123.0)
    assert lib.drx_sumsq(x.ptr(), n, C.c_void_p(out.data_ptr()), 0, _stream()) == 0
    s, b = du.sumsq(x0[:n])
    got = float(out.cpu().numpy()[0])
    assert abs(got - s) <= b, (got, s, b)
    worst = abs(got - s) / b if b else 0.0
    assert lib.drx_sumsq(y.ptr(), 300, C.c_void_p(out.data_ptr()), 1, _stream()) == 0
    s2, b2 = du.sumsq(x0[:n], y0)
    got2 = float(out.cpu().numpy()[0])
    assert abs(got2 - s2) <= b2, (got2, s2, b2)
    worst = max(worst, abs(got2 - s2) / b2)
    if n == 0:
        assert got == 0.0
        assert lib.drx_sumsq(x.ptr(), 0, C.c_void_p(out.data_ptr()), 1, _stream()) == 0
        assert float(out.cpu().numpy()[0]) == got2
    torch.cuda.synchronize()
    assert float(out.cpu().numpy()[-1]) == OUT_GUARD and _same_bits(x.get(), x0) and _same_bits(y.get(), y0)
    _report('drx_sumsq', f'n {n}', worst)


def test_lib_sumsq_skips_none_and_empty_and_takes_views():
    import torch
    L = _lib()
    a0, b0 = _spread(1, 1000).reshape(20, 50), _spread(2, 777)
    a, b = _dev(a0), _dev(b0)
    view = a[:, ::2]
    assert not view.is_contiguous()
    got = L.sumsq([None, torch.empty(0, device='cuda'), view, b])
    s, bound = du.sumsq(a0[:, ::2], b0)
    assert abs(got - s) <= bound, (got, s, bound)
    assert L.sumsq([None, torch.empty(0, device='cuda')]) == 0.0 and L.sumsq([]) == 0.0
    assert _same_bits(a.cpu().numpy(), a0)
    _report('_lib.sumsq', 'list', abs(got - s) / bound)
