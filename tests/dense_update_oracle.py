"""The dense (Keras-Adam) update family of csrc/drx_generic.hip and k_adam_segments of csrc/drx_caser.hip as plain NumPy float64, with a
forward error bound for an fp32 implementation next to every expected array: drx_adam_dense, drx_adam_segments, drx_rows_csr_adam,
drx_rows_csr_adam_outer, drx_rows_csr_adam_multi (rows_adam per table), drx_rows_dot, drx_sumsq.  No torch, no libdrx: nothing here
shares a line with the kernels.  The input families of tests/test_gpu_dense_update.py are built here too, so that
tests/test_dense_update_oracle.py can run an fp32 NumPy replay of the same operations over them without a GPU.

The bound (u = 2^-23, TWICE fp32's unit roundoff: room for fused multiply-adds and second-order terms; a row named by c lookups):
    dg = (c + 2) u (sum|rows| + |l2c p|)                  any summation order of c terms, the l2 term, one more rounding
    dm = (1 - b1) dg + 4 u (|m| + |gt|)
    dv = (1 - b2) 2 |gt| dg + 4 u (|v| + gt^2)
    ds = min(dv / (2 sqrt(v1)), sqrt(dv)) + u sqrt(v1)     (error of sqrt(v1); the second arm: v1 -> 0)
    dp = alpha (dm / den_lo + |m1| ds / (den den_lo)) + 4 u (|p| + alpha |m1| / den_lo),   den = sqrt(v1) + eps, den_lo = max(den - ds, eps)
It is a function of the inputs alone.  Errors already in p, m, v (a second step after an fp32 first one) enter through `din`:
dm += b1 dm_in, dv += b2 dv_in, dp += dp_in, dg += l2c dp_in (m1 = b1 m + (1 - b1) gt, and so on).
Hyper-parameters cross the C ABI as floats: the oracle rounds them to fp32 first, and forms 1 - beta in fp32 like TF's ApplyAdam."""
import math
from collections import namedtuple

import numpy as np

U = 2.0 ** -23
HP = dict(alpha=1e-2, alpha_s=2e-2, l2c=1e-3, b1=0.9, b2=0.999, eps=1e-7)
SPLIT = 64                        # lookups from which the kernel cuts a row's sum into slices (kCsrSplit)
LDS = (4, 16, 20, 52, 100, 132, 256, 260, 516, 1024)

Adam = namedtuple('Adam', 'p m v dp dm dv')


def f32(x):
    return np.float32(x).astype(np.float64) if isinstance(x, np.ndarray) else float(np.float32(x))


def omb(beta):
    """1 - beta as TF's ApplyAdam and the kernels form it: in fp32"""
    return float(np.float32(1.0) - np.float32(beta))


def geom(ld):
    """(G, J): G lanes per row, J float4 per lane — the header's row geometry (include/drx.h, csrc/drx_common.hpp pick_geom)"""
    for top, g in ((16, 4), (32, 8), (64, 16), (128, 32), (256, 64)):
        if ld <= top:
            return g, 1
    return (64, 2) if ld <= 512 else (64, 4)


def gpb(ld):
    return 256 // geom(ld)[0]


def csr_from_keys(keys, n_rows):
    """row_ptr [n_rows + 1], order [T]: the lookups grouped by the row they name, a row's lookups ascending (stable)"""
    keys = np.asarray(keys, dtype=np.int64)
    assert keys.size == 0 or (keys.min() >= 0 and keys.max() < n_rows)
    order = np.argsort(keys, kind='stable').astype(np.int32)
    row_ptr = np.zeros(n_rows + 1, dtype=np.int32)
    row_ptr[1:] = np.cumsum(np.bincount(keys, minlength=n_rows))
    return row_ptr, order


def _adam(p, m, v, g, absg, c, alpha, l2c, b1, b2, eps, exact_sums=False, din=None):
    """ApplyAdam of gt = g + l2c p elementwise in float64 and the bound above; absg = sum of the |terms| of g, c their number"""
    alpha, l2c, eps = f32(alpha), f32(l2c), f32(eps)
    o1, o2 = omb(b1), omb(b2)
    gt = g + l2c * p
    m1 = m + (gt - m) * o1
    v1 = v + (gt * gt - v) * o2
    s = np.sqrt(v1)
    den = s + eps
    p1 = p - m1 * alpha / den
    dg = np.zeros_like(p) if exact_sums else (c + 2) * U * (absg + np.abs(l2c * p))
    dp_in = dm_in = dv_in = 0.0
    if din is not None:
        dp_in, dm_in, dv_in = din
        dg = dg + np.abs(l2c) * dp_in
    dm = o1 * dg + 4 * U * (np.abs(m) + np.abs(gt)) + (1 - o1) * dm_in
    dv = o2 * 2 * np.abs(gt) * dg + 4 * U * (np.abs(v) + gt * gt) + (1 - o2) * dv_in
    with np.errstate(divide='ignore', invalid='ignore'):
        ds = np.where(s > 0, np.minimum(dv / (2 * s), np.sqrt(dv)), np.sqrt(dv)) + U * s
    den_lo = np.maximum(den - ds, eps)
    dp = alpha * (dm / den_lo + np.abs(m1) * ds / (den * den_lo)) + 4 * U * (np.abs(p) + alpha * np.abs(m1) / den_lo) + dp_in
    return Adam(p1, m1, v1, dp, dm, dv)


def _row_sums(x, row_ptr, order):
    """per row: the float64 sum of x[order[q]] over the row's lookups (x [T] or [T, ld]); rows with no lookup get 0"""
    n_rows = len(row_ptr) - 1
    out = np.zeros((n_rows,) + x.shape[1:], dtype=np.float64)
    cnt = np.diff(row_ptr)
    has = cnt > 0
    if has.any():
        out[has] = np.add.reduceat(np.asarray(x, dtype=np.float64)[order], row_ptr[:-1][has].astype(np.int64), axis=0)
    return out


def rows_adam(p, m, v, row_ptr, order, rows, alpha, l2c, b1, b2, eps, scalars=None, exact_sums=False):
    """drx_rows_csr_adam / _outer on one table.  rows [T, ld] float64: the gradient row of lookup o (outer form: scale[o] * src[o // group]
    formed in float64 by the caller).  scalars = (p_s, m_s, v_s, src_s, alpha_s): the per-row scalar channel, no l2.
    Returns Adam for the table, and Adam for the scalars (or None)."""
    p, m, v = (np.asarray(a, dtype=np.float64) for a in (p, m, v))
    rows = np.asarray(rows, dtype=np.float64)
    c = np.diff(row_ptr).astype(np.float64)
    tab = _adam(p, m, v, _row_sums(rows, row_ptr, order), _row_sums(np.abs(rows), row_ptr, order), c[:, None], alpha, l2c, b1, b2, eps,
                exact_sums)
    sc = None
    if scalars is not None:
        ps, ms, vs, src_s, alpha_s = scalars
        ps, ms, vs, src_s = (np.asarray(a, dtype=np.float64) for a in (ps, ms, vs, src_s))
        sc = _adam(ps, ms, vs, _row_sums(src_s, row_ptr, order), _row_sums(np.abs(src_s), row_ptr, order), c, alpha_s, 0.0, b1, b2, eps,
                   exact_sums)
    return tab, sc


def adam_flat(p, m, v, g, alpha, l2c, b1, b2, eps, din=None):
    """drx_adam_dense (g may be None: pure decay) — alpha and l2c may be arrays (one value per element)"""
    p, m, v = (np.asarray(a, dtype=np.float64) for a in (p, m, v))
    g = np.zeros_like(p) if g is None else np.asarray(g, dtype=np.float64)
    return _adam(p, m, v, g, np.abs(g), 1.0, alpha, l2c, b1, b2, eps, din=din)


def adam_segments(p, m, v, g, start, length, alpha, l2, b1, b2, eps):
    """drx_adam_segments: segment s = elements [start[s], start[s] + length[s]) with its own alpha and l2; elements of no segment stay as
    they are (bound 0).  Returns Adam and the mask of the elements that belong to a segment."""
    p, m, v, g = (np.asarray(a, dtype=np.float64) for a in (p, m, v, g))
    a = np.zeros_like(p)
    l = np.zeros_like(p)
    inside = np.zeros(p.shape, dtype=bool)
    for s0, n, al, l2c in zip(start, length, alpha, l2):
        assert not inside[s0:s0 + n].any()
        a[s0:s0 + n], l[s0:s0 + n], inside[s0:s0 + n] = f32(al), f32(l2c), True
    r = _adam(p, m, v, g, np.abs(g), 1.0, a, l, b1, b2, eps)
    keep = lambda new, old: np.where(inside, new, old)
    zero = lambda d: np.where(inside, d, 0.0)
    return Adam(keep(r.p, p), keep(r.m, m), keep(r.v, v), zero(r.dp), zero(r.dm), zero(r.dv)), inside


def rows_dot(x, table, bias=None):
    """out[b, n] = x[b] . table[n] (+ bias[n]) and the bound (ld + 1) u (sum|x w| + |bias|)"""
    x, table = np.asarray(x, dtype=np.float64), np.asarray(table, dtype=np.float64)
    b = np.zeros(table.shape[0]) if bias is None else np.asarray(bias, dtype=np.float64)
    return x @ table.T + b[None, :], (table.shape[1] + 1) * U * (np.abs(x) @ np.abs(table).T + np.abs(b)[None, :])


def sumsq(*arrays):
    """sum of the exact float64 squares of all the arrays' elements (math.fsum) and the bound n 2^-52 sum x^2"""
    n, parts = 0, []
    for a in arrays:
        a = np.asarray(a, dtype=np.float64).ravel()
        n += a.size
        parts.append(math.fsum((a * a).tolist()))           # (an fp32 value's square is exact in float64: 48 bits)
    s = math.fsum(parts)
    return s, n * 2.0 ** -52 * s


# ---- the input families --------------------------------------------------------------------------------------------------------------
def count_profile(ld, rng):
    """lookups per row for a table of 2 gpb + 3 rows: 0 (first row and others), 1, 3, 4, 5 (the four-wide unroll and its tail), 63, 64,
    65 (the split threshold), ~150, 256 (gpb >= 8), ~600.  One round of gpb rows has no row of >= 64 lookups, one has two or more, and the last valid
    row of the partial third round has ~600."""
    g = gpb(ld)
    n_rows = 2 * g + 3
    if g == 4:
        return np.array([0, 1, 3, 4, 5, 63, 64, 65, 0, 150 + int(rng.integers(0, 8)), 600 - int(rng.integers(0, 8))], dtype=np.int64)
    cnt = rng.integers(0, 7, size=n_rows).astype(np.int64)
    cnt[:6] = (0, 1, 3, 4, 5, 63)
    cnt[7] = 0
    cnt[g], cnt[g + 3], cnt[2 * g - 1] = 64, 65, 150 + int(rng.integers(0, 8))
    cnt[g + 1] = 256                  # (per = 1024 / gpb: the one count here whose LAST slice is not empty at every gpb >= 8)
    cnt[2 * g] = 0
    cnt[-1] = 600 - int(rng.integers(0, 8))
    assert cnt[:g].max() < SPLIT and (cnt[g:2 * g] >= SPLIT).sum() >= 2 and cnt.max() <= 600
    return cnt


def capped_counts(ld, cap, rng):
    """cap * gpb + 5 rows — past the launch's cap of `cap` workgroups, so the row loop makes a second trip: most rows 0 or 1 lookups, a
    row of ~200 in the first trip, rows of ~300 in the second (one of them the table's last row, alone in a partly valid round)"""
    g = gpb(ld)
    n_rows = cap * g + 5
    cnt = rng.integers(0, 2, size=n_rows).astype(np.int64)
    cnt[0] = 0
    cnt[101], cnt[cap * g + 2], cnt[-1] = 200, 300, 310
    cnt[cap * g + 1] = 5
    return cnt


def make_table(seed, ld, counts, group=0, scalars=False, first_step=False):
    """One table's inputs, fp32 / int32 NumPy arrays: p0, m0, v0 [n_rows, ld], src ([T, ld], or [ceil(T / group), ld] in the outer form),
    scale [T] (the per-lookup scalars; None without the scalar channel), ps0, ms0, vs0 [n_rows], row_ptr, order.
    General inputs: U(-0.5, 0.5) rows, p and m, v in [0.01, 0.26].  first_step: m0 = v0 = 0 and every gradient a multiple of 1/256 in
    [-0.5, 0.5] (sums of 600 of them are exact in fp32 in any order)."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    n_rows, T = len(counts), int(counts.sum())
    keys = rng.permutation(np.repeat(np.arange(n_rows), counts))
    row_ptr, order = csr_from_keys(keys, n_rows)
    assert (np.diff(row_ptr) == counts).all()
    scalars = scalars or group > 0
    n_src = (T + group - 1) // group if group else T
    f = np.float32
    if first_step:
        draw = lambda *s: (rng.integers(-128, 129, size=s) / 256.0).astype(f)
    else:
        draw = lambda *s: (rng.random(s) - 0.5).astype(f)
    t = dict(ld=ld, n_rows=n_rows, T=T, group=group, counts=counts, row_ptr=row_ptr, order=order, first_step=first_step,
             src=draw(max(n_src, 1), ld), scale=draw(max(T, 1)) if scalars else None,
             p0=(rng.random((n_rows, ld)) - 0.5).astype(f), ps0=(rng.random(n_rows) - 0.5).astype(f) if scalars else None)
    if first_step:
        t['m0'], t['v0'] = np.zeros((n_rows, ld), f), np.zeros((n_rows, ld), f)
        t['ms0'], t['vs0'] = (np.zeros(n_rows, f), np.zeros(n_rows, f)) if scalars else (None, None)
    else:
        t['m0'], t['v0'] = (rng.random((n_rows, ld)) - 0.5).astype(f), (0.01 + 0.25 * rng.random((n_rows, ld))).astype(f)
        t['ms0'], t['vs0'] = ((rng.random(n_rows) - 0.5).astype(f), (0.01 + 0.25 * rng.random(n_rows)).astype(f)) if scalars else (None, None)
    return t


def lookup_rows(t):
    """the float64 gradient row of every lookup of table t: src[o], or scale[o] * src[o // group] formed in float64"""
    src = t['src'].astype(np.float64)
    if not t['group']:
        return src[:t['T']]
    o = np.arange(t['T'])
    return t['scale'].astype(np.float64)[:t['T'], None] * src[o // t['group']]


def expected_table(t, alpha=HP['alpha'], alpha_s=HP['alpha_s'], l2c=HP['l2c'], b1=HP['b1'], b2=HP['b2'], eps=HP['eps']):
    """rows_adam on table t of make_table (first_step tables: the sums are exact, dg = 0 — l2c must be 0 then)"""
    assert not (t['first_step'] and l2c)
    sc = (t['ps0'], t['ms0'], t['vs0'], t['scale'][:t['T']], alpha_s) if t['scale'] is not None else None
    return rows_adam(t['p0'], t['m0'], t['v0'], t['row_ptr'], t['order'], lookup_rows(t), alpha, l2c, b1, b2, eps, scalars=sc,
                     exact_sums=t['first_step'])


# the tables of the single-launch tests: (name, ld, group, scalars, first_step); counts = count_profile(ld) unless capped
def single_cases():
    out = []
    for ld in LDS:
        out.append((f'plain-ld{ld}', ld, 0, False, False))
        out.append((f'plain-scalars-ld{ld}', ld, 0, True, False))
    for ld in (52, 260):
        out.append((f'first-step-ld{ld}', ld, 0, True, True))
    for group in (1, 3, 12):
        for ld in (16, 100, 260):
            out.append((f'outer-g{group}-ld{ld}', ld, group, True, False))
    return out


def single_table(name):
    import zlib
    _, ld, group, scalars, first = next(c for c in single_cases() if c[0] == name)
    seed = zlib.crc32(name.encode())
    return make_table(seed, ld, count_profile(ld, np.random.default_rng(seed + 1)), group, scalars, first)


def capped_table(ld=132, cap=8192, scalars=True, group=0, seed=77):
    return make_table(seed, ld, capped_counts(ld, cap, np.random.default_rng(seed + 1)), group, scalars)


# drx_rows_csr_adam_multi: four tables of different G, plain and outer, with and without scalars, one of a single row (70 lookups: split over
# a workgroup with one valid row), one past the per-table cap of 4096 workgroups; every table its own alpha, alpha_s, l2c
MULTI_HP = ((1e-2, 2e-2, 1e-3), (5e-3, 3e-2, 2e-3), (2e-2, 1e-2, 0.0), (8e-3, 1.5e-2, 5e-4))


def multi_tables():
    r = lambda s: np.random.default_rng(s)
    return [make_table(901, 16, count_profile(16, r(11)), 0, True),
            make_table(902, 100, count_profile(100, r(12)), 3, True),
            make_table(903, 52, np.array([70]), 0, False),
            make_table(904, 132, capped_counts(132, 4096, r(14)), 0, True)]


def segment_layout():
    """24 segments (lens 0, 1, around 64, around 64 * 256 = one grid pass of drx_adam_segments, ...) with gaps of 0 - 5 elements between
    them: start, len, alpha, l2, and the array's length"""
    lens = [0, 1, 63, 64, 65, 16383, 16384, 16385, 2, 3, 4, 5, 7, 255, 256, 257, 1000, 1023, 1024, 1025, 31, 33, 127, 129]
    rng = np.random.default_rng(24)
    start, at = [], 3
    for n in lens:
        start.append(at)
        at += n + int(rng.integers(0, 6))
    alpha = (5e-3 + 1.5e-2 * rng.random(24)).tolist()
    l2 = [0.0 if i % 3 == 0 else float(x) for i, x in enumerate(2e-3 * rng.random(24))]
    return start, lens, alpha, l2, at + 4


def flat_inputs(seed, n, with_g=True):
    rng = np.random.default_rng(seed)
    f = np.float32
    return ((rng.random(n) - 0.5).astype(f), (rng.random(n) - 0.5).astype(f), (0.01 + 0.25 * rng.random(n)).astype(f),
            (rng.random(n) - 0.5).astype(f) if with_g else None)
