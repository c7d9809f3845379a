"""The dense update rules beside Adam — sgd, momentum, nesterov, adagrad, rmsprop, rmsprop_momentum (include/drx.h DrxOptRule) — as
plain NumPy float64 over flat arrays, segments and CSR-summed rows, with a forward error bound for an fp32 implementation next to every
expected array.  The row sums and the table builders are tests/dense_update_oracle.py's; no torch, no libdrx: nothing here shares a line
with the kernels.  This text is the definition of record of the rules (there is no TensorFlow to pin them against):

    gt = g + l2c p
    sgd               p1 = p - lr gt
    momentum          a1 = a mu - gt lr;                  p1 = p + a1
    nesterov          a1 = a mu - gt lr;                  p1 = p + (a1 mu - gt lr)
    adagrad           a1 = a + gt gt;                     p1 = p - lr gt / (sqrt(a1) + eps)
    rmsprop           r1 = r + (gt gt - r)(1 - rho);      p1 = p - lr gt / (sqrt(r1) + eps)            (eps outside the root)
    rmsprop_momentum  r1 as above;  m1 = m mu + (gt lr) / sqrt(r1 + eps);  p1 = p - m1                 (eps inside the root)

The bound (u = 2^-23, TWICE fp32's unit roundoff, as in dense_update_oracle: every line below is one to three fp32 operations, each
within u / 2 relative of its exact result, fused or not — a fused multiply-add rounds once where the unfused pair rounds twice, so a
bound for the unfused form covers both; 4 u on the magnitudes of a line's terms leaves room for second-order terms):
    dg  = (c + 2) u (sum|rows| + |l2c p|)                                     c summed rows in any order, the l2 term, one more rounding
    sgd               dp  = lr dg + 4 u (|p| + lr |gt|)
    momentum          da  = lr dg + 4 u (|a mu| + lr |gt|);                     dp = da + 4 u (|p| + |a1|)
    nesterov          da  as above;                                             dp = mu da + lr dg + 4 u (|p| + |a1 mu| + lr |gt|)
    adagrad           da  = (2 |gt| + dg) dg + 4 u (|a| + gt^2)
    rmsprop           dr  = (1 - rho)(2 |gt| + dg) dg + 4 u (|r| + gt^2)
      both:           ds  = min(dx / (2 s), sqrt(dx)) + u s,  s = sqrt(x1)       (x = a or r; the second arm: x1 -> 0)
                      dp  = lr (dg / den_lo + |gt| ds / (den den_lo)) + 4 u (|p| + lr |gt| / den_lo),   den = s + eps, den_lo = max(den - ds, eps)
    rmsprop_momentum  dr  as above;  y = r1 + eps, dy = dr + u y;  den = sqrt(y), dd = min(dy / (2 den), sqrt(dy)) + u den, den_lo = den - dd > 0
                      dm  = lr (dg / den_lo + |gt| dd / (den den_lo)) + 4 u (|m mu| + lr |gt| / den_lo);   dp = dm + 4 u (|p| + |m1|)
It is a function of the inputs alone.  Errors already in p and the slots (a later step after an fp32 earlier one) enter through
`din` = (dp, ds1, ds2): dg += |l2c| dp_in, da += mu da_in (adagrad: da_in; rmsprop: rho dr_in), dm += mu dm_in, dp += dp_in.
Hyper-parameters cross the C ABI as floats: the oracle rounds them to fp32 first and forms 1 - rho in fp32, like the kernels."""
from collections import namedtuple

import numpy as np

import dense_update_oracle as du
from dense_update_oracle import U, f32, omb

KINDS = ('sgd', 'momentum', 'nesterov', 'adagrad', 'rmsprop', 'rmsprop_momentum')
CODE = {'adam': 0, 'adagrad': 1, 'rowwise_adagrad': 2, 'sgd': 3, 'momentum': 4, 'nesterov': 5, 'rmsprop': 6, 'rmsprop_momentum': 7}   # DRX_OPT_*
N_SLOTS = {'sgd': 0, 'momentum': 1, 'nesterov': 1, 'adagrad': 1, 'rmsprop': 1, 'rmsprop_momentum': 2, 'adam': 2}
# (lr, lr_s, l2c) as dense_update_oracle.HP has (alpha, alpha_s, l2c); mu = momentum, rho, eps
HP = dict(lr=1e-2, lr_s=2e-2, l2c=1e-3, mu=0.9, rho=0.9, eps=1e-7)

Rule = namedtuple('Rule', 'p s1 s2 dp ds1 ds2')          # s1 / s2 (and their bounds): None where the rule has no such slot


def _root(x1, dx):
    """s = sqrt(x1) and the error of an fp32 root of an x1 known to dx"""
    s = np.sqrt(x1)
    with np.errstate(divide='ignore', invalid='ignore'):
        ds = np.where(s > 0, np.minimum(dx / (2 * s), np.sqrt(dx)), np.sqrt(dx)) + U * s
    return s, ds


def apply(kind, p, s1, s2, g, absg, c, lr, l2c, mu=0.0, rho=0.0, eps=0.0, exact_sums=False, din=None):
    """one step of rule `kind` on gt = g + l2c p elementwise in float64, and the bound of the head; absg = sum of the |terms| of g, c
    their number.  lr and l2c may be arrays (one value per element)."""
    assert kind in KINDS
    lr, l2c, mu, eps = f32(lr), f32(l2c), f32(mu), f32(eps)
    o2 = omb(rho)
    gt = g + l2c * p
    dg = np.zeros_like(p) if exact_sums else (c + 2) * U * (absg + np.abs(l2c * p))
    dp_in = d1_in = d2_in = 0.0
    if din is not None:
        dp_in, d1_in, d2_in = (0.0 if d is None else d for d in din)
        dg = dg + np.abs(l2c) * dp_in
    ag = np.abs(gt)
    if kind == 'sgd':
        p1 = p - lr * gt
        return Rule(p1, None, None, lr * dg + 4 * U * (np.abs(p) + lr * ag) + dp_in, None, None)
    if kind in ('momentum', 'nesterov'):
        a1 = s1 * mu - gt * lr
        da = lr * dg + 4 * U * (np.abs(s1 * mu) + lr * ag) + mu * d1_in
        if kind == 'momentum':
            return Rule(p + a1, a1, None, da + 4 * U * (np.abs(p) + np.abs(a1)) + dp_in, da, None)
        return Rule(p + (a1 * mu - gt * lr), a1, None, mu * da + lr * dg + 4 * U * (np.abs(p) + np.abs(a1 * mu) + lr * ag) + dp_in, da, None)
    if kind == 'adagrad':
        x1 = s1 + gt * gt
        dx = (2 * ag + dg) * dg + 4 * U * (np.abs(s1) + gt * gt) + d1_in
    else:
        x1 = s1 + (gt * gt - s1) * o2
        dx = o2 * (2 * ag + dg) * dg + 4 * U * (np.abs(s1) + gt * gt) + (1 - o2) * d1_in
    if kind == 'rmsprop_momentum':
        y = x1 + eps
        den, dd = _root(y, dx + U * y)
        den_lo = den - dd
        assert (den_lo > 0).all()
        m1 = s2 * mu + (gt * lr) / den
        dm = lr * (dg / den_lo + ag * dd / (den * den_lo)) + 4 * U * (np.abs(s2 * mu) + lr * ag / den_lo) + mu * d2_in
        return Rule(p - m1, x1, m1, dm + 4 * U * (np.abs(p) + np.abs(m1)) + dp_in, dx, dm)
    s, ds = _root(x1, dx)
    den = s + eps
    den_lo = np.maximum(den - ds, eps)
    p1 = p - lr * gt / den
    dp = lr * (dg / den_lo + ag * ds / (den * den_lo)) + 4 * U * (np.abs(p) + lr * ag / den_lo) + dp_in
    return Rule(p1, x1, None, dp, dx, None)


def step_size(kind, p, s1, g, lr, l2c, mu):
    """the size of the step the rule takes, as the bound is compared against: lr |gt|, or |s1 mu| for the momentum rules of SGD"""
    if kind in ('momentum', 'nesterov'):
        return np.abs(np.asarray(s1, dtype=np.float64) * f32(mu))
    return f32(lr) * np.abs(np.asarray(g, dtype=np.float64) + f32(l2c) * np.asarray(p, dtype=np.float64))


def _f64(*arrays):
    return tuple(None if a is None else np.asarray(a, dtype=np.float64) for a in arrays)


def rule_flat(kind, p, s1, s2, g, lr, l2c, mu=HP['mu'], rho=HP['rho'], eps=HP['eps'], din=None):
    """drx_opt_dense (g may be None: pure decay)"""
    p, s1, s2 = _f64(p, s1, s2)
    g = np.zeros_like(p) if g is None else np.asarray(g, dtype=np.float64)
    return apply(kind, p, s1, s2, g, np.abs(g), 1.0, lr, l2c, mu, rho, eps, din=din)


def rule_segments(kind, p, s1, s2, g, start, length, alpha, l2, mu=HP['mu'], rho=HP['rho'], eps=HP['eps']):
    """drx_opt_segments: segment s = elements [start[s], start[s] + length[s]) with its own step size and l2; elements of no segment stay
    as they are (bound 0).  Returns Rule and the mask of the elements that belong to a segment."""
    p, s1, s2, g = _f64(p, s1, s2, g)
    a, l = np.zeros_like(p), np.zeros_like(p)
    inside = np.zeros(p.shape, dtype=bool)
    for s0, n, al, l2c in zip(start, length, alpha, l2):
        assert not inside[s0:s0 + n].any()
        a[s0:s0 + n], l[s0:s0 + n], inside[s0:s0 + n] = al, l2c, True
    r = apply(kind, p, s1, s2, g, np.abs(g), 1.0, a, l, mu, rho, eps)
    keep = lambda new, old: None if new is None else np.where(inside, new, old)
    zero = lambda d: None if d is None else np.where(inside, d, 0.0)
    return Rule(keep(r.p, p), keep(r.s1, s1), keep(r.s2, s2), zero(r.dp), zero(r.ds1), zero(r.ds2)), inside


def rule_rows(kind, p, s1, s2, row_ptr, order, rows, lr, l2c, mu=HP['mu'], rho=HP['rho'], eps=HP['eps'], scalars=None, exact_sums=False):
    """drx_rows_csr_opt / _outer on one table.  rows [T, ld] float64: the gradient row of lookup o (dense_update_oracle.lookup_rows).
    scalars = (p_s, s1_s, s2_s, src_s, lr_s): the per-row scalar channel, no l2.  Returns Rule for the table and for the scalars (or None)."""
    p, s1, s2 = _f64(p, s1, s2)
    rows = np.asarray(rows, dtype=np.float64)
    c = np.diff(row_ptr).astype(np.float64)
    tab = apply(kind, p, s1, s2, du._row_sums(rows, row_ptr, order), du._row_sums(np.abs(rows), row_ptr, order), c[:, None], lr, l2c, mu, rho,
                eps, exact_sums)
    sc = None
    if scalars is not None:
        ps, s1s, s2s, src_s, lr_s = scalars
        ps, s1s, s2s, src_s = _f64(ps, s1s, s2s, src_s)
        sc = apply(kind, ps, s1s, s2s, du._row_sums(src_s, row_ptr, order), du._row_sums(np.abs(src_s), row_ptr, order), c, lr_s, 0.0, mu, rho,
                   eps, exact_sums)
    return tab, sc


def table_slots(kind, t, fresh=False):
    """(s1_0, s2_0, s1s_0, s2s_0) of rule `kind` for a table of dense_update_oracle.make_table, None where the rule has no such slot: the
    signed m0 serves as a momentum accumulator, the positive v0 as Adagrad's / RMSprop's accumulator.  fresh: the slots of a first step
    (zeros; Adagrad: Keras's initial_accumulator_value 0.1)."""
    sc = t['scale'] is not None
    if fresh:
        init = np.float32(0.1 if kind == 'adagrad' else 0.0)
        full = lambda like: None if like is None else np.full_like(like, init)
        m, v, ms, vs = full(t['m0']), full(t['v0']), full(t['ms0']) if sc else None, full(t['vs0']) if sc else None
    else:
        m, v, ms, vs = t['m0'], t['v0'], t['ms0'] if sc else None, t['vs0'] if sc else None
    if kind == 'sgd':
        return None, None, None, None
    if kind in ('momentum', 'nesterov'):
        return m, None, ms, None
    if kind in ('adagrad', 'rmsprop'):
        return v, None, vs, None
    return v, m, vs, ms


def expected_table(kind, t, lr=HP['lr'], lr_s=HP['lr_s'], l2c=HP['l2c'], mu=HP['mu'], rho=HP['rho'], eps=HP['eps'], fresh=False):
    """rule_rows on table t of make_table with table_slots' slots (first_step tables: the sums are exact, dg = 0 — l2c must be 0 then)"""
    assert not (t['first_step'] and l2c)
    s1, s2, s1s, s2s = table_slots(kind, t, fresh)
    sc = (t['ps0'], s1s, s2s, t['scale'][:t['T']], lr_s) if t['scale'] is not None else None
    return rule_rows(kind, t['p0'], s1, s2, t['row_ptr'], t['order'], du.lookup_rows(t), lr, l2c, mu, rho, eps, scalars=sc,
                     exact_sums=t['first_step'])


def flat_slots(kind, m, v):
    """(s1_0, s2_0) for the flat inputs of dense_update_oracle.flat_inputs (p, m, v, g)"""
    return {0: (None, None), 1: (m, None) if kind in ('momentum', 'nesterov') else (v, None), 2: (v, m)}[N_SLOTS[kind]]
