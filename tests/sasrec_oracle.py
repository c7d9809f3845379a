"""SASRec (Kang & McAuley, ICDM 2018) as plain NumPy float64: the definition of record of the model drecpy_amd trains with drx_sas_step
and serves through drx_sas_query_rows (include/drx.h "SASRec").  No torch, no libdrx: nothing here shares a line with the kernels.

    parameters E [n_items, H] input embeddings; Pos [L, H] learned positions; per block b = 0 .. blocks - 1 the names Wq{b}, Wk{b}, Wv{b},
               W1{b}, W2{b} [H, H], b1{b}, b2{b}, ln1_g{b}, ln1_b{b}, ln2_g{b}, ln2_b{b} [H]; lnf_g, lnf_b [H]; Q [n_items, H], b [n_items].
               No user table.
    window     (the ordered L items S before the target, target i, negatives j_1 .. j_r): before [B, L], after [B, 1 + r] (the target
               first) — the layout of oracle/data_oracle.py::list_sample_counter at n_targets = 1 (its uid plays no part)
    positions  a sequence of m <= L items occupies positions L - m .. L - 1: the newest item is at L - 1.  Ids are given LEFT-aligned with
               -1 = absent (serving's baskets; a training window is full) and shifted here.  Absent positions are never keys and are
               not computed as queries.
    forward    X0_t = E[s_t] + Pos[t];  per block: A = LN(X; ln1), q, k, v = A Wq, A Wk, A Wv, S_tj = q_t . k_j / sqrt(H) for present
               j <= t, P = softmax_j(S), X' = X + P v, F = LN(X'; ln2), X'' = X' + relu(F W1 + b1) W2 + b2;  h = LN(X_{L-1}; lnf);
               LN(x) = (x - mean) / sqrt(var + 1e-5) g + beta, the biased variance over the H columns.  An empty basket: h = 0.
    score      x(S, i) = h . Q[i] + b[i]
    loss       (1 / (B r)) sum_w sum_k softplus(-D_wk),  D_wk = x(S, i) - x(S, j_k);  g_wk = -sigmoid(-D_wk) / (B r)
    update     every row of E and Q, every entry of Pos and of the five matrices of every block adds reg * itself to its gradient (the
               biases, LN gains and offsets and b none); then one dense rule (tests/optim_oracle.py; Adam: tests/dense_update_oracle.py).
               Under Adam the step size of an apply is Keras's lr_t of its counter n_applies * step + position + 1 (E registered first,
               then the small weights, then Q with b: positions 0, 1, 2 of 3)."""
import numpy as np

import bpr_oracle as bo
import fpmc_oracle as fo

MATRICES = ('Wq', 'Wk', 'Wv', 'W1', 'W2')
VECTORS = ('b1', 'b2', 'ln1_g', 'ln1_b', 'ln2_g', 'ln2_b')
EPS = 1e-5
HP = bo.HP
softplus = bo.softplus
replay32 = fo.replay32
twin_of = fo.twin_of
baskets_of = fo.baskets_of


def n_blocks(p):
    return sum(1 for k in p if k.startswith('Wq'))


def small_names(blocks):
    """the small weights in the order of the flat array: the regularised ones, then the others"""
    return (['Pos'] + [f'{m}{b}' for b in range(blocks) for m in MATRICES] + [f'{v}{b}' for b in range(blocks) for v in VECTORS]
            + ['lnf_g', 'lnf_b'])


def names(blocks):
    return ['E'] + small_names(blocks) + ['Q', 'b']


def regularised(name):
    return name in ('E', 'Q', 'Pos') or name[:2] in MATRICES


def _ln(x, g, beta):
    mean = x.mean(axis=-1, keepdims=True)
    xc = x - mean
    rstd = 1.0 / np.sqrt((xc * xc).mean(axis=-1, keepdims=True) + EPS)
    xhat = (xc * rstd).astype(x.dtype)
    return (xhat * g + beta).astype(x.dtype), xhat, rstd.astype(x.dtype)


def _ln_back(dy, xhat, rstd, g):
    """(dx, dg, dbeta) of y = xhat g + beta, the sums of dg and dbeta over every leading axis"""
    dxh = dy * g
    dx = rstd * (dxh - dxh.mean(axis=-1, keepdims=True) - xhat * (dxh * xhat).mean(axis=-1, keepdims=True))
    lead = tuple(range(dy.ndim - 1))
    return dx.astype(dy.dtype), (dy * xhat).sum(axis=lead), dy.sum(axis=lead)


def shift(ids):
    """left-aligned ids [B, L] with -1 = absent -> right-aligned: the m present ids of a row at columns L - m .. L - 1"""
    ids = np.asarray(ids)
    out = np.full_like(ids, -1)
    for w, row in enumerate(ids):
        row = row[row >= 0]
        if len(row):
            out[w, ids.shape[1] - len(row):] = row
    return out


def forward(p, ids):
    """(h [B, H], what the backward pass needs) for left-aligned ids [B, L], an id < 0 = absent"""
    pos = shift(ids)
    B, L = pos.shape
    H = p['Pos'].shape[1]
    dt = p['E'].dtype
    on = pos >= 0
    x = np.where(on[:, :, None], p['E'][np.maximum(pos, 0)] + p['Pos'][None, :, :], 0).astype(dt)
    mask = on[:, :, None] & on[:, None, :] & np.tril(np.ones((L, L), bool))[None]
    inv = float(H) ** -0.5
    tape = []
    for b in range(n_blocks(p)):
        a, xh1, rs1 = _ln(x, p[f'ln1_g{b}'], p[f'ln1_b{b}'])
        q, k, v = a @ p[f'Wq{b}'], a @ p[f'Wk{b}'], a @ p[f'Wv{b}']
        s = np.where(mask, np.einsum('bth,bjh->btj', q, k) * inv, -np.inf)
        top = np.where(mask.any(axis=2, keepdims=True), s.max(axis=2, keepdims=True), 0)
        e = np.where(mask, np.exp(np.where(mask, s - top, 0)), 0)
        den = e.sum(axis=2, keepdims=True)
        P = (e / np.where(den > 0, den, 1)).astype(dt)
        x1 = (x + np.einsum('btj,bjh->bth', P, v)).astype(dt)
        f, xh2, rs2 = _ln(x1, p[f'ln2_g{b}'], p[f'ln2_b{b}'])
        r = np.maximum(f @ p[f'W1{b}'] + p[f'b1{b}'], 0)
        x2 = np.where(on[:, :, None], x1 + r @ p[f'W2{b}'] + p[f'b2{b}'], 0).astype(dt)
        tape.append(dict(x=x, a=a, xh1=xh1, rs1=rs1, q=q, k=k, v=v, P=P, x1=x1, f=f, xh2=xh2, rs2=rs2, r=r))
        x = x2
    last, xhf, rsf = _ln(x[:, L - 1], p['lnf_g'], p['lnf_b'])
    h = np.where(on[:, L - 1:L], last, 0).astype(dt)
    return h, dict(pos=pos, on=on, blocks=tape, x=x, xhf=xhf, rsf=rsf, inv=inv)


def query_rows(p, baskets, uids=None):
    """h of the basket of every user named, [n, H]; baskets [n_users, L] left-aligned, -1 = absent"""
    baskets = np.asarray(baskets)
    uids = np.arange(len(baskets)) if uids is None else np.asarray(uids)
    return forward(p, baskets[uids])[0]


def scores(p, baskets):
    """x(basket of u, i) for every user and item, [n_users, n_items]"""
    return query_rows(p, baskets) @ p['Q'].T + p['b'][None, :]


def deltas(p, before, after):
    """D_wk, [B, r]"""
    after = np.asarray(after)
    x = np.einsum('wh,wjh->wj', forward(p, before)[0], p['Q'][after]) + p['b'][after]
    return x[:, :1] - x[:, 1:]


def loss(p, before, after):
    return float(np.mean(softplus(-deltas(p, before, after))))


def gradients(p, before, after):
    """(loss, {name: gradient}, h): the data gradients of the batch (no regularisation), the backward pass by hand"""
    before, after = np.asarray(before), np.asarray(after)
    B, L = before.shape
    r_ = after.shape[1] - 1
    dt = p['E'].dtype
    h, T = forward(p, before)
    on = T['on']
    i, j = after[:, 0], after[:, 1:]
    x = np.einsum('wh,wjh->wj', h, p['Q'][after]) + p['b'][after]
    d = x[:, :1] - x[:, 1:]
    g = -(1.0 / (1.0 + np.exp(d))) / (B * r_)              # -sigmoid(-d) / (B r), [B, r]
    grads = {n: np.zeros_like(p[n]) for n in names(len(T['blocks']))}
    gsum = g.sum(axis=1)
    np.add.at(grads['Q'], i, gsum[:, None] * h)
    np.add.at(grads['b'], i, gsum)
    for k in range(r_):
        np.add.at(grads['Q'], j[:, k], -g[:, k, None] * h)
        np.add.at(grads['b'], j[:, k], -g[:, k])
    dh = np.einsum('wk,wkh->wh', g, p['Q'][i][:, None, :] - p['Q'][j])
    dh = np.where(on[:, L - 1:L], dh, 0).astype(dt)
    dlast, grads['lnf_g'], grads['lnf_b'] = _ln_back(dh, T['xhf'], T['rsf'], p['lnf_g'])
    dx = np.zeros_like(T['x'])
    dx[:, L - 1] = dlast
    for b in range(len(T['blocks']) - 1, -1, -1):
        t = T['blocks'][b]
        dx = np.where(on[:, :, None], dx, 0).astype(dt)
        grads[f'W2{b}'] = np.einsum('bth,btc->hc', t['r'], dx)
        grads[f'b2{b}'] = dx.sum(axis=(0, 1))
        du = ((dx @ p[f'W2{b}'].T) * (t['r'] > 0)).astype(dt)
        grads[f'W1{b}'] = np.einsum('bth,btc->hc', t['f'], du)
        grads[f'b1{b}'] = du.sum(axis=(0, 1))
        df, grads[f'ln2_g{b}'], grads[f'ln2_b{b}'] = _ln_back(du @ p[f'W1{b}'].T, t['xh2'], t['rs2'], p[f'ln2_g{b}'])
        dx1 = (dx + df).astype(dt)
        dP = np.einsum('bth,bjh->btj', dx1, t['v'])
        dv = np.einsum('btj,bth->bjh', t['P'], dx1)
        ds = (t['P'] * (dP - (t['P'] * dP).sum(axis=2, keepdims=True)) * T['inv']).astype(dt)
        dq = np.einsum('btj,bjh->bth', ds, t['k'])
        dk = np.einsum('btj,bth->bjh', ds, t['q'])
        for m, dm in (('Wq', dq), ('Wk', dk), ('Wv', dv)):
            grads[f'{m}{b}'] = np.einsum('bth,btc->hc', t['a'], dm)
        da = dq @ p[f'Wq{b}'].T + dk @ p[f'Wk{b}'].T + dv @ p[f'Wv{b}'].T
        dxa, grads[f'ln1_g{b}'], grads[f'ln1_b{b}'] = _ln_back(da.astype(dt), t['xh1'], t['rs1'], p[f'ln1_g{b}'])
        dx = (dx1 + dxa).astype(dt)
    dx = np.where(on[:, :, None], dx, 0).astype(dt)
    grads['Pos'] = dx.sum(axis=0)
    np.add.at(grads['E'], T['pos'][on], dx[on])
    return float(np.mean(softplus(-d))), {k: v.astype(dt) for k, v in grads.items()}, h


def init_state(p, kind):
    """{name: [s1, s2]} of rule `kind`, as tests/bpr_oracle.py::init_state"""
    n = 2 if kind == 'adam' else bo.oo.N_SLOTS[kind]
    init = 0.1 if kind == 'adagrad' else 0.0
    return {name: [np.full_like(p[name], init) if s < n else None for s in range(2)] for name in p}


def step_sizes(p, step_idx, kind='adam', hp=HP, applies=(3, 0, 1, 2)):
    """{name: step size} of a step: E, the small weights, Q with b"""
    n, je, js, ji = applies
    if kind == 'adam':
        a_e, a_s, a_i = (bo.adam_alpha(hp['lr'], n * step_idx + j + 1, hp['b1'], hp['b2']) for j in (je, js, ji))
    else:
        a_e = a_s = a_i = hp['lr']
    return {name: a_e if name == 'E' else a_i if name in ('Q', 'b') else a_s for name in p}


def l2_of(name, hp=HP):
    return hp['reg'] if regularised(name) else 0.0


def apply_gradients(p, state, step_idx, g, kind='adam', hp=HP, applies=(3, 0, 1, 2)):
    alphas = step_sizes(p, step_idx, kind, hp, applies)
    for name in list(p):
        new = bo.apply_rule(kind, p[name], state[name][0], state[name][1], g[name], alphas[name], l2_of(name, hp), hp)
        # (the float32 replay: the gradients were formed in float32; the rule's results are rounded to float32 as they are stored)
        p[name], state[name][0], state[name][1] = (a if a is None else a.astype(p[name].dtype) for a in new)


def step(p, state, step_idx, uid, before, after, kind='adam', hp=HP, applies=(3, 0, 1, 2)):
    """One training step in place on p (float64 arrays) and state; returns the loss of the batch before the update.  uid is the
    sampler's and plays no part.  applies = (n, j_input, j_small, j_item)."""
    L, g, _ = gradients(p, before, after)
    apply_gradients(p, state, step_idx, g, kind, hp, applies)
    return L


def windows(twin, B, L, r, seed):
    """(uid [B], before [B, L], after [B, 1 + r]) of draw `seed`: the list sampler's counter-based stream at n_targets = 1"""
    from oracle.data_oracle import list_sample_counter
    return list_sample_counter(twin, B, L, 1, r, seed)


def init_params(rng, n_items, H, L, blocks):
    """the tests' weights: uniform(-0.5, 0.5) / sqrt(width) (a bias: width 1); LN gains 1 + uniform(-0.5, 0.5), offsets
    uniform(-0.5, 0.5): the softmax is not flat and the LN gradients are exercised.  Rounded to fp32 (what the device holds), as float64"""
    f = lambda width, *shape: (rng.uniform(-0.5, 0.5, size=shape) / np.sqrt(width)).astype(np.float32).astype(np.float64)
    gain = lambda: (1.0 + rng.uniform(-0.5, 0.5, size=H)).astype(np.float32).astype(np.float64)
    p = {'E': f(H, n_items, H), 'Pos': f(H, L, H)}
    for b in range(blocks):
        for m in MATRICES:
            p[f'{m}{b}'] = f(H, H, H)
    for b in range(blocks):
        p.update({f'b1{b}': f(1, H), f'b2{b}': f(1, H), f'ln1_g{b}': gain(), f'ln1_b{b}': f(1, H), f'ln2_g{b}': gain(), f'ln2_b{b}': f(1, H)})
    p.update({'lnf_g': gain(), 'lnf_b': f(1, H), 'Q': f(H, n_items, H), 'b': f(H, n_items)})
    return p
