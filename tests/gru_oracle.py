"""GRU4Rec (Hidasi, Karatzoglou, Baltrunas, Tikk 2016) as plain NumPy float64: the definition of record of the model drecpy_amd trains
with drx_gru_step and serves through drx_gru_query_rows (include/drx.h "GRU4Rec").  No torch, no libdrx: nothing here shares a line with
the kernels.

    parameters E [n_items, K] input embeddings; Wx [K, 3 H], Wh [H, 3 H], bx [3 H], bhn [H]: the gates, columns z | r | n;
               Q [n_items, H], b [n_items].  No user table: the sequence is the session.
    window     (the ordered L items S before the target, target i, negatives j_1 .. j_r): before [B, L], after [B, 1 + r] (the target
               first) — the layout of oracle/data_oracle.py::list_sample_counter at n_targets = 1 (its uid plays no part)
    cell       h_0 = 0, x_t = E[s_t];  z_t = sigmoid(x_t Wx_z + h_{t-1} Wh_z + bx_z);  r_t = sigmoid(x_t Wx_r + h_{t-1} Wh_r + bx_r);
               n_t = tanh(x_t Wx_n + bx_n + r_t (.) (h_{t-1} Wh_n + bhn));  h_t = (1 - z_t) (.) n_t + z_t (.) h_{t-1}
               (torch's GRU cell; an id < 0 is no step: the row keeps its h)
    score      x(S, i) = h_L . Q[i] + b[i]
    loss       (1 / (B r)) sum_w sum_k softplus(-D_wk),  D_wk = x(S, i) - x(S, j_k);  g_wk = -sigmoid(-D_wk) / (B r)
    update     every row of E and Q and every entry of Wx, Wh adds reg * itself to its gradient (bx, bhn, b none); then one dense rule
               (tests/optim_oracle.py; Adam: tests/dense_update_oracle.py).  Under Adam the step size of an apply is Keras's lr_t of its
               counter n_applies * step + position + 1 (E registered first, then the small weights, then Q with b: positions 0, 1, 2
               of 3).
    serving    the basket of a user: up to L item ids, left-aligned, -1 = absent; the cell runs over the ids present, an empty basket
               gives h = 0 and the score b[i]."""
import numpy as np

import bpr_oracle as bo
import fpmc_oracle as fo

NAMES = ('E', 'Wx', 'Wh', 'bx', 'bhn', 'Q', 'b')
SMALL = ('Wx', 'Wh', 'bx', 'bhn')
HP = bo.HP
softplus = bo.softplus
replay32 = fo.replay32
twin_of = fo.twin_of
baskets_of = fo.baskets_of


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def run_cell(p, ids):
    """(h after the last step [B, H], what the backward pass needs per step) for ids [B, L], an id < 0 = no step"""
    ids = np.asarray(ids)
    B, L = ids.shape
    H = p['Wh'].shape[0]
    h = np.zeros((B, H), dtype=p['E'].dtype)
    steps = []
    for t in range(L):
        on = ids[:, t] >= 0
        x = np.where(on[:, None], p['E'][np.maximum(ids[:, t], 0)], 0).astype(p['E'].dtype)
        px = x @ p['Wx'] + p['bx']
        ph = h @ p['Wh']
        z = _sigmoid(px[:, :H] + ph[:, :H])
        r = _sigmoid(px[:, H:2 * H] + ph[:, H:2 * H])
        hn = ph[:, 2 * H:] + p['bhn']
        n = np.tanh(px[:, 2 * H:] + r * hn)
        new = np.where(on[:, None], (1.0 - z) * n + z * h, h).astype(h.dtype)
        steps.append((x, h, z, r, n, hn, on))
        h = new
    return h, steps


def hidden(p, ids):
    return run_cell(p, ids)[0]


def deltas(p, before, after):
    """D_wk, [B, r]"""
    after = np.asarray(after)
    x = np.einsum('wh,wjh->wj', hidden(p, before), p['Q'][after]) + p['b'][after]
    return x[:, :1] - x[:, 1:]


def loss(p, before, after):
    return float(np.mean(softplus(-deltas(p, before, after))))


def gradients(p, before, after):
    """(loss, {name: gradient}): the data gradients of the batch (no regularisation), backward through time by hand"""
    before, after = np.asarray(before), np.asarray(after)
    B, L = before.shape
    r_ = after.shape[1] - 1
    H = p['Wh'].shape[0]
    h, steps = run_cell(p, before)
    i, j = after[:, 0], after[:, 1:]
    x = np.einsum('wh,wjh->wj', h, p['Q'][after]) + p['b'][after]
    d = x[:, :1] - x[:, 1:]
    g = -(1.0 / (1.0 + np.exp(d))) / (B * r_)              # -sigmoid(-d) / (B r), [B, r]
    grads = {n: np.zeros_like(p[n]) for n in NAMES}
    gsum = g.sum(axis=1)
    np.add.at(grads['Q'], i, gsum[:, None] * h)
    np.add.at(grads['b'], i, gsum)
    for k in range(r_):
        np.add.at(grads['Q'], j[:, k], -g[:, k, None] * h)
        np.add.at(grads['b'], j[:, k], -g[:, k])
    dh = np.einsum('wk,wkh->wh', g, p['Q'][i][:, None, :] - p['Q'][j])
    for t in range(L - 1, -1, -1):
        x_t, hp, z, r, n, hn, on = steps[t]
        m = on[:, None]
        da_n = np.where(m, dh * (1.0 - z) * (1.0 - n * n), 0)
        da_z = np.where(m, dh * (hp - n) * z * (1.0 - z), 0)
        da_r = da_n * hn * r * (1.0 - r)
        dgx = np.concatenate([da_z, da_r, da_n], axis=1).astype(h.dtype)
        dgh = np.concatenate([da_z, da_r, da_n * r], axis=1).astype(h.dtype)
        grads['Wx'] += x_t.T @ dgx
        grads['Wh'] += hp.T @ dgh
        grads['bx'] += dgx.sum(axis=0)
        grads['bhn'] += dgh[:, 2 * H:].sum(axis=0)
        np.add.at(grads['E'], before[on, t], (dgx @ p['Wx'].T)[on])
        dh = np.where(m, dh * z + dgh @ p['Wh'].T, dh).astype(h.dtype)
    return float(np.mean(softplus(-d))), grads


def init_state(p, kind):
    """{name: [s1, s2]} of rule `kind`, as tests/bpr_oracle.py::init_state"""
    n = 2 if kind == 'adam' else bo.oo.N_SLOTS[kind]
    init = 0.1 if kind == 'adagrad' else 0.0
    return {name: [np.full_like(p[name], init) if s < n else None for s in range(2)] for name in NAMES}


def step_sizes(step_idx, kind='adam', hp=HP, applies=(3, 0, 1, 2)):
    """{name: step size} of a step: E, the small weights, Q with b"""
    n, je, js, ji = applies
    if kind == 'adam':
        a_e, a_s, a_i = (bo.adam_alpha(hp['lr'], n * step_idx + j + 1, hp['b1'], hp['b2']) for j in (je, js, ji))
    else:
        a_e = a_s = a_i = hp['lr']
    return {'E': a_e, 'Wx': a_s, 'Wh': a_s, 'bx': a_s, 'bhn': a_s, 'Q': a_i, 'b': a_i}


def l2_of(name, hp=HP):
    return hp['reg'] if name in ('E', 'Wx', 'Wh', 'Q') else 0.0


def apply_gradients(p, state, step_idx, g, kind='adam', hp=HP, applies=(3, 0, 1, 2)):
    alphas = step_sizes(step_idx, kind, hp, applies)
    for name in NAMES:
        new = bo.apply_rule(kind, p[name], state[name][0], state[name][1], g[name], alphas[name], l2_of(name, hp), hp)
        # (the float32 replay: the gradients were formed in float32; the rule's results are rounded to float32 as they are stored)
        p[name], state[name][0], state[name][1] = (a if a is None else a.astype(p[name].dtype) for a in new)


def step(p, state, step_idx, uid, before, after, kind='adam', hp=HP, applies=(3, 0, 1, 2)):
    """One training step in place on p (float64 arrays) and state; returns the loss of the batch before the update.  uid is the
    sampler's and plays no part.  applies = (n, j_input, j_small, j_item)."""
    L, g = gradients(p, before, after)
    apply_gradients(p, state, step_idx, g, kind, hp, applies)
    return L


def query_rows(p, baskets, uids=None):
    """h after the cell has run over the basket's ids present, per user, [n, H]; baskets [n_users, L], -1 = absent"""
    baskets = np.asarray(baskets)
    uids = np.arange(len(baskets)) if uids is None else np.asarray(uids)
    return hidden(p, baskets[uids])


def scores(p, baskets):
    """x(basket of u, i) for every user and item, [n_users, n_items]"""
    return query_rows(p, baskets) @ p['Q'].T + p['b'][None, :]


def windows(twin, B, L, r, seed):
    """(uid [B], before [B, L], after [B, 1 + r]) of draw `seed`: the list sampler's counter-based stream at n_targets = 1"""
    from oracle.data_oracle import list_sample_counter
    return list_sample_counter(twin, B, L, 1, r, seed)


def init_params(rng, n_items, K, H):
    """the tests' weights: uniform(-0.5, 0.5) / sqrt(width) (a bias: width 1), rounded to fp32 (what the device holds), as float64"""
    f = lambda width, *shape: (rng.uniform(-0.5, 0.5, size=shape) / np.sqrt(width)).astype(np.float32).astype(np.float64)
    return {'E': f(K, n_items, K), 'Wx': f(K, K, 3 * H), 'Wh': f(H, H, 3 * H), 'bx': f(1, 3 * H), 'bhn': f(1, H), 'Q': f(H, n_items, H),
            'b': f(H, n_items)}
