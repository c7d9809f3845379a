"""LightGCN (He, Deng, Wang, Li, Zhang, Wang, SIGIR 2020) as plain NumPy float64: the definition of record of the model drecpy_amd trains
with drx_lgcn_step and serves through drx_lgcn_final (include/drx.h "LightGCN").  No torch, no libdrx: nothing here shares a line with
the kernels.  The adjacency is a DENSE [N, N] matrix: this is for test sizes.

    parameters P [n_users, K], Q [n_items, K];  E0 = [P ; Q]: the N = n_users + n_items nodes are the users, then the items
    graph      rows: one ascending list of positive item ids per user (duplicates merged).  d_v = degree of node v, w_v = d_v^(-1/2),
               0 where d_v = 0;  A[r, c] = w_r w_c on every edge (u, n_users + i), both ways: A is symmetric
    final      Ebar = (1 / (layers + 1)) sum_{l = 0 .. layers} A^l E0          (a node without edges keeps E0 / (layers + 1))
    score      x(u, i) = Ebar[u] . Ebar[n_users + i]
    loss       L = (1 / T) sum_t softplus(-D_t),  D_t = x(u, i) - x(u, j);  g_t = -sigmoid(-D_t) / T
    gradients  G = dL / dEbar: G[u] += g_t (Ebar[i'] - Ebar[j']), G[i'] += g_t Ebar[u], G[j'] -= g_t Ebar[u];
               dE0 = (1 / (layers + 1)) sum_l A^l G          (A symmetric)
    update     every row of P and Q adds reg * row to its gradient — dense, not the paper's batch rows only —; then one dense rule
               (tests/optim_oracle.py; Adam: tests/dense_update_oracle.py).  Under Adam the step size of an apply is Keras's lr_t of its
               counter n_applies * step + position + 1 (P registered first, then Q: positions 0 and 1 of 2).
    batch      tests/bpr_oracle.py's sample() on the same frame

horner() is the recurrence the device runs (S <- X, `layers` times S <- X + A S, then / (layers + 1)); final() and backward() state the
model in the sum form.  replay32: the same functions on float32 arrays."""
import numpy as np

import bpr_oracle as bo
import fpmc_oracle as fo

HP = bo.HP
NAMES = ('P', 'Q')
replay32 = fo.replay32
softplus = bo.softplus


def degree_weights(rows, n_items):
    """w [N] float64"""
    n_users = len(rows)
    deg = np.zeros(n_users + n_items)
    for u, row in enumerate(rows):
        row = sorted(set(int(i) for i in row))
        deg[u] = len(row)
        for i in row:
            deg[n_users + i] += 1
    w = np.zeros_like(deg)
    w[deg > 0] = 1.0 / np.sqrt(deg[deg > 0])
    return w


def adjacency(rows, n_items, dtype=np.float64):
    """the dense normalised adjacency [N, N]"""
    n_users = len(rows)
    w = degree_weights(rows, n_items)
    A = np.zeros((n_users + n_items,) * 2)
    for u, row in enumerate(rows):
        for i in set(int(i) for i in row):
            A[u, n_users + i] = A[n_users + i, u] = w[u] * w[n_users + i]
    return A.astype(dtype)


def power_mean(A, X, layers):
    """(1 / (layers + 1)) sum_{l = 0 .. layers} A^l X, term by term"""
    dt = X.dtype.type
    total, term = X.copy(), X
    for _ in range(layers):
        term = A @ term
        total = total + term
    return total / dt(layers + 1)


def horner(A, X, layers):
    """the same by the recurrence S <- X + A S"""
    dt = X.dtype.type
    S = X
    for _ in range(layers):
        S = X + A @ S
    return S / dt(layers + 1)


def final(p, A, layers):
    """Ebar [N, K]"""
    return power_mean(A.astype(p['P'].dtype), np.concatenate([p['P'], p['Q']]), layers)


def scores(p, A, layers):
    """x(u, i) for all pairs [n_users, n_items]"""
    E, nu = final(p, A, layers), len(p['P'])
    return E[:nu] @ E[nu:].T


def differences(E, nu, uid, pos, neg):
    return np.einsum('tk,tk->t', E[uid], E[nu + pos] - E[nu + neg])


def loss(p, A, layers, uid, pos, neg):
    return float(np.mean(softplus(-differences(final(p, A, layers), len(p['P']), uid, pos, neg))))


def embedding_gradient(E, nu, uid, pos, neg):
    """(loss, G = dL / dEbar [N, K])"""
    dt = E.dtype.type
    d = differences(E, nu, uid, pos, neg)
    g = (-(dt(1) / (dt(1) + np.exp(d))) / dt(len(uid))).astype(E.dtype)                   # -sigmoid(-d) / T
    G = np.zeros_like(E)
    np.add.at(G, uid, g[:, None] * (E[nu + pos] - E[nu + neg]))
    np.add.at(G, nu + pos, g[:, None] * E[uid])
    np.add.at(G, nu + neg, -g[:, None] * E[uid])
    return float(np.mean(softplus(-d))), G


def backward(A, G, layers):
    """dE0 from G: A is symmetric, so it is the forward form on G"""
    return power_mean(A, G, layers)


def gradients(p, A, layers, uid, pos, neg):
    """(loss, {'P', 'Q'}): the data gradients of the batch (no regularisation)"""
    A = A.astype(p['P'].dtype)
    nu = len(p['P'])
    L, G = embedding_gradient(final(p, A, layers), nu, np.asarray(uid), np.asarray(pos), np.asarray(neg))
    d = backward(A, G, layers)
    return L, {'P': d[:nu], 'Q': d[nu:]}


def init_state(p, kind):
    """{name: [s1, s2]} of rule `kind`, as tests/bpr_oracle.py::init_state"""
    n = 2 if kind == 'adam' else bo.oo.N_SLOTS[kind]
    init = 0.1 if kind == 'adagrad' else 0.0
    return {name: [np.full_like(p[name], init) if s < n else None for s in range(2)] for name in NAMES}


def step_sizes(step_idx, kind='adam', hp=HP, applies=(2, 0, 1)):
    n, ju, ji = applies
    if kind == 'adam':
        return {'P': bo.adam_alpha(hp['lr'], n * step_idx + ju + 1, hp['b1'], hp['b2']),
                'Q': bo.adam_alpha(hp['lr'], n * step_idx + ji + 1, hp['b1'], hp['b2'])}
    return {'P': hp['lr'], 'Q': hp['lr']}


def step(p, state, A, layers, step_idx, uid, pos, neg, kind='adam', hp=HP, applies=(2, 0, 1)):
    """One training step in place on p and state (float64, or float32 for the replay); returns the loss of the batch before the update."""
    L, g = gradients(p, A, layers, uid, pos, neg)
    alphas = step_sizes(step_idx, kind, hp, applies)
    for name in NAMES:
        new = bo.apply_rule(kind, p[name], state[name][0], state[name][1], g[name], alphas[name], hp['reg'], hp)
        p[name], state[name][0], state[name][1] = (a if a is None else a.astype(p[name].dtype) for a in new)
    return L


def init_params(rng, n_users, n_items, K):
    """the tests' weights: uniform(-0.5, 0.5) / sqrt(K) TIMES 4 — the propagation averages, and scores of O(0.1 - 1) keep the loss away
    from log 2 —, rounded to fp32 (what the device holds), as float64"""
    f = lambda *shape: (4.0 * rng.uniform(-0.5, 0.5, size=shape) / np.sqrt(K)).astype(np.float32).astype(np.float64)
    return {'P': f(n_users, K), 'Q': f(n_items, K)}
