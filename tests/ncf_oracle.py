"""NeuMF (He, Liao, Zhang, Nie, Hu, Chua: "Neural Collaborative Filtering", WWW 2017) as plain NumPy float64: the definition of record of
the model drecpy_amd trains with drx_ncf_step and serves through drx_ncf_half_rows / drx_ncf_score_rows / drx_ncf_pair_scores
(include/drx.h "NeuMF").  No torch, no libdrx: nothing here shares a line with the kernels.

    parameters Pg [n_users, Kg], Pm [n_users, Km], Qg [n_items, Kg], Qm [n_items, Km]; W1 [2 Km, f_1], b1 [f_1], Wl [f_{l-1}, f_l],
               bl [f_l] (l = 2 .. n); hg [Kg], hm [f_n], b0 [1]                       (a dict by these names; n from the names present)
    forward    a_0 = [Pm[u] ; Qm[i]],  z_l = W_l^T a_{l-1} + b_l,  a_l = relu(z_l);  x(u, i) = sum_k hg[k] Pg[u, k] Qg[i, k] + hm . a_n + b0
               relu's derivative at 0 is 0 (A > 0 <=> Z > 0)
    loss       L = (1 / B) sum_b [max(x, 0) - y x + log1p(exp(-|x|))] over B point samples (u, i, y), y in {0, 1}; g_b = (sigmoid(x_b) - y_b) / B
    update     every entry of the four tables, of the W_l, of hg and hm adds reg * itself to its gradient (the b_l and b0 none); then one
               dense rule (tests/optim_oracle.py; Adam: tests/dense_update_oracle.py).  Under Adam the step size of an apply is Keras's
               lr_t of its counter n_applies * step + position + 1 (user table first, then item table, then the small weights:
               positions 0, 1, 2 of 3).
    batches    oracle/data_oracle.py::point_sample_counter (the device point sampler's CPU restatement), seed by seed.
Every forward pass records the smallest |z| over all hidden pre-activations it evaluated in `seen` (reset_seen() clears it): the tests
assert a margin from relu's kink as a condition on their inputs."""
import numpy as np

import bpr_oracle as bo

HP = bo.HP
seen = {'min_abs_z': np.inf}


def reset_seen():
    seen['min_abs_z'] = np.inf


def n_layers(p):
    return sum(1 for k in p if k.startswith('W'))


def names(p):
    """user table halves, item table halves, then the small weights in the order of include/drx.h's flat array"""
    n = n_layers(p)
    return ['Pg', 'Pm', 'Qg', 'Qm'] + [f'{w}{l}' for l in range(1, n + 1) for w in ('W', 'b')] + ['hg', 'hm', 'b0']


def regularised(name):
    return not name.startswith('b')


def position(name):
    """the apply (0: user table, 1: item table, 2: small weights) a parameter belongs to"""
    return 0 if name[0] == 'P' else 1 if name[0] == 'Q' else 2


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e)).astype(x.dtype)


def _hidden(p, z1):
    """(a_n, [z_1 .. z_n], [a_1 .. a_n]) from the first layer's pre-activations [.., f_1]"""
    zs, acts, z = [], [], z1
    for l in range(1, n_layers(p) + 1):
        if l > 1:
            z = acts[-1] @ p[f'W{l}'] + p[f'b{l}']
        zs.append(z)
        acts.append(np.maximum(z, 0))
        if z.size and z.dtype == np.float64:               # (the float32 replay's own pre-activations are not the oracle's)
            seen['min_abs_z'] = min(seen['min_abs_z'], float(np.min(np.abs(z))))
    return acts[-1], zs, acts


def forward(p, uid, iid):
    """(x [B], cache) with the concatenated first layer"""
    uid, iid = np.asarray(uid), np.asarray(iid)
    a0 = np.concatenate([p['Pm'][uid], p['Qm'][iid]], axis=1)
    an, zs, acts = _hidden(p, a0 @ p['W1'] + p['b1'])
    x = (p['Pg'][uid] * p['Qg'][iid]) @ p['hg'] + an @ p['hm'] + p['b0'][0]
    return x, (a0, zs, acts)


def logits(p):
    """x(u, i) for every user and item, [n_users, n_items] (the concatenated first layer)"""
    U, N = len(p['Pg']), len(p['Qg'])
    u, i = np.repeat(np.arange(U), N), np.tile(np.arange(N), U)
    return forward(p, u, i)[0].reshape(U, N)


def half_rows(p):
    """(users [n_users, f_1 + Kg], items [n_items, f_1 + Kg]): what a pair's logit needs from one side alone
    [W_1[:Km]^T Pm[u] + b_1 | hg (.) Pg[u]] and [W_1[Km:]^T Qm[i] | Qg[i]]"""
    Km = p['Pm'].shape[1]
    return (np.concatenate([p['Pm'] @ p['W1'][:Km] + p['b1'], p['hg'] * p['Pg']], axis=1),
            np.concatenate([p['Qm'] @ p['W1'][Km:], p['Qg']], axis=1))


def logits_split(p):
    """logits() with the first layer split into its user half and its item half (the scorer's form)"""
    hu, hi = half_rows(p)
    f1 = p['W1'].shape[1]
    an, _, _ = _hidden(p, hu[:, None, :f1] + hi[None, :, :f1])
    return an @ p['hm'] + hu[:, f1:] @ hi[:, f1:].T + p['b0'][0]


def bce(x, y):
    return np.maximum(x, 0) - y * x + np.log1p(np.exp(-np.abs(x)))


def loss(p, uid, iid, y):
    return float(np.mean(bce(forward(p, uid, iid)[0], np.asarray(y, p['Pg'].dtype))))


def gradients(p, uid, iid, y):
    """(loss, {name: gradient}): the data gradients of the batch (no regularisation)"""
    uid, iid = np.asarray(uid), np.asarray(iid)
    dt = p['Pg'].dtype
    y = np.asarray(y, dt)
    B, Km, n = len(uid), p['Pm'].shape[1], n_layers(p)
    x, (a0, zs, acts) = forward(p, uid, iid)
    g = ((sigmoid(x) - y) / dt.type(B)).astype(dt)
    grads = {k: np.zeros_like(v) for k, v in p.items()}
    pg, qg = p['Pg'][uid], p['Qg'][iid]
    grads['hg'] = (g[:, None] * (pg * qg)).sum(axis=0)
    grads['hm'] = (g[:, None] * acts[-1]).sum(axis=0)
    grads['b0'] = np.array([g.sum()], dt)
    np.add.at(grads['Pg'], uid, (g[:, None] * p['hg']) * qg)
    np.add.at(grads['Qg'], iid, (g[:, None] * p['hg']) * pg)
    da = g[:, None] * p['hm'][None, :]
    for l in range(n, 0, -1):
        dz = np.where(zs[l - 1] > 0, da, 0).astype(dt)
        grads[f'W{l}'] = (a0 if l == 1 else acts[l - 2]).T @ dz
        grads[f'b{l}'] = dz.sum(axis=0)
        da = dz @ p[f'W{l}'].T
    np.add.at(grads['Pm'], uid, da[:, :Km])
    np.add.at(grads['Qm'], iid, da[:, Km:])
    return float(np.mean(bce(x, y))), grads


def init_state(p, kind):
    """{name: [s1, s2]} of rule `kind`, as tests/bpr_oracle.py::init_state"""
    n = 2 if kind == 'adam' else bo.oo.N_SLOTS[kind]
    init = 0.1 if kind == 'adagrad' else 0.0
    return {name: [np.full_like(p[name], init) if s < n else None for s in range(2)] for name in names(p)}


def step_sizes(step_idx, kind='adam', hp=HP, applies=(3, 0, 1, 2)):
    """(alpha of the user table, of the item table, of the small weights)"""
    n, positions = applies[0], applies[1:]
    if kind != 'adam':
        return (hp['lr'],) * 3
    return tuple(bo.adam_alpha(hp['lr'], n * step_idx + j + 1, hp['b1'], hp['b2']) for j in positions)


def step(p, state, step_idx, uid, iid, y, kind='adam', hp=HP, applies=(3, 0, 1, 2)):
    """One training step in place on p and state; returns the loss of the batch before the update.  (On float32 arrays — the replay —
    the gradients are formed in float32 and every stored value is rounded to float32.)"""
    L, g = gradients(p, uid, iid, y)
    alphas = step_sizes(step_idx, kind, hp, applies)
    for name in names(p):
        new = bo.apply_rule(kind, p[name], state[name][0], state[name][1], g[name], alphas[position(name)],
                            hp['reg'] if regularised(name) else 0.0, hp)
        p[name], state[name][0], state[name][1] = (a if a is None else np.asarray(a).astype(p[name].dtype) for a in new)
    return L


def fit(p, frame, n_steps, B, neg_ratio, draw_seed, kind='adam', hp=HP):
    """n_steps steps in place on the draws of point_sample_counter: frame = (pos_indptr, pos_indices, rec_indptr or None, rec_indices
    or None, n_users, n_items); draw_seed(k) = the seed of batch k = 1, 2, ...  Returns the losses."""
    from oracle.data_oracle import point_sample_counter
    st, out = init_state(p, kind), []
    for s in range(n_steps):
        uid, iid, y, _, exhausted = point_sample_counter(*frame, B, neg_ratio, draw_seed(s + 1) & bo.M64)
        assert not exhausted.any()
        out.append(step(p, st, s, uid, iid, y, kind, hp))
    return out


def init_params(rng, n_users, n_items, Kg, Km, layers, bias_scale=0.2):
    """the tests' weights, rounded to fp32 (what the device holds), as float64: tables and kernels uniform(-0.5, 0.5) / sqrt(fan-in), h
    uniform(-0.5, 0.5); the biases uniform(-bias_scale, bias_scale) so that no pre-activation is exactly 0"""
    f = lambda scale, *shape: (rng.uniform(-0.5, 0.5, size=shape) * scale).astype(np.float32).astype(np.float64)
    p = {'Pg': f(Kg ** -0.5, n_users, Kg), 'Pm': f(Km ** -0.5, n_users, Km), 'Qg': f(Kg ** -0.5, n_items, Kg), 'Qm': f(Km ** -0.5, n_items, Km)}
    fin = 2 * Km
    for l, fo in enumerate(layers, 1):
        p[f'W{l}'], p[f'b{l}'] = f(2.0 * fin ** -0.5, fin, fo), f(2 * bias_scale, fo)
        fin = fo
    p['hg'], p['hm'], p['b0'] = f(1.0, Kg), f(1.0, fin), f(2 * bias_scale, 1)
    return p


def replay32(p):
    """the parameters as float32 arrays: the same functions then run in float32 — the oracle's own float32 replay"""
    return {k: np.asarray(v, np.float32) for k, v in p.items()}
