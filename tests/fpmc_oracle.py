"""FPMC (Rendle, Freudenthaler, Schmidt-Thieme 2010) as plain NumPy float64: the definition of record of the model drecpy_amd trains with
drx_fpmc_step and serves through drx_fpmc_query_rows (include/drx.h "FPMC").  No torch, no libdrx: nothing here shares a line with the
kernels.

    tables     P [n_users, K] user, Q [n_items, K] item as target of the user term, M [n_items, K] item as previous item,
               N [n_items, K] item as target of the transition term, b [n_items]
    window     (u, the ordered L items S before the target, target i, negatives j_1 .. j_r): uid [B], before [B, L], after [B, 1 + r]
               (the target first) — the layout of oracle/data_oracle.py::list_sample_counter at n_targets = 1
    score      x(u, S, i) = P[u] . Q[i] + mean_{l in S} M[l] . N[i] + b[i]          (S a list: a repeated item counts twice)
    loss       (1 / (B r)) sum_w sum_k softplus(-D_wk),  D_wk = x(u, S, i) - x(u, S, j_k);  g_wk = -sigmoid(-D_wk) / (B r)
    gradients  dP[u] += g (Q[i] - Q[j]);  dM[l] += (g / L) (N[i] - N[j]) for every l in S;  dQ[i] += g P[u];  dQ[j] -= g P[u];
               dN[i] += g mean M;  dN[j] -= g mean M;  db[i] += g;  db[j] -= g
    update     every row of P, M, Q and N adds reg * row to its gradient (b none); then one dense rule (tests/optim_oracle.py; Adam:
               tests/dense_update_oracle.py).  Under Adam the step size of an apply is Keras's lr_t of its counter
               n_applies * step + position + 1 (P registered first, then M, then Q | N with b: positions 0, 1, 2 of 3).
    serving    the basket of a user: up to L item ids, -1 = absent; the mean runs over the ids present, an empty basket gives a zero
               transition term.
`hold` = names of tables a step leaves as they are (('M', 'N') at M = N = 0: the BPR-MF restriction of the model)."""
import numpy as np

import bpr_oracle as bo

NAMES = ('P', 'M', 'Q', 'N', 'b')
HP = bo.HP
softplus = bo.softplus


def context(p, before):
    """mean_{l in S} M[l] per window, [B, K]"""
    return p['M'][np.asarray(before)].mean(axis=1)


def deltas(p, uid, before, after):
    """D_wk, [B, r]"""
    after = np.asarray(after)
    pu, mb = p['P'][np.asarray(uid)], context(p, before)
    x = np.einsum('wk,wjk->wj', pu, p['Q'][after]) + np.einsum('wk,wjk->wj', mb, p['N'][after]) + p['b'][after]
    return x[:, :1] - x[:, 1:]


def loss(p, uid, before, after):
    return float(np.mean(softplus(-deltas(p, uid, before, after))))


def gradients(p, uid, before, after):
    """(loss, {name: gradient}): the data gradients of the batch (no regularisation)"""
    uid, before, after = np.asarray(uid), np.asarray(before), np.asarray(after)
    B, L = before.shape
    r = after.shape[1] - 1
    d = deltas(p, uid, before, after)
    g = -(1.0 / (1.0 + np.exp(d))) / (B * r)              # -sigmoid(-d) / (B r), [B, r]
    pu, mb = p['P'][uid], context(p, before)
    grads = {n: np.zeros_like(p[n]) for n in NAMES}
    i, j = after[:, 0], after[:, 1:]
    dq = np.einsum('wk,wkf->wf', g, p['Q'][i][:, None, :] - p['Q'][j])
    dn = np.einsum('wk,wkf->wf', g, p['N'][i][:, None, :] - p['N'][j])
    np.add.at(grads['P'], uid, dq)
    for l in range(L):
        np.add.at(grads['M'], before[:, l], dn / L)
    gsum = g.sum(axis=1)
    np.add.at(grads['Q'], i, gsum[:, None] * pu)
    np.add.at(grads['N'], i, gsum[:, None] * mb)
    np.add.at(grads['b'], i, gsum)
    for k in range(r):
        np.add.at(grads['Q'], j[:, k], -g[:, k, None] * pu)
        np.add.at(grads['N'], j[:, k], -g[:, k, None] * mb)
        np.add.at(grads['b'], j[:, k], -g[:, k])
    return float(np.mean(softplus(-d))), grads


def init_state(p, kind):
    """{name: [s1, s2]} of rule `kind`, as tests/bpr_oracle.py::init_state"""
    n = 2 if kind == 'adam' else bo.oo.N_SLOTS[kind]
    init = 0.1 if kind == 'adagrad' else 0.0
    return {name: [np.full_like(p[name], init) if s < n else None for s in range(2)] for name in NAMES}


def step(p, state, step_idx, uid, before, after, kind='adam', hp=HP, applies=(3, 0, 1, 2), hold=()):
    """One training step in place on p (float64 arrays) and state; returns the loss of the batch before the update.
    applies = (n, j_user, j_transition, j_item)."""
    L, g = gradients(p, uid, before, after)
    n, ju, jm, ji = applies
    if kind == 'adam':
        a_u, a_m, a_i = (bo.adam_alpha(hp['lr'], n * step_idx + j + 1, hp['b1'], hp['b2']) for j in (ju, jm, ji))
    else:
        a_u = a_m = a_i = hp['lr']
    for name, alpha, l2c in (('P', a_u, hp['reg']), ('M', a_m, hp['reg']), ('Q', a_i, hp['reg']), ('N', a_i, hp['reg']), ('b', a_i, 0.0)):
        if name in hold:
            continue
        new = bo.apply_rule(kind, p[name], state[name][0], state[name][1], g[name], alpha, l2c, hp)
        # (the float32 replay: the gradients above were formed in float32; the rule's results are rounded to float32 as they are stored)
        p[name], state[name][0], state[name][1] = (a if a is None else a.astype(p[name].dtype) for a in new)
    return L


def query_rows(p, baskets, uids=None):
    """[P[u] | mean of M over the basket's ids present] per user, [n, 2 K]; baskets [n_users, L], -1 = absent"""
    baskets = np.asarray(baskets)
    uids = np.arange(len(baskets)) if uids is None else np.asarray(uids)
    K = p['P'].shape[1]
    out = np.zeros((len(uids), 2 * K), dtype=p['P'].dtype)
    for q, u in enumerate(uids):
        ids = [int(x) for x in baskets[u] if x >= 0]
        out[q, :K] = p['P'][u]
        if ids:
            out[q, K:] = p['M'][ids].mean(axis=0)
    return out


def scores(p, baskets):
    """x(u, basket of u, i) for every user and item, [n_users, n_items]"""
    return query_rows(p, baskets) @ np.concatenate([p['Q'], p['N']], axis=1).T + p['b'][None, :]


def baskets_of(twin, n_users, L):
    """[n_users, L] int32, -1 = absent: the last min(L, len) ids of every group's row of the sampler twin's seq_ids, by group value"""
    out = np.full((n_users, L), -1, np.int32)
    for g, u in enumerate(np.asarray(twin['group_value'])):
        row = np.asarray(twin['seq_ids'][int(twin['indptr'][g]):int(twin['indptr'][g + 1])])[-L:]
        out[int(u), :len(row)] = row
    return out


def twin_of(sequences, n_items, L, r):
    """The arrays ListSampler.twin_host_arrays() gives for one ordered id sequence per user (group g = user g), windows of L + 1 and r
    negatives: what oracle/data_oracle.py::list_sample_counter draws from."""
    lens = np.array([len(s) for s in sequences], np.int64)
    indptr = np.zeros(len(sequences) + 1, np.int64)
    indptr[1:] = np.cumsum(lens)
    held = [sorted(set(int(x) for x in s)) for s in sequences]
    held_indptr = np.zeros(len(sequences) + 1, np.int64)
    held_indptr[1:] = np.cumsum([len(h) for h in held])
    eligible = np.array([g for g, s in enumerate(sequences) if len(s) >= L + 1 and n_items - len(held[g]) >= r], np.int32)
    return {'indptr': indptr, 'seq_ids': np.array([x for s in sequences for x in s], np.int32), 'held_indptr': held_indptr,
            'held': np.array([x for h in held for x in h], np.int32), 'group_value': np.arange(len(sequences), dtype=np.int32),
            'eligible': eligible, 'n_ids': int(n_items)}


def init_params(rng, n_users, n_items, K):
    """the tests' weights: uniform(-0.5, 0.5) / sqrt(K), rounded to fp32 (what the device holds), as float64"""
    f = lambda *shape: (rng.uniform(-0.5, 0.5, size=shape) / np.sqrt(K)).astype(np.float32).astype(np.float64)
    return {'P': f(n_users, K), 'M': f(n_items, K), 'Q': f(n_items, K), 'N': f(n_items, K), 'b': f(n_items)}


def replay32(p):
    """the parameters as float32 arrays: the same functions then run in float32 — the oracle's own float32 replay"""
    return {k: np.asarray(v, np.float32) for k, v in p.items()}
