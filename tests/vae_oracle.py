"""Mult-VAE / Mult-DAE (Liang, Krishnan, Hoffman, Jebara, WWW 2018) as plain NumPy float64: the definition of record of the model
drecpy_amd trains with drx_vae_step and serves through drx_vae_query_rows (include/drx.h "Mult-VAE").  No torch, no libdrx: nothing here
shares a line with the kernels.

    parameters W_in [n_items, H]; b_in [H]; W_e [H, E], b_e [E] (E = 2 latent where variational, else latent); W_d [latent, H], b_d [H];
               W_out [n_items, H], b_out [n_items]
    batch      rows: one ascending array P_u of item ids per batch row; keep: one bool array per row (lookup j kept) or None;
               eps [B, latent] or None
    forward    x1 = c_b sum_{kept j} W_in[P_u[j]] + b_in, c_b = 1 / (sqrt(N_u) (1 - dropout)), N_u = |P_u| (a row without positives:
               x1 = b_in); h1 = tanh(x1); [mu | logvar] = h1 W_e + b_e; z = mu + eps exp(logvar / 2), or mu where eps is None or the
               model is not variational; h2 = tanh(z W_d + b_d); logit_i = h2 . W_out[i] + b_out[i]
    loss       mean_b [ -sum_{i in P_u} log softmax(logit)_i + kl_weight KL_b ],  KL_b = -1/2 sum (1 + logvar - mu^2 - exp(logvar))
               kl_weight = beta_t = beta min(1, (step + 1) / anneal_steps), beta where anneal_steps == 0; no L2 value in the loss
    update     every row of W_in and W_out and every entry of W_e and W_d adds reg * itself to its gradient (the biases none); then one
               dense rule (tests/optim_oracle.py; Adam: tests/dense_update_oracle.py).  Under Adam the step size of an apply is Keras's
               lr_t of its counter n_applies * step + position + 1 (W_in first, then the small weights, then W_out with b_out).
    randomness (functions of the draw seed alone) users: default_rng(seed).choice(eligible, min(batch_size, len), replace=False);
               keep bit of lookup j of row b: hash_u32(2 seed, b, j) >= q_threshold(dropout); noise of (b, c): Box-Muller
               sqrt(-2 ln u1) cos(2 pi u2), u1 = (w1 + 1) / 2^32, u2 = w2 / 2^32, w1, w2 = hash_u32(2 seed + 1, b, 2 c), (.., 2 c + 1)"""
import numpy as np

import bpr_oracle as bo
import fpmc_oracle as fo

HP = bo.HP
replay32 = fo.replay32
SMALL = ('W_e', 'W_d', 'b_in', 'b_e', 'b_d')          # the order of the flat array: the regularised ones first
NAMES = ('W_in',) + SMALL + ('W_out', 'b_out')
M64 = (1 << 64) - 1


def regularised(name):
    return name.startswith('W')


def is_variational(p):
    return p['W_e'].shape[1] == 2 * p['W_d'].shape[0]


def beta_t(beta, anneal_steps, step):
    return float(beta) if anneal_steps == 0 else float(beta) * min(1.0, (step + 1) / anneal_steps)


# ---- randomness ------------------------------------------------------------------------------------------------------------------------
def hash_u32(seed, a, b):
    """csrc/drx_common.hpp hash_u32 on uint64 arrays a, b (a scalar seed): the top 32 bits of a splitmix64-style mix"""
    with np.errstate(over='ignore'):
        x = np.uint64(seed & M64) + np.asarray(a, np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.asarray(b, np.uint64) * np.uint64(0xD1B54A32D192ED03)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (x >> np.uint64(32)).astype(np.uint32)


def q_threshold(q):
    t = float(np.float32(q)) * 4294967296.0
    return 0 if t <= 0.0 else 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def keep_bits(seed, lens, dropout):
    """flat bool [sum lens]: lookup j of row b, rows one behind the other"""
    lens = np.asarray(lens, np.int64)
    b = np.repeat(np.arange(len(lens)), lens)
    j = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
    return hash_u32(2 * seed, b, j) >= np.uint32(q_threshold(dropout))


def noise_words(seed, B, latent):
    """uint32 [B, latent, 2]"""
    b, c = np.meshgrid(np.arange(B), np.arange(latent), indexing='ij')
    return np.stack([hash_u32(2 * seed + 1, b, 2 * c), hash_u32(2 * seed + 1, b, 2 * c + 1)], axis=-1)


def noise_of(words, dtype=np.float64):
    """Box-Muller on the words, every operation in `dtype`"""
    f = dtype
    w1, w2 = words[..., 0].astype(f), words[..., 1].astype(f)
    u1 = (w1 + f(1.0)) * f(2.0 ** -32)
    u2 = w2 * f(2.0 ** -32)
    return (np.sqrt(f(-2.0) * np.log(u1)) * np.cos(f(2.0 * np.pi) * u2)).astype(f)


def draw_users(seed, eligible, batch_size):
    eligible = np.asarray(eligible)
    return np.random.default_rng(seed).choice(eligible, size=min(int(batch_size), len(eligible)), replace=False)


def split(flat, lens):
    return np.split(np.asarray(flat), np.cumsum(lens)[:-1]) if len(lens) else []


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def encode(p, rows, keep=None, eps=None, dropout=0.0):
    """the tape of the forward pass up to h2: every array in the dtype of p"""
    dt = p['W_in'].dtype.type
    B, H = len(rows), p['W_in'].shape[1]
    L = p['W_d'].shape[0]
    bag = np.zeros((B, H), dt)
    cb = np.zeros(B, dt)
    for b, row in enumerate(rows):
        row = np.asarray(row, np.int64)
        if len(row):
            cb[b] = dt(1.0) / (np.sqrt(dt(len(row))) * (dt(1.0) - dt(dropout)))
            kept = row if keep is None else row[np.asarray(keep[b], bool)]
            bag[b] = p['W_in'][kept].sum(axis=0) if len(kept) else 0
    h1 = np.tanh(cb[:, None] * bag + p['b_in']).astype(dt)
    ml = (h1 @ p['W_e'] + p['b_e']).astype(dt)
    mu = ml[:, :L]
    var = is_variational(p)
    lv = ml[:, L:] if var else None
    noisy = var and eps is not None
    z = (mu + np.asarray(eps, dt) * np.exp(lv / dt(2.0))).astype(dt) if noisy else mu
    h2 = np.tanh(z @ p['W_d'] + p['b_d']).astype(dt)
    return dict(cb=cb, h1=h1, mu=mu, lv=lv, z=z, h2=h2, eps=np.asarray(eps, dt) if noisy else None)


def gradients(p, rows, keep=None, eps=None, dropout=0.0, kl_weight=0.0):
    """(loss, {name: data gradient}, h2) of the batch; no regularisation"""
    dt = p['W_in'].dtype.type
    B, N = len(rows), p['W_out'].shape[0]
    t = encode(p, rows, keep, eps, dropout)
    logits = (t['h2'] @ p['W_out'].T + p['b_out']).astype(dt)
    top = logits.max(axis=1, keepdims=True)
    ex = np.exp(logits - top)
    den = ex.sum(axis=1, keepdims=True)
    logsm = (logits - top) - np.log(den)
    member = np.zeros((B, N), dt)
    for b, row in enumerate(rows):
        member[b, np.asarray(row, np.int64)] = 1
    n_u = member.sum(axis=1, keepdims=True)
    loss = -(member * logsm).sum(axis=1)
    var = is_variational(p)
    kw = dt(kl_weight)
    if var:
        mu, lv = t['mu'], t['lv']
        loss = loss + kw * (dt(-0.5) * (1 + lv - mu * mu - np.exp(lv)).sum(axis=1))
    dlogit = ((n_u * (ex / den) - member) / dt(B)).astype(dt)
    g = {'W_out': dlogit.T @ t['h2'], 'b_out': dlogit.sum(axis=0)}
    da2 = ((dlogit @ p['W_out']) * (1 - t['h2'] * t['h2'])).astype(dt)
    g['W_d'], g['b_d'] = t['z'].T @ da2, da2.sum(axis=0)
    dz = (da2 @ p['W_d'].T).astype(dt)
    if var:
        dmu = dz + kw / dt(B) * t['mu']
        dlv = kw / dt(B) * (dt(0.5) * (np.exp(t['lv']) - 1))
        if t['eps'] is not None:
            dlv = dlv + dz * t['eps'] * (dt(0.5) * np.exp(t['lv'] / dt(2.0)))
        de = np.concatenate([dmu, dlv], axis=1).astype(dt)
    else:
        de = dz
    g['W_e'], g['b_e'] = t['h1'].T @ de, de.sum(axis=0)
    dx1 = ((de @ p['W_e'].T) * (1 - t['h1'] * t['h1'])).astype(dt)
    g['b_in'] = dx1.sum(axis=0)
    g['W_in'] = np.zeros_like(p['W_in'])
    for b, row in enumerate(rows):
        row = np.asarray(row, np.int64)
        kept = row if keep is None else row[np.asarray(keep[b], bool)]
        g['W_in'][kept] += t['cb'][b] * dx1[b]              # (a row's items are distinct)
    return float(np.mean(loss)), {k: v.astype(dt) for k, v in g.items()}, t['h2']


def scores(p, rows):
    """x(u, i) for the users whose positives are `rows` x every item: z = mu, no dropout"""
    return encode(p, rows)['h2'] @ p['W_out'].T + p['b_out']


def init_state(p, kind):
    """{name: [s1, s2]} of rule `kind`, as tests/bpr_oracle.py::init_state"""
    n = 2 if kind == 'adam' else bo.oo.N_SLOTS[kind]
    init = 0.1 if kind == 'adagrad' else 0.0
    return {name: [np.full_like(p[name], init) if s < n else None for s in range(2)] for name in p}


def step_sizes(p, step_idx, kind='adam', hp=HP, applies=(3, 0, 1, 2)):
    """{name: step size} of a step: W_in, the small weights, W_out with b_out"""
    n, ji, js, jo = applies
    if kind == 'adam':
        a_i, a_s, a_o = (bo.adam_alpha(hp['lr'], n * step_idx + j + 1, hp['b1'], hp['b2']) for j in (ji, js, jo))
    else:
        a_i = a_s = a_o = hp['lr']
    return {name: a_i if name == 'W_in' else a_o if name in ('W_out', 'b_out') else a_s for name in p}


def l2_of(name, hp=HP):
    return hp['reg'] if regularised(name) else 0.0


def apply_gradients(p, state, step_idx, g, kind='adam', hp=HP, applies=(3, 0, 1, 2)):
    alphas = step_sizes(p, step_idx, kind, hp, applies)
    for name in list(p):
        new = bo.apply_rule(kind, p[name], state[name][0], state[name][1], g[name], alphas[name], l2_of(name, hp), hp)
        p[name], state[name][0], state[name][1] = (a if a is None else a.astype(p[name].dtype) for a in new)


def step(p, state, step_idx, rows, keep=None, eps=None, dropout=0.0, kl_weight=0.0, kind='adam', hp=HP, applies=(3, 0, 1, 2)):
    """One training step in place on p and state; returns (the loss of the batch before the update, h2 of the batch)"""
    L, g, h2 = gradients(p, rows, keep, eps, dropout, kl_weight)
    apply_gradients(p, state, step_idx, g, kind, hp, applies)
    return L, h2


def init_params(rng, n_items, H, latent, variational=True, scale=1.0):
    """the tests' weights: uniform(-0.5, 0.5) / sqrt(width) (a bias: width 1) times `scale`, so that the softmax is not flat.  Rounded to
    fp32 (what the device holds), as float64"""
    f = lambda width, *shape: (scale * rng.uniform(-0.5, 0.5, size=shape) / np.sqrt(width)).astype(np.float32).astype(np.float64)
    E = 2 * latent if variational else latent
    return {'W_in': f(H, n_items, H), 'W_e': f(H, H, E), 'W_d': f(latent, latent, H), 'b_in': f(1, H), 'b_e': f(1, E), 'b_d': f(1, H),
            'W_out': f(H, n_items, H), 'b_out': f(H, n_items)}
