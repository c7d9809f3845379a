"""fit(optimizer=...) with the dense rules beside Adam, end to end: CDAE reference mode (bce and mse) against the gradients of
oracle/cdae_oracle.py pushed through tests/optim_oracle.py in float64 — same injected weights, sampler and corruption streams as
tests/test_gpu_fit.py — after 1 and 10 steps, predictions within 1e-5 relative; the quiet loop in the library against the step-by-step
loop, bit for bit; a hooks-only model through the tape step under SGD with momentum against its closed form; early stopping's revert,
snapshot / restore with zero, one and two slots, save / load; and what keeps refusing."""
import random

import numpy as np
import pytest

import optim_oracle as oo
from oracle import cdae_oracle as co
from oracle import data_oracle as do
from helpers import batch_rows, load_frames
from test_optim_oracle import _rule32

pytestmark = pytest.mark.gpu

LR, REG, MU, RHO = 1e-2, 1e-3, 0.9, 0.9


def _frame():
    f = load_frames()['pt_int_dense']          # 64 users x 40 items, values 0..5 (zeros exercise the threshold)
    return {k: v.copy() for k, v in f.items()}


def _optimizer(rule):
    from drecpy_amd import optimizers as op
    return {'sgd': lambda: op.SGD(LR), 'momentum': lambda: op.SGD(LR, MU), 'nesterov': lambda: op.SGD(LR, MU, nesterov=True),
            'adagrad': lambda: op.Adagrad(LR), 'rmsprop': lambda: op.RMSprop(LR, RHO), 'rmsprop_momentum': lambda: op.RMSprop(LR, RHO, MU)}[rule]()


def _oracle_fit(frame, K, epochs, B, seed, weights, rule, loss='bce', q=0.2, thr=1e-3, neg_ratio=5, dtype=np.float64):
    """tests/test_gpu_fit.py's _oracle_fit with co.dense_grads' gradients (their L2 term included) through optim_oracle's rule"""
    uid, _ = do.first_appearance_codes(frame['user'].tolist())
    iid, _ = do.first_appearance_codes(frame['item'].tolist())
    U, N = int(uid.max()) + 1, int(iid.max()) + 1
    indptr, cols, vals = do.interaction_csr(uid, iid, frame['interaction'], U, N)
    sampler = do.PointSamplerOracle(uid, iid, frame['interaction'], neg_ratio, thr, seed)
    rng = random.Random(seed)
    p = {k: np.asarray(v, dtype).copy() for k, v in weights.items()}
    init = 0.1 if rule == 'adagrad' else 0.0
    slots = {k: [np.full(v.shape, init) if i < oo.N_SLOTS[rule] else None for i in range(2)] for k, v in p.items()}
    tmat = np.zeros((U, N), dtype=bool)
    for u in range(U):
        s, e = indptr[u], indptr[u + 1]
        tmat[u, cols[s:e][vals[s:e] >= thr]] = True
    for step in range(epochs):
        batch = sampler.sample(B)
        uids = np.array([b[0] for b in batch])
        t = tmat[uids]
        keep = do.corruption_keep_mask(rng, B, N, q)
        xt = (t & keep).astype(dtype) / dtype(1.0 - q)
        _, g, _ = co.dense_grads(p, uids, xt, t, REG, loss)
        for name in co.VAR_ORDER:
            if dtype == np.float32:                   # the same fit in fp32, every operation rounded: what fp32 arithmetic alone drifts by
                s1, s2 = (None if a is None else a.astype(np.float32) for a in slots[name])
                r = _rule32(rule, p[name], s1, s2, g[name].astype(np.float32), LR, 0.0, MU, RHO, 1e-7, False)
                p[name], slots[name] = r[0], [r[1], r[2]]
            else:
                r = oo.rule_flat(rule, p[name], slots[name][0], slots[name][1], g[name], LR, 0.0, MU, RHO, 1e-7)
                p[name], slots[name] = r.p, [r.s1, r.s2]
    return p, slots, tmat


def _worst(model, p, tmat):
    return max(float(np.max(np.abs(model._predict(u) - co.predict_row(p, u, tmat[u])) / np.abs(co.predict_row(p, u, tmat[u])))) for u in range(tmat.shape[0]))


@pytest.mark.parametrize('rule', ['sgd', 'nesterov', 'adagrad', 'rmsprop', 'rmsprop_momentum'])
@pytest.mark.parametrize('K,loss', [(50, 'bce'), (16, 'mse')])
def test_cdae_reference_mode_matches_the_oracle_after_1_and_10_steps(rule, K, loss):
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender import CDAE
    frame = _frame()
    ds = InteractionDataset.read_df(frame, verbose=False)
    w = co.init_params(np.random.default_rng(7), 64, 40, K, np.float32)
    B, seed = 32, 10
    for epochs in (1, 10):
        model = CDAE(hidden_factors=K, corruption_level=0.2, loss=loss, seed=seed, verbose=False)
        model.fit(ds, epochs=epochs, batch_size=B, learning_rate=LR, reg_rate=REG, neg_ratio=5, initial_weights=w, optimizer=_optimizer(rule))
        assert model.optimizer.kind == rule and model._engine.opt_kind == oo.CODE[rule]
        e = model._engine
        assert (e.s1 is None) == (oo.N_SLOTS[rule] < 1) and (e.s2 is None) == (oo.N_SLOTS[rule] < 2)        # only the slots the rule has
        p, slots, tmat = _oracle_fit(frame, K, epochs, B, seed, w, rule, loss)
        worst = _worst(model, p, tmat)
        gate = 1e-5
        if epochs == 10:                                       # as the 50-step Adam gate: twice the drift of the same fit in fp32, at least 1e-5
            p32, _, _ = _oracle_fit(frame, K, epochs, B, seed, w, rule, loss, dtype=np.float32)
            drift = max(float(np.max(np.abs(co.predict_row(p32, u, tmat[u]).astype(np.float64) - co.predict_row(p, u, tmat[u]))
                                     / np.abs(co.predict_row(p, u, tmat[u])))) for u in range(64))
            gate = max(1e-5, 2 * drift)
            print(f'[cdae {loss} {rule}] fp32 oracle drift after {epochs} steps {drift:.3g}')
        print(f'[cdae {loss} {rule}] {epochs} steps: worst relative prediction error {worst:.3g} (gate {gate:.3g})')
        assert worst < gate, (epochs, worst, gate)
        if e.s1 is not None:                                   # the slots too: W's against the oracle's
            np.testing.assert_allclose(e.s1[0][:, :K].cpu().numpy(), slots['W'][0], rtol=1e-4, atol=1e-9)


@pytest.mark.parametrize('rule', ['sgd', 'rmsprop_momentum'])
@pytest.mark.parametrize('B,K,loss', [(300, 50, 'bce'), (70, 300, 'mse')])
def test_cdae_dense_steps_past_the_tile_path_match_the_oracle(rule, B, K, loss):
    """B > 256, or rows too wide for a batch held in LDS twice: drx_cdae_step_dense takes k_out_dense (a group of lanes per output unit,
    the batch in sub-batches) instead of k_out_dense_tile — its row update and its bias update with the slots the rule has.  Three
    engine steps against cdae_oracle.dense_grads through optim_oracle; predictions within 1e-5 relative."""
    import torch
    from drecpy_amd.engine import CdaeEngine
    from helpers import synth_history, x_tilde
    rng = np.random.default_rng(B + K)
    U, N, q = 90, 150, 0.2
    p = co.init_params(rng, U, N, K, np.float64)
    indptr, indices = synth_history(rng, U, N, 10)
    eng = CdaeEngine(U, N, K)
    eng.set_params(**p)
    eng.set_history(indptr, indices)
    o = _optimizer(rule)
    eng.init_optimizer(rule, LR, REG, eps=getattr(o, 'epsilon', None), momentum=o.momentum, rho=getattr(o, 'rho', 0.9))
    assert (eng.s1 is None) == (rule == 'sgd') and (eng.s2 is None) == (rule == 'sgd')
    slots = {k: [np.zeros(v.shape) if i < oo.N_SLOTS[rule] else None for i in range(2)] for k, v in p.items()}
    for step in range(3):
        uids = rng.integers(0, U, size=B)
        t, keep_off, _ = batch_rows(indptr, indices, uids, N)
        keep = (rng.random(keep_off[-1]) >= q).astype(np.uint8)
        _, _, kept = batch_rows(indptr, indices, uids, N, keep)
        bt, alive = eng.make_batch(uids, keep_off=keep_off, keep=keep, q=q)
        eng.step_dense(step, bt, loss)
        _, g, _ = co.dense_grads(p, uids, x_tilde(t, kept, float(np.float32(q)), np.float64), t, REG, loss)
        for name in co.VAR_ORDER:
            r = oo.rule_flat(rule, p[name], slots[name][0], slots[name][1], g[name], LR, 0.0, MU, RHO, 1e-7)
            p[name], slots[name] = r.p, [r.s1, r.s2]
    torch.cuda.synchronize()
    _, pred = eng.forward(np.arange(U))
    tp, _, _ = batch_rows(indptr, indices, np.arange(U), N)
    _, po = co.forward(p, np.arange(U), tp.astype(np.float64))
    worst = float(np.max(np.abs(pred.cpu().numpy() - po) / np.abs(po)))
    print(f'[cdae k_out_dense {loss} {rule} B {B} K {K}] worst relative prediction error {worst:.3g}')
    assert worst < 1e-5, worst
    got = eng.get_params()
    np.testing.assert_allclose(got['b_'], p['b_'], rtol=0, atol=2e-6)          # (the bias update of the same kernel)


def test_string_forms_and_the_step_size_of_fit():
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender import CDAE
    frame = _frame()
    ds = InteractionDataset.read_df(frame, verbose=False)
    w = co.init_params(np.random.default_rng(7), 64, 40, 16, np.float32)
    for name, rule in (('sgd', 'sgd'), ('rmsprop', 'rmsprop'), ('adagrad', 'adagrad')):
        model = CDAE(hidden_factors=16, corruption_level=0.2, seed=10, verbose=False)
        model.fit(ds, epochs=3, batch_size=32, learning_rate=LR, reg_rate=REG, neg_ratio=5, initial_weights=w, optimizer=name)
        assert model.optimizer.kind == rule and model.optimizer.learning_rate == LR
        p, _, tmat = _oracle_fit(frame, 16, 3, 32, 10, w, rule)
        assert _worst(model, p, tmat) < 1e-5


@pytest.mark.parametrize('rule', ['adagrad', 'momentum'])
def test_quiet_fit_in_the_library_equals_the_step_by_step_loop(rule):
    """drx_cdae_fit_dense against drx_cdae_step_dense step by step: bit-identical tables and slots"""
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender import CDAE
    ds = InteractionDataset.read_df(_frame(), verbose=False)
    w = co.init_params(np.random.default_rng(5), 64, 40, 24, np.float32)
    out = []
    for fused in (True, False):
        m = CDAE(hidden_factors=24, corruption_level=0.3, seed=21, verbose=False)
        m.fused_fit = fused
        m.fit(ds, epochs=7, batch_size=16, learning_rate=LR, reg_rate=REG, neg_ratio=3, initial_weights=w, optimizer=_optimizer(rule))
        e = m._engine
        out.append([t.cpu().numpy().copy() for t in e.tables() + e.s1])
    assert all(np.array_equal(x, y) for x, y in zip(*out))
    assert not np.array_equal(out[0][0][:, :24], w['W'])


def test_early_stopping_reverts_a_momentum_fit_and_snapshots_carry_every_slot_count():
    import torch
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender import CDAE, MaxValidationValueRule
    frame = _frame()
    ds = InteractionDataset.read_df(frame, verbose=False)
    w = co.init_params(np.random.default_rng(3), 64, 40, 8, np.float32)
    calls = []

    def cb(m):
        calls.append(len(calls))
        return {'val': -abs(len(calls) - 2)}          # best at the 2nd callback (epoch 4)
    model = CDAE(hidden_factors=8, seed=10, verbose=False)
    model.fit(ds, epochs=8, batch_size=16, learning_rate=LR, reg_rate=REG, initial_weights=w, epoch_callback_fn=cb, epoch_callback_freq=2,
              early_stopping_rule=MaxValidationValueRule('val'), early_stopping_freq=2, optimizer=_optimizer('momentum'))
    p4, slots4, tmat = _oracle_fit(frame, 8, 4, 16, 10, w, 'momentum')
    assert _worst(model, p4, tmat) < 1e-5
    e = model._engine
    snap4 = model.epoch_weights[4]
    assert snap4['s2'] is None and len(snap4['s1']) == 5
    np.testing.assert_allclose(snap4['s1'][0][:, :8].cpu().numpy(), slots4['W'][0], rtol=1e-4, atol=1e-9)
    e.restore(snap4, with_optimizer=True)                                 # parameters AND the accumulators of epoch 4
    assert all(torch.equal(a, b) for a, b in zip(e.tables() + e.s1, snap4['p'] + snap4['s1']))
    for rule in ('sgd', 'rmsprop_momentum'):                              # zero and two slots
        m = CDAE(hidden_factors=8, seed=10, verbose=False)
        m.fit(ds, epochs=2, batch_size=16, learning_rate=LR, reg_rate=REG, initial_weights=w, optimizer=_optimizer(rule))
        e = m._engine
        snap = e.snapshot()
        m.fused_fit = False
        uids = np.arange(16)
        _, keep_off, _ = batch_rows(m._hist_indptr, m._hist_indices, uids, m.n_items)
        bt, alive = e.make_batch(uids, keep_off=keep_off, q=0.2, mask_seed=5)
        e.step_dense(2, bt)
        torch.cuda.synchronize()
        assert not torch.equal(e.W2T, snap['p'][1])
        e.restore(snap, with_optimizer=True)
        live = e.tables() + (e.s1 or []) + (e.s2 or [])
        kept = snap['p'] + (snap.get('s1') or []) + (snap.get('s2') or [])
        assert len(live) == len(kept) == 5 * (1 + oo.N_SLOTS[rule]) and all(torch.equal(a, b) for a, b in zip(live, kept))


def test_save_and_load_round_trip_an_rmsprop_model(tmp_path):
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender import CDAE, RecommenderABC
    frame = _frame()
    ds = InteractionDataset.read_df(frame, verbose=False)
    model = CDAE(hidden_factors=8, seed=10, verbose=False)
    model.fit(ds, epochs=5, batch_size=16, optimizer='rmsprop')
    assert model.optimizer.kind == 'rmsprop'
    raw_u, raw_i = frame['user'][0], frame['item'][0]
    path = str(tmp_path / 'cdae_rmsprop.bin')
    model.save(path)
    again = RecommenderABC.load(path)
    assert abs(again.predict(raw_u, raw_i) - model.predict(raw_u, raw_i)) < 1e-7
    assert [i for _, i in model.recommend(raw_u, n=6, novelty=True)] == [i for _, i in again.recommend(raw_u, n=6, novelty=True)]


def test_hooks_only_model_trains_through_the_tape_step_with_sgd_momentum():
    """tests/test_gpu_tape.py's hooks-only matrix factorisation under SGD(momentum=0.9): one apply_gradients per registered item through
    drx_opt_dense, against the closed form in float64"""
    import torch
    from drecpy_amd import optimizers as op
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender import RecommenderABC, Variable
    from drecpy_amd.Sampler import PointSampler
    K, B, EPOCHS, lr, reg = 6, 32, 5, 0.05, 0.01
    rng = np.random.default_rng(1)

    class TapeMF(RecommenderABC):
        def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
            self.P = Variable(kwds['P0'], name='P')
            self.Q = Variable(kwds['Q0'], name='Q')
            self.bias = Variable([0.1], name='bias')
            self._register_trainables([self.P, self.Q])
            self._register_trainable(self.bias)
            self._sampler = PointSampler(self.interaction_dataset, neg_ratio, self.interaction_threshold, self.seed)

        def _sample_batch(self, batch_size, **kwds):
            return self._sampler.sample(batch_size)

        def _predict_batch(self, batch_samples, **kwds):
            u = torch.tensor([t[0] for t in batch_samples], device='cuda')
            i = torch.tensor([t[1] for t in batch_samples], device='cuda')
            y = torch.tensor([self._standardize_value(t[2]) for t in batch_samples], dtype=torch.float32, device='cuda')
            return (self.P.tensor[u] * self.Q.tensor[i]).sum(dim=1) + self.bias.tensor, y

        def _compute_batch_loss(self, predictions, desired_values, **kwds):
            return ((predictions - desired_values) ** 2).mean()

        def _compute_reg_loss(self, reg_rate, batch_size, trainable_models, trainable_layers, trainable_weights, **kwds):
            return reg_rate * sum((w.tensor ** 2).sum() for w in trainable_weights[:2]) / batch_size

        def _predict(self, uid, iid, **kwds):
            return float((self.P.tensor[uid] * self.Q.tensor[iid]).sum() + self.bias.tensor[0])

    frame = {'user': np.random.default_rng(4).integers(0, 30, 400), 'item': np.random.default_rng(5).integers(0, 25, 400),
             'interaction': np.random.default_rng(6).integers(1, 6, 400)}
    ds = InteractionDataset.read_df(frame, verbose=False)
    m0 = TapeMF(seed=3, verbose=False)
    m0._bind_dataset(ds, False)
    U, N = m0.n_users, m0.n_items
    P0, Q0 = rng.normal(0, 0.3, (U, K)).astype(np.float32), rng.normal(0, 0.3, (N, K)).astype(np.float32)
    m = TapeMF(seed=3, verbose=False)
    m.fit(ds, epochs=EPOCHS, batch_size=B, learning_rate=lr, reg_rate=reg, neg_ratio=2, P0=P0, Q0=Q0, optimizer=op.SGD(lr, momentum=0.9))
    assert m.optimizer.kind == 'momentum' and m.optimizer.iterations == 3 * EPOCHS
    smp = PointSampler(ds, 2, m.interaction_threshold, 3)
    p = {'P': P0.astype(np.float64), 'Q': Q0.astype(np.float64), 'bias': np.array([np.float32(0.1)], np.float64)}
    acc = {k: np.zeros_like(v) for k, v in p.items()}
    for s in range(EPOCHS):
        batch = smp.sample(B)
        u = np.array([t[0] for t in batch]); i = np.array([t[1] for t in batch])
        y = np.array([m._standardize_value(t[2]) for t in batch], np.float32).astype(np.float64)
        d = 2.0 * ((p['P'][u] * p['Q'][i]).sum(axis=1) + p['bias'][0] - y) / B
        g = {'P': np.zeros_like(p['P']), 'Q': np.zeros_like(p['Q']), 'bias': np.array([d.sum()])}
        np.add.at(g['P'], u, d[:, None] * p['Q'][i])
        np.add.at(g['Q'], i, d[:, None] * p['P'][u])
        g['P'] += 2 * reg * p['P'] / B
        g['Q'] += 2 * reg * p['Q'] / B
        for name in ('P', 'Q', 'bias'):
            r = oo.rule_flat('momentum', p[name], acc[name], None, g[name], lr, 0.0, 0.9)
            p[name], acc[name] = r.p, r.s1
    np.testing.assert_allclose(m.P.numpy(), p['P'], rtol=0, atol=2e-5)
    np.testing.assert_allclose(m.Q.numpy(), p['Q'], rtol=0, atol=2e-5)
    np.testing.assert_allclose(m.bias.numpy(), p['bias'], rtol=0, atol=2e-5)
    assert np.abs(m.P.numpy() - P0).max() > 1e-2


def test_what_keeps_refusing():
    from drecpy_amd import optimizers as op
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender import CDAE
    ds = InteractionDataset.read_df(_frame(), verbose=False)
    for forced in ('sgd', 'rmsprop', op.SGD(0.1, 0.9)):
        with pytest.raises(Exception, match='sparse_optimizer'):
            CDAE(hidden_factors=8, mode='sampled', seed=1, verbose=False).fit(ds, epochs=1, batch_size=16, optimizer=forced)
    with pytest.raises(Exception, match='rowwise_adagrad'):
        CDAE(hidden_factors=8, seed=1, verbose=False).fit(ds, epochs=1, batch_size=16, optimizer='rowwise_adagrad')
    with pytest.raises(Exception, match='Unsupported optimizer'):
        CDAE(hidden_factors=8, seed=1, verbose=False).fit(ds, epochs=1, batch_size=16, optimizer='adadelta')


# ---- DMF and Caser: the engines' steps against the oracles' gradients through optim_oracle ----------------------------------------------
RULES = ['sgd', 'nesterov', 'adagrad', 'rmsprop', 'rmsprop_momentum']


def _apply(rule, p, slots, g, names, lr, dtype):
    """one apply of `rule` to the variables `names` (the oracle's gradients carry their L2 term)"""
    for name in names:
        if dtype == np.float32:
            s1, s2 = (None if a is None else a.astype(np.float32) for a in slots[name])
            r = _rule32(rule, p[name], s1, s2, g[name].astype(np.float32), lr, 0.0, MU, RHO, 1e-7, False)
            p[name], slots[name] = r[0], [r[1], r[2]]
        else:
            r = oo.rule_flat(rule, p[name], slots[name][0], slots[name][1], g[name], lr, 0.0, MU, RHO, 1e-7)
            p[name], slots[name] = r.p, [r.s1, r.s2]


def _fresh(rule, p):
    init = 0.1 if rule == 'adagrad' else 0.0
    return {k: [np.full(v.shape, init) if i < oo.N_SLOTS[rule] else None for i in range(2)] for k, v in p.items()}


def _engine_optimizer(rule, lr):
    from drecpy_amd import optimizers as op
    return {'sgd': lambda: op.SGD(lr), 'momentum': lambda: op.SGD(lr, MU), 'nesterov': lambda: op.SGD(lr, MU, nesterov=True),
            'adagrad': lambda: op.Adagrad(lr), 'rmsprop': lambda: op.RMSprop(lr, RHO), 'rmsprop_momentum': lambda: op.RMSprop(lr, RHO, MU)}[rule]()


def _dmf_problem():
    from oracle import dmf_oracle as dm
    rng = np.random.default_rng(1 * 7 + 33)                      # tests/test_gpu_dmf.py's smallest case: towers (16,) / (24, 16), B = 33
    U, N = 70, 90
    u, i = rng.integers(0, U, size=1500), rng.integers(0, N, size=1500)
    _, first = np.unique(u * N + i, return_index=True)
    u, i = u[np.sort(first)], i[np.sort(first)]
    v = rng.integers(1, 6, size=len(u)).astype(np.float64)
    csr, csc = do.interaction_csr(u, i, v, U, N), do.interaction_csr(i, u, v, N, U)
    dense = np.zeros((U, N))
    dense[u, i] = v
    p = dm.init_params(rng, U, N, (16,), (24, 16), np.float64)
    for k in p:
        if k.endswith('_b'):
            p[k] = rng.normal(0, 0.05, size=p[k].shape)
    batches = [(rng.integers(0, U, size=33), rng.integers(0, N, size=33), rng.random(33)) for _ in range(10)]
    probe = (rng.integers(0, U, size=40), rng.integers(0, N, size=40))
    return U, N, csr, csc, dense, p, batches, probe


def _dmf_oracle(rule, steps, dtype, lr, reg):
    from oracle import dmf_oracle as dm
    U, N, csr, csc, dense, p0, batches, probe = _dmf_problem()
    p = {k: v.astype(dtype) for k, v in p0.items()}
    slots = _fresh(rule, p)
    dn = dense.astype(dtype)
    for uids, iids, y in batches[:steps]:
        _, g, _ = dm.loss_and_grads(p, dn[uids], dn[:, iids].T.copy(), y, reg, 1, 2, True)
        _apply(rule, p, slots, g, list(p), lr, dtype)
    want, _ = dm.forward(p, dn[probe[0]], dn[:, probe[1]].T.copy(), 1, 2, True)
    return np.asarray(want, np.float64)


@pytest.mark.parametrize('update', ['scan', 'scatter'])
@pytest.mark.parametrize('rule', RULES)
def test_dmf_steps_match_the_oracle_after_1_and_10_steps(rule, update):
    """small weights (drx_dmf_step_small_opt), the first-layer kernels by the scan (drx_dmf_k0_update with the rule) and by the fallback
    (touches -> drx_scatter_rows -> drx_opt_dense)"""
    from drecpy_amd.engine_dmf import DmfEngine
    lr, reg = 2e-3, 1e-3
    U, N, csr, csc, dense, p0, batches, probe = _dmf_problem()
    for steps in (1, 10):
        eng = DmfEngine(U, N, (16,), (24, 16), True)
        eng.set_interactions(csr, csc)
        eng.first_layer_update = update
        eng.set_params(p0)
        eng.reg = reg
        eng.set_optimizer(_engine_optimizer(rule, lr))
        assert [sum(s is not None for s in eng.state[n]) for n in ('K0u', 'K0i', 'sw')] == [oo.N_SLOTS[rule]] * 3
        for step, (uids, iids, y) in enumerate(batches[:steps]):
            eng.step(step, uids, iids, y)
        pred = eng.predict(*probe).cpu().numpy()
        want = _dmf_oracle(rule, steps, np.float64, lr, reg)
        worst = float(np.max(np.abs(pred - want) / np.maximum(np.abs(want), 1e-6)))
        gate = 1e-5
        if steps == 10:
            drift = float(np.max(np.abs(_dmf_oracle(rule, steps, np.float32, lr, reg) - want) / np.maximum(np.abs(want), 1e-6)))
            gate = max(1e-5, 2 * drift)
            print(f'[dmf {update} {rule}] fp32 oracle drift after {steps} steps {drift:.3g}')
        print(f'[dmf {update} {rule}] {steps} steps: worst relative prediction error {worst:.3g} (gate {gate:.3g})')
        assert worst < gate, (steps, worst, gate)


@pytest.mark.parametrize('rule', ['momentum', 'rmsprop_momentum', 'sgd'])
def test_dmf_host_batches_and_device_prepared_batches_agree(rule):
    """tests/test_gpu_dmf.py's device-batch equality under another rule: bit-identical parameters, over more steps than the ring of cached
    argument structs has slots, with a change of rule in between (the cache key carries the rule)"""
    import torch
    from drecpy_amd.engine_dmf import DmfEngine
    from oracle import dmf_oracle as dm
    rng = np.random.default_rng(17)
    U, N, B = 120, 80, 200
    u, i = rng.integers(0, U, size=2500), rng.integers(0, N, size=2500)
    _, first = np.unique(u * N + i, return_index=True)
    u, i = u[np.sort(first)], i[np.sort(first)]
    v = rng.integers(1, 6, size=len(u)).astype(np.float64)
    csr, csc = do.interaction_csr(u, i, v, U, N), do.interaction_csr(i, u, v, N, U)
    p = dm.init_params(rng, U, N, (32, 16), (24, 16), np.float64)
    engs = []
    for _ in range(2):
        e = DmfEngine(U, N, (32, 16), (24, 16), True)
        e.set_interactions(csr, csc)
        e.set_params(p)
        e.reg = 1e-3
        e.set_optimizer(_engine_optimizer(rule, 2e-3))
        engs.append(e)
    for step in range(9):
        if step == 6:
            for e in engs:
                e.set_optimizer(_engine_optimizer('nesterov' if rule != 'nesterov' else 'sgd', 2e-3))
        uu = rng.integers(0, U, size=B).astype(np.int32)
        ii = rng.integers(0, N // 4, size=B).astype(np.int32)
        y = rng.random(B).astype(np.float32)
        engs[0].step(step, uu, ii, y)
        engs[1].step(step, engs[1].prepare_batch_device(B, 0, 0, triples=[torch.as_tensor(a).cuda() for a in (uu, ii, y)]))
    ga, gb = engs[0].get_params(), engs[1].get_params()
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k
    assert not np.array_equal(ga['u0_k'], p['u0_k'].astype(np.float32))


def _caser_problem():
    from oracle import caser_oracle as ca
    d, L, n_v, n_h, T, neg, B = 16, 3, 2, 8, 2, 2, 37            # tests/test_gpu_caser.py's smallest parity case, with dropout
    rng = np.random.default_rng(d + B)
    U, N = 40, 150
    p = ca.init_params(rng, U, N, L, d, n_v, n_h, np.float64)
    nx = n_v + L * n_h
    batches = [(rng.integers(0, U, size=B), rng.integers(0, N, size=(B, L)), rng.integers(0, N, size=(B, T + T * neg)),
                rng.random((B, nx)) >= 0.5) for _ in range(10)]
    probe = (rng.integers(0, U, size=5), rng.integers(0, N, size=(5, L)))
    return (U, N, L, T, neg, d, n_v, n_h), p, batches, probe


def _caser_oracle(rule, steps, dtype, lr, reg):
    from oracle import caser_oracle as ca
    (U, N, L, T, neg, d, n_v, n_h), p0, batches, probe = _caser_problem()
    p = {k: v.astype(dtype) for k, v in p0.items()}
    slots = _fresh(rule, p)
    for uids, before, after, keep in batches[:steps]:
        _, g, _ = ca.loss_and_grads(p, uids, before, after, T, reg, keep, 0.5)
        _apply(rule, p, slots, g, list(p), lr, dtype)
    return np.stack([np.asarray(ca.rank_scores(p, probe[0][r], probe[1][r]), np.float64) for r in range(5)])


@pytest.mark.parametrize('update', ['csr', 'scatter'])
@pytest.mark.parametrize('rule', RULES)
def test_caser_steps_match_the_oracle_after_1_and_10_steps(rule, update):
    """small weights (drx_caser_step_small_opt), the lookup tables through the fused CSR update (drx_rows_csr_opt_multi) and through
    the fallback (drx_scatter_rows + drx_opt_dense).  Scores cross zero: the error is taken relative to max(1, max |score|) of the row,
    as tests/test_gpu_caser.py takes it."""
    from drecpy_amd.engine_caser import CaserEngine
    lr, reg = 5e-3, 1e-4
    (U, N, L, T, neg, d, n_v, n_h), p0, batches, probe = _caser_problem()
    for steps in (1, 10):
        eng = CaserEngine(U, N, L, T, neg, d, n_v, n_h)
        eng.table_update = update
        eng.set_params(p0)
        eng.reg = reg
        eng.set_optimizer(_engine_optimizer(rule, lr))
        assert all(sum(s is not None for s in st) == oo.N_SLOTS[rule] for st in eng.state.values())
        for step, (uids, before, after, keep) in enumerate(batches[:steps]):
            eng.step(step, uids, before, after, keep, 0.5)
        sc = eng.scores_all(*probe).cpu().numpy()
        want = _caser_oracle(rule, steps, np.float64, lr, reg)
        scale = np.maximum(1.0, np.max(np.abs(want), axis=1, keepdims=True))
        worst = float(np.max(np.abs(sc - want) / scale))
        gate = 1e-5
        if steps == 10:
            drift = float(np.max(np.abs(_caser_oracle(rule, steps, np.float32, lr, reg) - want) / scale))
            gate = max(1e-5, 2 * drift)
            print(f'[caser {update} {rule}] fp32 oracle drift after {steps} steps {drift:.3g}')
        print(f'[caser {update} {rule}] {steps} steps: worst relative score error {worst:.3g} (gate {gate:.3g})')
        assert worst < gate, (steps, worst, gate)


def test_dmf_and_caser_fit_take_the_optimizer_argument():
    """fit(optimizer=...) reaches the engines: kind, hyper-parameters and slots; an unknown one is still refused"""
    from drecpy_amd import optimizers as op
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender import DMF
    frame = _frame()
    ds = InteractionDataset.read_df(frame, verbose=False)
    m = DMF(user_factors=[16, 8], item_factors=[16, 8], seed=3, verbose=False)
    m.fit(ds, epochs=3, batch_size=32, learning_rate=1e-3, optimizer=op.RMSprop(2e-3, rho=0.8, momentum=0.5))
    e = m._engine
    assert (e.opt_kind, e.lr, e.beta1, e.beta2) == ('rmsprop_momentum', 2e-3, 0.5, 0.8) and all(s is not None for s in e.state['sw'])
    assert float(e.state['sw'][0].abs().max()) > 0
    m = DMF(user_factors=[16, 8], item_factors=[16, 8], seed=3, verbose=False)
    m.fit(ds, epochs=3, batch_size=32, learning_rate=0.05, optimizer='sgd')
    assert m._engine.opt_kind == 'sgd' and m._engine.lr == 0.05 and m._engine.state['K0u'] == (None, None)
    with pytest.raises(Exception, match='rowwise_adagrad|dense rules'):
        DMF(user_factors=[16, 8], item_factors=[16, 8], seed=3, verbose=False).fit(ds, epochs=1, batch_size=32, optimizer='rowwise_adagrad')
    from drecpy_amd.Recommender import Caser
    # Caser: the rule reaches CaserEngine.set_optimizer after _pre_fit
    frame_c = {k: v.copy() for k, v in load_frames()['ls_int_ts'].items()}          # (tests/test_gpu_caser.py's fit fixture)
    dsc = InteractionDataset.read_df(frame_c, verbose=False)
    for optimizer, kind, n_slots in ((op.SGD(0.01, momentum=0.9, nesterov=True), 'nesterov', 1), ('rmsprop', 'rmsprop', 1), ('sgd', 'sgd', 0)):
        m = Caser(L=5, T=3, d=16, n_v=2, n_h=8, dropout_rate=0.5, seed=10, verbose=False)
        m.fit(dsc, epochs=3, batch_size=24, learning_rate=5e-3, reg_rate=1e-6, neg_ratio=2, optimizer=optimizer)
        e = m._engine
        assert e.opt_kind == kind and e.lr == m.optimizer.learning_rate
        assert all(sum(s is not None for s in st) == n_slots for st in e.state.values())
        if n_slots:
            assert float(e.state['item_emb'][0].abs().max()) > 0
    with pytest.raises(Exception, match='dense rules'):
        Caser(L=5, T=3, d=16, n_v=2, n_h=8, seed=10, verbose=False).fit(dsc, epochs=1, batch_size=24, optimizer='rowwise_adagrad')
