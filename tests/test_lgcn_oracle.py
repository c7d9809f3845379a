"""tests/lgcn_oracle.py held to torch.autograd and to its own two forms (no GPU): the gradient of the batch loss with respect to P and Q
over a dense adjacency, the Horner recurrence against the sum of powers forward and backward, the conventions for nodes without edges,
and layers = 0 against tests/bpr_oracle.py with its bias held at zero."""
import numpy as np
import pytest

import bpr_oracle as bo
import lgcn_oracle as lo

U, N = 9, 13


def _rows():
    """user 0 holds every item but the last, user 1 nothing, item 12 is held by nobody, item 5 by every user with a row"""
    rng = np.random.default_rng(5)
    rows = [list(range(N - 1)), []]
    for u in range(2, U):
        rows.append(sorted(set(rng.choice(N - 1, size=int(rng.integers(1, 6)), replace=False).tolist() + [5])))
    return rows


def _batch(T, seed):
    rng = np.random.default_rng(seed)
    uid = rng.integers(0, U, size=T)
    pos = rng.integers(0, N, size=T)
    neg = (pos + 1 + rng.integers(0, N - 1, size=T)) % N
    return uid, pos, neg


@pytest.mark.parametrize('layers', [0, 1, 2, 3, 4])
def test_the_gradient_is_autograds(layers):
    import torch
    rows, K = _rows(), 6
    p = lo.init_params(np.random.default_rng(layers), U, N, K)
    A = lo.adjacency(rows, N)
    uid, pos, neg = _batch(40, 11 + layers)
    L, g = lo.gradients(p, A, layers, uid, pos, neg)
    P, Q = (torch.tensor(p[n], dtype=torch.float64, requires_grad=True) for n in lo.NAMES)
    At = torch.tensor(A)
    E0 = torch.cat([P, Q])
    total, term = E0, E0
    for _ in range(layers):
        term = At @ term
        total = total + term
    E = total / (layers + 1)
    u, i, j = (torch.as_tensor(a) for a in (uid, U + pos, U + neg))
    d = (E[u] * (E[i] - E[j])).sum(dim=1)
    want = torch.nn.functional.softplus(-d).mean()
    want.backward()
    assert L == pytest.approx(float(want.detach()), rel=1e-13)
    assert L == pytest.approx(lo.loss(p, A, layers, uid, pos, neg), rel=1e-13)
    for name, t in (('P', P), ('Q', Q)):
        scale = float(t.grad.abs().max())
        assert scale > 0
        assert np.max(np.abs(g[name] - t.grad.numpy())) <= 1e-13 * scale, name


@pytest.mark.parametrize('layers', [0, 1, 2, 3, 4])
def test_horner_equals_the_sum_of_powers_forward_and_backward(layers):
    rows = _rows()
    A = lo.adjacency(rows, N)
    assert np.array_equal(A, A.T)
    rng = np.random.default_rng(layers)
    for X in (rng.normal(size=(U + N, 5)), rng.normal(size=(U + N, 1))):          # an embedding table, a gradient
        a, b = lo.power_mean(A, X, layers), lo.horner(A, X, layers)
        assert np.max(np.abs(a - b)) <= 1e-14 * np.max(np.abs(a))
    # backward IS the forward form on G: <backward(G), X> = <G, forward(X)>
    G, X = rng.normal(size=(U + N, 4)), rng.normal(size=(U + N, 4))
    assert np.sum(lo.backward(A, G, layers) * X) == pytest.approx(np.sum(G * lo.power_mean(A, X, layers)), rel=1e-12)
    assert np.max(np.abs(lo.horner(A, G, layers) - lo.backward(A, G, layers))) <= 1e-14 * np.max(np.abs(G))


def test_nodes_without_edges():
    rows = _rows()
    w, A = lo.degree_weights(rows, N), lo.adjacency(rows, N)
    assert w[1] == 0 and w[U + N - 1] == 0 and w[0] == 1.0 / np.sqrt(N - 1) and w[U + 5] == 1.0 / np.sqrt(U - 1)
    assert not A[1].any() and not A[:, U + N - 1].any() and np.isfinite(A).all()
    assert A[0, U + 5] == w[0] * w[U + 5] and not A[:U, :U].any() and not A[U:, U:].any()
    assert lo.degree_weights([[3, 3, 1]], 4)[0] == 1.0 / np.sqrt(2.0)                       # duplicates merged
    for layers in (0, 2, 4):
        p = lo.init_params(np.random.default_rng(1), U, N, 3)
        E = lo.final(p, A, layers)
        assert np.array_equal(E[1], p['P'][1] / (layers + 1)) and np.array_equal(E[U + N - 1], p['Q'][N - 1] / (layers + 1))
        # a triple on the isolated user moves that user's row alone among the users; the isolated item gets no gradient from others
        L, g = lo.gradients(p, A, layers, np.array([1]), np.array([5]), np.array([N - 1]))
        assert g['P'][1].any() and g['Q'][N - 1].any()
        L, g = lo.gradients(p, A, layers, np.array([2]), np.array([5]), np.array([3]))
        assert not g['P'][1].any() and not g['Q'][N - 1].any()
        assert g['P'][0].any() == (layers >= 2)                                   # user 0 is two hops from user 2


def test_no_layers_is_bpr_with_its_bias_at_zero():
    K = 5
    p = lo.init_params(np.random.default_rng(3), U, N, K)
    A = lo.adjacency(_rows(), N)
    b = dict(p, bq=np.zeros(N))
    uid, pos, neg = _batch(30, 2)
    assert np.array_equal(lo.scores(p, A, 0), bo.scores(b))
    L, g = lo.gradients(p, A, 0, uid, pos, neg)
    Lb, gb = bo.gradients(b, uid, pos, neg)
    assert L == pytest.approx(Lb, rel=1e-14)
    for name in lo.NAMES:
        assert np.max(np.abs(g[name] - gb[name])) <= 1e-15, name
    # and one Adam step moves P and Q as BPR's does
    st, stb = lo.init_state(p, 'adam'), bo.init_state(b, 'adam')
    lo.step(p, st, A, 0, 0, uid, pos, neg)
    bo.step(b, stb, 0, uid, pos, neg)
    for name in lo.NAMES:
        assert np.max(np.abs(p[name] - b[name])) <= 1e-15, name


@pytest.mark.parametrize('kind', ['adam', 'adagrad', 'sgd', 'momentum', 'nesterov', 'rmsprop'])
def test_a_step_and_its_float32_replay(kind):
    rows, K, layers = _rows(), 4, 2
    A = lo.adjacency(rows, N)
    p = lo.init_params(np.random.default_rng(4), U, N, K)
    p32 = lo.replay32(p)
    st, st32 = lo.init_state(p, kind), lo.init_state(p32, kind)
    p0 = {k: v.copy() for k, v in p.items()}
    for s in range(3):
        uid, pos, neg = _batch(20, 30 + s)
        L = lo.step(p, st, A, layers, s, uid, pos, neg, kind)
        L32 = lo.step(p32, st32, A, layers, s, uid, pos, neg, kind)
        assert L32 == pytest.approx(L, abs=1e-5)
    n = 2 if kind == 'adam' else bo.oo.N_SLOTS[kind]
    for name in lo.NAMES:
        assert p32[name].dtype == np.float32 and p[name].dtype == np.float64
        assert (p[name] != p0[name]).all()                                         # dense regularisation: every row moves
        assert np.max(np.abs(p32[name] - p[name])) <= 1e-4
        assert [s is not None for s in st[name]] == [k < n for k in range(2)]
