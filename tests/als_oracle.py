"""ALS for implicit-feedback WMF (Hu, Koren, Volinsky 2008) as plain NumPy: the definition of record of the model drecpy_amd trains with
drx_als_gram / drx_als_solve_rows / drx_als_loss (include/drx.h "ALS / WMF").  No torch, no libdrx: nothing here shares a line with the
kernels.  Every function takes dtype= (float64 by default): with float32 it is the fp32 replay whose own error against float64 scales
the GPU tests' bound.

    frame      CSR of the positives (indptr, indices, w): preference 1, confidence c = 1 + w, w = alpha r >= 0; every other cell of the
               n_users x n_items matrix has preference 0 and confidence 1
    objective  L(X, Y) = sum_ui c_ui (p_ui - x_u . y_i)^2 + lam (|X|^2 + |Y|^2), over ALL cells
    half-step  with Y fixed, G = Y^T Y and S_u the positives of u:
                   A_u = G + sum_{i in S_u} w_ui y_i y_i^T + lam I,   b_u = sum_{i in S_u} (1 + w_ui) y_i,   x_u = A_u^-1 b_u
               (x_u = 0 exactly where S_u is empty); the item half is the same call on the transposed CSR with X and Y swapped
    sweep      the user half, then the item half on the new X
    loss       L = <X^T X, Y^T Y>_F + sum over positives of [c (1 - s)^2 - s^2] + lam (|X|^2 + |Y|^2),  s = x_u . y_i"""
import numpy as np


class Frame:
    """the positives of a dense [n_users, n_items] weight matrix W (w > 0 marks a positive; w == 0 is no entry) in both orientations"""

    def __init__(self, W):
        W = np.asarray(W, dtype=np.float64)
        self.n_users, self.n_items = W.shape
        self.W = W
        self.csr = self._csr(W)
        self.csr_t = self._csr(W.T)

    @staticmethod
    def _csr(W):
        indptr = np.zeros(W.shape[0] + 1, np.int64)
        indptr[1:] = np.cumsum((W > 0).sum(axis=1))
        rows, cols = np.nonzero(W > 0)                          # row-major: columns ascending inside a row
        return indptr, cols.astype(np.int32), W[rows, cols]


def half_step(other, csr, lam, dtype=np.float64):
    """[n_rows, K]: x_r = A_r^-1 b_r for every row of the CSR (indptr, indices, w) against the fixed factors `other`"""
    indptr, indices, w = csr
    Y = np.asarray(other, dtype=dtype)
    K = Y.shape[1]
    G = Y.T @ Y
    out = np.zeros((len(indptr) - 1, K), dtype=dtype)
    lamI = (dtype(lam) * np.eye(K, dtype=dtype)).astype(dtype)
    for r in range(len(indptr) - 1):
        s, e = int(indptr[r]), int(indptr[r + 1])
        if e == s:
            continue
        Ys, ws = Y[indices[s:e]], np.asarray(w[s:e], dtype=dtype)
        A = (G + (Ys * ws[:, None]).T @ Ys + lamI).astype(dtype)
        b = ((dtype(1) + ws)[:, None] * Ys).sum(axis=0, dtype=dtype)
        out[r] = np.linalg.solve(A, b)
    return out


def sweep(p, frame, lam, dtype=np.float64):
    """one sweep in place on p = {'X', 'Y'}: the user half, then the item half; returns p"""
    p['X'] = half_step(p['Y'], frame.csr, lam, dtype)
    p['Y'] = half_step(p['X'], frame.csr_t, lam, dtype)
    return p


def loss(p, frame, lam, dtype=np.float64):
    """L in the sparse form (no dense matrix)"""
    X, Y = np.asarray(p['X'], dtype=dtype), np.asarray(p['Y'], dtype=dtype)
    indptr, indices, w = frame.csr
    rows = np.repeat(np.arange(frame.n_users), np.diff(indptr))
    s = np.einsum('ek,ek->e', X[rows], Y[indices]).astype(dtype)
    c = dtype(1) + np.asarray(w, dtype=dtype)
    one = dtype(1)
    return float(((X.T @ X) * (Y.T @ Y)).sum(dtype=dtype) + (c * (one - s) ** 2 - s ** 2).sum(dtype=dtype)
                 + dtype(lam) * ((X * X).sum(dtype=dtype) + (Y * Y).sum(dtype=dtype)))


def loss_dense(p, frame, lam):
    """L as the sum over all cells (float64): what `loss` must equal"""
    X, Y = np.asarray(p['X'], np.float64), np.asarray(p['Y'], np.float64)
    P = (frame.W > 0).astype(np.float64)
    C = 1.0 + frame.W
    return float((C * (P - X @ Y.T) ** 2).sum() + lam * ((X * X).sum() + (Y * Y).sum()))


def scores(p):
    return np.asarray(p['X'], np.float64) @ np.asarray(p['Y'], np.float64).T


def fit(p, frame, lam, sweeps, dtype=np.float64):
    """(p after `sweeps` sweeps, [L after every sweep]) from a copy of p"""
    p = {k: np.asarray(v, dtype=dtype).copy() for k, v in p.items()}
    losses = []
    for _ in range(sweeps):
        sweep(p, frame, lam, dtype)
        losses.append(loss(p, frame, lam, dtype))
    return p, losses


def init_params(rng, n_users, n_items, K, std=0.01):
    """the tests' weights: normal(0, std) rounded to fp32 (what the device holds), as float64"""
    f = lambda *shape: rng.normal(0.0, std, size=shape).astype(np.float32).astype(np.float64)
    return {'X': f(n_users, K), 'Y': f(n_items, K)}


def random_frame(rng, n_users, n_items, density=0.3, alpha=40.0, empty_user=None, empty_item=None, full_user=None):
    """a dense-random frame with ratings 1..5 and w = alpha r; the named user / item without positives, the named user with all items"""
    R = rng.integers(1, 6, size=(n_users, n_items)) * (rng.random((n_users, n_items)) < density)
    if full_user is not None:
        R[full_user] = rng.integers(1, 6, size=n_items)
    if empty_user is not None:
        R[empty_user] = 0
    if empty_item is not None:
        R[:, empty_item] = 0
    return Frame(alpha * R.astype(np.float64))
