"""NumPy restatement of the KNN baselines' arithmetic in the device's terms (include/drx.h, drx_knn_*):
co-rating sums accumulated in float32 (exact for integer ratings; `acc=np.float64` gives the float64 variant the tolerance tests
compare against), the epilogue in float64 as single operations in the stated order, similarities rounded to float32 once,
heapq.nlargest keys, and the aggregation in float64 in neighbour-list order.  No GPU, no reference import."""
from heapq import nlargest

import numpy as np

METRICS = ('cosine', 'adjusted_cosine', 'cosine_cf', 'jaccard', 'msd', 'pearson')


def csr_of(rows, cols, vals, R):
    """(indptr int64, indices int32 ascending per row, values float32) of unique (row, col) triples"""
    rows, cols, vals = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(vals, np.float32)
    order = np.lexsort((cols, rows))
    indptr = np.zeros(R + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(rows, minlength=R))
    return indptr, cols[order].astype(np.int32), vals[order]


def transpose_csr(csr, R, C):
    indptr, indices, values = csr
    rows = np.repeat(np.arange(R), np.diff(indptr))
    return csr_of(indices, rows, values, C)


def dense_of(csr, R, C):
    indptr, indices, values = csr
    X = np.zeros((R, C), np.float32)
    X[np.repeat(np.arange(R), np.diff(indptr)), indices] = values
    return X


def row_stats(csr, R):
    """per row, sequential float64 sums over its non-zero entries in CSR order: (cnt, mean, sqrt(sum x^2), sqrt(sum (x - mean)^2))"""
    indptr, _, values = csr
    cnt, mean, norm, cnorm = np.zeros(R, np.int64), np.zeros(R), np.zeros(R), np.zeros(R)
    for r in range(R):
        v = [float(x) for x in values[indptr[r]:indptr[r + 1]] if x != 0]
        s = f2 = c2 = 0.0
        for x in v:
            s = s + x
            f2 = f2 + x * x
        mu = s / len(v) if v else 0.0
        for x in v:
            d = x - mu
            c2 = c2 + d * d
        cnt[r], mean[r], norm[r], cnorm[r] = len(v), mu, np.sqrt(f2), np.sqrt(c2)
    return cnt, mean, norm, cnorm


def max_diff_of(csr, R, C):
    """msd's quirk: max(X) - min(X) of the SPARSE matrix, whose minimum counts the implicit zeros"""
    indptr, _, values = csr
    hi = float(values.max()) if len(values) else 0.0
    lo = float(values.min()) if len(values) else 0.0
    if len(values) < R * C:
        hi, lo = max(hi, 0.0), min(lo, 0.0)
    return hi - lo


def similarities(csr, R, C, metric, m, shrinkage, max_diff=None, acc=np.float32, raw=False):
    """float32 [R, R], symmetric, 0 where the pair is dropped, not positive, or on the diagonal.  x is the row with the smaller id.
    raw=True: float64 and signed instead (what the reference's _similarities holds, 0 where absent)."""
    X = dense_of(csr, R, C).astype(acc)
    M = (X != 0).astype(acc)
    cnt, mean, norm, cnorm = row_stats(csr, R)
    f8 = np.float64
    n = (M @ M.T).astype(f8)
    Sxy = (X @ X.T).astype(f8)
    Sx = (X @ M.T).astype(f8)             # [i, j]: sum of x_i over the columns i and j share
    Sy = Sx.T
    Sxx = ((X * X) @ M.T).astype(f8)
    Syy = Sxx.T
    keep = n > 0
    with np.errstate(all='ignore'):
        if metric == 'cosine':
            den = norm[:, None] * norm[None, :]
            keep &= den != 0
            s = Sxy / den
        elif metric == 'adjusted_cosine':
            mx, my = mean[:, None], mean[None, :]
            den = cnorm[:, None] * cnorm[None, :]
            keep &= den != 0
            t = Sxy - my * Sx
            t = t - mx * Sy
            t = t + (n * mx) * my
            s = t / den
        elif metric == 'cosine_cf':
            keep &= Sxy != 0
            s = Sxy / (np.sqrt(Sxx) * np.sqrt(Syy))
        elif metric == 'jaccard':
            s = n / ((cnt[:, None].astype(f8) + cnt[None, :].astype(f8)) - n)
        elif metric == 'msd':
            md = float(max_diff_of(csr, R, C) if max_diff is None else max_diff)
            s = 1.0 - (((Sxx + Syy) - 2.0 * Sxy) / (md * md)) / n
        elif metric == 'pearson':
            vx, vy = Sxx - (Sx * Sx) / n, Syy - (Sy * Sy) / n
            keep &= (vx > 0) & (vy > 0)
            s = (Sxy - (Sx * Sy) / n) / (np.sqrt(vx) * np.sqrt(vy))
        else:
            raise ValueError(metric)
        if m > 0:
            keep &= n >= m
        if shrinkage is not None:
            s = s * (n / ((n + float(shrinkage)) + 1e-6))
        s = np.where(keep, s, 0.0)
    if not raw:
        s = s.astype(np.float32)
        s = np.where(s > 0, s, np.float32(0)).astype(np.float32)
    upper = np.triu(s, 1)
    return upper + upper.T


def neighbours(S, k):
    """(idx int32 [R, k], sim float32 [R, k]): per row the k largest (sim, id) with sim > 0 among the other rows, -1 / 0 behind them"""
    R = S.shape[0]
    idx, sim = np.full((R, k), -1, np.int32), np.zeros((R, k), np.float32)
    for i in range(R):
        best = nlargest(k, ((float(S[i, j]), j) for j in range(R) if j != i and S[i, j] > 0))
        for t, (s, j) in enumerate(best):
            idx[i, t], sim[i, t] = j, s
    return idx, sim


def aggregate(terms, agg):
    """terms: [(s, r)] in neighbour-list order -> the prediction, or None without a term"""
    num = den = 0.0
    for s, r in terms:
        if agg == 'weighted_mean':
            num = num + float(s) * float(r)
            den = den + float(s)
        else:
            num = num + float(r)
            den = den + 1.0
    return num / den if den > 0 else None


def _row_dict(csr, r):
    indptr, indices, values = csr
    return {int(c): float(v) for c, v in zip(indices[indptr[r]:indptr[r + 1]], values[indptr[r]:indptr[r + 1]])}


def pair_score(kind, agg, ucsr, nb_idx, nb_sim, u, i, fallback=None):
    """the prediction of user u for item i (or None) from the user-major CSR; fallback: means indexed by user (item KNN) / item (user KNN)"""
    terms = []
    if kind == 'item':
        rated = _row_dict(ucsr, u)
        for j, s in zip(nb_idx[i], nb_sim[i]):
            if j < 0:
                break
            if int(j) in rated:
                terms.append((s, rated[int(j)]))
    else:
        for v, s in zip(nb_idx[u], nb_sim[u]):
            if v < 0:
                break
            r = _row_dict(ucsr, int(v)).get(int(i))
            if r is not None:
                terms.append((s, r))
    value = aggregate(terms, agg)
    if value is None and fallback is not None:
        value = float(fallback[u if kind == 'item' else i])
    return value


def score_rows(kind, agg, ucsr, n_items, nb_idx, nb_sim, uids, fallback=None):
    """(out float32 [R, n_items], has bool [R, n_items]) for the users `uids`; fallback [n_users] (item KNN only): the user's value where an
    item has no term"""
    R = len(uids)
    out, has = np.zeros((R, n_items), np.float32), np.zeros((R, n_items), bool)
    for r, u in enumerate(uids):
        if kind == 'item':
            rated = _row_dict(ucsr, int(u))
            for i in range(n_items):
                if nb_idx[i, 0] < 0:
                    continue
                v = aggregate([(s, rated[int(j)]) for j, s in zip(nb_idx[i], nb_sim[i]) if j >= 0 and int(j) in rated], agg)
                if v is not None:
                    out[r, i], has[r, i] = np.float32(v), True
            if fallback is not None:
                out[r, ~has[r]], has[r] = np.float32(fallback[u]), True
        else:
            terms = {}
            for v, s in zip(nb_idx[u], nb_sim[u]):
                if v < 0:
                    break
                for c, x in _row_dict(ucsr, int(v)).items():
                    terms.setdefault(c, []).append((s, x))
            for c, t in terms.items():
                out[r, c], has[r, c] = np.float32(aggregate(t, agg)), True
    return out, has


def row_means(csr, R):
    indptr, _, values = csr
    out = np.zeros(R)
    for r in range(R):
        s = 0.0
        for x in values[indptr[r]:indptr[r + 1]]:
            s = s + float(x)
        out[r] = s / (indptr[r + 1] - indptr[r]) if indptr[r + 1] > indptr[r] else 0.0
    return out


def check_neighbours_against(S_ref, idx, sim, tol):
    """The tolerance rule: (i) every listed neighbour's similarity is within tol of the reference's value for that pair; (ii) every
    unlisted row has a reference similarity <= floor + tol, the floor being the list's last similarity if the list is full, else 0."""
    R, k = idx.shape
    for i in range(R):
        listed = [int(j) for j in idx[i] if j >= 0]
        assert len(set(listed)) == len(listed) and i not in listed, (i, listed)
        for t, j in enumerate(listed):
            assert abs(float(sim[i, t]) - float(S_ref[i, j])) <= tol, (i, j, float(sim[i, t]), float(S_ref[i, j]))
        floor = float(sim[i, k - 1]) if len(listed) == k else 0.0
        for j in range(R):
            if j != i and j not in listed:
                assert float(S_ref[i, j]) <= floor + tol, (i, j, float(S_ref[i, j]), floor)


def check_list_against(ref, got, bound):
    """A ranked list [(score, id)] against the reference's: the same ids, every score within `bound` of the reference's score for
    that id, and the order equal up to swaps among entries whose reference scores differ by less than `bound`."""
    assert len(ref) == len(got), (ref, got)
    ref_score = {int(i): float(s) for s, i in ref}
    assert sorted(ref_score) == sorted(int(i) for _, i in got), (ref, got)
    for t, (s, i) in enumerate(got):
        assert abs(float(s) - ref_score[int(i)]) <= bound, (t, s, i, ref_score[int(i)])
        assert abs(ref_score[int(i)] - float(ref[t][0])) <= bound, (t, i, ref, got)
