"""NumPy restatement of what drx_knn_recommend / drx_knn_rank_lists select and count (include/drx.h), on top of
knn_oracle.score_rows: one row of float32 predictions `scores` [n_items], `has` [n_items] (the items with a prediction) and the
user's exclusion row.  Order is drx_topk's: descending prediction, ties to the larger item id — heapq.nlargest over (score, iid).
No GPU, no reference import."""
import numpy as np


def full_keys(scores):
    """uint64 [n_items]: (ordered float32 bits << 32 | item), -0.0 carried as +0.0: a larger key stands earlier in the list"""
    s = np.ascontiguousarray(scores, np.float32).copy()
    s[s == 0] = 0.0
    u = s.view(np.uint32)
    bits = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint64)
    return (bits << np.uint64(32)) | np.arange(len(s), dtype=np.uint64)


def eligible(has, excl_row, n_items):
    ok = np.asarray(has, bool).copy()
    if excl_row is not None:
        x = np.asarray(excl_row, np.int64)
        ok[x[(x >= 0) & (x < n_items)]] = False
    return ok


def topn(scores, has, excl_row, n):
    """(idx int32 [n], val float32 [n]): the n best eligible items, -1 / -inf behind the last one"""
    N = len(scores)
    keys = full_keys(scores)
    items = np.flatnonzero(eligible(has, excl_row, N))
    best = items[np.argsort(keys[items])[::-1]][:n]
    idx, val = np.full(n, -1, np.int32), np.full(n, -np.inf, np.float32)
    idx[:len(best)] = best
    val[:len(best)] = np.asarray(scores, np.float32)[best]
    val[:len(best)][val[:len(best)] == 0] = 0.0
    return idx, val


def ranks(scores, has, excl_row, targets):
    """(rank int32 [T], score float32 [T]): the number of eligible items other than the target ahead of it — its position in topn's
    list with n unbounded, the target's own exclusion ignored —; -1 / -inf for a target outside the row or without a prediction"""
    N = len(scores)
    keys = full_keys(scores)
    ok = eligible(has, excl_row, N)
    rank, score = np.full(len(targets), -1, np.int32), np.full(len(targets), -np.inf, np.float32)
    for p, t in enumerate(targets):
        t = int(t)
        if not 0 <= t < N or not has[t]:
            continue
        ahead = ok & (keys > keys[t])
        ahead[t] = False
        rank[p] = int(ahead.sum())
        score[p] = np.float32(0.0) if scores[t] == 0 else np.float32(scores[t])
    return rank, score
