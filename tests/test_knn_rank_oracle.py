"""tests/knn_rank_oracle.py against brute force: heapq.nlargest over (score, iid) and positions in that list, on random rows with
many ties.  No GPU."""
from heapq import nlargest

import numpy as np
import pytest

import knn_rank_oracle as kro


def _row(seed, N):
    rng = np.random.default_rng(seed)
    scores = rng.choice(np.array([-1.5, -0.0, 0.0, 0.5, 1.0, 2.25, 3.0, 4.5], np.float32), N)     # few values: many ties
    has = rng.random(N) < 0.7
    excl = np.flatnonzero(rng.random(N) < 0.3)
    return scores, has, excl


def _listed(scores, has, excl):
    out = set(excl.tolist()) if excl is not None else set()
    return nlargest(len(scores), ((float(scores[i]), i) for i in range(len(scores)) if has[i] and i not in out))


@pytest.mark.parametrize('seed,N', [(1, 1), (2, 7), (3, 64), (4, 65), (5, 300)])
@pytest.mark.parametrize('with_excl', [False, True])
def test_topn_is_nlargest(seed, N, with_excl):
    scores, has, excl = _row(seed, N)
    excl = excl if with_excl else None
    want = _listed(scores, has, excl)
    for n in (1, 3, N, N + 5):
        idx, val = kro.topn(scores, has, excl, n)
        assert idx.dtype == np.int32 and val.dtype == np.float32 and len(idx) == len(val) == n
        k = min(n, len(want))
        assert idx[:k].tolist() == [i for _, i in want[:k]]
        assert val[:k].tolist() == [s for s, _ in want[:k]] and not np.signbit(val[:k][val[:k] == 0]).any()
        assert (idx[k:] == -1).all() and np.isneginf(val[k:]).all()


@pytest.mark.parametrize('seed,N', [(6, 1), (7, 9), (8, 64), (9, 130)])
def test_ranks_are_list_positions(seed, N):
    scores, has, excl = _row(seed, N)
    rng = np.random.default_rng(seed + 100)
    targets = np.concatenate([rng.integers(0, N, 40), [-1, N, 0, 0]])
    for x in (None, excl):
        rank, score = kro.ranks(scores, has, x, targets)
        out = set(x.tolist()) if x is not None else set()
        for p, t in enumerate(targets.tolist()):
            if not 0 <= t < N or not has[t]:
                assert rank[p] == -1 and np.isneginf(score[p])
                continue
            # the target's own exclusion is ignored: its position in the list of the others plus itself
            listed = nlargest(N, ((float(scores[i]), i) for i in range(N) if has[i] and (i == t or i not in out)))
            assert listed[rank[p]][1] == t and score[p] == scores[t]


def test_unbounded_list_and_ranks_agree():
    scores, has, excl = _row(11, 90)
    idx, _ = kro.topn(scores, has, excl, 90)
    rank, _ = kro.ranks(scores, has, excl, np.arange(90))
    for i in range(90):
        at = np.flatnonzero(idx == i)
        if len(at):
            assert rank[i] == at[0]
        else:
            assert not has[i] or i in excl
