"""Bit identity of the engines' four query calls (recommend, rank_items, rank_lists, pair_scores) between two commits.

    python scripts/rows_query_ab.py --out a.json             # on each commit (needs a GPU): a sha256 per output tensor
    python scripts/rows_query_ab.py --compare a.json b.json  # anywhere: every digest equal, or the list of those that differ

Only the engines' public calls are used, so the same file runs in a checkout of an earlier commit.  A small CdaeEngine, DmfEngine and
CaserEngine from fixed seeds, exclusions set; every call at the default chunk and at chunks of 7, 37 and 64; every request with
duplicated users in permuted order, items outside the catalogue (-1 and n_items) and — rank_lists — rows with empty lists, among them
a run longer than the smallest chunk, and users that own several rows.  The empty requests' shapes and dtypes are recorded too.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

U, N, R = 100, 3000, 150
CHUNKS = (None, 7, 37, 64)


def csr_of(rows):
    ip = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return ip, np.concatenate(rows).astype(np.int32)


def histories(rng):
    return [np.sort(rng.choice(N, int(rng.integers(5, 60)), replace=False)) for _ in range(U)]


def cdae_engine():
    from drecpy_amd.engine import CdaeEngine
    rng, K = np.random.default_rng(101), 50
    eng = CdaeEngine(U, N, K)
    eng.set_params(W=rng.normal(0, 0.3, (N, K)), W_=rng.normal(0, 0.3, (K, N)), V=rng.normal(0, 0.3, (U, K)), b=rng.normal(0, 0.1, K),
                   b_=rng.normal(0, 0.3, N))
    ip, ix = csr_of(histories(rng))
    eng.set_history(ip, ix)
    eng.set_exclusions(ip, ix)
    return eng, ()


def dmf_engine():
    from drecpy_amd.engine_dmf import DmfEngine
    rng, factors = np.random.default_rng(102), (64, 32)
    rows = histories(rng)
    ip, ix = csr_of(rows)
    uid = np.repeat(np.arange(U), np.diff(ip))
    val = rng.integers(1, 6, len(ix)).astype(np.float64)
    order = np.lexsort((uid, ix))                                     # the transpose: by item, then user
    t_ip = np.concatenate([[0], np.cumsum(np.bincount(ix, minlength=N))]).astype(np.int64)
    p = {}
    for tower, n_in in (('u', N), ('i', U)):
        prev = n_in
        for l, f in enumerate(factors):
            p[f'{tower}{l}_k'] = rng.normal(0, 0.5, (prev, f)).astype(np.float32)
            p[f'{tower}{l}_b'] = rng.normal(-0.2, 0.1, f).astype(np.float32)
            prev = f
    eng = DmfEngine(U, N, list(factors), list(factors))
    eng.set_interactions((ip, ix, val), (t_ip, uid[order].astype(np.int32), val[order]))
    eng.set_params(p)
    eng.set_exclusions(ip, ix)
    return eng, ()


def caser_engine():
    from drecpy_amd.engine_caser import CaserEngine
    from oracle import caser_oracle as ca
    rng, L, d = np.random.default_rng(103), 5, 64
    p = ca.init_params(rng, U, N, L, d, 4, 16, np.float32)
    p['item_emb'] = rng.normal(0, 0.5, p['item_emb'].shape).astype(np.float32)
    p['user_emb'] = rng.normal(0, 0.5, p['user_emb'].shape).astype(np.float32)
    p['W1'] = rng.normal(0, 2.0 / np.sqrt(2 * d), p['W1'].shape).astype(np.float32)
    p['b1'] = rng.normal(0, 0.3, p['b1'].shape).astype(np.float32)
    eng = CaserEngine(U, N, L, 3, 3, d, 4, 16)
    eng.set_params(p)
    eng.set_exclusions(*csr_of(histories(rng)))
    return eng, (L,)


def requests(rng, query_width):
    """rows (duplicated users, permuted) with their per-row query arrays, one item per row, and a CSR of lists over the same rows"""
    uids = rng.permutation(np.concatenate([np.arange(U), rng.integers(0, U, R - U)])).astype(np.int32)
    query = [rng.integers(0, N, (R, w)).astype(np.int32) for w in query_width]
    items = rng.integers(0, N, R).astype(np.int32)
    items[rng.choice(R, 12, replace=False)] = np.tile([-1, N], 6)
    lists = [np.sort(rng.integers(0, N, int(rng.integers(0, 9)))) for _ in range(R)]
    for r in range(40, 49):                                            # a run of empty rows: whole chunks of 7 without a target
        lists[r] = lists[r][:0]
    lists[3] = np.concatenate([[-1], lists[3], [N]])                   # outside the catalogue, still ascending
    lists[R - 1] = np.sort(rng.choice(N, 70, replace=False))           # longer than any group: several walks
    indptr, targets = csr_of(lists)
    return uids, query, items, indptr, targets


def digest(t):
    a = t.cpu().numpy()
    return hashlib.sha256(a.tobytes()).hexdigest()


def describe(t):
    return f'{t.dtype} {list(t.shape)}'


def run():
    import torch
    out = {}
    for name, make in (('cdae', cdae_engine), ('dmf', dmf_engine), ('caser', caser_engine)):
        eng, query_width = make()
        uids, query, items, indptr, targets = requests(np.random.default_rng(7), query_width)
        res = out[name] = {}
        for chunk in CHUNKS:
            tag = 'default' if chunk is None else str(chunk)
            for excl in (None, False):
                idx, val = eng.recommend(uids, *query, 10, exclude=excl, chunk_users=chunk)
                res[f'recommend/exclude={excl}/{tag}'] = {'idx': digest(idx), 'val': digest(val)}
                rank, score = eng.rank_items(uids, *query, items, exclude=excl, chunk_rows=chunk)
                res[f'rank_items/exclude={excl}/{tag}'] = {'rank': digest(rank), 'score': digest(score)}
                rank, score = eng.rank_lists(uids, *query, indptr, targets, exclude=excl, chunk_rows=chunk)
                res[f'rank_lists/exclude={excl}/{tag}'] = {'rank': digest(rank), 'score': digest(score)}
            res[f'pair_scores/{tag}'] = {'score': digest(eng.pair_scores(uids, *query, items, chunk_pairs=chunk))}
        res['pair_scores/all outside'] = {'score': digest(eng.pair_scores(uids[:9], *[q[:9] for q in query], np.full(9, N, np.int32)))}
        none, no_query = np.zeros(0, np.int32), [q[:0] for q in query]
        res['empty'] = {'recommend': [describe(t) for t in eng.recommend(none, *no_query, 10)],
                        'rank_items': [describe(t) for t in eng.rank_items(none, *no_query, none)],
                        'rank_lists': [describe(t) for t in eng.rank_lists(none, *no_query, np.zeros(1, np.int64), none)],
                        'rank_lists with rows': [describe(t) for t in eng.rank_lists(uids[:2], *[q[:2] for q in query], np.zeros(3, np.int64), none)],
                        'pair_scores': [describe(eng.pair_scores(none, *no_query, none))]}
        torch.cuda.synchronize()
    return out


def differences(a, b, path=''):
    if isinstance(a, dict) and isinstance(b, dict):
        return [d for k in sorted(set(a) | set(b)) for d in differences(a.get(k), b.get(k), f'{path}/{k}')]
    return [] if a == b else [path]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out')
    ap.add_argument('--compare', nargs=2, metavar=('A', 'B'))
    args = ap.parse_args()
    if args.compare:
        a, b = (json.load(open(f)) for f in args.compare)
        diff = differences(a, b)
        n = sum(len(v) for side in a.values() for v in side.values())
        print(json.dumps({'digests': n, 'differ': diff}))
        sys.exit(1 if diff else 0)
    res = run()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({name: len(v) for name, v in res.items()}))


if __name__ == '__main__':
    main()
