"""Writes tests/golden/knn.json and knn.npz from the reference's UserKNN / ItemKNN (dev container only: oracle/ref_import.py imports
the reference; nothing at test time does).  Data only: the frame, and what the reference computes on it.

    python scripts/gen_golden_knn.py            # rewrites both files, byte for byte the same every time

(a) knn.npz — the frame, and for both classes x six metrics x the settings (k, m, shrinkage) in SETTINGS (in that order)
    `_similarities` as the lower triangle of the symmetric matrix in internal ids (row i > j, 0 where absent) in fixed point,
    int32 of s x 2^30 (similarities lie in [-1, 1]; the step is 1e-9, the gate of the tests 1e-6), and the ids of `_neighbours`
    (-1 behind a list's end; their similarities are in the matrix).
(b) For the configurations whose neighbour lists are unambiguous (no similarity below 1e-9, no gap below 1e-6 between adjacent
    entries or at the k boundary — asserted here per recorded configuration): predict() over a grid of pairs, rank() for a few
    users and recommend(n=5) with novelty on and off, for a choice of aggregations and use_averages."""
import io
import json
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

N_USERS, N_ITEMS, DENSITY, SEED = 70, 37, 0.35, 20
METRICS = ('cosine', 'adjusted_cosine', 'cosine_cf', 'jaccard', 'msd', 'pearson')
SETTINGS = ((5, 2, 10), (20, 5, 100), (3, 0, None))
GRID_USERS, GRID_ITEMS = range(0, N_USERS, 7), range(0, N_ITEMS, 5)
LIST_USERS = (3, 31, 64)


def frame():
    """unique (user, item) pairs, ratings 1..5, rows shuffled so that internal ids differ from the raw order"""
    rng = np.random.default_rng(SEED)
    cells = np.flatnonzero(rng.random(N_USERS * N_ITEMS) < DENSITY)
    rng.shuffle(cells)
    return {'user': [int(100 + c // N_ITEMS) for c in cells], 'item': [int(500 + c % N_ITEMS) for c in cells],
            'interaction': [int(v) for v in rng.integers(1, 6, size=len(cells))]}


def lower_triangle(sims, n):
    return np.round(np.array([sims.get(i, {}).get(j, 0) for i in range(n) for j in range(i)], np.float64) * 2.0 ** 30).astype(np.int32)


def write_npz(path, arrays):
    """np.load reads it; fixed member dates, so the file is the same bytes every time"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + '.npy', (1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def unambiguous(model, n, k):
    """every list: similarities >= 1e-9, gaps >= 1e-6 between adjacent entries and to the best row left out"""
    for i in range(n):
        listed = model._neighbours[i]
        sims = [s for s, _ in listed]
        if any(s < 1e-9 for s in sims) or any(a - b < 1e-6 for a, b in zip(sims, sims[1:])):
            return False
        ids = {j for _, j in listed}
        rest = [model._get_sim(i, j) for j in range(n) if j != i and j not in ids]
        rest = [s for s in rest if s is not None and s > 0]
        if len(listed) == k and rest and sims[-1] - max(rest) < 1e-6:
            return False
        if any(0 < s < 1e-9 for s in rest):
            return False
    return True


def main():
    from ref_import import import_reference
    import_reference()
    import pandas as pd
    from DRecPy.Dataset import InteractionDataset
    from DRecPy.Recommender.Baseline import ItemKNN, UserKNN

    fr = frame()
    out = {'settings': [list(s) for s in SETTINGS], 'metrics': list(METRICS), 'predictions': []}
    arrays = {'frame': np.array([fr['user'], fr['item'], fr['interaction']], np.int32)}
    lower, lists = {'user': [], 'item': []}, {'user': [], 'item': []}
    users, items = sorted(set(fr['user'])), sorted(set(fr['item']))
    grid = [(users[u], items[i]) for u in GRID_USERS for i in GRID_ITEMS]
    rank_items = [items[i] for i in range(0, N_ITEMS, 2)]
    qualified = {'user': [], 'item': []}
    for kind, cls in (('user', UserKNN), ('item', ItemKNN)):
        for metric in METRICS:
            for k, m, shrinkage in SETTINGS:
                ds = InteractionDataset.read_df(pd.DataFrame(fr), verbose=False)
                model = cls(k=k, m=m, sim_metric=metric, shrinkage=shrinkage, verbose=False)
                model.fit(ds)
                n = model.n_users if kind == 'user' else model.n_items
                lower[kind].append(lower_triangle(model._similarities, n))
                ids = np.full((n, max(s[0] for s in SETTINGS)), -1, np.int16)
                for i in range(n):
                    ids[i, :len(model._neighbours[i])] = [j for _, j in model._neighbours[i]]
                lists[kind].append(ids)
                if unambiguous(model, n, k):
                    qualified[kind].append((metric, k, m, shrinkage))
    out['qualified'] = {kind: [list(q) for q in qs] for kind, qs in qualified.items()}
    for kind, cls in (('user', UserKNN), ('item', ItemKNN)):
        qs = qualified[kind]
        assert len(qs) >= 2, f'{kind}: fewer than two unambiguous configurations'
        picks = [(qs[0], 'weighted_mean', False), (qs[1], 'mean', False), (qs[-1], 'mean', True)]
        for (metric, k, m, shrinkage), aggregation, use_averages in picks:
            ds = InteractionDataset.read_df(pd.DataFrame(fr), verbose=False)
            model = cls(k=k, m=m, sim_metric=metric, shrinkage=shrinkage, aggregation=aggregation, use_averages=use_averages, verbose=False)
            model.fit(ds)
            assert unambiguous(model, model.n_users if kind == 'user' else model.n_items, k)
            rec = {'type': kind, 'metric': metric, 'k': k, 'm': m, 'shrinkage': shrinkage, 'aggregation': aggregation,
                   'use_averages': use_averages, 'predict': [model.predict(u, i, skip_errors=True) for u, i in grid], 'rank': {}, 'recommend': {}}
            for u in LIST_USERS:
                user = users[u]
                rec['rank'][str(user)] = [[float(s), int(i)] for s, i in model.rank(user, rank_items, novelty=False)]
                rec['recommend'][str(user)] = {str(nov): [[float(s), int(i)] for s, i in model.recommend(user, n=5, novelty=nov)]
                                               for nov in (True, False)}
            out['predictions'].append(rec)
    out['pairs'], out['rank_items'] = [list(p) for p in grid], rank_items
    for kind in ('user', 'item'):
        arrays['lower_' + kind], arrays['neighbours_' + kind] = np.stack(lower[kind]), np.stack(lists[kind])
    path = os.path.join(ROOT, 'tests', 'golden', 'knn')
    write_npz(path + '.npz', arrays)
    with open(path + '.json', 'w') as f:
        json.dump(out, f, separators=(',', ':'))
        f.write('\n')
    print({e: os.path.getsize(path + e) for e in ('.json', '.npz')}, 'bytes;', {k: len(v) for k, v in qualified.items()}, 'qualified')


if __name__ == '__main__':
    main()
