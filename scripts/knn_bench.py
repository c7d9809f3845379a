"""Device time of the KNN baselines' neighbour table and of one recommend_batch, on the synthetic MovieLens-shaped sets.

    python scripts/knn_bench.py [--type user|item] [--shape ml-100k|ml-1m] [--metric adjusted_cosine] [--k 20] [--out profiles/knn_neighbours.json]
    python scripts/knn_bench.py --mode recommend [--out profiles/knn_recommend.json]        (both types x both shapes in one process)

Timed by HIP events on the stream the calls run on, after warm-up calls; median, min and max over the repetitions:
  neighbours        one drx_knn_neighbours call (memset + scatter + row statistics + the MFMA tile walk + the merge), scratch allocated
                    outside the timed region;
  recommend_batch   model.recommend_batch(2048 users, n = 10) on the score-matrix route (engine.fused = False): drx_knn_score_rows +
                    drx_topk per chunk, with the host work between them (device events and wall clock side by side).
The MFMA rate counts the products the tile walk issues: (R up to 32)^2 x (C up to 8) x 2 FLOP per sum the metric reads — the full
square, both triangles.  At the ml-100k shape the NumPy oracle (tests/knn_oracle.py: float32 matrix products, float64 epilogue,
a Python nlargest per row) is timed once as context.  The result is merged into the output file under "<type>/<shape>/<metric>".

--mode recommend: the fused routes (drx_knn_recommend / drx_knn_rank_lists) against the routes they replace, in ONE process and
alternating, host wall time around the public call (which ends in the download of its result), median (min - max) of --reps after
a warm-up call of each:
  recommend_batch   model.recommend_batch(943 / 2048 users, n = 10, as_arrays=True): fused, and with engine.fused = False the
                    score-matrix route (host mask, drx_knn_score_rows, drx_topk, a Python loop per entry); hook_wall_ms: the same
                    two routes at the hook the public call stands on (BaseKNN._recommend_batch: internal ids in, arrays out),
                    without the public call's id mapping and list building, which both routes share;
  catalogue_ranks   model.catalogue_ranks(256 users x 10 seeded items each): fused, and RecommenderABC._catalogue_ranks bound in its
                    place (one _recommend(uid, n_items) and a Python dict per distinct user).
Both routes' results are compared (they must be equal); one entry per "<type>/<shape>" goes into the output file."""
import argparse
import json
import os
import sys
import time
from statistics import median

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N_SUMS = {'cosine': 2, 'adjusted_cosine': 4, 'cosine_cf': 4, 'jaccard': 1, 'msd': 4, 'pearson': 6}


def events_ms(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    ms, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(e0.elapsed_time(e1))
    return {'device_ms': {'median': median(ms), 'min': min(ms), 'max': max(ms)}, 'wall_ms': {'median': median(wall), 'min': min(wall)},
            'reps': reps, 'warmup': warmup}


def alternating_wall_ms(fns, reps):
    """{name: {'median', 'min', 'max'}} of the host wall time of each callable, taken in turns after one warm-up call of each"""
    import torch
    for fn in fns.values():
        fn()
    wall = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    return {name: {'median': median(w), 'min': min(w), 'max': max(w)} for name, w in wall.items()}


def recommend_mode(a):
    import types
    import torch
    from drecpy_amd import synth
    from drecpy_amd.Recommender import RecommenderABC
    from drecpy_amd.Recommender.Baseline import ItemKNN, UserKNN
    doc = {}
    for shape in ('ml-100k', 'ml-1m'):
        ds = synth.dataset(shape, with_timestamp=False)
        for kind in ('item', 'user'):
            model = (UserKNN if kind == 'user' else ItemKNN)(k=a.k, m=5, sim_metric=a.metric, shrinkage=100, verbose=False)
            model.fit(ds)
            eng, mds = model._engine, model.interaction_dataset
            users = [mds.uid_to_user(u) for u in range(min(2048, eng.n_users))]
            rng = np.random.default_rng(7)
            pair_users = [u for u in users[:256] for _ in range(10)]
            pair_items = [mds.iid_to_item(int(i)) for i in rng.integers(0, eng.n_items, len(pair_users))]
            got = {}

            def batch(fused):
                eng.fused = fused
                got['batch', fused] = model.recommend_batch(users, n=10, as_arrays=True)
                eng.fused = True

            def ranks(fused):
                if not fused:
                    model._catalogue_ranks = types.MethodType(RecommenderABC._catalogue_ranks, model)
                got['ranks', fused] = model.catalogue_ranks(pair_users, pair_items, return_scores=True)
                if not fused:
                    del model._catalogue_ranks
            res = {'type': kind, 'shape': shape, 'metric': a.metric, 'k': a.k, 'n_users': eng.n_users, 'n_items': eng.n_items,
                   'device': torch.cuda.get_device_name(0), 'reps': a.reps,
                   'timed': 'host wall ms around the public call, the two routes in turns in one process after a warm-up call of each'}
            t = alternating_wall_ms({'fused': lambda: batch(True), 'score_matrix': lambda: batch(False)}, a.reps)
            res['recommend_batch'] = {'users': len(users), 'n': 10, 'wall_ms': t,
                                      'equal': all(np.array_equal(x, y) for x, y in zip(got['batch', True], got['batch', False]))}
            uids = np.arange(len(users), dtype=np.int64)

            def hook(fused):
                eng.fused = fused
                got['hook', fused] = model._recommend_batch(uids, 10, True)
                eng.fused = True
            res['recommend_batch']['hook_wall_ms'] = alternating_wall_ms({'fused': lambda: hook(True), 'score_matrix': lambda: hook(False)}, a.reps)
            res['recommend_batch']['equal'] &= all(np.array_equal(x, y) for x, y in zip(got['hook', True], got['hook', False]))
            t = alternating_wall_ms({'fused': lambda: ranks(True), 'base_class': lambda: ranks(False)}, a.reps)
            res['catalogue_ranks'] = {'users': 256, 'pairs': len(pair_users), 'wall_ms': t,
                                      'equal': all(np.array_equal(x, y) for x, y in zip(got['ranks', True], got['ranks', False]))}
            assert res['recommend_batch']['equal'] and res['catalogue_ranks']['equal'], res
            doc[f'{kind}/{shape}'] = res
            print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('{\n' + ',\n'.join(f' {json.dumps(k)}: {json.dumps(v, sort_keys=True)}' for k, v in sorted(doc.items())) + '\n}\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['neighbours', 'recommend'], default='neighbours')
    ap.add_argument('--type', choices=['user', 'item'], default='item')
    ap.add_argument('--shape', choices=['ml-100k', 'ml-1m'], default='ml-100k')
    ap.add_argument('--metric', default='adjusted_cosine')
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, 'profiles', 'knn_neighbours.json' if a.mode == 'neighbours' else 'knn_recommend.json')
    if a.mode == 'recommend':
        return recommend_mode(a)

    import torch
    from drecpy_amd import _lib, synth
    from drecpy_amd.Recommender.Baseline import ItemKNN, UserKNN
    L = _lib.lib()
    ds = synth.dataset(a.shape, with_timestamp=False)
    model = (UserKNN if a.type == 'user' else ItemKNN)(k=a.k, m=5, sim_metric=a.metric, shrinkage=100, verbose=False)
    t0 = time.perf_counter()
    model.fit(ds)
    fit_s = time.perf_counter() - t0
    eng = model._engine
    d_csr, R, C = (eng._u, eng.n_users, eng.n_items) if a.type == 'user' else (eng._i, eng.n_items, eng.n_users)
    need = int(L.drx_knn_neighbours_scratch_bytes(R, C, a.k, 0))
    scratch = torch.empty(need, dtype=torch.uint8, device=eng.device)
    idx = torch.empty(R, a.k, dtype=torch.int32, device=eng.device)
    sim = torch.empty(R, a.k, dtype=torch.float32, device=eng.device)
    st = _lib.stream_ptr(eng.device)

    def neighbours():
        _lib.check(L.drx_knn_neighbours(_lib.ptr(d_csr[0]), _lib.ptr(d_csr[1]), _lib.ptr(d_csr[2]), d_csr[3], R, C, _lib.KNN_METRICS[a.metric],
                                        a.k, 5, 100.0, 5.0, 0, _lib.ptr(idx), _lib.ptr(sim), _lib.ptr(scratch), need, st), 'drx_knn_neighbours')
    res = {'type': a.type, 'shape': a.shape, 'metric': a.metric, 'k': a.k, 'rows': R, 'columns': C, 'nnz': d_csr[3],
           'device': torch.cuda.get_device_name(0), 'scratch_bytes': need, 'fit_wall_s': fit_s,
           'timed': 'HIP events around the call on its stream after warm-up; median / min / max over the repetitions'}
    res['neighbours'] = events_ms(neighbours, 2, a.reps)
    flop = float((R + 31) // 32 * 32) ** 2 * ((C + 7) // 8 * 8) * 2 * N_SUMS[a.metric]
    res['neighbours']['mfma_flop'] = flop
    res['neighbours']['mfma_tflops_at_median'] = flop / (res['neighbours']['device_ms']['median'] * 1e-3) / 1e12
    assert torch.equal(idx, eng.nb_idx) and torch.equal(sim, eng.nb_sim)                # the timed call computes the model's table

    users = [model.interaction_dataset.uid_to_user(u) for u in range(min(2048, eng.n_users))]
    eng.fused = False                                                                   # (the fused route: --mode recommend)
    res['recommend_batch'] = events_ms(lambda: model.recommend_batch(users, n=10, as_arrays=True), 1, max(3, a.reps // 2))
    res['recommend_batch']['users'] = len(users)

    if a.shape == 'ml-100k':
        import knn_oracle as ko
        csr = ds.interaction_csr(transpose=a.type == 'item')
        csr = (np.asarray(csr[0], np.int64), np.asarray(csr[1], np.int32), np.asarray(csr[2], np.float32))
        t0 = time.perf_counter()
        o_idx, o_sim = ko.neighbours(ko.similarities(csr, R, C, a.metric, 5, 100, max_diff=5.0), a.k)
        res['cpu_oracle_wall_s'] = time.perf_counter() - t0
        res['equals_cpu_oracle'] = bool(np.array_equal(o_idx, idx.cpu().numpy()) and np.array_equal(o_sim, sim.cpu().numpy()))

    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc[f'{a.type}/{a.shape}/{a.metric}'] = res
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('{\n' + ',\n'.join(f' {json.dumps(k)}: {json.dumps(v, sort_keys=True)}' for k, v in sorted(doc.items())) + '\n}\n')   # a line per run
    print(json.dumps(res))


if __name__ == '__main__':
    main()
