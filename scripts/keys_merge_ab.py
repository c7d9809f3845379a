"""The calls that end in the shared ordering network (csrc/drx_keys.hpp: order_keys_desc, k_lists_merge), timed for ONE build of the
library; run once on the parent commit's build and once on the tree's in the same job, then compared.

    python scripts/keys_merge_ab.py [--lib path/to/libdrx.so] --out one_build.json
    python scripts/keys_merge_ab.py --compare parent.json tree.json --out profiles/keys_merge_ab.json

  topk_lds            drx_topk, 2048 rows x 3706 scores, k = 100: k_topk_lds (k above the one-wave selection's 64)
  topk_select_order   drx_topk, 64 rows x 100 000 scores, k = 1000: k_topk_select + k_topk_order
  recommend_1m        drx_rows_recommend on CDAE hidden rows, N = 1 M, R = 16 384, K = 128, n = 10: k_recommend + the merge
  recommend_ml1m      the same at N = 3706, R = 6040
  knn_neighbours      drx_knn_neighbours, ItemKNN on the synthetic ml-100k set, adjusted cosine, k = 20 (scripts/knn_bench.py's shape)
HIP events around the library call alone, one warm-up call, median and min of 20 calls (recommend_bench.spread_ms).  --compare: a tree
median passes if it is no more than the parent's median plus the spread, the sum of the two series' min-to-median distances."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
REPS = 20


def measure(lib_path):
    import torch
    from drecpy_amd import _lib
    if lib_path:
        _lib.LIB_PATH = os.path.abspath(lib_path)
    import recommend_bench as rb
    L, dev = _lib.lib(), torch.device('cuda:0')
    st = _lib.stream_ptr(dev)
    res = {'library': os.path.relpath(_lib.LIB_PATH, ROOT), 'device': torch.cuda.get_device_name(0)}

    def topk(R, n, k):
        g = torch.Generator(device=dev).manual_seed(R + n)
        scores = torch.randn(R, n, generator=g, device=dev)
        oi, ov = torch.empty(R, k, dtype=torch.int32, device=dev), torch.empty(R, k, device=dev)
        sb = int(L.drx_topk_scratch_bytes_k(R, n, k))
        sc = torch.empty(max(sb, 16), dtype=torch.uint8, device=dev)
        return rb.spread_ms(lambda: _lib.check(L.drx_topk(_lib.ptr(scores), None, R, n, k, _lib.ptr(oi), _lib.ptr(ov), _lib.ptr(sc) if sb else None,
                                                           sb, st), 'drx_topk'), REPS)
    with rb.step(120):
        res['topk_lds'] = topk(2048, 3706, 100)
        res['topk_select_order'] = topk(64, 100_000, 1000)
    print(res, flush=True)

    for name, N, R in (('recommend_ml1m', 3706, 6040), ('recommend_1m', 1_000_000, 16384)):
        with rb.step(400):
            eng, _, _ = rb.cdae_engine(R, N, 128)
            uid = torch.arange(R, dtype=torch.int32, device=dev)
            h, x, n = eng._hidden_rows(uid), eng._excl, 10
            oi, ov = torch.empty(R, n, dtype=torch.int32, device=dev), torch.empty(R, n, device=dev)
            sb = int(L.drx_rows_recommend_scratch_bytes(R, N, eng.ld, n))
            sc = torch.empty(sb, dtype=torch.uint8, device=dev)
            res[name] = rb.spread_ms(lambda: _lib.check(L.drx_rows_recommend(
                _lib.ptr(eng.W2T), _lib.ptr(eng.b2), N, eng.ld, _lib.DRX_REC_SIGMOID_BIAS, _lib.ptr(h), _lib.ptr(uid), R, n, _lib.ptr(x[0]),
                _lib.ptr(x[1]), _lib.ptr(oi), _lib.ptr(ov), _lib.ptr(sc), sb, st), 'drx_rows_recommend'), REPS)
            del eng, h, sc
        print(name, res[name], flush=True)

    with rb.step(300):
        from drecpy_amd import synth
        from drecpy_amd.Recommender.Baseline import ItemKNN
        model = ItemKNN(k=20, m=5, sim_metric='adjusted_cosine', shrinkage=100, verbose=False)
        model.fit(synth.dataset('ml-100k', with_timestamp=False))
        eng = model._engine
        csr, R, C = eng._i, eng.n_items, eng.n_users
        need = int(L.drx_knn_neighbours_scratch_bytes(R, C, 20, 0))
        sc = torch.empty(need, dtype=torch.uint8, device=dev)
        idx, sim = torch.empty(R, 20, dtype=torch.int32, device=dev), torch.empty(R, 20, device=dev)
        res['knn_neighbours'] = rb.spread_ms(lambda: _lib.check(L.drx_knn_neighbours(
            _lib.ptr(csr[0]), _lib.ptr(csr[1]), _lib.ptr(csr[2]), csr[3], R, C, _lib.KNN_METRICS['adjusted_cosine'], 20, 5, 100.0, 5.0, 0,
            _lib.ptr(idx), _lib.ptr(sim), _lib.ptr(sc), need, st), 'drx_knn_neighbours'), REPS)
        assert torch.equal(idx, eng.nb_idx) and torch.equal(sim, eng.nb_sim)
    print('knn_neighbours', res['knn_neighbours'], flush=True)
    return res


def compare(parent, tree):
    parent.pop('library', None), tree.pop('library', None)        # (where each build lay during the job)
    out = {'timed': 'HIP events around the library call, median and min of 20 calls after a warm-up call, both builds in one job',
           'rule': 'tree median <= parent median + (parent median - parent min) + (tree median - tree min)', 'parent': parent, 'tree': tree,
           'verdict': {}}
    for name, p in parent.items():
        if isinstance(p, dict):
            t = tree[name]
            limit = p['median_ms'] + (p['median_ms'] - p['min_ms']) + (t['median_ms'] - t['min_ms'])
            out['verdict'][name] = {'limit_ms': limit, 'tree_median_ms': t['median_ms'], 'passes': t['median_ms'] <= limit}
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None)
    ap.add_argument('--compare', nargs=2, metavar=('PARENT.json', 'TREE.json'))
    ap.add_argument('--out', required=True)
    a = ap.parse_args()
    doc = compare(*(json.load(open(f)) for f in a.compare)) if a.compare else measure(a.lib)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(doc.get('verdict', doc)))
