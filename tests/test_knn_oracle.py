"""The KNN baselines without a GPU: the NumPy oracle (tests/knn_oracle.py) against what the reference computed on the fixture frame
(tests/golden/knn.json, scripts/gen_golden_knn.py); include/drx.h and the bindings agree on the drx_knn_* entry points; the
constructor's errors; fit() refusing a frame outside the domain before it touches a device."""
import json
import os
import re

import numpy as np
import pytest

import knn_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-6                      # similarities lie in [-1, 1]


def load_golden():
    """knn.json (settings, predictions, lists) and knn.npz (the frame, the similarity matrices in fixed point, the neighbour ids) as one
    dict: g['similarities'] holds one entry per class x metric x setting, in the generator's order"""
    with open(os.path.join(ROOT, 'tests', 'golden', 'knn.json')) as f:
        g = json.load(f)
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'knn.npz'))
    g['frame'] = dict(zip(('user', 'item', 'interaction'), z['frame'].tolist()))
    g['similarities'] = []
    for kind in ('user', 'item'):
        configs = [(me, k, m, s) for me in g['metrics'] for k, m, s in g['settings']]
        for (me, k, m, s), lower, ids in zip(configs, z['lower_' + kind], z['neighbours_' + kind]):
            g['similarities'].append({'type': kind, 'metric': me, 'k': k, 'm': m, 'shrinkage': s, 'lower': lower / 2.0 ** 30,
                                      'neighbours': [[int(j) for j in row if j >= 0] for row in ids]})
    return g


def golden_dataset(g):
    from drecpy_amd.Dataset import InteractionDataset
    fr = g['frame']
    ds = InteractionDataset.read_df({'user': np.array(fr['user']), 'item': np.array(fr['item']),
                                     'interaction': np.array(fr['interaction'], dtype=np.float64)}, verbose=False)
    ds.assign_internal_ids()
    return ds


def csr32(csr):
    return np.asarray(csr[0], np.int64), np.asarray(csr[1], np.int32), np.asarray(csr[2], np.float32)


def reference_matrix(lower, n):
    S = np.zeros((n, n))
    S[np.tril_indices(n, -1)] = lower
    return S + S.T


@pytest.fixture(scope='module')
def golden():
    g = load_golden()
    ds = golden_dataset(g)
    U, N = ds.count_unique('uid'), ds.count_unique('iid')
    return g, ds, {'user': (csr32(ds.interaction_csr()), U, N), 'item': (csr32(ds.interaction_csr(transpose=True)), N, U)}


def test_the_fixture_covers_what_it_should(golden):
    g, _, _ = golden
    seen = {(c['type'], c['metric'], c['k'], c['m'], c['shrinkage']) for c in g['similarities']}
    assert seen == {(t, me, k, m, s) for t in ('user', 'item') for me in ko.METRICS for k, m, s in ((5, 2, 10), (20, 5, 100), (3, 0, None))}
    preds = g['predictions']
    for kind in ('user', 'item'):
        assert {p['aggregation'] for p in preds if p['type'] == kind} == {'mean', 'weighted_mean'}
        assert any(p['use_averages'] for p in preds if p['type'] == kind)
        assert all([p['metric'], p['k'], p['m'], p['shrinkage']] in g['qualified'][kind] for p in preds if p['type'] == kind)
    assert any(v is None for p in preds for v in p['predict'])


def test_similarities_and_neighbours_against_the_reference(golden):
    g, _, mats = golden
    worst = {}
    for c in g['similarities']:
        csr, R, C = mats[c['type']]
        S_ref = reference_matrix(c['lower'], R)
        raw = ko.similarities(csr, R, C, c['metric'], c['m'], c['shrinkage'], raw=True)
        err = float(np.max(np.abs(raw - S_ref)))
        worst[c['metric']] = max(worst.get(c['metric'], 0.0), err)
        assert err <= TOL, (c['type'], c['metric'], c['k'], err)
        idx, sim = ko.neighbours(ko.similarities(csr, R, C, c['metric'], c['m'], c['shrinkage']), c['k'])
        ko.check_neighbours_against(S_ref, idx, sim, TOL)
        if [c['metric'], c['k'], c['m'], c['shrinkage']] in g['qualified'][c['type']]:       # unambiguous lists: id for id
            assert [[int(j) for j in row if j >= 0] for row in idx] == c['neighbours']
    print('max |oracle - reference| per metric:', worst)


def test_the_reference_passes_its_own_rule(golden):
    g, _, mats = golden
    for c in g['similarities']:
        R = mats[c['type']][1]
        S_ref = reference_matrix(c['lower'], R)
        idx = np.full((R, c['k']), -1, np.int32)
        sim = np.zeros((R, c['k']), np.float32)
        for i, row in enumerate(c['neighbours']):
            idx[i, :len(row)] = row
            sim[i, :len(row)] = [S_ref[i, j] for j in row]
        ko.check_neighbours_against(S_ref, idx, sim, TOL)


def test_predictions_and_lists_against_the_reference(golden):
    g, ds, mats = golden
    ucsr, U, N = mats['user']
    bound = TOL * float(max(g['frame']['interaction']))
    for p in g['predictions']:
        csr, R, C = mats[p['type']]
        idx, sim = ko.neighbours(ko.similarities(csr, R, C, p['metric'], p['m'], p['shrinkage']), p['k'])
        fb = None
        if p['use_averages']:
            fb = ko.row_means(ucsr, U) if p['type'] == 'item' else ko.row_means(mats['item'][0], N)
        for (user, item), want in zip(g['pairs'], p['predict']):
            got = ko.pair_score(p['type'], p['aggregation'], ucsr, idx, sim, ds.user_to_uid(user), ds.item_to_iid(item), fb)
            assert (got is None) == (want is None), (p['type'], p['metric'], user, item, got, want)
            assert got is None or abs(got - want) <= bound, (p['type'], p['metric'], user, item, got, want)
        # rank() and recommend() from the oracle's score rows
        for user, ref in p['rank'].items():
            uid = ds.user_to_uid(int(user))
            out, has = ko.score_rows(p['type'], p['aggregation'], ucsr, N, idx, sim, [uid], fb if p['type'] == 'item' else None)
            cand = [ds.item_to_iid(i) for i in g['rank_items']]
            got = sorted(((float(out[0, i]), i) for i in cand if has[0, i]), reverse=True)
            ko.check_list_against([(s, ds.item_to_iid(i)) for s, i in ref], got, bound)
            rated = set(ucsr[1][ucsr[0][uid]:ucsr[0][uid + 1]].tolist())
            for novelty, ref5 in p['recommend'][user].items():
                pool = [i for i in range(N) if has[0, i] and not (novelty == 'True' and i in rated)]
                got = sorted(((float(out[0, i]), i) for i in pool), reverse=True)[:5]
                ko.check_list_against([(s, ds.item_to_iid(i)) for s, i in ref5], got, bound)


# ---- binding -------------------------------------------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, 'include', 'drx.h')) as f:
        return re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)


def _n_args(header, name):
    m = re.search(r'\b' + name + r'\s*\(([^;]*?)\)\s*;', header, flags=re.S)
    assert m, f'{name} is not declared in include/drx.h'
    return len([a for a in m.group(1).split(',') if a.strip()])


@pytest.mark.parametrize('name,n,wide', [('drx_knn_neighbours', 17, [3]), ('drx_knn_score_rows', 19, [5]), ('drx_knn_pair_scores', 18, [5, 13]),
                                          ('drx_knn_neighbours_scratch_bytes', 4, []), ('drx_knn_score_rows_scratch_bytes', 3, []),
                                          ('drx_knn_row_means', 6, [2])])
def test_header_and_bindings_agree(name, n, wide):
    import ctypes as C
    from drecpy_amd import _lib
    assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    assert _n_args(_header(), name) == len(args) == n
    assert res is (C.c_size_t if name.endswith('_bytes') else C.c_int)
    assert [j for j, a in enumerate(args) if a is C.c_int64] == wide            # nnz and P are the 64-bit counts
    if name == 'drx_knn_neighbours':
        assert [j for j, a in enumerate(args) if a is C.c_double] == [9, 10]     # shrinkage, max_diff


def test_the_metric_codes_match_the_header():
    from drecpy_amd import _lib
    h = _header()
    for name, code in _lib.KNN_METRICS.items():
        assert re.search(r'#define\s+DRX_KNN_' + name.upper() + r'\s+' + str(code) + r'\b', h), name
    for name, code in list(_lib.KNN_AGGREGATIONS.items()) + [('user', _lib.KNN_USER), ('item', _lib.KNN_ITEM)]:
        assert re.search(r'#define\s+DRX_KNN_' + name.upper() + r'\s+' + str(code) + r'\b', h), name


# ---- the public classes, as far as no device is needed -----------------------------------------------------------------------------
def test_the_package_exports_the_baselines():
    from drecpy_amd import Recommender
    from drecpy_amd.Recommender.Baseline import BaseKNN, ItemKNN, UserKNN
    from drecpy_amd.engine import RowsRecommender
    from drecpy_amd.engine_knn import KnnEngine
    assert Recommender.Baseline.ItemKNN is ItemKNN and 'Baseline' in Recommender.__all__
    assert issubclass(ItemKNN, BaseKNN) and issubclass(UserKNN, BaseKNN) and (ItemKNN.type, UserKNN.type) == ('item', 'user')
    assert issubclass(KnnEngine, RowsRecommender) and KnnEngine.DENSE_BUDGET_BYTES == 8 << 30
    for name in ('topk', 'masked_topk', 'matrix_chunk_users'):
        assert name not in vars(KnnEngine)                                       # inherited
    m = ItemKNN(verbose=False)
    assert (m.k, m.m, m.sim_metric, m.aggregation, m.shrinkage, m.use_averages) == (20, 5, 'adjusted_cosine', 'weighted_mean', 100, False)
    assert hasattr(ItemKNN, '_rank_rows') and not hasattr(m, '_do_batch')


def test_constructor_errors():
    from drecpy_amd.Recommender.Baseline import ItemKNN, UserKNN
    for cls in (ItemKNN, UserKNN):
        with pytest.raises(Exception, match='There is no similarity metric corresponding to the name "euclid".'):
            cls(sim_metric='euclid', verbose=False)
        with pytest.raises(Exception, match='There is no aggregation approach corresponding to the name "median".'):
            cls(aggregation='median', verbose=False)
        with pytest.raises(Exception, match=r'outside the domain of the neighbour kernel \(1..128\)'):
            cls(k=129, verbose=False)
        assert cls(k=128, verbose=False).k == 128


def _frame(rows):
    from drecpy_amd.Dataset import InteractionDataset
    u, i, v = zip(*rows)
    return InteractionDataset.read_df({'user': np.array(u), 'item': np.array(i), 'interaction': np.array(v, dtype=np.float64)}, verbose=False)


def test_fit_refuses_what_lies_outside_the_domain(monkeypatch):
    from drecpy_amd.Recommender.Baseline import ItemKNN, UserKNN
    from drecpy_amd.engine_knn import KnnEngine
    ok = [(1, 1, 3.0), (1, 2, 4.0), (2, 1, 5.0), (2, 2, 1.0), (3, 2, 2.0)]
    for cls in (ItemKNN, UserKNN):
        with pytest.raises(Exception, match='duplicate'):
            cls(verbose=False).fit(_frame(ok + [(1, 2, 2.0)]))
        with pytest.raises(Exception, match='zero-valued interaction'):
            cls(verbose=False).fit(_frame(ok + [(3, 1, 0.0)]))
        monkeypatch.setattr(KnnEngine, 'DENSE_BUDGET_BYTES', 1024)
        with pytest.raises(MemoryError, match='DENSE_BUDGET_BYTES = 1024'):
            cls(verbose=False).fit(_frame(ok))
        monkeypatch.undo()
