"""The C ABI of the KNN baselines' fused top-n and catalogue ranks: include/drx.h declares drx_knn_recommend, drx_knn_rank_lists and
their scratch sizes, drecpy_amd/_lib.py binds them with matching argument counts; KnnEngine has recommend and rank_lists, BaseKNN its
own _catalogue_ranks.  No GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, 'include', 'drx.h')) as f:
        return re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)


def _n_args(header, name):
    m = re.search(r'\b' + name + r'\s*\(([^;]*?)\)\s*;', header, flags=re.S)
    assert m, f'{name} is not declared in include/drx.h'
    return len([a for a in m.group(1).split(',') if a.strip()])


def test_header_and_bindings_agree():
    from drecpy_amd import _lib
    h = _header()
    for name, n_args in (('drx_knn_recommend_scratch_bytes', 4), ('drx_knn_recommend', 22), ('drx_knn_rank_lists_scratch_bytes', 4),
                         ('drx_knn_rank_lists', 24)):
        assert name in _lib.SIGNATURES, name
        assert _n_args(h, name) == len(_lib.SIGNATURES[name][1]) == n_args, name
    # the model arguments are those of drx_knn_score_rows, in its order
    lead = _lib.SIGNATURES['drx_knn_score_rows'][1][:12]
    assert _lib.SIGNATURES['drx_knn_recommend'][1][:12] == lead and _lib.SIGNATURES['drx_knn_rank_lists'][1][:12] == lead


def test_the_engine_and_the_classes_have_the_fused_routes():
    from drecpy_amd.engine import RowsRecommender
    from drecpy_amd.engine_knn import KnnEngine
    from drecpy_amd.Recommender.Baseline import ItemKNN, UserKNN
    from drecpy_amd.Recommender.Baseline.base_knn import BaseKNN
    from drecpy_amd.Recommender.recommender_abc import RecommenderABC
    assert 'recommend' in vars(KnnEngine) and 'rank_lists' in vars(KnnEngine)
    assert KnnEngine.set_exclusions is RowsRecommender.set_exclusions and KnnEngine.FUSED_MAX_N == 128
    assert '_catalogue_ranks' in vars(BaseKNN) and BaseKNN._catalogue_ranks is not RecommenderABC._catalogue_ranks
    assert '_recommend_batch' in vars(BaseKNN)
    for cls in (ItemKNN, UserKNN):
        assert cls._catalogue_ranks is BaseKNN._catalogue_ranks and cls._recommend_batch is BaseKNN._recommend_batch
