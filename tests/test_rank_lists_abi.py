"""The C ABI of the list form of the catalogue-rank entry point: include/drx.h declares drx_rows_rank_lists, its scratch size and its
group size, drecpy_amd/_lib.py binds them with matching argument counts; the engines share one rank_lists.
No GPU."""
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
    for name, n_args in (('drx_rows_rank_lists_group', 1), ('drx_rows_rank_lists_scratch_bytes', 4), ('drx_rows_rank_lists', 17)):
        assert name in _lib.SIGNATURES, name
        assert _n_args(h, name) == len(_lib.SIGNATURES[name][1]) == n_args, name


def test_the_engines_share_one_launcher_and_each_has_rank_lists():
    from drecpy_amd.engine import CdaeEngine, RowsRecommender
    from drecpy_amd.engine_caser import CaserEngine
    from drecpy_amd.engine_dmf import DmfEngine
    assert RowsRecommender.RANK_LISTS_MIN_MEAN >= 1.0
    for cls in (CdaeEngine, DmfEngine, CaserEngine):
        assert cls.rank_lists is RowsRecommender.rank_lists and cls.rank_lists_group is RowsRecommender.rank_lists_group
        assert 'rank_lists' in vars(RowsRecommender) and 'rank_lists' not in vars(cls) and 'rank_ld' in vars(cls)
        assert cls.RANK_LISTS_MIN_MEAN == RowsRecommender.RANK_LISTS_MIN_MEAN


def test_pairs_grouped_into_rows_of_one_user():
    """the host half of the routing: a stable order by (user, item), a row per user and per `group` items of it"""
    import numpy as np
    from drecpy_amd.Recommender.recommender_abc import RecommenderABC
    uids = np.array([3, 1, 3, 3, 1, 3, 3, 3, 2])
    iids = np.array([5, 2, -1, 7, 1, 9, 4, 4, 0])
    order, starts, indptr = RecommenderABC._grouped_pairs(uids, iids, 2)
    assert uids[order].tolist() == [1, 1, 2, 3, 3, 3, 3, 3, 3] and iids[order].tolist() == [1, 2, 0, -1, 4, 4, 5, 7, 9]
    assert order[4:6].tolist() == [6, 7]                              # stable: equal pairs keep their order
    assert starts.tolist() == [0, 2, 3, 5, 7] and indptr.tolist() == [0, 2, 3, 5, 7, 9] and indptr.dtype == np.int64
    order, starts, indptr = RecommenderABC._grouped_pairs(uids, iids, 32)
    assert starts.tolist() == [0, 2, 3] and indptr.tolist() == [0, 2, 3, 9]
