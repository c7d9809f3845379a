"""The C ABI of the generic scorer-selector: include/drx.h declares drx_rows_recommend / drx_rows_recommend_scratch_bytes and the
DRX_REC_* epilogues, and drecpy_amd/_lib.py binds them with matching argument counts and constants.  No GPU."""
import os
import re

import pytest

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
    for name in ('drx_rows_recommend', 'drx_rows_recommend_scratch_bytes', 'drx_cdae_recommend', 'drx_cdae_recommend_scratch_bytes'):
        assert name in _lib.SIGNATURES, name
        assert _n_args(h, name) == len(_lib.SIGNATURES[name][1]), name
    assert _n_args(h, 'drx_rows_recommend') == 16 and _n_args(h, 'drx_rows_recommend_scratch_bytes') == 4
    for name, value in (('DRX_REC_SIGMOID_BIAS', 0), ('DRX_REC_BIAS', 1), ('DRX_REC_CLIP', 2)):
        m = re.search(r'#define\s+' + name + r'\s+(-?\d+)', h)
        assert m and int(m.group(1)) == value == getattr(_lib, name), name


def test_the_engines_share_one_launcher():
    """the four calls, the chunked launch and the exclusion upload live in one place (no GPU needed to see it)"""
    from drecpy_amd.engine import CdaeEngine, RowsRecommender
    from drecpy_amd.engine_caser import CaserEngine
    from drecpy_amd.engine_dmf import DmfEngine
    from drecpy_amd.engine_knn import KnnEngine
    assert RowsRecommender.__module__ == 'drecpy_amd.engine_rows'
    calls = ('recommend', 'rank_items', 'rank_lists', 'pair_scores')
    for cls in (CdaeEngine, DmfEngine, CaserEngine):
        assert issubclass(cls, RowsRecommender)
        for name in calls:
            assert getattr(cls, name) is getattr(RowsRecommender, name) and name in vars(RowsRecommender), (cls, name)
            assert name not in vars(cls), (cls, name)
        assert cls.set_exclusions is RowsRecommender.set_exclusions
        # ... and so do the score-matrix route's selection and the upload of host ids
        for name in ('topk', 'masked_topk', '_dev_i32'):
            assert getattr(cls, name) is getattr(RowsRecommender, name) and name in vars(RowsRecommender), (cls, name)
        # what an engine declares instead: its table, its query rows, the rows' width and the epilogue
        for name in ('_score_table', '_query_rows', 'rank_ld', 'EPILOGUE'):
            assert name in vars(cls), (cls, name)
    # KnnEngine scores with kernels of its own, from the shared scratch keeper and request helpers
    assert issubclass(KnnEngine, RowsRecommender) and KnnEngine._rows_scratch is RowsRecommender._rows_scratch
    assert '_fused_scratch' not in vars(KnnEngine) and 'recommend' in vars(KnnEngine)
    for name in ('_recommend_request', '_rank_lists_request', '_exclusions', '_chunks'):
        assert getattr(KnnEngine, name) is getattr(RowsRecommender, name), name
    # no engine or model borrows them from the CDAE engine any more
    from drecpy_amd import engine_dense, engine_dmf, engine_knn
    from drecpy_amd.Recommender import caser
    assert 'CdaeEngine' not in vars(engine_dmf) and 'CdaeEngine' not in vars(caser)
    assert engine_dense.RowsRecommender is engine_knn.RowsRecommender is RowsRecommender


def test_an_engine_without_a_score_table_says_so():
    from drecpy_amd.engine import RowsRecommender

    class Bare(RowsRecommender):
        pass
    for call in (lambda e: e._score_table(), lambda e: e.rank_ld(), lambda e: e._query_rows(None)):
        with pytest.raises(NotImplementedError, match='Bare'):
            call(Bare())


@pytest.mark.parametrize('n_items', [1, 7, 3706, 1_000_000])
def test_users_per_chunk_of_the_score_matrix_route(n_items):
    """the chunk function of ranking_evaluation and CdaeEngine's score-matrix route against the literal expression; 4 * n_items * 7
    bytes are the 7 users per chunk tests/test_evaluation.py forces"""
    from drecpy_amd.engine import RowsRecommender
    for budget in (1 << 30, 4 * n_items * 7):
        want = max(1, min(budget // (4 * n_items), ((1 << 31) - 1) // n_items))
        assert RowsRecommender.matrix_chunk_users(n_items, budget) == want
    assert RowsRecommender.matrix_chunk_users(n_items, 4 * n_items * 7) == 7
