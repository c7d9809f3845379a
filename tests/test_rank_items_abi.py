"""The C ABI of the catalogue-rank entry point: include/drx.h declares drx_rows_rank_items / drx_rows_rank_items_scratch_bytes and
drecpy_amd/_lib.py binds them with matching argument counts; the engines share one launcher.  No GPU."""
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
    for name, n_args in (('drx_rows_rank_items', 16), ('drx_rows_rank_items_scratch_bytes', 3)):
        assert name in _lib.SIGNATURES, name
        assert _n_args(h, name) == len(_lib.SIGNATURES[name][1]) == n_args, name


def test_the_engines_share_one_launcher():
    from drecpy_amd.engine import CdaeEngine, RowsRecommender
    from drecpy_amd.engine_caser import CaserEngine
    from drecpy_amd.engine_dmf import DmfEngine
    for cls in (CdaeEngine, DmfEngine, CaserEngine):
        assert cls.rank_items is RowsRecommender.rank_items and cls.rank_is_fused is RowsRecommender.rank_is_fused
        assert 'rank_items' in vars(RowsRecommender) and 'rank_items' not in vars(cls)
