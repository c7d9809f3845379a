"""The C ABI of the generic scorer-selector: include/drx.h declares drx_rows_recommend / drx_rows_recommend_scratch_bytes and the
DRX_REC_* epilogues, and drecpy_amd/_lib.py binds them with matching argument counts and constants.  No GPU."""
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
    for name in ('drx_rows_recommend', 'drx_rows_recommend_scratch_bytes', 'drx_cdae_recommend', 'drx_cdae_recommend_scratch_bytes'):
        assert name in _lib.SIGNATURES, name
        assert _n_args(h, name) == len(_lib.SIGNATURES[name][1]), name
    assert _n_args(h, 'drx_rows_recommend') == 16 and _n_args(h, 'drx_rows_recommend_scratch_bytes') == 4
    for name, value in (('DRX_REC_SIGMOID_BIAS', 0), ('DRX_REC_BIAS', 1), ('DRX_REC_CLIP', 2)):
        m = re.search(r'#define\s+' + name + r'\s+(-?\d+)', h)
        assert m and int(m.group(1)) == value == getattr(_lib, name), name


def test_the_engines_share_one_launcher():
    """the chunked launch and the exclusion upload live in one place (no GPU needed to see it)"""
    from drecpy_amd.engine import CdaeEngine, RowsRecommender
    from drecpy_amd.engine_caser import CaserEngine
    from drecpy_amd.engine_dmf import DmfEngine
    for cls in (CdaeEngine, DmfEngine, CaserEngine):
        assert issubclass(cls, RowsRecommender) and cls._rows_recommend is RowsRecommender._rows_recommend
        assert cls.set_exclusions is RowsRecommender.set_exclusions and 'recommend' in vars(cls)
