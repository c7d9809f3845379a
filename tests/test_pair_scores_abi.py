"""The pair scorer without a GPU: include/drx.h declares drx_rows_pair_scores and drecpy_amd/_lib.py binds it with a matching argument
count; the engines share one launcher; the predictive metrics and predictive_evaluation against a stub model; the default
_predict_pairs hook of RecommenderABC on a stub subclass."""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- binding and wiring ---------------------------------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, 'include', 'drx.h')) as f:
        return re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)


def _n_args(header, name):
    m = re.search(r'\b' + name + r'\s*\(([^;]*?)\)\s*;', header, flags=re.S)
    assert m, f'{name} is not declared in include/drx.h'
    return len([a for a in m.group(1).split(',') if a.strip()])


def test_header_and_bindings_agree():
    import ctypes as C
    from drecpy_amd import _lib
    assert 'drx_rows_pair_scores' in _lib.SIGNATURES
    res, args = _lib.SIGNATURES['drx_rows_pair_scores']
    assert _n_args(_header(), 'drx_rows_pair_scores') == len(args) == 12
    assert res is C.c_int and args[9] is C.c_int64                    # P is the one 64-bit count
    assert [j for j, a in enumerate(args) if a is C.c_int32] == [2, 3, 4, 6]


def test_the_engines_share_one_launcher():
    from drecpy_amd.engine import CdaeEngine, RowsRecommender
    from drecpy_amd.engine_caser import CaserEngine
    from drecpy_amd.engine_dmf import DmfEngine
    for cls in (CdaeEngine, DmfEngine, CaserEngine):
        assert cls.pair_scores is RowsRecommender.pair_scores
        assert 'pair_scores' in vars(RowsRecommender) and 'pair_scores' not in vars(cls)


def test_the_evaluation_package_exports_the_process_and_its_metrics():
    from drecpy_amd import Evaluation
    from drecpy_amd.Evaluation import MAE, MSE, RMSE, PredictiveMetricABC, predictive_evaluation
    assert callable(predictive_evaluation)
    for cls in (RMSE, MSE, MAE):
        assert issubclass(cls, PredictiveMetricABC) and cls().name == cls.__name__ and cls.__name__ in Evaluation.__all__
    assert 'predictive_evaluation' in Evaluation.__all__ and 'PredictiveMetricABC' in Evaluation.__all__
    with pytest.raises(TypeError):
        PredictiveMetricABC()


def test_the_metrics_are_their_numpy_formulas():
    from drecpy_amd.Evaluation import MAE, MSE, RMSE
    t = np.array([1.0, 5.0, 3.0, 4.0, 2.0, 5.0])
    p = np.array([1.5, 4.0, 3.0, 1.0, 2.25, 4.75])
    assert MSE()(t, p) == float(np.mean((p - t) ** 2)) == 10.375 / 6
    assert RMSE()(list(t), list(p)) == math.sqrt(float(np.mean((p - t) ** 2)))
    assert MAE()(t, p) == float(np.mean(np.abs(p - t))) == 5.0 / 6
    assert MSE()([2], [2]) == 0.0


# ---- predictive_evaluation against a stub model ---------------------------------------------------------------------------------------
class _StubModel:
    """predict = 0.1 user + 0.01 item (a value with more than 4 decimals in the metrics); user 9 and item 9 are unknown"""

    def __init__(self, rows):
        from drecpy_amd.Dataset import InteractionDataset
        self.interaction_dataset = InteractionDataset.read_df({'user': np.array([r[0] for r in rows]), 'item': np.array([r[1] for r in rows]),
                                                               'interaction': np.array([r[2] for r in rows])}, verbose=False)
        self.asked, self.batches = [], []

    def predict(self, user, item, skip_errors=False):
        self.asked.append((user, item))
        if user == 9 or item == 9:
            if skip_errors:
                return None
            raise AssertionError(f'Item {item} was not found.' if item == 9 else f'User {user} was not found.')
        return 0.1 * user + 0.01 * item + 1 / 3

    def predict_pairs(self, users, items, skip_errors=False):
        self.batches.append(len(users))
        n = len(self.asked)
        out = np.array([np.nan if v is None else v for v in (self.predict(u, i, skip_errors) for u, i in zip(users, items))], np.float64)
        del self.asked[n:]
        return out


ROWS = [(1, 2, 3.0), (2, 9, 4.0), (3, 1, 1.0), (9, 4, 5.0), (4, 4, 2.0), (5, 6, 5.0), (6, 2, 4.0), (7, 7, 1.0)]


def _by_hand(rows, n, count_none):
    from drecpy_amd.Evaluation import MSE, RMSE
    t, p = [], []
    for u, i, v in rows:
        if len(p) >= n:
            break
        known = u != 9 and i != 9
        if known or count_none:
            t.append(v)
            p.append(0.1 * u + 0.01 * i + 1 / 3 if known else 0)
    return {'RMSE': round(RMSE()(t, p), 4), 'MSE': round(MSE()(t, p), 4)}, len(p)


@pytest.mark.parametrize('count_none', [False, True])
@pytest.mark.parametrize('n', [None, 1, 3, 5, 8, 100])
def test_both_modes_select_the_same_rows(n, count_none):
    from drecpy_amd.Evaluation import predictive_evaluation
    model = _StubModel(ROWS)
    want, made = _by_hand(ROWS, len(ROWS) if n is None else n, count_none)
    loop = predictive_evaluation(model, n_test_predictions=n, count_none_predictions=count_none, verbose=False, batched=False)
    assert model.batches == []
    asked = len(model.asked)
    fused = predictive_evaluation(model, n_test_predictions=n, count_none_predictions=count_none, verbose=False)
    assert model.batches and len(model.batches) == 1 and len(model.asked) == asked          # ONE predict_pairs call, no predict
    assert loop == fused == want and list(loop) == ['RMSE', 'MSE']
    for v in loop.values():
        assert v == round(v, 4) and isinstance(v, float)
    # n counts predictions MADE, not rows seen: with the unknown pairs skipped, 3 predictions take 5 rows and 5 take 7
    if n in (3, 5) and not count_none:
        assert asked == {3: 5, 5: 7}[n] and made == n


def test_a_test_set_of_its_own_and_other_metrics():
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Evaluation import MAE, predictive_evaluation
    model = _StubModel(ROWS)
    ds_te = InteractionDataset.read_df({'user': np.array([2, 9, 3]), 'item': np.array([2, 2, 3]), 'interaction': np.array([1.0, 2.0, 5.0])},
                                       verbose=False)
    want = round((abs(0.22 + 1 / 3 - 1.0) + abs(0.33 + 1 / 3 - 5.0)) / 2, 4)
    for batched in (True, False):
        assert predictive_evaluation(model, ds_te, metrics=[MAE()], verbose=False, batched=batched) == {'MAE': want}
    want0 = round((abs(0.22 + 1 / 3 - 1.0) + 2.0 + abs(0.33 + 1 / 3 - 5.0)) / 3, 4)
    for batched in (True, False):
        assert predictive_evaluation(model, ds_te, count_none_predictions=True, metrics=[MAE()], verbose=False, batched=batched) == {'MAE': want0}

    class OnlyPredict:                                                 # a model object without predict_pairs: the loop, whatever `batched`
        interaction_dataset = model.interaction_dataset
        predict = staticmethod(lambda user, item, skip_errors=False: 3.0)
    assert predictive_evaluation(OnlyPredict(), ds_te, metrics=[MAE()], verbose=False) == {'MAE': round((2 + 1 + 2) / 3, 4)}


def test_errors():
    from drecpy_amd.Evaluation import HitRatio, predictive_evaluation
    model = _StubModel(ROWS)
    for batched in (True, False):
        with pytest.raises(AssertionError, match='Item 9 was not found.'):
            predictive_evaluation(model, skip_errors=False, verbose=False, batched=batched)
        # the walk ends before the first unknown pair: nothing to raise
        assert set(predictive_evaluation(model, skip_errors=False, n_test_predictions=1, verbose=False, batched=batched)) == {'RMSE', 'MSE'}
        with pytest.raises(AssertionError, match=r'The number of test users \(0\) should be > 0.'):
            predictive_evaluation(model, n_test_predictions=0, verbose=False, batched=batched)
        with pytest.raises(AssertionError, match='to be an instance of type PredictiveMetricABC.'):
            predictive_evaluation(model, metrics=[HitRatio()], verbose=False, batched=batched)
        with pytest.raises(AssertionError, match='Expected "metrics" argument to be a list and found'):
            predictive_evaluation(model, metrics=(), verbose=False, batched=batched)


# ---- the default hook, on a stub subclass ---------------------------------------------------------------------------------------------
def _stub_recommender(predict):
    from drecpy_amd.Dataset import InteractionDataset
    from drecpy_amd.Recommender.recommender_abc import RecommenderABC

    class Stub(RecommenderABC):
        def _pre_fit(self, learning_rate, neg_ratio, reg_rate, **kwds):
            pass

        def _sample_batch(self, batch_size, **kwds):
            pass

        def _predict_batch(self, batch_samples, **kwds):
            pass

        def _compute_batch_loss(self, predictions, desired_values, **kwds):
            pass

        def _predict(self, uid, iid, **kwds):
            return predict(uid, iid)
    model = Stub(verbose=False)
    ds = InteractionDataset.read_df({'user': np.array([10, 11, 12, 10]), 'item': np.array([70, 71, 72, 73]), 'interaction': np.array([1, 2, 3, 4])},
                                    verbose=False)
    ds.assign_internal_ids()
    model.interaction_dataset, model.fitted = ds, True
    return model


def test_the_default_hook_is_one_predict_per_pair():
    model = _stub_recommender(lambda uid, iid: None if (uid, iid) == (1, 1) else uid + iid / 7)
    users, items = [12, 10, 11, 10, 11], [70, 73, 70, 70, 73]
    got = model.predict_pairs(users, items)
    assert got.dtype == np.float64 and got.tolist() == [model.predict(u, i) for u, i in zip(users, items)] == [2.0, 3 / 7, 1.0, 0.0, 1 + 3 / 7]
    assert model.predict_pairs([], []).shape == (0,) and model.predict_pairs([], []).dtype == np.float64
    # None -> NaN under skip_errors, predict's exceptions without
    some = model.predict_pairs([12, 11, 5, 10, 10], [70, 71, 70, 9, 73], skip_errors=True)
    assert np.isnan(some).tolist() == [False, True, True, True, False] and some[0] == 2.0 and some[4] == 3 / 7
    assert [model.predict(u, i, skip_errors=True) for u, i in zip([11, 5, 10], [71, 70, 9])] == [None, None, None]
    with pytest.raises(Exception, match=r'Failed to predict\(user_id=11, item_id=71\): None was returned.'):
        model.predict_pairs([12, 11], [70, 71])
    with pytest.raises(AssertionError, match='User 5 was not found.'):
        model.predict_pairs([12, 5], [70, 71])
    with pytest.raises(AssertionError, match='Item 9 was not found.'):
        model.predict_pairs([12, 10], [70, 9])
    with pytest.raises(AssertionError, match='parallel sequences'):
        model.predict_pairs([12, 10], [70])
    model.fitted = False
    with pytest.raises(AssertionError, match='requires to be fitted'):
        model.predict_pairs([12], [70])


def test_a_model_without_point_predictions():
    def refuse(uid, iid):
        raise NotImplementedError('This model does not support point-based predictions.')
    model = _stub_recommender(refuse)
    with pytest.raises(NotImplementedError, match='point-based'):
        model.predict_pairs([12, 10], [70, 73])
    assert np.isnan(model.predict_pairs([12, 10, 5], [70, 73, 70], skip_errors=True)).all()
    failing = _stub_recommender(lambda uid, iid: 1 / (uid - 1))          # one pair fails: under skip_errors it alone is lost
    got = failing.predict_pairs([10, 11, 12], [70, 70, 70], skip_errors=True)
    assert np.isnan(got).tolist() == [False, True, False] and got[0] == -1.0 and got[2] == 1.0


def test_a_predicted_nan_is_a_prediction():
    """predict() returns a NaN the model predicts; only None is 'no prediction'"""
    model = _stub_recommender(lambda uid, iid: float('nan') if uid == 1 else float(uid))
    assert math.isnan(model.predict(11, 70))
    got = model.predict_pairs([10, 11, 12], [70, 70, 70])             # skip_errors=False: nothing raises
    assert np.isnan(got).tolist() == [False, True, False] and got[2] == 2.0
