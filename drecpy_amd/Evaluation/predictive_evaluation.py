"""RMSE / MSE / MAE over the model's point predictions with the protocol of DRecPy/Evaluation/Processes/predictive_evaluation.py:7-65 —
same arguments, same walk over the test rows in their order, same counting of predictions MADE, same assertions, same rounding — but
with batched=True (the default) every prediction comes from ONE `model.predict_pairs` call instead of one `model.predict` per row: on
CDAE and DMF that is the fused pair scorer (two rows per pair), not a forward over the catalogue per row.
batched=False, or a model object without predict_pairs, is the per-row loop.  Both modes select the same rows: a row whose prediction
is None (NaN from predict_pairs) is skipped, or counted as a prediction of 0 under count_none_predictions, and the walk stops once
n_test_predictions predictions have been made.  A prediction that is not a scalar counts as None in both modes (CDAE's _predict
answers an unknown item, iid None, with the user's whole row of predictions, as the reference's does: that is no point prediction, and
predict_pairs reports NaN for it).  A batched value may differ from predict()'s in the last ulp (RecommenderABC.predict_pairs)."""
import logging
import math

from .metrics import MSE, RMSE, PredictiveMetricABC


def _plain(x):
    return x.item() if hasattr(x, 'item') else x


def _point(pred):
    return None if pred is None or getattr(pred, 'ndim', 0) != 0 else pred


def predictive_evaluation(model, ds_test=None, count_none_predictions=False, n_test_predictions=None, skip_errors=True, **kwds):
    ds_test = model.interaction_dataset if ds_test is None else ds_test
    if n_test_predictions is None:
        n_test_predictions = len(ds_test)
    assert n_test_predictions > 0, f'The number of test users ({n_test_predictions}) should be > 0.'
    metrics = kwds.get('metrics', [RMSE(), MSE()])
    assert isinstance(metrics, list), f'Expected "metrics" argument to be a list and found {type(metrics)}. ' \
        f'Should contain instances of PredictiveMetricABC.'
    for m in metrics:
        assert isinstance(m, PredictiveMetricABC), f'Expected metric {m} to be an instance of type PredictiveMetricABC.'
    n_test_predictions = min(n_test_predictions, len(ds_test))
    rows = [tuple(_plain(x) for x in row) for row in ds_test.values(['user', 'item', 'interaction'], to_list=True)]

    if kwds.get('batched', True) and hasattr(model, 'predict_pairs'):
        # a None can only come back under skip_errors (predict raises otherwise), and only then can the walk pass row n_test_predictions
        # without counting it: in every other case the first n_test_predictions rows are all it reads.  In that one case (the defaults
        # with an n_test_predictions below the test set's length) ALL rows are scored, for the sake of the one call: a pair costs two
        # rows on the device, but a caller who wants 100 predictions out of a million rows should pass a frame of about that size
        if count_none_predictions or not skip_errors:
            rows = rows[:n_test_predictions]
        values = model.predict_pairs([r[0] for r in rows], [r[1] for r in rows], skip_errors=skip_errors) if rows else []
        predictions = (None if math.isnan(v) else float(v) for v in values)
    else:
        predictions = (_point(model.predict(user, item, skip_errors=skip_errors)) for user, item, _ in rows)     # (lazy: stops with the walk)

    y_true, y_pred = [], []
    for (_, _, interaction), pred in zip(rows, predictions):
        if pred is None:
            if not count_none_predictions:
                continue
            pred = 0
        y_pred.append(pred)
        y_true.append(interaction)
        if len(y_pred) >= n_test_predictions:                        # (n_test_predictions >= 1: no prediction is asked for beyond it)
            break
    if kwds.get('verbose', True):
        logging.info(f'predictive evaluation: {len(y_pred)} predictions over {len(rows)} test rows')
    return {m.name: round(m(y_true, y_pred), 4) for m in metrics}
