"""Top-N recommendation evaluation with the protocol of DRecPy/Evaluation/Processes/recommendation_evaluation.py (used by
examples/caser.py:17-18): per test user `model.recommend(user, n=max(k), novelty)` against the user's (sampled) test
positives; user i draws from `random.Random(seed + i)`; result keys `metric@k`, rounded to 4 decimals.
batched=True (default off: the loop above) draws every user's positives first — same streams, same skipping — and asks the model for all
lists in ONE `model.recommend_batch` call.
batched='ranks': the same protocol, but instead of lists ONE `model.catalogue_ranks` call for every (user, item) row of the drawn
users' test data; each user's first min(max(k), eligible items) positions are rebuilt from the ranks (a position holds the test item
whose rank it is, else a placeholder of relevance 0) and fed to the same metrics — no list is selected, so max(k) is not bounded by
the fused selector's 128.  It takes no `ignore_low_predictions_threshold`."""
import logging
import random

from ._protocol import MetricTable, as_k_list, resolve_metrics, sample_positives


def recommendation_evaluation(model, ds_test=None, n_test_users=None, k=10, n_pos_interactions=None, novelty=False,
                              ignore_low_predictions_threshold=None, seed=0, max_concurrent_threads=4, batched=False, **kwds):
    assert n_test_users is None or n_test_users > 0, f'The number of test users ({n_test_users}) should be > 0.'
    assert n_pos_interactions is None or n_pos_interactions > 0, \
        f'The number of positive interactions ({n_pos_interactions}) should be None or an integer > 0.'
    threshold = kwds.get('interaction_threshold', model.interaction_threshold)
    ks = as_k_list(k)
    table = MetricTable(resolve_metrics(kwds), ks)
    ds_test = model.interaction_dataset if ds_test is None else ds_test
    users = ds_test.unique('user').values_list('user', to_list=True)
    if n_test_users is not None:
        users = users[:n_test_users]
    if isinstance(batched, str):
        assert batched == 'ranks', f"batched: False, True or 'ranks' (got {batched!r})"
        assert ignore_low_predictions_threshold is None, \
            "batched='ranks' places items by their catalogue rank: it takes no ignore_low_predictions_threshold."
    if batched:
        return _evaluate_batched(model, ds_test, users, table, ks, threshold, n_pos_interactions, novelty,
                                 ignore_low_predictions_threshold, seed, by_ranks=batched == 'ranks')
    for offset, user in enumerate(users):
        user = user.item() if hasattr(user, 'item') else user
        try:
            user_ds = ds_test.select(f'user == {user}')
            drawn = sample_positives(user_ds, threshold, n_pos_interactions, random.Random(seed + offset))
            if drawn is None or not drawn[0]:
                continue
            relevant, best, _ = drawn
            ranked = model.recommend(user, n=max(ks), novelty=novelty, skip_invalid_items=True,
                                     interaction_threshold=ignore_low_predictions_threshold)
            recommendations = [item for _, item in ranked]
            relevancies = {item: (user_ds.select_one(f'item == {item}', ['interaction'], to_list=True) or 0)
                           for item in set(relevant) | set(recommendations)}
        except Exception as err:          # the reference logs and skips the user
            logging.error(err)
            continue
        table.add(recommendations, relevant, best, relevancies)
    return table.result()


class _Other:
    """An item of a rebuilt list that is none of the user's test items: unique, relevance 0, equal to no id (nor its text)."""
    __slots__ = ()


def _lists_from_ranks(model, drawn_users, n, novelty):
    """What recommend_batch(n) would list, as far as the metrics can tell, from ONE model.catalogue_ranks call over every (user, item)
    row of the drawn users' test data: position p of a user's list holds the test item whose catalogue rank is p, every other of
    the first min(n, eligible items) positions an _Other.  [[(None, item), ...], ...] like recommend_batch's lists."""
    pair_users, pair_items, owner = [], [], []
    for j, (user, user_ds, _, _) in enumerate(drawn_users):
        items = user_ds.values_list('item', to_list=True)
        pair_users += [user] * len(items)
        pair_items += [item.item() if hasattr(item, 'item') else item for item in items]
        owner += [j] * len(items)
    ranks = model.catalogue_ranks(pair_users, pair_items, novelty=novelty)
    ds = model.interaction_dataset
    excl_ptr = model._exclusion_csr()[0] if novelty else None
    lists = []
    for user, _, _, _ in drawn_users:
        taken = int(excl_ptr[ds.user_to_uid(user) + 1] - excl_ptr[ds.user_to_uid(user)]) if novelty else 0
        lists.append([(None, _Other()) for _ in range(min(n, model.n_items - taken))])
    for j, item, rank in zip(owner, pair_items, ranks):
        if 0 <= rank < len(lists[j]):
            lists[j][rank] = (None, ds.iid_to_item(ds.item_to_iid(item)))
    return lists


def _evaluate_batched(model, ds_test, users, table, ks, threshold, n_pos_interactions, novelty, low_threshold, seed, by_ranks=False):
    drawn_users = []
    for offset, user in enumerate(users):
        user = user.item() if hasattr(user, 'item') else user
        try:
            user_ds = ds_test.select(f'user == {user}')
            drawn = sample_positives(user_ds, threshold, n_pos_interactions, random.Random(seed + offset))
            if drawn is None or not drawn[0]:
                continue
            if model.interaction_dataset.user_to_uid(user) is None:        # (logged and skipped, as recommend() raising in the loop is)
                raise Exception(f'User {user} was not found.')
        except Exception as err:
            logging.error(err)
            continue
        drawn_users.append((user, user_ds, drawn[0], drawn[1]))
    if not drawn_users:
        return table.result()
    if by_ranks:
        lists = _lists_from_ranks(model, drawn_users, max(ks), novelty)
    else:
        lists = model.recommend_batch([u for u, _, _, _ in drawn_users], n=max(ks), novelty=novelty, interaction_threshold=low_threshold)
    for (user, user_ds, relevant, best), ranked in zip(drawn_users, lists):
        try:
            recommendations = [item for _, item in ranked]
            relevancies = {item: 0 if isinstance(item, _Other) else (user_ds.select_one(f'item == {item}', ['interaction'], to_list=True) or 0)
                           for item in set(relevant) | set(recommendations)}
        except Exception as err:
            logging.error(err)
            continue
        table.add(recommendations, relevant, best, relevancies)
    return table.result()
