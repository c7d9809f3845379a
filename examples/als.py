"""ALS / WMF rated by its rankings: HR@k / NDCG@k with one held-out item per user against 100 sampled negatives — the "MF" baseline of
the CDAE paper, on the protocol of examples/bpr.py — and the fused serving calls on the fitted model.
    python examples/als.py [--movielens /data/ml-100k] [--epochs 15] [--quiet]"""
from _common import arguments, split, stopwatch

from drecpy_amd.Evaluation import NDCG, HitRatio, ranking_evaluation
from drecpy_amd.Recommender.Baseline import ALS


def main():
    args = arguments(default_epochs=15, dataset_name='ml-100k')
    train, test = split(args, 'ml-100k', hold_out=1)
    # one fit() "epoch" is one sweep: every user row solved exactly, then every item row
    als = ALS(factors=64, alpha=40.0, interaction_threshold=3, seed=10, verbose=not args.quiet)
    with stopwatch(f'fit ({args.epochs} sweeps)'):
        als.fit(train, epochs=args.epochs, reg_rate=0.1)
    with stopwatch('ranking evaluation'):
        scores = ranking_evaluation(als, test, n_pos_interactions=1, n_neg_interactions=100, generate_negative_pairs=True, novelty=True,
                                    k=list(range(1, 11)), metrics=[HitRatio(), NDCG()], seed=10, verbose=False)
    for name, value in scores.items():
        print(f'  {name:14s} {value}')
    users = test.unique('user').values_list('user', to_list=True)[:5]
    with stopwatch('recommend_batch (5 users, n = 5)'):
        lists = als.recommend_batch(users, n=5)
    for user, top in zip(users, lists):
        print(f'  user {user}: ' + ', '.join(f'{item} ({score:.3f})' for score, item in top))


if __name__ == '__main__':
    main()
