"""NeuMF rated by its rankings: HR@k / NDCG@k with one held-out item per user against 100 sampled negatives — the neural baseline the DMF
paper reports against, on the protocol of examples/bpr.py — and the batched serving calls on the fitted model.
    python examples/ncf.py [--movielens /data/ml-100k] [--epochs 2000] [--quiet]"""
from _common import arguments, split, stopwatch

from drecpy_amd.Evaluation import NDCG, HitRatio, ranking_evaluation
from drecpy_amd.Recommender.Baseline import NeuMF


def main():
    args = arguments(default_epochs=2000, dataset_name='ml-100k')
    train, test = split(args, 'ml-100k', hold_out=1)
    # one fit() "epoch" is one mini-batch: batch_size point samples, a negative with probability neg_ratio / (neg_ratio + 1)
    ncf = NeuMF(factors=8, mlp_factors=32, layers=(32, 16, 8), interaction_threshold=3, seed=10, verbose=not args.quiet)
    with stopwatch(f'fit ({args.epochs} steps of 4096 point samples)'):
        ncf.fit(train, epochs=args.epochs, batch_size=4096, learning_rate=0.001, neg_ratio=4, reg_rate=1e-6)
    with stopwatch('ranking evaluation'):
        scores = ranking_evaluation(ncf, test, n_pos_interactions=1, n_neg_interactions=100, generate_negative_pairs=True, novelty=True,
                                    k=list(range(1, 11)), metrics=[HitRatio(), NDCG()], seed=10, verbose=False)
    for name, value in scores.items():
        print(f'  {name:14s} {value}')
    users = test.unique('user').values_list('user', to_list=True)[:5]
    with stopwatch('recommend_batch (5 users, n = 5)'):
        lists = ncf.recommend_batch(users, n=5)
    for user, top in zip(users, lists):
        print(f'  user {user}: ' + ', '.join(f'{item} ({score:.3f})' for score, item in top))


if __name__ == '__main__':
    main()
