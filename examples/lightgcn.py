"""LightGCN rated by its rankings: HR@k / NDCG@k with one held-out item per user against 100 sampled negatives — the graph-convolution
successor of BPR-MF, on the protocol of examples/bpr.py — and the fused serving calls on the fitted model.
    python examples/lightgcn.py [--movielens /data/ml-100k] [--epochs 2000] [--quiet]"""
from _common import arguments, split, stopwatch

from drecpy_amd.Evaluation import NDCG, HitRatio, ranking_evaluation
from drecpy_amd.Recommender.Baseline import LightGCN


def main():
    args = arguments(default_epochs=2000, dataset_name='ml-100k')
    train, test = split(args, 'ml-100k', hold_out=1)
    # one fit() "epoch" is one mini-batch: batch_size triples, neg_ratio negatives drawn for every (user, positive) pair; every step
    # propagates all embeddings over the whole graph of the training positives, 3 times forward and 3 times backward
    lgcn = LightGCN(factors=64, layers=3, init_std=0.01, interaction_threshold=3, seed=10, verbose=not args.quiet)
    with stopwatch(f'fit ({args.epochs} steps of 4096 triples)'):
        lgcn.fit(train, epochs=args.epochs, batch_size=4096, learning_rate=0.01, neg_ratio=4, reg_rate=1e-4)
    with stopwatch('ranking evaluation'):
        scores = ranking_evaluation(lgcn, test, n_pos_interactions=1, n_neg_interactions=100, generate_negative_pairs=True, novelty=True,
                                    k=list(range(1, 11)), metrics=[HitRatio(), NDCG()], seed=10, verbose=False)
    for name, value in scores.items():
        print(f'  {name:14s} {value}')
    users = test.unique('user').values_list('user', to_list=True)[:5]
    with stopwatch('recommend_batch (5 users, n = 5)'):
        lists = lgcn.recommend_batch(users, n=5)
    for user, top in zip(users, lists):
        print(f'  user {user}: ' + ', '.join(f'{item} ({score:.3f})' for score, item in top))


if __name__ == '__main__':
    main()
