"""ItemKNN rated by its rankings: HR@k / NDCG@k with one held-out item per user against 100 sampled negatives (DRecPy's
examples/item_knn_cf_ranking.py) — the baseline figure to put beside a deep model's.
    python examples/item_knn_cf_ranking.py [--movielens /data/ml-100k]"""
from _common import arguments, split, stopwatch

from drecpy_amd.Evaluation import NDCG, HitRatio, ranking_evaluation
from drecpy_amd.Recommender.Baseline import ItemKNN


def main():
    args = arguments(default_epochs=0, dataset_name='ml-100k')
    train, test = split(args, 'ml-100k', hold_out=1)
    item_cf = ItemKNN(k=5, m=1, shrinkage=50, sim_metric='adjusted_cosine', verbose=not args.quiet)
    with stopwatch('fit (similarities and neighbours)'):
        item_cf.fit(train)
    with stopwatch('ranking evaluation'):
        scores = ranking_evaluation(item_cf, test, n_pos_interactions=1, n_neg_interactions=100, generate_negative_pairs=True, novelty=True,
                                    k=list(range(1, 11)), metrics=[HitRatio(), NDCG()], seed=10, verbose=False)
    for name, value in scores.items():
        print(f'  {name:14s} {value}')


if __name__ == '__main__':
    main()
