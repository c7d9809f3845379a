"""ItemKNN rated by its predictions: RMSE / MSE of predict() over a held-out set (DRecPy's examples/item_knn_cf_predictive.py).
The neighbour table is built on the GPU (co-rating sums on the matrix cores), the test pairs are answered by one predict_pairs call.
    python examples/item_knn_cf_predictive.py [--movielens /data/ml-100k]"""
from _common import arguments, split, stopwatch

from drecpy_amd.Evaluation import predictive_evaluation
from drecpy_amd.Recommender.Baseline import ItemKNN


def main():
    args = arguments(default_epochs=0, dataset_name='ml-100k')
    train, test = split(args, 'ml-100k')
    item_cf = ItemKNN(k=15, m=1, shrinkage=100, sim_metric='adjusted_cosine', verbose=not args.quiet)
    with stopwatch('fit (similarities and neighbours)'):
        item_cf.fit(train)
    with stopwatch('predictive evaluation'):
        scores = predictive_evaluation(item_cf, test, skip_errors=True, verbose=False)
    for name, value in scores.items():
        print(f'  {name:14s} {value}')


if __name__ == '__main__':
    main()
