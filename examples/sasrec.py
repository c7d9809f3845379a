"""SASRec: the self-attention model that superseded Caser, GRU4Rec and FPMC (Kang & McAuley 2018), trained from the ListSampler windows
they train on, ordered by timestamp; scored with recommendation_evaluation (top-N against the held-out items) on the protocol of
examples/caser.py, examples/fpmc.py and examples/gru4rec.py, so the four can be set side by side.
    python examples/sasrec.py [--movielens /data/ml-1m] [--epochs 100]"""
from _common import arguments, split, stopwatch

from drecpy_amd.Evaluation import recommendation_evaluation
from drecpy_amd.Recommender.Baseline import SASRec


def main():
    args = arguments(default_epochs=100, dataset_name='ml-1m')
    train, test = split(args, 'ml-1m', min_user_interactions=20)
    model = SASRec(hidden=64, L=10, blocks=2, sort_column='timestamp', seed=10, verbose=not args.quiet)
    with stopwatch(f'fit, {args.epochs} epochs of 512 windows'):
        model.fit(train, epochs=args.epochs, batch_size=512, learning_rate=1e-3, reg_rate=1e-6, neg_ratio=3)
    scores = recommendation_evaluation(model, test, n_test_users=200, k=[1, 5, 10], novelty=True, seed=10, verbose=False)
    for name, value in scores.items():
        print(f'  {name:14s} {value}')
    users = test.unique('user').values_list('user', to_list=True)[:5]
    with stopwatch('recommend_batch (5 users, n = 5)'):
        lists = model.recommend_batch(users, n=5)
    for user, top in zip(users, lists):
        print(f'  user {user}: ' + ', '.join(f'{item} ({score:.3f})' for score, item in top))


if __name__ == '__main__':
    main()
