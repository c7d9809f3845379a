from .base_knn import BaseKNN


class UserKNN(BaseKNN):
    """User-based KNN collaborative filtering (DRecPy/Recommender/Baseline/user_knn.py): the neighbours of a user are the k most
    similar users; a prediction aggregates the ratings those neighbours gave the item.  rank() / recommend() list only items that
    at least one neighbour rated (user_knn.py:69-95 has no use_averages fallback there).

    Public methods: fit(), predict(), predict_pairs(), rank(), recommend(), recommend_batch().  Attributes: see BaseKNN."""
    type = 'user'
