from .base_knn import BaseKNN


class ItemKNN(BaseKNN):
    """Item-based KNN collaborative filtering (DRecPy/Recommender/Baseline/item_knn.py): the neighbours of an item are the k most
    similar items; a prediction aggregates the ratings the user gave those neighbours.  With use_averages, predict() and rank() fall
    back to the user's mean rating where no neighbour has a term (item_knn.py:64-96), so every candidate gets a score.

    Public methods: fit(), predict(), predict_pairs(), rank(), recommend(), recommend_batch().  Attributes: see BaseKNN."""
    type = 'item'
