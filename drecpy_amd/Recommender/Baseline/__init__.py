from .base_knn import BaseKNN
from .item_knn import ItemKNN
from .user_knn import UserKNN

__all__ = ['BaseKNN', 'ItemKNN', 'UserKNN']
