from .als import ALS
from .base_knn import BaseKNN
from .bpr import BPR
from .fpmc import FPMC
from .gru4rec import GRU4Rec
from .item_knn import ItemKNN
from .lightgcn import LightGCN
from .multvae import MultVAE
from .ncf import NeuMF
from .sasrec import SASRec
from .user_knn import UserKNN

__all__ = ['ALS', 'BaseKNN', 'BPR', 'FPMC', 'GRU4Rec', 'ItemKNN', 'LightGCN', 'MultVAE', 'NeuMF', 'SASRec', 'UserKNN']
