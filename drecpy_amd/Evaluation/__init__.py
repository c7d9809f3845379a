from .metrics import (DCG, MAE, MSE, NDCG, RMSE, AveragePrecision, FScore, HitRatio, Precision, PredictiveMetricABC, RankingMetricABC,
                      Recall, ReciprocalRank)
from .predictive_evaluation import predictive_evaluation
from .ranking_evaluation import ranking_evaluation
from .recommendation_evaluation import recommendation_evaluation
from .splits import leave_k_out

__all__ = ['ranking_evaluation', 'recommendation_evaluation', 'predictive_evaluation', 'leave_k_out', 'RankingMetricABC', 'DCG', 'NDCG', 'HitRatio',
           'ReciprocalRank', 'Recall', 'Precision', 'FScore', 'AveragePrecision', 'PredictiveMetricABC', 'RMSE', 'MSE', 'MAE']
