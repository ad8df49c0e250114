"""reference: maskrcnn_benchmark/engine/ -- of the training loop this package carries what combines the losses."""
from .trainer_sparse3d import LOSS_WEIGHT_KEYS, loss_weighted_sum

__all__ = ["LOSS_WEIGHT_KEYS", "loss_weighted_sum"]
