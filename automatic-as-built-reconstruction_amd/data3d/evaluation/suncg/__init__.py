"""SUNCG-style detection evaluation on the device: see suncg_eval."""
from .suncg_eval import eval_detection_suncg, evaluate_dataset, result_str  # noqa: F401
