"""`data3d.evaluation.evaluate`: the name the reference's training loop calls after an epoch.  Here it scores a data
set's predictions on the device (suncg.suncg_eval.evaluate_dataset -> eval_glue.detection_eval).  Only what that needs is
read; what the reference's call passes besides (an output folder, an epoch number, `is_train`, `box_only`) is accepted by
keyword and not used, because nothing is written or drawn here."""
from .suncg.suncg_eval import evaluate_dataset


def evaluate(dataset, predictions, iou_thresh_eval, eval_aug_thickness=None, **not_used):
    return evaluate_dataset(dataset, predictions, iou_thresh_eval, eval_aug_thickness)
