"""loss_weighted_sum of the reference's trainer (maskrcnn_benchmark/engine/trainer_sparse3d.py:42-61): the loss dict of a
training step against cfg.MODEL.LOSS.WEIGHTS.  Host arithmetic on 0-dim device tensors: one multiplication and one
addition per key, no host read."""

# position in MODEL.LOSS.WEIGHTS of every loss name (trainer_sparse3d.py:44-52); a key of the loss dict takes the weight of
# the first name, in this order, that it contains -- so the per-group keys (`loss_classifier_roi_1`, ...) find theirs
LOSS_WEIGHT_KEYS = ("loss_objectness", "loss_rpn_box_reg", "loss_classifier_roi", "loss_box_reg_roi", "geometric_pull_loss",
                    "semantic_pull_loss", "semantic_push_loss")


def loss_weighted_sum(loss_dict, loss_weights):
    """Scales every entry of `loss_dict` by its weight IN PLACE, as the reference does (its trainer logs the weighted
    values), and returns their sum.  `loss_weights`: the seven values of MODEL.LOSS.WEIGHTS.  A key that contains none of
    the seven names raises KeyError (the reference would take the weight of the key before it)."""
    if len(loss_weights) != len(LOSS_WEIGHT_KEYS):
        raise ValueError("loss_weights must hold %d values, got %r" % (len(LOSS_WEIGHT_KEYS), loss_weights))
    loss_sum = 0
    for key in loss_dict:
        for name, weight in zip(LOSS_WEIGHT_KEYS, loss_weights):
            if name in key:
                break
        else:
            raise KeyError("loss_weighted_sum: no weight for %r" % (key,))
        loss_dict[key] = loss_dict[key] * weight
        loss_sum = loss_sum + loss_dict[key]
    return loss_sum
