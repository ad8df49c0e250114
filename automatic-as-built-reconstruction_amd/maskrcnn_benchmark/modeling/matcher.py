"""Matcher (reference: maskrcnn_benchmark/modeling/matcher.py:12-106) as the holder of the two IoU thresholds and the two
constants.  The matching itself runs inside the kernels that have the IoU in registers: with set_low_quality_matches_ in
aabr_rpn_label_generation (rpn_glue.rpn_label_matches), without it in aabr_roi_targets (roi_glue.box_head_targets) --
the box head builds its Matcher with allow_low_quality_matches=False (box_head_3d/loss.py:578-582)."""


class Matcher(object):
    BELOW_LOW_THRESHOLD = -1
    BETWEEN_THRESHOLDS = -2

    def __init__(self, high_threshold, low_threshold, allow_low_quality_matches=False, yaw_threshold=3.1416 * 0.4):
        assert low_threshold <= high_threshold
        self.high_threshold = high_threshold
        self.low_threshold = low_threshold
        self.allow_low_quality_matches = allow_low_quality_matches
        self.yaw_threshold = yaw_threshold
