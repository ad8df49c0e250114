"""`merge_by_corners` and `merge_walls_by_corners` under the reference's names (maskrcnn_benchmark/structures/
bounding_box_3d.py:843-923): wall ends that meet at a joint are snapped to a common point and the walls rebuilt from the
snapped corners.  The reference loops over the 2W corners of one scene in Python, a dozen small kernels and two host reads
per corner; here a call is one launch of csrc/merge_corners.hip (roi_glue.merge_by_corners), whatever the number of scenes.

This module holds these two functions only -- it is not a port of BoxList3D.  `boxlist` is duck-typed: `.bbox3d` [n, 7],
`.mode` and, for merge_by_corners, `get_field('labels')`.  As upstream the list's `bbox3d` is overwritten in place and the
list returned.  The lists of this package are yx_zb; `mode == 'standard'` raises ValueError.  As an extension both
functions accept a list (or tuple) of box lists: the whole batch is then one launch, and the list of lists is returned.
(Upstream's merge_by_corners does not hand its `threshold` on to merge_walls_by_corners; here it is used.)"""
import roi_glue

WALL_LABEL = 1        # `boxlist.get_field('labels') == 1` upstream


def _lists(boxlist):
    many = isinstance(boxlist, (list, tuple))
    lists = list(boxlist) if many else [boxlist]
    for b in lists:
        if getattr(b, "mode", "yx_zb") != "yx_zb":
            raise ValueError("merge_by_corners: the box lists of this package are yx_zb, got mode %r" % (b.mode,))
    return many, lists


def _write_back(lists, outs):
    for b, o in zip(lists, outs):
        b.bbox3d.copy_(o)          # in place; the rows that are no wall receive the bits they already hold


def merge_by_corners(boxlist, threshold=0.1):
    """the rows with label 1 are the walls of a scene; the other rows keep their bits"""
    many, lists = _lists(boxlist)
    outs = roi_glue.merge_by_corners([b.bbox3d for b in lists], [b.get_field("labels") for b in lists],
                                     threshold=threshold, wall_label=WALL_LABEL)
    _write_back(lists, outs)
    return boxlist if many else lists[0]


def merge_walls_by_corners(boxlist, threshold=0.1):
    """every row is a wall"""
    many, lists = _lists(boxlist)
    outs = roi_glue.merge_by_corners([b.bbox3d for b in lists], None, threshold=threshold)
    _write_back(lists, outs)
    return boxlist if many else lists[0]
