"""Merging walls by their corners on the device (csrc/merge_corners.hip through roi_glue.merge_by_corners): bit-equal to
the numpy restatement (tests/merge_corners_ref.py), merged flags included, on the hand-built scenes of
tests/merge_corners_host.py, a scene at the built limit and set A of the golden file -- ALL scenes in ONE call, computed
once per module; then the reference names, the PostProcessor option and the launch count."""
import os

import numpy as np
import pytest
import torch

import merge_corners_host as H
import merge_corners_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"


def _same(a, b):
    """equal bits, or NaN on both sides"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "merge_corners_golden.npz")))


@pytest.fixture(scope="module")
def batch(golden):
    """every scene of this file in one call: name -> dict(boxes, labels, want, want_merged, trace, got, got_merged)"""
    import roi_glue
    scenes = dict(H.hand_built_scenes())
    scenes["limit"] = H.limit_scene(roi_glue.merge_corners_max_walls())
    for si in range(int(golden["a_scenes"])):
        b = golden["a%d_in" % si]
        scenes["golden a%d" % si] = (b, np.ones(len(b), np.int64))
    names = list(scenes)
    res = {}
    for name in names:
        boxes, labels = scenes[name]
        tr = {}
        want, want_merged = R.merge_scene(boxes, labels, 0.1, trace=tr)
        res[name] = dict(boxes=boxes, labels=labels, want=want, want_merged=want_merged, trace=tr)
    t_boxes = [torch.from_numpy(res[n]["boxes"]).to(DEV) for n in names]
    t_labels = [torch.from_numpy(res[n]["labels"]).to(DEV) for n in names]
    outs, merged = roi_glue.merge_by_corners(t_boxes, t_labels, threshold=0.1, return_merged=True)
    again, merged_again = roi_glue.merge_by_corners(t_boxes, t_labels, threshold=0.1, return_merged=True)
    torch.cuda.synchronize()
    for n, o, m, o2, m2, tb in zip(names, outs, merged, again, merged_again, t_boxes):
        res[n].update(got=o.cpu().numpy(), got_merged=m.cpu().numpy(), again=o2.cpu().numpy(),
                      merged_again=m2.cpu().numpy(), t_boxes=tb, t_labels=t_labels[names.index(n)], t_out=o)
    return res


@pytest.mark.parametrize("name", ["no rows", "no wall", "one wall", "L", "T", "cross", "six", "skip", "chain",
                                  "interleaved", "300 walls", "limit"])
def test_scene_is_bit_equal_to_the_restatement(batch, name):
    s = batch[name]
    assert name in ("no rows", "no wall", "one wall") or s["trace"]["margin"] >= 1e-3   # a condition on the inputs
    assert s["got"].shape == s["boxes"].shape and s["got_merged"].shape == (len(s["boxes"]), 2)
    assert _same(s["got"], s["want"])
    assert (s["got_merged"] == s["want_merged"]).all()
    sel = s["labels"] == 1
    assert R.same_bits(s["got"][~sel], s["boxes"][~sel]) and not s["got_merged"][~sel].any()
    if sel.any():
        assert (s["got"][sel, 2] == s["got"][sel, 2][0]).all()                    # the scene's mean z0 on every wall
    if name == "skip":
        big = [did for ids, did in s["trace"]["steps"] if len(ids) > 1]
        assert len(big) == 5 and not any(big) and not s["got_merged"].any()
    if name == "chain":
        # the restatement's sequential rule first (the frozen corners would give a group of three), then the device
        c0 = s["trace"]["corners0"]
        x, y, z = (np.ascontiguousarray(c0[:, d]) for d in range(3))
        frozen = max(len(R.step(x.copy(), y.copy(), z.copy(), i, 0.1)[0]) for i in range(len(c0)))
        assert frozen == 3 and max(len(ids) for ids, _ in s["trace"]["steps"]) == 2
        assert s["got_merged"].sum() == 2
    if name == "300 walls":
        assert sel.sum() == 300 and s["got_merged"].sum() > 300
    if name == "limit":
        assert sel.sum() == len(s["boxes"]) >= 2048


def test_two_runs_give_the_same_bits(batch):
    for name, s in batch.items():
        assert _same(s["got"], s["again"]) and (s["got_merged"] == s["merged_again"]).all(), name


def test_golden_set_a_is_bit_equal_to_the_reference(batch, golden):
    for si in range(int(golden["a_scenes"])):
        s = batch["golden a%d" % si]
        assert R.same_bits(s["got"], golden["a%d_out" % si]), si
        assert (s["got_merged"] == golden["a%d_merged" % si]).all(), si


def test_one_over_the_limit_raises():
    import roi_glue
    limit = roi_glue.merge_corners_max_walls()
    with pytest.raises(ValueError, match="at most %d walls" % limit):
        roi_glue.merge_by_corners([torch.zeros(limit + 1, 7, device=DEV)])


class _List(object):
    def __init__(self, bbox3d, labels=None, size3d=None):
        self.bbox3d, self.mode, self._labels, self.size3d = bbox3d, "yx_zb", labels, size3d

    def get_field(self, name):
        assert name == "labels"
        return self._labels

    def __len__(self):
        return int(self.bbox3d.shape[0])


def test_reference_names_single_lists_and_list_of_lists(batch):
    from maskrcnn_benchmark.structures.bounding_box_3d import merge_by_corners, merge_walls_by_corners
    names = ["interleaved", "cross", "no wall", "chain"]
    lists = [_List(batch[n]["t_boxes"].clone(), batch[n]["t_labels"]) for n in names]
    ptrs = [l.bbox3d.data_ptr() for l in lists]
    assert merge_by_corners(lists) is lists                                       # the whole batch: one launch
    for n, l, p in zip(names, lists, ptrs):
        assert l.bbox3d.data_ptr() == p                                           # overwritten in place
        assert _same(l.bbox3d.cpu().numpy(), batch[n]["got"]), n
        one = _List(batch[n]["t_boxes"].clone(), batch[n]["t_labels"])
        assert merge_by_corners(one) is one and _same(one.bbox3d.cpu().numpy(), batch[n]["got"]), n   # per scene
    # merge_walls_by_corners: every row is a wall
    walls = batch["T"]["t_boxes"].clone()
    l = _List(walls)
    assert merge_walls_by_corners(l) is l and _same(l.bbox3d.cpu().numpy(), batch["T"]["got"])
    two = [_List(batch["T"]["t_boxes"].clone()), _List(batch["six"]["t_boxes"].clone())]
    merge_walls_by_corners(two)
    assert _same(two[0].bbox3d.cpu().numpy(), batch["T"]["got"]) and _same(two[1].bbox3d.cpu().numpy(), batch["six"]["got"])


def _head_inputs():
    """two scenes of wall proposals (rooms) and a few door proposals; logits that make every row a confident detection
    of its class; zero regression: the detections are the proposals"""
    props, logits = [], []
    for seed, (gx, gy) in enumerate(((2, 2), (3, 1))):
        walls = np.array(H.rooms(gx, gy, jitter=0.003, seed=20 + seed), np.float32)
        doors = H.other_rows(3, 30 + seed)
        doors[:, 0:2] += 40.0
        doors[:, 6] = 0.0
        p = np.concatenate([walls, doors])
        lg = np.full((len(p), 3), -4.0, np.float32)
        lg[:len(walls), 1] = 4.0 + 0.01 * np.arange(len(walls))
        lg[len(walls):, 2] = 4.0 + 0.01 * np.arange(len(doors))
        props.append(p), logits.append(lg)
    return props, np.concatenate(logits)


def test_post_processor_with_and_without_the_merge():
    import roi_glue
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    from maskrcnn_benchmark.modeling.roi_heads.box_head_3d.inference import PostProcessor
    props, logits = _head_inputs()
    boxes = [_List(torch.from_numpy(p).to(DEV)) for p in props]
    x = (torch.from_numpy(logits).to(DEV), torch.zeros(len(logits), 21, device=DEV), None)
    coder = BoxCoder3D(is_corner_roi=False, weights=(10.0, 10.0, 10.0, 5.0, 5.0, 5.0, 2.0))
    kw = dict(score_thresh=0.05, nms=0.5, nms_aug_thickness=None, detections_per_img=100, box_coder=coder)
    plain = PostProcessor(**kw)(x, boxes)
    # the default is what it was: recomputed through roi_glue.box_detections
    direct = roi_glue.box_detections(x[0], x[1], [b.bbox3d for b in boxes], score_thresh=0.05, nms=0.5,
                                     nms_aug_thickness=None, detections_per_img=100, class_specific=True, box_coder=coder)
    for d, p in zip(direct, plain):
        assert len(p) == len(d["bbox3d"]) > 6
        assert R.same_bits(p.bbox3d.cpu().numpy(), d["bbox3d"].cpu().numpy())
        assert torch.equal(p.get_field("labels"), d["labels"]) and torch.equal(p.get_field("scores"), d["scores"])
        assert torch.equal(p.get_field("rows"), d["rows"])
    merged = PostProcessor(merge_by_corner=True, **kw)(x, boxes)
    want = roi_glue.merge_by_corners([p.bbox3d for p in plain], [p.get_field("labels") for p in plain])
    moved = 0
    for m, p, w in zip(merged, plain, want):
        assert R.same_bits(m.bbox3d.cpu().numpy(), w.cpu().numpy())
        for f in ("labels", "scores", "rows"):
            assert torch.equal(m.get_field(f), p.get_field(f))
        walls = (p.get_field("labels") == 1).cpu().numpy()
        assert R.same_bits(m.bbox3d.cpu().numpy()[~walls], p.bbox3d.cpu().numpy()[~walls])
        moved += int((m.bbox3d != p.bbox3d).any(1).sum())
    assert moved > 6                                                              # the option does something


def _device_ops(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [ev.name for ev in prof.events() if str(ev.device_type).endswith("CUDA")]
    return names


def test_the_call_is_one_kernel_launch_whatever_the_number_of_scenes(batch):
    """the C entry itself, on prepared device arrays: one device operation for 1 scene and for 7"""
    import _hip
    lib = _hip.load()
    for names in (["cross"], ["no rows", "L", "interleaved", "no wall", "300 walls", "six", "chain"]):
        boxes = torch.cat([batch[n]["t_boxes"] for n in names]).contiguous()
        labels = torch.cat([batch[n]["t_labels"] for n in names]).contiguous()
        n_b = [len(batch[n]["boxes"]) for n in names]
        begin = torch.tensor(np.concatenate([[0], np.cumsum(n_b)]).astype(np.int64)).to(DEV)
        out = torch.empty_like(boxes)
        flags = torch.empty((len(boxes), 2), dtype=torch.int32, device=DEV)

        def call():
            _hip.check(lib.aabr_merge_walls_by_corners(_hip.ptr(boxes), _hip.ptr(labels), len(boxes), _hip.ptr(begin),
                                                       len(n_b), max(n_b), 1, 0.1, _hip.ptr(out), _hip.ptr(flags),
                                                       _hip.stream()))

        ops = _device_ops(call)
        assert len(ops) == 1 and "k_merge_walls_by_corners" in ops[0], ops
        want = np.concatenate([batch[n]["got"] for n in names])
        assert _same(out.cpu().numpy(), want)
