"""Generate tests/golden/corner_loss_golden.npz by IMPORTING the reference's corner-connection code and running it on the CPU
(build container only; needs /root/reference):

  * maskrcnn_benchmark/structures/bounding_box_3d.py:270-291,451-477   BoxList3D.get_2top_corners_offseted,
                                                                        get_connect_corner_ids
  * maskrcnn_benchmark/modeling/roi_heads/box_head_3d/loss.py:22-99    get_prop_ids_per_targ
  * loss.py:250-293                                                     subsample_standard (the remap of pos_prop_ids to the
                                                                        sampled list), with `prepare_targets` and the sampler
                                                                        of the instance replaced by the recorded inputs
  * loss.py:384-499                                                     corner_connection_loss, fp32, with torch autograd

The imports go the way of gen_corner_golden.py (placeholders for numba / spconv / open3d, `np.float`), plus empty
placeholder modules for what loss.py imports and this fixture does not run: maskrcnn_benchmark.layers,
structures.boxlist_ops_3d, modeling.seperate_classifier, modeling.box_coder_3d.  The reference runs unedited, with one default changed from outside: `Tensor.sort` is stable while
get_prop_ids_per_targ runs (stable_tensor_sort below).  The matcher
is not run: matched_idx is an input of the fixture (the proposals are jittered copies of their targets, so it is known by
construction).  The integer counts are not values the reference returns; they are counted here from the reference's own
tables and fp32 corner coordinates.

Conditions on the recorded inputs, asserted below in float64 (tests/corner_loss_ref.py):
  * no compared distance lies within 1e-3 of its threshold (0.1 target corners, 0.2 table entries, 0.5 corner pairs);
  * every matched proposal is sampled and the scenes of a case have equal sample sizes -- the regime in which the
    reference agrees with this package's definition;
  * the semantic vectors have norm about 0.3, so that the push term is not 0;
  * some corner has more than 8 candidates, some target more than four positives, some target none, some target corner
    more than three neighbours.
The committed fixture is data only (inputs + expected outputs)."""
import contextlib
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_iou_golden as G  # noqa: E402
import corner_box_ref as CB  # noqa: E402
import corner_loss_ref as CL  # noqa: E402

REF = "/root/reference"
F = np.float32


def wall(x0, y0, x1, y1, zb=0.0, th=0.08, h=2.7):
    """a wall between two end points of its bottom centre line, as a yx_zb box"""
    return CB.from_2corners(np.array([[x0, y0, x1, y1, zb, zb + h, th]]))[0]


def room_scene(rng, ox, oy, junction):
    """a rectangular room whose four walls meet at their ends; `junction`: five more walls that all end in one point, so
    that a target corner there has four neighbours"""
    L, W = 4.0 + rng.uniform(0, 1), 3.0 + rng.uniform(0, 1)
    walls = [wall(ox, oy, ox + L, oy + 0.02), wall(ox + L, oy, ox + L + 0.02, oy + W), wall(ox, oy + W, ox + L, oy + W + 0.02),
             wall(ox, oy, ox + 0.02, oy + W)]
    if junction:
        jx, jy = ox + 10.0, oy
        walls += [wall(jx, jy, jx + 3.0, jy + 0.03), wall(jx - 3.0, jy - 0.03, jx, jy), wall(jx, jy, jx + 0.03, jy + 3.0),
                  wall(jx - 0.03, jy - 3.0, jx, jy), wall(jx, jy, jx + 2.0, jy + 2.1)]
    walls.append(wall(ox + 20.0, oy + 20.0, ox + 23.0, oy + 20.5))           # a lone wall
    return np.array(walls, F)


def jitter(rng, box, k):
    out = np.repeat(box[None], k, 0).astype(np.float64)
    out[:, 0:3] += rng.normal(0, 0.012, (k, 3))
    out[:, 3:6] *= rng.uniform(0.95, 1.05, (k, 3))
    out[:, 6] += rng.normal(0, 0.004, k)
    return out.astype(F)


def make_scene(rng, ox, oy, junction, per_target, n_neg, n_neg_sampled):
    tg = room_scene(rng, ox, oy, junction)
    assert len(per_target) == len(tg)
    props, midx = [], []
    for g, k in enumerate(per_target):
        props.append(jitter(rng, tg[g], k))
        midx += [g] * k
    far = np.array([wall(ox - 30 - 5 * i, oy + 3 * i, ox - 27 - 5 * i, oy + 3 * i + 0.4) for i in range(n_neg)], F)
    props.append(far.reshape(-1, 7))
    midx += [-1] * n_neg
    props, midx = np.concatenate(props).astype(F), np.array(midx, np.int64)
    order = rng.permutation(len(props))                       # the positives of a target are not adjacent rows
    props, midx = props[order], midx[order]
    neg = np.nonzero(midx < 0)[0]
    keep = np.sort(np.concatenate([np.nonzero(midx >= 0)[0], rng.choice(neg, n_neg_sampled, replace=False)]))
    return tg, props, midx, keep.astype(np.int64)


CASES = {
    # per scene: (junction, positives per target, negatives, sampled negatives); equal sample sizes inside a case
    "a": [(True, [3, 2, 1, 0, 3, 3, 3, 6, 3, 1], 6, 3), (False, [4, 5, 2, 2, 0], 20, 15)],
    "b": [(True, [1, 1, 1, 1, 4, 4, 4, 4, 4, 0], 4, 2)],
}


def import_reference():
    G._install_placeholders()
    import collections
    import collections.abc
    collections.Iterable = collections.abc.Iterable
    np.float = float
    sys.modules["open3d"] = types.ModuleType("open3d")
    o3u = types.ModuleType("open3d_util")
    o3u.draw_cus = o3u.gen_animation = None
    sys.modules["open3d_util"] = o3u
    sys.path.insert(0, REF)
    for name, attrs in (("maskrcnn_benchmark.layers", ("smooth_l1_loss",)),
                        ("maskrcnn_benchmark.structures.boxlist_ops_3d", ("boxlist_iou_3d",)),
                        ("maskrcnn_benchmark.modeling.seperate_classifier", ("SeperateClassifier",)),
                        ("maskrcnn_benchmark.modeling.box_coder_3d", ("BoxCoder3D",))):
        mod = types.ModuleType(name)
        for a in attrs:
            setattr(mod, a, None)
        sys.modules[name] = mod
    bb = importlib.import_module("maskrcnn_benchmark.structures.bounding_box_3d")
    loss = importlib.import_module("maskrcnn_benchmark.modeling.roi_heads.box_head_3d.loss")
    return bb, loss


@contextlib.contextmanager
def stable_tensor_sort():
    """get_prop_ids_per_targ orders the positives with `Tensor.sort()`, whose order among equal keys torch leaves open
    (this build returns the equal keys of these inputs in descending row).  The package defines the order as the stable
    one -- by matched target, then ascending row -- so the reference runs here with `stable=True` as the default of that
    call; nothing else of it changes."""
    orig = torch.Tensor.sort

    def sort(self, *a, **k):
        k.setdefault("stable", True)
        return orig(self, *a, **k)

    torch.Tensor.sort = sort
    try:
        yield
    finally:
        torch.Tensor.sort = orig


def margins_ok(seed, scenes):
    """the first condition on the inputs a seed draws, through the restatement: every compared distance keeps 1e-3 from
    its threshold (the seeds are tried in ascending order, so the fixture is reproducible)"""
    rng = np.random.default_rng(seed)
    for si, (junction, per_target, n_neg, n_neg_s) in enumerate(scenes):
        tg, props, midx, keep = make_scene(rng, 50.0 * si, 10.0 * si, junction, per_target, n_neg, n_neg_s)
        conn, mg = CL.target_connect(CL.top_corners(tg))
        pos_pos, ids = CL.prop_tables(midx, keep, conn)
        sem = torch.zeros((len(keep), 16), dtype=torch.float64)
        if mg < 1e-3 or CL.scene_losses(sem, pos_pos, ids, CL.top_corners(props[keep][pos_pos]))[2] < 1e-3:
            return False
    return True


def main():
    bb, loss = import_reference()
    t = torch.from_numpy
    out, seen = {}, dict(cut=False, many=False, none=False, crowded=False)
    for ci, (case, scenes) in enumerate(sorted(CASES.items())):
        seed = next(s for s in range(300 + 100 * ci, 400 + 100 * ci) if margins_ok(s, scenes))
        print(case, "seed", seed)
        rng = np.random.default_rng(seed)
        inst = object.__new__(loss.FastRCNNLossComputation)
        proposals, targets, prepared, masks, data = [], [], ([], [], [], []), ([], []), []
        for si, (junction, per_target, n_neg, n_neg_s) in enumerate(scenes):
            tg, props, midx, keep = make_scene(rng, 50.0 * si, 10.0 * si, junction, per_target, n_neg, n_neg_s)
            tgl = bb.BoxList3D(t(tg.copy()), None, "yx_zb", None, {})
            prl = bb.BoxList3D(t(props.copy()), None, "yx_zb", None, {"prediction": True})
            # BoxList3D wraps the yaw into [-pi/2, pi/2) (the same wall): the fixture records the boxes the reference holds
            tg, props = tgl.bbox3d.numpy().copy(), prl.bbox3d.numpy().copy()
            tg_conn = tgl.get_connect_corner_ids()
            with stable_tensor_sort():
                ids, pos_prop = loss.get_prop_ids_per_targ(t(midx.copy()), tg_conn)
            labels = t((midx >= 0).astype(np.int64))
            for lst, v in zip(prepared, (labels, torch.zeros((len(props), 7)), ids, pos_prop)):
                lst.append(v)
            pos_m = t((midx >= 0).astype(np.uint8))
            neg_m = torch.zeros(len(props), dtype=torch.uint8)
            neg_m[t(keep[midx[keep] < 0])] = 1
            masks[0].append(pos_m)
            masks[1].append(neg_m)
            proposals.append(prl)
            targets.append(tgl)
            data.append((tg, props, midx, keep, tg_conn.numpy(), tgl.get_2top_corners_offseted()[0].reshape(-1, 3).numpy()))
        inst.prepare_targets = lambda p, q: prepared
        inst.fg_bg_sampler = lambda labels: masks
        sampled = inst.subsample_standard(proposals, targets)                 # the reference's remap, unedited
        m = [len(s) for s in sampled]
        assert len(set(m)) == 1, "the scenes of a case need equal sample sizes"
        sem = (np.random.default_rng(400 + ci).normal(0, 0.3 / np.sqrt(8), (sum(m), 16))).astype(F)
        sem_t = t(sem.copy()).requires_grad_(True)
        res = inst.corner_connection_loss(sem_t)
        out["%s_losses" % case] = np.array([res[k].item() for k in CL.KEYS], F)
        out["%s_d_pull" % case] = torch.autograd.grad(res[CL.KEYS[1]], sem_t, retain_graph=True)[0].numpy()
        out["%s_d_push" % case] = torch.autograd.grad(res[CL.KEYS[2]], sem_t, retain_graph=True)[0].numpy()
        out["%s_sem" % case] = sem
        out["%s_scenes" % case] = np.array([len(scenes)], np.int64)
        counts, tabs = [], ([], [], [])
        for si, (tg, props, midx, keep, tg_conn, tg_xyz) in enumerate(data):
            key = "%s_s%d_" % (case, si)
            pos_pos = inst._pos_prop_ids[si].numpy()
            ids = inst._connect_proC_ids_each_proC[si].numpy()
            assert np.array_equal(sampled[si].bbox3d.numpy(), props[keep])
            xyz = sampled[si][inst._pos_prop_ids[si]].get_2top_corners_offseted()[0].reshape(-1, 3).numpy()
            out.update({key + "targets": tg, key + "proposals": props, key + "matched_idx": midx, key + "samp_rows": keep,
                        key + "tg_connect": tg_conn.astype(np.int64), key + "tg_xyz": tg_xyz.astype(F),
                        key + "pos_pos": pos_pos.astype(np.int64), key + "connect_ids": ids.astype(np.int64),
                        key + "corner_xyz": xyz.astype(F)})
            # ---- the conditions, in float64 through the restatement
            assert (midx[keep] >= 0).sum() == (midx >= 0).sum(), "a matched proposal is not sampled"
            assert (CB.tie_margin(tg) >= 1e-3).all() and (CB.tie_margin(props[keep]) >= 1e-3).all()
            r_conn, mg = CL.target_connect(CL.top_corners(tg))
            assert mg >= 1e-3, "a target corner pair within 1e-3 of 0.1"
            assert np.array_equal(r_conn, tg_conn)
            r_pos, r_ids = CL.prop_tables(midx, keep, tg_conn)
            assert np.array_equal(r_pos, pos_pos) and np.array_equal(r_ids, ids)
            d = np.linalg.norm(CL.top_corners(tg)[:, None] - CL.top_corners(tg)[None], axis=2)
            seen["crowded"] |= bool((((d < 0.1).sum(1) - 1) > 3).any())
            per = np.bincount(midx[midx >= 0], minlength=len(tg))
            seen["many"] |= bool((per > 4).any())
            seen["none"] |= bool((per == 0).any())
            for k, s in enumerate(pos_pos):                               # candidates before the cut
                for c in range(2):
                    tc = 2 * midx[keep[s]] + c
                    group = [tc] + [e for e in tg_conn[tc] if e >= 0]
                    seen["cut"] |= sum(min(per[e >> 1], 4) for e in group) > 8
            # the counts, from the reference's tables and its fp32 coordinates
            n = 2 * len(pos_pos)
            conn = np.eye(n, dtype=bool)
            x64 = xyz.astype(np.float64)
            geo_cnt = 0
            for i in range(n):
                for e in ids[i]:
                    if e >= 0:
                        conn[e, i] = True
                        geo_cnt += int(np.linalg.norm(x64[e] - x64[i]) < 0.2)
            close = np.linalg.norm(x64[:, None] - x64[None], axis=2) < 0.5
            counts.append([geo_cnt, int(conn.sum()), int((~conn & close).sum()), n])
            for lst, v in zip(tabs, (pos_pos, ids, CL.top_corners(props[keep][pos_pos]))):
                lst.append(v)
        out["%s_counts" % case] = np.array(counts, np.int64)
        ref = CL.batch_losses(sem, m, *tabs)
        assert ref["margin"] >= 1e-3, "a proposal corner pair within 1e-3 of 0.2 / 0.5: %g" % ref["margin"]
        assert np.array_equal(ref["counts"], out["%s_counts" % case])
        assert out["%s_losses" % case][2] > 0, "the push term is 0"
        print(case, "reference fp32:", out["%s_losses" % case], "restatement:", [ref[k] for k in CL.KEYS], "counts",
              counts, "margin %.3g" % ref["margin"])
        print("   relative error of the reference's fp32 values:",
              [CL.rel_err(out["%s_losses" % case][i], ref[k]) for i, k in enumerate(CL.KEYS)],
              CL.rel_err(out["%s_d_pull" % case], ref["d_pull"]), CL.rel_err(out["%s_d_push" % case], ref["d_push"]))
    assert all(seen.values()), seen
    for k, v in out.items():
        assert v.dtype in (np.float32, np.int64) and (v.dtype == np.int64 or np.isfinite(v).all()), k
    np.savez_compressed(os.path.join(HERE, "corner_loss_golden.npz"), **out)
    print("wrote corner_loss_golden.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
