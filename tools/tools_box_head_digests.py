"""Dev tool: one SHA-256 per case over the raw bytes of everything the box head's public roi_glue functions return --
box_head_loss / box_head_loss_grouped (losses, flag and both gradients), box_detections / box_detections_grouped (the
lists and the `debug` arrays `prob`, `boxes`, `info`), box_head_targets / box_head_targets_grouped (the lists and the
`debug` arrays).  Keys are hashed in sorted order with each tensor's dtype and shape; NaN outputs are compared as bytes.

Two libraries compute the same thing bit for bit when their lists are equal line for line: run this file once from a
checkout of each (it uses the package and the library of the tree it lies in), in a fresh process each.
profiles/box_head_fold_digests.txt holds such a pair.  The inputs are the case builders of the tests
(tests/test_gpu_roi_loss.py, test_gpu_roi_post.py, test_gpu_sep_head.py, roi_post_ref.py); nothing in a test depends on
this tool."""
import argparse
import hashlib
import importlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
importlib.import_module("automatic-as-built-reconstruction_amd")
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
W = (10.0, 10.0, 10.0, 5.0, 5.0, 5.0, 10.0)


def digest(obj):
    h = hashlib.sha256()

    def feed(o):
        if torch.is_tensor(o):
            t = o.detach().cpu().contiguous()
            h.update(("%s%s" % (t.dtype, tuple(t.shape))).encode())
            h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
        elif isinstance(o, dict):
            for k in sorted(o):
                h.update(str(k).encode())
                feed(o[k])
        elif isinstance(o, (list, tuple)):
            h.update(("[%d" % len(o)).encode())
            for v in o:
                feed(v)
        else:                                               # info words, counts, the seed, None
            h.update(repr(o).encode())

    feed(obj)
    return h.hexdigest()


def plain_loss_cases(roi_glue):
    def run(c, class_specific, dtype, n, bad_label=False):
        g = torch.Generator().manual_seed(1000 * c + 10 * n + class_specific)
        labels = torch.randint(0, c, (n,), generator=g)
        if bad_label:
            labels[3], labels[n // 2], labels[n - 1] = c, -1, 1 << 40
        tgt = torch.randn(n, 7, generator=g) * 0.3
        k = c if class_specific else 1
        logits = (torch.randn(n, c, generator=g) * 2).to(DEV, dtype).requires_grad_()
        reg = (torch.randn(n, 7 * k, generator=g) * 0.3 + tgt.repeat(1, k) * 0.9).to(DEV, dtype).requires_grad_()
        cls, box, flag = roi_glue.box_head_loss(logits, reg, labels.to(DEV), tgt.to(DEV), class_specific=class_specific,
                                                return_flag=True)
        (cls + 2 * box).backward()
        return digest({"cls": cls, "box": box, "flag": flag, "grad_logits": logits.grad, "grad_reg": reg.grad})

    for c in (2, 7, 33):
        for class_specific in (True, False):
            for dtype in (torch.float32, torch.bfloat16):
                for n in (0, 1, 257, 5000):
                    yield ("loss plain C %d %s %s n %d" % (c, "specific" if class_specific else "agnostic",
                                                           str(dtype).split(".")[1], n),
                           run(c, class_specific, dtype, n))
    yield "loss plain C 7 specific float32 n 700 labels out of range", run(7, True, torch.float32, 700, True)


def grouped_loss_cases(T):
    def run(logits, reg, sep, lab, tgt):
        cls, box, flag, gx, gr = T._run_loss(logits, reg, sep, lab, tgt)
        return digest({"cls": cls, "box": box, "flag": flag, "grad_logits": gx, "grad_reg": gr})

    for dtype in (torch.float32, torch.bfloat16):
        for n in (0, 1, 300, 5000):
            yield "loss grouped %s n %d" % (str(dtype).split(".")[1], n), run(*T._loss_inputs(n, dtype, 40 + n))
    logits, reg, sep, lab, tgt = T._loss_inputs(700, torch.float32, 9)
    lab[sep == 1] = 0
    sep[sep == 1] = 2
    yield "loss grouped n 700 empty group", run(logits, reg, sep, lab, tgt)
    logits, reg, sep, lab, tgt = T._loss_inputs(700, torch.float32, 10)
    sep[3], sep[350] = 3, -1
    yield "loss grouped n 700 sep_id out of range", run(logits, reg, sep, lab, tgt)
    logits, reg, sep, lab, tgt = T._loss_inputs(700, torch.float32, 10)
    sep[10], lab[10], lab[699] = 1, 2, -1                   # group 1 has 2 columns
    yield "loss grouped n 700 label out of range", run(logits, reg, sep, lab, tgt)


def detection_cases(roi_glue, TP, T, BoxCoder3D):
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    for class_specific in (True, False):
        logits, reg, props = TP._main_case(class_specific)
        reg = reg * np.tile(np.array(W, np.float32), reg.shape[1] // 7)
        for corner in (False, True):
            dbg = {}
            dets = roi_glue.box_detections(t(logits), t(reg), [t(p) for p in props], class_specific=class_specific,
                                           nms_aug_thickness=(0.2, 0.2), detections_per_img=100, debug=dbg,
                                           box_coder=BoxCoder3D(corner, W))
            yield ("detections plain C 7 %s %s" % ("specific" if class_specific else "agnostic",
                                                   "corner" if corner else "centroid"), digest({"dets": dets, "debug": dbg}))
    for name, seed, sep_bad, kw in (("main", 0, False, dict(detections_per_img=100)),
                                    ("negative threshold", 1, False, dict(score_thresh=-1.0, detections_per_img=50)),
                                    ("negative threshold sep_id out of range", 1, True, dict(score_thresh=-1.0))):
        logits, reg, props, sep_id = T._det_case(seed)
        if sep_bad:
            sep_id[7], sep_id[405] = 3, -1
        for corner in (False, True):
            dbg = {}
            dets = roi_glue.box_detections_grouped(t(logits), t(reg), [t(p) for p in props], t(sep_id.astype(np.int32)),
                                                   T.GROUPS, nms_aug_thickness=(0.2, 0.2), debug=dbg,
                                                   box_coder=BoxCoder3D(corner, W), **kw)
            yield "detections grouped %s %s" % (name, "corner" if corner else "centroid"), digest({"dets": dets, "debug": dbg})


def target_cases(roi_glue, TL, T, BoxCoder3D):
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    props, gts, tls = TL._scenes([1000, 300, 2000, 0], [37, 5, 300, 4], 3)
    for corner_groups in (False, True):
        dbg = {}
        out = roi_glue.box_head_targets([t(p) for p in props], [t(g) for g in gts], [t(l) for l in tls], 0.6, 0.3, TL.AUG,
                                        500, 0.25, W, 11, debug=dbg, box_coder=BoxCoder3D(corner_groups, W),
                                        corner_groups=corner_groups)
        yield "targets plain corner_groups %d" % corner_groups, digest({"out": out, "debug": dbg})
    sizes, gtc = [[40, 9, 12], [5, 33, 0]], [[7, 3, 5], [4, 6, 0]]
    props, gts, tls = T._grouped_case(sizes, gtc, T.GROUPS, 6)
    dbg = {}
    out = roi_glue.box_head_targets_grouped([t(p) for p in props], sizes, [t(g) for g in gts], [t(l) for l in tls],
                                            T.GROUPS, 0.6, 0.3, T.AUG, 16, 0.25, W, 7, debug=dbg)
    yield "targets grouped", digest({"out": out, "debug": dbg})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the list to this file")
    args = ap.parse_args()
    import roi_glue
    import test_gpu_roi_loss as TL
    import test_gpu_roi_post as TP
    import test_gpu_sep_head as T
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    lines = []
    for cases in (plain_loss_cases(roi_glue), grouped_loss_cases(T), detection_cases(roi_glue, TP, T, BoxCoder3D),
                  target_cases(roi_glue, TL, T, BoxCoder3D)):
        for name, h in cases:
            lines.append("%s %s" % (name, h))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fo_:
            fo_.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
