"""Dev tool: time the RPN stages of the separated classifier (MODEL.SEPARATE_CLASSES with SEPARATE_RPN) -- head forward +
backward (rpn_glue.rpn_head_grouped), labels (rpn_label_matches_grouped), loss forward + backward (rpn_loss_grouped) and
proposals (rpn_proposals_grouped), one grouped call each -- against (b) the per-group loop built only from the
single-group entry points: the plain head with each group's weight rows sliced out, rpn_label_matches, rpn_loss and
rpn_proposals once per group, which is what the reference does (modeling/seperate_classifier.py:68-109).

Shape: `--scenes` 4 scenes of `--points` points, 2 maps, C = 128, A = 4 yaws, G = 3 groups ([[wall], [window]] of four
classes), `--gt` 30 ground-truth boxes per scene, batch 256 per segment; fp32.

Both paths alternate inside one process: `--repeats` windows of `--iters` calls each after `--warmup` calls, the HOST clock
around a window that ends in a device synchronise (these stages are bound by launches and host reads, which device events
would not see); median and spread (min .. max) over the windows.  The library calls of one call of each path are counted
by wrapping the loaded library's functions.  Writes the text report to `--out` (profiles/sep_rpn_timing.txt).  Nothing in
a test depends on these figures."""
import argparse
import importlib
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
importlib.import_module("automatic-as-built-reconstruction_amd")
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
C, A, G = 128, 4, 3
CLASSES = ("background", "wall", "door", "window")
IDS = [[1], [3]]
STRIDES = [[4.0] * 3, [8.0] * 3]
AUG = {"target_Y": 0.4, "anchor_Y": 0, "target_Z": 0.8, "anchor_Z": 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--gt", type=int, default=30)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sep_rpn_timing.txt"))
    args = ap.parse_args()
    import _hip
    import rpn_glue
    import sparseconvnet as scn
    import synth_scenes as S
    from maskrcnn_benchmark.modeling.rpn.anchor_generator_sparse3d import make_anchor_generator
    from maskrcnn_benchmark.modeling.seperate_classifier import SeperateClassifier
    nb = args.scenes
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    torch.manual_seed(2)
    locs, feats = S.make_batch(nb, args.points, 31, 20)
    layer = scn.InputLayer(3, list(S.FULL_SCALE), mode=4)
    c1 = scn.Convolution(3, 9, 32, 2, 2, False).to(DEV)
    c2 = scn.Convolution(3, 32, C, 2, 2, False).to(DEV)
    c3 = scn.Convolution(3, C, C, 2, 2, False).to(DEV)
    with torch.no_grad():
        x = layer([torch.as_tensor(locs).to(DEV), torch.as_tensor(feats).to(DEV)])
        m0 = c2(c1(x))
        maps = [m0, c3(m0)]
    gen = make_anchor_generator(rpn_glue.rpn_cfg(C=C, yaws=(0, -1.57, -0.785, 0.785), strides=STRIDES, voxel_scale=20.0))
    assert gen.num_anchors_per_location() == A
    sc = SeperateClassifier(IDS, len(CLASSES), False, "RPN")
    rng = np.random.default_rng(0)
    gts = [t(S.make_gt_boxes(args.gt, 3 + b)) for b in range(nb)]
    labels = [t(rng.integers(1, 4, args.gt).astype(np.int64)) for _ in range(nb)]
    gp = torch.Generator().manual_seed(0)
    par = [(torch.randn(C, C, generator=gp) / C ** 0.5), 0.1 * torch.randn(C, generator=gp),
           torch.randn(A * G, C, generator=gp) / C ** 0.5, torch.randn(A * G, generator=gp),
           0.1 * torch.randn(7 * A * G, C, generator=gp) / C ** 0.5, 0.1 * torch.randn(7 * A * G, generator=gp)]
    par = [p.to(DEV).requires_grad_() for p in par]
    fl = [m.features.detach().clone().requires_grad_() for m in maps]
    sliced = [(par[0], par[1], par[2].detach().view(A, G, C)[:, g].contiguous().requires_grad_(),
               par[3].detach().view(A, G)[:, g].contiguous().requires_grad_(),
               par[4].detach().view(A, G, 7, C)[:, g].reshape(7 * A, C).contiguous().requires_grad_(),
               par[5].detach().view(A, G, 7)[:, g].reshape(7 * A).contiguous().requires_grad_()) for g in range(G)]

    def clear():
        for q in par + fl + [p for s in sliced for p in s[2:]]:
            q.grad = None

    def head_grouped():
        clear()
        obj, reg = rpn_glue.rpn_head_grouped(fl, *par, G)
        torch.autograd.backward(obj + reg, [torch.ones_like(v) for v in obj + reg])

    def head_loop():
        clear()
        for g in range(G):
            obj, reg = rpn_glue.rpn_head(fl, *sliced[g])
            torch.autograd.backward(obj + reg, [torch.ones_like(v) for v in obj + reg])

    boxes, _local, _rows, _counts = rpn_glue.rpn_group_targets(gts, labels, sc)
    flat = [boxes[b][g] for b in range(nb) for g in range(G)]
    lab_kw = dict(batch_size=nb, yaw_threshold=0.7, regression_targets=True)

    def labels_grouped():
        return rpn_glue.rpn_label_matches_grouped(maps, gen.cell_anchors, STRIDES, 20.0, flat, G, AUG, 6, 0.55, 0.2, **lab_kw)

    def labels_loop():
        return [rpn_glue.rpn_label_matches(maps, gen.cell_anchors, STRIDES, 20.0, [boxes[b][g] for b in range(nb)], AUG, 6,
                                           0.55, 0.2, **lab_kw) for g in range(G)]

    with torch.no_grad():
        obj, reg = rpn_glue.rpn_head_grouped(fl, *par, G)
    obj_l = [o.clone().requires_grad_() for o in obj]
    reg_l = [r.clone().requires_grad_() for r in reg]
    obj_s = [[o[g].clone().requires_grad_() for o in obj] for g in range(G)]
    reg_s = [[r[g].clone().requires_grad_() for r in reg] for g in range(G)]
    lab_g = labels_grouped()
    lab_p = labels_loop()

    def loss_grouped():
        for q in obj_l + reg_l:
            q.grad = None
        lo, lb = rpn_glue.rpn_loss_grouped(maps, obj_l, reg_l, lab_g, gen.cell_anchors, G, 256, 0.5, seed=1)
        (lo.sum() + lb.sum()).backward()

    def loss_loop():
        for g in range(G):
            for q in obj_s[g] + reg_s[g]:
                q.grad = None
            lo, lb = rpn_glue.rpn_loss(maps, obj_s[g], reg_s[g], lab_p[g], gen.cell_anchors, 256, 0.5, seed=1)
            (lo + lb).backward()

    pr_kw = dict(batch_size=nb)

    def proposals_grouped():
        return rpn_glue.rpn_proposals_grouped(maps, obj, reg, G, gen.cell_anchors, STRIDES, 20.0, 2000, 1000, 0.5, (0.3, 0.3),
                                              **pr_kw)

    def proposals_loop():
        return [rpn_glue.rpn_proposals(maps, obj_s[g], reg_s[g], gen.cell_anchors, STRIDES, 20.0, 2000, 1000, 0.5, (0.3, 0.3),
                                       **pr_kw) for g in range(G)]

    lib = _hip.load()

    def library_calls(fn):
        """the library's functions one call of `fn` goes through, counted"""
        calls, saved = {}, {}
        for name in _hip._SIGS:
            f = getattr(lib, name, None)
            if f is None or name in ("aabr_last_error", "aabr_version"):
                continue
            saved[name] = f

            def wrap(*a, _f=f, _n=name):
                calls[_n] = calls.get(_n, 0) + 1
                return _f(*a)
            setattr(lib, name, wrap)
        try:
            with torch.no_grad() if fn in (proposals_grouped, proposals_loop) else torch.enable_grad():
                fn()
        finally:
            for name, f in saved.items():
                setattr(lib, name, f)
        return calls

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.iters

    lines = ["Separated-classifier RPN: %d scenes, maps of %s sites, C = %d, A = %d, G = %d groups, %d ground-truth boxes per "
             "scene; fp32" % (nb, [int(m.features.shape[0]) for m in maps], C, A, G, args.gt),
             "(a) grouped = one grouped call per stage; (b) loop = the single-group call once per group (the plain head on "
             "sliced weights, rpn_label_matches, rpn_loss, rpn_proposals)",
             "median of %d windows of %d calls after %d warm-up calls (min .. max); host clock around a window that ends in a "
             "device synchronise" % (args.repeats, args.iters, args.warmup),
             "kernel launches of the head: grouped 1 forward + 2 backward; loop %d x (1 + 2)" % G,
             "kernel launches of the loss: grouped 1 memset + 4 per 16 segments + 1 forward (%d segments), 1 per 16 segments "
             "backward; loop %d x (1 memset + 4 + 1 forward, 1 backward)" % (nb * G, G)]
    for name, a, b in (("head forward + backward", head_grouped, head_loop),
                       ("labels (IoU, match, encode)", labels_grouped, labels_loop),
                       ("loss forward + backward", loss_grouped, loss_loop),
                       ("proposals (top-k, decode, NMS)", proposals_grouped, proposals_loop)):
        for fn in (a, b):
            for _ in range(args.warmup):
                fn()
        ts = {a: [], b: []}
        for _ in range(args.repeats):
            for fn in (a, b):
                ts[fn].append(window(fn))
        med = {}
        for label, fn in (("grouped", a), ("loop", b)):
            v = sorted(ts[fn])
            med[label] = v[len(v) // 2]
            calls = library_calls(fn)
            lines.append("%-32s %-8s %8.3f ms (%.3f .. %.3f)  library calls: %d (%s)"
                         % (name, label, med[label], v[0], v[-1], sum(calls.values()),
                            ", ".join("%s x %d" % (k.replace("aabr_", ""), n) for k, n in sorted(calls.items()))))
        lines.append("%-32s grouped / loop = %.2f" % (name, med["grouped"] / med["loop"]))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fo_:
        fo_.write(text)


if __name__ == "__main__":
    main()
