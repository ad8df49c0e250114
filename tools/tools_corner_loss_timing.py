"""Dev tool: time the corner-connection stage of the corner-ROI box head (csrc/corner_loss.hip) against a plain torch
composition of the same definition on the device -- the reference's arithmetic (bounding_box_3d.py:270-291,451-477;
box_head_3d/loss.py:22-99,384-499) in this project's own words: per scene dense distance matrices, sorts and gathers for
the tables, [n, n, 8] / [n, n, 3] differences with autograd for the losses.

  tables   roi_glue.box_head_targets(corner_groups=True) minus the same call without the flag (the 3 launches the flag
           adds) against `torch_tables` on the outputs of the call without the flag;
  loss     roi_glue.corner_connection_loss forward + backward (3 launches) against `torch_loss` forward + backward.

Shapes: `--shapes` scenes x positives, default 4 x 128 (BATCH_SIZE_PER_IMAGE 512, POSITIVE_FRACTION 0.25) and 1 x 32.
Both sides alternate inside one process: `--repeats` windows of `--iters` calls after `--warmup` calls, device events
around a window that ends in a synchronise; median (min .. max) over the windows.  The two sides are checked against
each other before anything is timed.  Writes the text report to `--out` (profiles/corner_loss_timing.txt)."""
import argparse
import importlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
importlib.import_module("automatic-as-built-reconstruction_amd")
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
KEYS = ("geometric_pull_loss", "semantic_pull_loss", "semantic_push_loss")


def make_scene(rng, p):
    """rooms of four walls that meet at their ends, on a grid; p positives (jittered copies, taking turns over the walls)
    and 3 p far negatives"""
    rooms = max(1, p // 12)
    tg = []
    for r in range(rooms):
        ox, oy = 7.0 * (r % 6), 6.0 * (r // 6)
        for x0, y0, x1, y1 in ((ox, oy, ox + 4, oy + 0.02), (ox + 4, oy, ox + 4.02, oy + 3), (ox, oy + 3, ox + 4, oy + 3.02),
                               (ox, oy, ox + 0.02, oy + 3)):
            tg.append([x0, y0, x1, y1, 0.0, 2.7, 0.08])
    from utils3d.bbox3d_ops_torch import Box3D_Torch
    tg = Box3D_Torch.from_2corners_to_yxzb(torch.tensor(tg, dtype=torch.float32, device=DEV)).cpu().numpy()
    pos = tg[np.arange(p) % len(tg)].astype(np.float64)
    pos[:, 0:3] += rng.normal(0, 0.012, (p, 3))
    pos[:, 6] += rng.normal(0, 0.004, p)
    neg = np.tile(np.array([[0.0, -40.0, 0.0, 0.1, 2.0, 2.7, 0.1]]), (3 * p, 1))
    neg[:, 0] += 3.0 * np.arange(3 * p)
    props = np.concatenate([pos, neg]).astype(np.float32)
    return tg, props[rng.permutation(len(props))]


def top_corners(boxes):
    from utils3d.bbox3d_ops_torch import Box3D_Torch
    c = Box3D_Torch.from_yxzb_to_2corners(boxes)
    p = torch.stack([c[:, [0, 1, 5]], c[:, [2, 3, 5]]], 1)
    off = p.mean(1, keepdim=True) - p
    return (p + off / off.norm(dim=2, keepdim=True) * c[:, 6].view(-1, 1, 1) * 0.5).reshape(-1, 3)


def torch_tables(tg, matched_idx, rows, boxes):
    """one scene: (pos_pos [p], connect_ids [2 p, 8], corner_xyz [2 p, 3]); rows: the sampled proposal rows, boxes theirs"""
    m = 2 * tg.shape[0]
    x = top_corners(tg)
    ar = torch.arange(m, device=DEV)
    near = (torch.cdist(x, x) < 0.1) & ~torch.eye(m, dtype=torch.bool, device=DEV)
    conn = ar.view(1, m).expand(m, m).masked_fill(~near, m).sort(1)[0][:, :3]
    conn = torch.where(conn < m, conn, torch.full_like(conn, -1))
    tgt = matched_idx[rows]
    pos = torch.nonzero(tgt >= 0).squeeze(1)
    st, order = torch.sort(tgt[pos], stable=True)
    pos_pos = pos[order]
    p = pos_pos.shape[0]
    k = torch.arange(p, device=DEV)
    rank = k - torch.searchsorted(st, st)
    firsts = torch.full((tg.shape[0], 4), -1, dtype=torch.int64, device=DEV)
    keep = rank < 4
    firsts[st[keep], rank[keep]] = k[keep]
    tc = (2 * st.view(-1, 1) + torch.arange(2, device=DEV).view(1, 2)).reshape(-1)               # [2 p]
    group = torch.cat([tc.view(-1, 1), conn[tc]], 1)                                             # [2 p, 4]
    f = firsts[group.clamp(min=0) >> 1]                                                           # [2 p, 4, 4]
    cand = torch.where((f >= 0) & (group >= 0).unsqueeze(2), 2 * f + (group & 1).unsqueeze(2), torch.full_like(f, -1))
    ids = cand.reshape(2 * p, 16).sort(1, descending=True)[0][:, :8]
    return pos_pos, ids.to(torch.int32), top_corners(boxes[pos_pos])


def torch_loss(sem, seg_rows, pos_pos, ids, xyz):
    tot, o = [0, 0, 0], 0
    for m, pp, cid, x in zip(seg_rows, pos_pos, ids, xyz):
        n = 2 * pp.shape[0]
        if n:
            s = sem[o:o + m][pp].reshape(n, 8)
            cid = cid.long()
            valid = cid >= 0
            conn = torch.eye(n, dtype=torch.bool, device=DEV)
            conn[cid[valid], torch.arange(n, device=DEV).view(n, 1).expand(n, 8)[valid]] = True
            gd = (x[cid.clamp(min=0)] - x.view(n, 1, 3)).norm(dim=2)
            act = valid & (gd < 0.2)
            tot[0] = tot[0] + (gd * act).sum() / (act.sum() - n).clamp(min=1)
            dist = (s.view(1, n, 8) - s.view(n, 1, 8)).norm(dim=2)
            tot[1] = tot[1] + (dist * conn).sum() / (conn.sum() - n).clamp(min=1)
            push = ~conn & ((x.view(n, 1, 3) - x.view(1, n, 3)).norm(dim=2) < 0.5)
            tot[2] = tot[2] + (torch.clamp(1.0 - dist, min=0) * push).sum() / push.sum().clamp(min=1)
        o += m
    return {k: v / len(seg_rows) for k, v in zip(KEYS, tot)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4x128,1x32")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "corner_loss_timing.txt"))
    args = ap.parse_args()
    import roi_glue
    from maskrcnn_benchmark.modeling.box_coder_3d import BoxCoder3D
    coder = BoxCoder3D(True, None)
    lines = ["corner-connection stage: csrc/corner_loss.hip against a plain torch composition of the same definition; fp32",
             "median of %d windows of %d calls after %d warm-up calls (min .. max); device events"
             % (args.repeats, args.iters, args.warmup)]

    def window(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters

    def race(fns):
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        ts = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                ts[k].append(window(fn))
        return {k: sorted(v) for k, v in ts.items()}

    for shape in args.shapes.split(","):
        nb, p = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(nb * 1000 + p)
        scenes = [make_scene(rng, p) for _ in range(nb)]
        tgs = [torch.as_tensor(s[0]).to(DEV) for s in scenes]
        props = [torch.as_tensor(s[1]).to(DEV) for s in scenes]
        tls = [torch.ones(len(s[0]), dtype=torch.int64, device=DEV) for s in scenes]

        def targets(flag, dbg=None):
            return roi_glue.box_head_targets(props, tgs, tls, 0.1, 0.1, None, 4 * p, 0.25, seed=3, box_coder=coder,
                                             corner_groups=flag, debug=dbg)

        dbg = {}
        out = targets(True, dbg)
        midx, o = [], 0
        for pr in props:
            midx.append(dbg["matched_idx"][o:o + len(pr)])
            o += len(pr)
        assert [len(d["pos_pos"]) for d in out] == [p] * nb, [len(d["pos_pos"]) for d in out]

        def tables_torch():
            return [torch_tables(tgs[b], midx[b], out[b]["rows"], out[b]["bbox3d"]) for b in range(nb)]

        for b, (pp, ids, xyz) in enumerate(tables_torch()):                      # the two sides agree
            assert torch.equal(pp, out[b]["pos_pos"]) and torch.equal(ids, out[b]["connect_ids"])
            assert float((xyz - out[b]["corner_xyz"]).abs().max()) < 1e-5
        seg = [len(d["rows"]) for d in out]
        tabs = ([d["pos_pos"] for d in out], [d["connect_ids"] for d in out], [d["corner_xyz"] for d in out])
        torch.manual_seed(0)
        sem = (torch.randn(sum(seg), 16, device=DEV) * (0.3 / 8 ** 0.5)).requires_grad_(True)

        def loss(fn):
            sem.grad = None
            l = fn(sem, seg, *tabs)
            (l[KEYS[1]] + l[KEYS[2]]).backward()
            return l

        a, ga = loss(roi_glue.corner_connection_loss), sem.grad.clone()
        b, gb = loss(torch_loss), sem.grad.clone()
        a, b = {k: v.detach() for k, v in a.items()}, {k: v.detach() for k, v in b.items()}
        for k in KEYS:
            assert abs(float(a[k]) - float(b[k])) <= 2e-6 * abs(float(b[k])) + 1e-9, (k, float(a[k]), float(b[k]))
        assert float((ga - gb).abs().max()) <= 2e-6 * float(gb.abs().max())
        t = race({"with": lambda: targets(True), "without": lambda: targets(False), "torch": tables_torch,
                  "hip": lambda: loss(roi_glue.corner_connection_loss), "ref": lambda: loss(torch_loss)})
        med = {k: v[len(v) // 2] for k, v in t.items()}
        fmt = lambda k: "%8.3f ms (%.3f .. %.3f)" % (med[k], t[k][0], t[k][-1])
        lines += ["", "%d scenes x %d positives (%d corners per scene, %d sampled rows per scene)" % (nb, p, 2 * p, seg[0]),
                  "  box_head_targets(corner_groups=True)    " + fmt("with"),
                  "  box_head_targets(corner_groups=False)   " + fmt("without"),
                  "  tables, device: the difference          %8.3f ms" % (med["with"] - med["without"]),
                  "  tables, torch composition               " + fmt("torch"),
                  "  loss forward + backward, device         " + fmt("hip"),
                  "  loss forward + backward, torch          " + fmt("ref"),
                  "  loss: torch / device = %.1f" % (med["ref"] / med["hip"])]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fo_:
        fo_.write(text)


if __name__ == "__main__":
    main()
