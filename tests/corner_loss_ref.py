"""Float64 restatement of the corner-connection losses of the corner-ROI box head and of their label side, written from
the definition ("Corner-connection losses") and the cited lines of the reference, not from the code under test:

  top_corners      structures/bounding_box_3d.py:270-291 (get_2top_corners_offseted): the two top corners of the two-corner
                   form (tests/corner_box_ref.py to_2corners), each moved towards their midpoint by half the thickness
  target_connect   bounding_box_3d.py:451-477 (get_connect_corner_ids): per corner the first three OTHER corners, in
                   ascending index, closer than 0.1; -1 where there are fewer
  prop_tables      box_head_3d/loss.py:22-99 (get_prop_ids_per_targ) and :276-292 (the remap to the sampled list), with this
                   package's definitions: the positives are the SAMPLED rows with matched_idx >= 0, ordered by (matched
                   target, row); a target keeps its first four; a corner's candidates are the kept positives' corners (of
                   the matching parity) of its own target corner and of that corner's connected ones -- 16 slots -- sorted
                   descending and cut to 8
  scene_losses     loss.py:384-499 (corner_connection_loss) for one scene, in torch float64 with autograd; the gradient of
                   a distance that is exactly 0 is 0
  batch_losses     the mean over the scenes; a scene without positives adds 0 and still counts

Inputs are taken at their float32 values and everything is evaluated in float64.  `margins` of the tables / losses are the
smallest distances of any compared length from its threshold: the callers keep them >= 1e-3, so no integer of a table or
a count depends on rounding."""
import numpy as np
import torch

import corner_box_ref as CB

TG_THRESHOLD, ACTIVE, CLOSE, DELTA = 0.1, 0.2, 0.5, 1.0
ETPN, IDS = 4, 8
KEYS = ("geometric_pull_loss", "semantic_pull_loss", "semantic_push_loss")


def top_corners(boxes):
    """yx_zb [t, 7] -> [2 t, 3]: corner 2 g + c of box g"""
    c = CB.to_2corners(np.asarray(boxes, np.float64).reshape(-1, 7))
    p = np.stack([c[:, [0, 1, 5]], c[:, [2, 3, 5]]], 1)                     # [t, 2, 3]
    off = p.mean(1, keepdims=True) - p
    return (p + off / np.linalg.norm(off, axis=2, keepdims=True) * c[:, 6].reshape(-1, 1, 1) * 0.5).reshape(-1, 3)


def _pair_dist(xyz):
    return np.linalg.norm(xyz[:, None, :] - xyz[None, :, :], axis=2)


def target_connect(xyz):
    """[m, 3] -> (int [m, 3], margin)"""
    m = xyz.shape[0]
    out = -np.ones((m, 3), np.int64)
    if m == 0:
        return out, np.inf
    d = _pair_dist(xyz)
    off = d[~np.eye(m, dtype=bool)]
    for i in range(m):
        js = [j for j in range(m) if j != i and d[i, j] < TG_THRESHOLD][:3]
        out[i, :len(js)] = js
    return out, (float(np.abs(off - TG_THRESHOLD).min()) if off.size else np.inf)


def prop_tables(matched_idx, samp_rows, tg_connect):
    """matched_idx int [n] (scene-local target of every proposal, < 0: none), samp_rows int [m] ascending (the scene's
    sample), tg_connect int [2 t, 3] -> (pos_pos int [p], connect_ids int [2 p, 8])"""
    matched_idx, samp_rows = np.asarray(matched_idx, np.int64), np.asarray(samp_rows, np.int64)
    tgt_of = matched_idx[samp_rows] if samp_rows.size else np.zeros(0, np.int64)
    pos = sorted((int(tgt_of[s]), s) for s in range(len(samp_rows)) if tgt_of[s] >= 0)       # (target, position)
    pos_pos = np.array([s for _, s in pos], np.int64)
    firsts = {}
    for k, (tg, _) in enumerate(pos):
        if len(firsts.setdefault(tg, [])) < ETPN:
            firsts[tg].append(k)
    ids = -np.ones((2 * len(pos), IDS), np.int64)
    for k, (tg, _) in enumerate(pos):
        for c in range(2):
            tc = 2 * tg + c
            group = [tc] + [int(e) for e in tg_connect[tc] if e >= 0]
            cand = sorted((2 * k2 + (e & 1) for e in group for k2 in firsts.get(e >> 1, [])), reverse=True)[:IDS]
            ids[2 * k + c, :len(cand)] = cand
    return pos_pos, ids


def scene_losses(sem_rows, pos_pos, connect_ids, xyz):
    """sem_rows: torch float64 [m, 16] (the scene's sampled rows); pos_pos [p]; connect_ids [2 p, 8]; xyz [2 p, 3] float64.
    Returns ((geometric, pull, push) torch 0-dim float64, counts [4] = geometric entries, connected pairs, push pairs, n,
    margin)"""
    n = 2 * len(pos_pos)
    zero = sem_rows.sum() * 0
    if n == 0:
        return (zero, zero, zero), np.array([0, 0, 0, 0], np.int64), np.inf
    xyz = np.asarray(xyz, np.float64)
    sem = sem_rows[torch.as_tensor(np.asarray(pos_pos, np.int64))].reshape(n, 8)
    conn = np.eye(n, dtype=bool)                                             # conn[a, i]: a is i or an entry of i's row
    geo_sum, geo_cnt, margin = 0.0, 0, np.inf
    for i in range(n):
        for e in connect_ids[i]:
            if e >= 0:
                conn[e, i] = True
                d = float(np.linalg.norm(xyz[e] - xyz[i]))
                margin = min(margin, abs(d - ACTIVE))
                if d < ACTIVE:
                    geo_sum, geo_cnt = geo_sum + d, geo_cnt + 1
    d2 = ((sem[None, :, :] - sem[:, None, :]) ** 2).sum(2)
    nz = d2 > 0
    dist = torch.where(nz, torch.sqrt(torch.where(nz, d2, torch.ones_like(d2))), torch.zeros_like(d2))
    geo = _pair_dist(xyz)
    margin = min(margin, float(np.abs(geo[~conn] - CLOSE).min()) if (~conn).any() else np.inf)
    push_mask = ~conn & (geo < CLOSE)
    pull = (dist * torch.as_tensor(conn, dtype=torch.float64)).sum() / max(int(conn.sum()) - n, 1)
    push = (torch.clamp(DELTA - dist, min=0) * torch.as_tensor(push_mask, dtype=torch.float64)).sum() \
        / max(int(push_mask.sum()), 1)
    geometric = zero + geo_sum / max(geo_cnt - n, 1)
    return (geometric, pull, push), np.array([geo_cnt, int(conn.sum()), int(push_mask.sum()), n], np.int64), margin


def batch_losses(sem, seg_rows, pos_pos, connect_ids, xyz):
    """sem: float array [n, 16]; the other arguments are per-scene lists.  Returns dict: the three losses (float), `counts`
    int [nb, 4], `d_pull` / `d_push` float64 [n, 16] (gradients of the two semantic losses), `margin`"""
    t = torch.tensor(np.asarray(sem, np.float64), dtype=torch.float64, requires_grad=True)
    tot, counts, margin, o = [t.sum() * 0] * 3, [], np.inf, 0
    for m, pp, ids, x in zip(seg_rows, pos_pos, connect_ids, xyz):
        ls, c, mg = scene_losses(t[o:o + m], np.asarray(pp), np.asarray(ids), x)
        tot = [a + b for a, b in zip(tot, ls)]
        counts.append(c)
        margin = min(margin, mg)
        o += m
    tot = [v / len(seg_rows) for v in tot]
    out = {k: float(v.detach()) for k, v in zip(KEYS, tot)}
    for name, v in (("d_pull", tot[1]), ("d_push", tot[2])):
        g, = torch.autograd.grad(v, t, retain_graph=True, allow_unused=True)
        out[name] = np.zeros(t.shape) if g is None else g.numpy()
    out["counts"], out["margin"] = np.array(counts, np.int64).reshape(-1, 4), margin
    return out


def rel_err(got, want):
    """the error measure of the tests: |got - want| / |want| for a loss; max |got - want| / max |want| for a gradient
    tensor (its elements are sums of terms of both signs, so an element's own magnitude says nothing about its error)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    den = np.abs(want).max() if want.size else 0.0
    return float(np.abs(got - want).max() / den) if den > 0 else float(np.abs(got - want).max() if want.size else 0.0)
