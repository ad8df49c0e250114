"""numpy restatement of the RPN loss (csrc/rpn_loss.hip, include/aabr_hip.h aabr_rpn_loss_forward): the selection key, the
selection rule and the reference's loss composition (modeling/rpn/loss_3d.py:201-251), for the tests."""
import numpy as np

M32 = np.uint64(0xffffffff)
GOLDEN = np.uint64(0x9E3779B9)


def fmix32(h):
    """murmur3's 32-bit finaliser on uint64 arrays holding 32-bit values"""
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & M32
    h ^= h >> np.uint64(16)
    return h


def chain_key(seed, *values):
    """h = fmix32(seed ^ 0x9E3779B9); h = fmix32(h ^ v) for every v (scalars or arrays, taken mod 2^32)"""
    h = fmix32(np.uint64(int(seed) & 0xffffffff) ^ GOLDEN)
    for v in values:
        h = fmix32(h ^ (np.asarray(v).astype(np.int64).astype(np.uint64) & M32))
    return h


def counts(P, N, batch_size_per_image=256, positive_fraction=0.5):
    """BalancedPositiveNegativeSampler's num_pos / num_neg (balanced_positive_negative_sampler.py:42-47)"""
    num_pos = min(P, int(batch_size_per_image * positive_fraction))
    return num_pos, min(N, batch_size_per_image - num_pos)


def pick(cls_mask, k, keys, *ties):
    """indices of the k entries of the class with the smallest (key, *ties), in that order"""
    idx = np.nonzero(cls_mask)[0]
    if k == 0 or idx.size == 0:
        return idx[:0]
    cols = [t[idx] for t in ties][::-1] + [keys[idx]]
    order = np.lexsort(cols)
    return idx[order[:k]]


def example_anchors(coords, counts_mb, b, A):
    """(map, x, y, z, a) of every anchor of example b in its label order [map][site][yaw]: coords[m] int [V_m, 4] of the
    map in the grid's row order (examples contiguous), counts_mb[m][b] sites of example b in map m"""
    out = []
    for m, c in enumerate(coords):
        s0 = int(sum(counts_mb[m][:b]))
        rows = c[s0:s0 + counts_mb[m][b]]
        n = rows.shape[0]
        mm = np.full(n * A, m, np.int64)
        xyz = np.repeat(rows[:, :3].astype(np.int64), A, axis=0)
        aa = np.tile(np.arange(A, dtype=np.int64), n)
        out.append(np.column_stack([mm, xyz, aa]))
    return np.concatenate(out, 0) if out else np.zeros((0, 5), np.int64)


def sample_maps(coords, counts_mb, A, matched, seed, batch_size_per_image=256, positive_fraction=0.5):
    """the sample of every example: list of (pos, neg) index arrays into the example's label list, in selection order.
    matched[b] = int64 matched indices of example b (>= 0 positive, -1 negative, -2 ignored)"""
    out = []
    for b, lab in enumerate(matched):
        an = example_anchors(coords, counts_mb, b, A)
        assert an.shape[0] == lab.shape[0]
        key = chain_key(seed, b, an[:, 0], an[:, 1], an[:, 2], an[:, 3], an[:, 4])
        pos_m, neg_m = lab >= 0, lab == -1
        kp, kn = counts(int(pos_m.sum()), int(neg_m.sum()), batch_size_per_image, positive_fraction)
        ties = [an[:, i] for i in range(5)]
        out.append((pick(pos_m, kp, key, *ties), pick(neg_m, kn, key, *ties)))
    return out


def sample_list(labels, seed, batch_size_per_image=256, positive_fraction=0.5):
    """the list form (aabr_sample_list): labels[b] with >= 1 positive, == 0 negative; key of (seed, example, index)"""
    out = []
    for b, lab in enumerate(labels):
        lab = np.asarray(lab)
        j = np.arange(lab.shape[0], dtype=np.int64)
        key = chain_key(seed, b, j)
        pos_m, neg_m = lab >= 1, lab == 0
        kp, kn = counts(int(pos_m.sum()), int(neg_m.sum()), batch_size_per_image, positive_fraction)
        out.append((pick(pos_m, kp, key, j), pick(neg_m, kn, key, j)))
    return out


def smooth_l1(d, beta):
    return np.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta)


def loss_and_grads(obj, reg, tgt, pos, neg, beta=1.0 / 9):
    """the reference composition (loss_3d.py:238-249) in float64 on concatenated lists: obj [n] logits, reg / tgt [n, 7],
    pos / neg sampled indices.  Returns (objectness_loss, box_loss, d obj, d reg) for unit upstream gradients."""
    obj = np.asarray(obj, np.float64)
    reg = np.asarray(reg, np.float64)
    tgt = np.asarray(tgt, np.float64)
    sampled = np.concatenate([pos, neg]).astype(np.int64)
    ns = sampled.size
    y = np.concatenate([np.ones(len(pos)), np.zeros(len(neg))])
    x = obj[sampled]
    with np.errstate(invalid="ignore", divide="ignore"):
        bce = (np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))).sum() / ns
        diff = reg[pos] - tgt[pos]
        box = smooth_l1(np.abs(diff), beta).sum() / ns
    g_obj = np.zeros_like(obj)
    g_reg = np.zeros_like(reg)
    if ns:
        g_obj[sampled] = (1.0 / (1.0 + np.exp(-x)) - y) / ns
        g_reg[pos] = np.where(np.abs(diff) < beta, diff / beta, np.sign(diff)) / ns
    return bce, box, g_obj, g_reg
