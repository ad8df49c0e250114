"""The anchor list's two host tables (csrc/anchor_list.h, rpn_glue._anchor_tables) without a GPU: the Python builder
against a brute-force enumeration of [example][map][site][yaw], every entry point's refusal of a bad table before any
launch, and fill_anchor_segs under the host sanitizers in a stand-alone program."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

# counts[m][b]; between them: a map empty for one example, a map empty for all, an example without sites, 1 and 8 maps
COUNTS = {
    "three_maps": [[5, 2, 0, 4], [3, 0, 0, 1], [0, 0, 0, 0]],
    "one_map": [[2, 0, 3]],
    "eight_maps": [[(3 * m + 5 * b) % 4 for b in range(5)] for m in range(8)],
}


def _enumerate(counts, A):
    """every anchor as (example, map, site row, yaw), example-major in list order, by walking the maps' rows"""
    n_maps, nb = len(counts), len(counts[0])
    out = []
    for b in range(nb):
        for m in range(n_maps):
            first = sum(counts[m][:b])
            for r in range(first, first + counts[m][b]):
                for a in range(A):
                    out.append((b, m, r, a))
    return out


@pytest.mark.parametrize("name", sorted(COUNTS))
@pytest.mark.parametrize("A", [1, 3])
def test_anchor_tables_against_enumeration(name, A):
    import rpn_glue
    counts = COUNTS[name]
    n_maps, nb = len(counts), len(counts[0])
    anchors = _enumerate(counts, A)
    seg, site, n_anchor = rpn_glue._anchor_tables(counts, A)
    assert len(seg) == nb * (n_maps + 1) and len(site) == nb * n_maps and len(n_anchor) == nb
    assert sum(n_anchor) == len(anchors)
    for b in range(nb):
        mine = [t for t in anchors if t[0] == b]
        sb, rb = seg[b * (n_maps + 1):(b + 1) * (n_maps + 1)], site[b * n_maps:(b + 1) * n_maps]
        assert sb[0] == 0 and sb[-1] == n_anchor[b] == len(mine)
        # list index j -> (map, row, yaw) through the tables, the way the kernels locate it
        for j, (_, m, r, a) in enumerate(mine):
            mm = max(q for q in range(n_maps) if q == 0 or j >= sb[q])
            assert (mm, rb[mm] + (j - sb[mm]) // A, (j - sb[mm]) % A) == (m, r, a)
    # a chunk that does not start at example 0: the same seg rows, absolute site rows
    for b0, b1 in ((1, nb), (nb - 1, nb), (1, 2), (0, nb)):
        s2, r2, n2 = rpn_glue._anchor_tables(counts, A, b0, b1)
        assert s2 == seg[b0 * (n_maps + 1):b1 * (n_maps + 1)]
        assert r2 == site[b0 * n_maps:b1 * n_maps]
        assert n2 == n_anchor[b0:b1]


def _bad_tables(n_maps, A):
    """two examples over n_maps maps, the second one's row broken three ways"""
    good = [0] + [A * (m + 1) for m in range(n_maps)]
    decreasing = list(good)
    decreasing[-1] = decreasing[-2] - A
    return {"non-decreasing": good + decreasing,
            "starts at 0": good + [v + A for v in good],
            "multiple of A": good + [0] + [v + 1 for v in good[1:]]}


def test_entry_points_refuse_bad_tables_before_any_launch():
    import _hip
    lib = _hip.load()
    one = 4096                                     # a non-null pointer nobody follows
    E, n_maps, A, nb = -1, 2, 3, 2
    ptrs = (_hip.C.c_void_p * 8)(*([one] * 8))
    site = _hip.i32xn([0] * (nb * n_maps))
    f = _hip.f32xn([1.0] * 8)
    k = _hip.i32xn([1] * nb)
    entries = {
        "aabr_rpn_decode_maps": lambda seg: lib.aabr_rpn_decode_maps(
            n_maps, ptrs, ptrs, ptrs, _hip.i32xn(list(seg)[n_maps + 1:]), site, f, one, A, 20.0, f, 10.0, 0.3, 0.3, one, 1,
            one, one, one, None),
        "aabr_rpn_gather_logits": lambda seg: lib.aabr_rpn_gather_logits(n_maps, ptrs, nb, seg, site, A, 64, one, None),
        "aabr_rpn_topk_maps": lambda seg: lib.aabr_rpn_topk_maps(n_maps, ptrs, nb, seg, site, A, k, one, 1, one, one, None),
        "aabr_rpn_label_generation_targets": lambda seg: lib.aabr_rpn_label_generation_targets(
            n_maps, ptrs, nb, seg, site, f, one, A, 20.0, ptrs, k, f, 6, 0, 0.55, 0.2, 0.7, 1, one, one, None, one, f, one,
            None),
        "aabr_rpn_loss_forward": lambda seg: lib.aabr_rpn_loss_forward(
            n_maps, ptrs, ptrs, ptrs, 0, A, nb, seg, site, ptrs, ptrs, 3, 256, 128, 1.0 / 9, one, one, one, one, one, None),
    }
    for name, call in entries.items():
        for what, seg in _bad_tables(n_maps, A).items():
            assert call(_hip.i32xn(seg)) == E, (name, what)
            err = lib.aabr_last_error()
            assert name.encode() in err and what.encode() in err, (name, what, err)


def test_fill_anchor_segs_under_host_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "anchor_list_host")
    base = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-o", exe,
            os.path.join(HERE, "anchor_list_host_harness.cpp")]
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    if r.returncode != 0:
        subprocess.check_call(base)                # the program itself must compile; only the runtime may be missing
        pytest.skip("host sanitizer runtime not installed: " + r.stderr.strip().splitlines()[-1])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout + r.stderr
