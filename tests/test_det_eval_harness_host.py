"""csrc/det_eval.h in a stand-alone program under the host sanitizers (tests/det_eval_host_harness.cpp; nothing is loaded
into Python): the descending-score order key against the restatement's ordering on a table with +-0, denormals, equal
scores, +-inf and NaN, and the 11-point accumulation against the restatement bit for bit on recorded flag sequences."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import det_eval_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32

SCORES = np.array([0.5, -0.0, 1e-45, 0.0, np.inf, 0.5, -1e-45, -np.inf, np.nan, 1e-40, 0.25, -3.0, 0.5, 1.0,
                   3.4028235e38, -0.0, np.nan, 0.70000005, 0.7, -1e-40], F)


def _sequences():
    """(n_pos, flags, pred_iou, scores) in score order: the golden's class 1, a class without ground truth, one whose
    first detection is a true positive at full recall, NaN / inf IoUs, and a long random one"""
    rng = np.random.default_rng(5)
    g = np.load(os.path.join(HERE, "golden", "det_eval_golden.npz"))
    org = g["org_1"]
    tp = np.rint(org[:, 1] * np.arange(1, len(org) + 1)).astype(np.int64)
    flags = np.diff(np.concatenate([[0], tp]))
    out = [(int(round(tp[-1] / org[-1, 0])), flags, org[:, 3].astype(F), org[:, 2].astype(F))]
    out.append((0, np.zeros(4, np.int64), np.zeros(4, F), np.array([0.9, 0.8, 0.8, 0.1], F)))
    out.append((1, np.array([1, 0, 0]), np.array([1.0, 0.3, 0.0], F), np.array([0.6, 0.6, 0.2], F)))
    out.append((3, np.array([0, 1, 1, 0, 1]), np.array([np.nan, 0.6, np.inf, 0.1, 0.55], F),
                np.array([0.9, 0.8, 0.7, 0.6, np.nan], F)))
    n = 700
    fl = (rng.random(n) < 0.4).astype(np.int64)
    out.append((int(fl.sum()) + 5, fl, rng.random(n).astype(F), np.sort(rng.integers(0, 50, n))[::-1].astype(F) / F(50)))
    return out


def _restated(n_pos, flags, iou, scores):
    """the restatement's class_curve on a sequence that is already in score order (scores descending, so its own
    ordering leaves the positions where they are)"""
    assert R.score_order(scores).tolist() == list(range(len(scores)))
    return R.class_curve(scores, flags.astype(np.int8), iou, n_pos)


def _hex32(a):
    return " ".join("%08x" % v for v in np.asarray(a, F).view(np.uint32))


def test_det_eval_header_under_host_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "det_eval_host")
    base = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-o", exe,
            os.path.join(HERE, "det_eval_host_harness.cpp")]
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    if r.returncode != 0:
        # only a missing sanitizer runtime (the linker cannot find libclang_rt.asan / ubsan) is a reason to skip, and only
        # if the program compiles without the sanitizers; any other failure of the sanitized build is a failure
        missing = re.search(r"(cannot (find|open)|no such file|unable to find)[^\n]*(clang_rt|asan|ubsan)", r.stderr, re.I)
        assert missing, "the sanitized build failed:\n" + r.stderr
        subprocess.check_call(base)
        pytest.skip("host sanitizer runtime not installed: " + missing.group(0))
    seqs = _sequences()
    cmds = ["S %d %s" % (len(SCORES), _hex32(SCORES))]
    for n_pos, flags, iou, scores in seqs:
        cmds.append("M %d %d" % (n_pos, len(flags)))
        cmds += ["%d %s %s" % (f, _hex32([u]), _hex32([s])) for f, u, s in zip(flags, iou, scores)]
    path = str(tmp_path / "commands.txt")
    with open(path, "w") as f:
        f.write("\n".join(cmds) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines[-1] == "ok", r.stdout + r.stderr
    order = [int(v) for v in lines[0].split()[1:]]
    assert lines[0].startswith("O") and order == R.score_order(SCORES).tolist()
    keys = [int(v, 16) for v in lines[1].split()[1:]]
    assert keys[1] == keys[3] == keys[15] and keys[8] == keys[16] == 0xffffffff      # -0.0 == +0.0; one key for NaN
    for (n_pos, flags, iou, scores), line in zip(seqs, lines[2:]):
        want = _restated(n_pos, flags, iou, scores)
        got = np.array([int(v, 16) for v in line.split()[1:]], np.uint64).view(np.float64)
        assert R.same_bits(got[0], want["ap"]), (n_pos, got[0], want["ap"])
        assert R.same_bits(got[1:].reshape(11, 4), want["steps"]), (n_pos, got[1:].reshape(11, 4), want["steps"])
