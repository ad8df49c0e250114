"""Generate tests/golden/rpn_head_golden.npz by IMPORTING the reference's own code (build container only; needs the
reference tree, /root/reference or $AABR_REFERENCE):

  * maskrcnn_benchmark/modeling/rpn/anchor_generator_sparse3d.py:207-241   generate_anchors_3d (both branches)
  * maskrcnn_benchmark/modeling/rpn/rpn_sparse3d.py:81-108                 RPNHead.__init__: state_dict names and shapes

Modules of the reference that do not import here (compiled extensions, viewers) are replaced by empty placeholders that
nothing below calls.  The committed fixture is data only: anchor arrays, the parameter names and their shapes.
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("AABR_REFERENCE", "/root/reference")


class _Anything(types.ModuleType):
    """a placeholder module: any attribute is a dummy class (decorators and base classes included)"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {"__init__": lambda self, *a, **k: None,
                               "__call__": lambda self, *a, **k: a[0] if a else self})


def _import(name, stubs=16):
    """import `name` from the reference, putting a placeholder wherever one of its imports fails"""
    for _ in range(stubs):
        try:
            return importlib.import_module(name)
        except ImportError as e:
            missing = getattr(e, "name", None)
            if not missing or missing == name:
                raise
            sys.modules[missing] = _Anything(missing)
    raise ImportError(name)


class _Cfg(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def main():
    sys.path.insert(0, REF)
    for alias, ty in (("float", float), ("int", int), ("bool", bool)):     # the reference was written for numpy < 1.20
        if not hasattr(np, alias):
            setattr(np, alias, ty)
    sys.modules["utils3d.bbox3d_ops"] = _Anything("utils3d.bbox3d_ops")    # a viewer, imported for DEBUG only
    ag = _import("maskrcnn_benchmark.modeling.rpn.anchor_generator_sparse3d")
    assert ag.__file__.startswith(REF)
    out = {}
    sets = {"a": ([[0.4, 1.5, 1.5], [1.5, 1.5, 1.0], [4, 4, 1.5], [0.2, 0.5, 3], [0.4, 1.5, 3], [0.6, 2.5, 3]],
                  (0, -1.57, -0.785, 0.785), [[1, 1, 1], [1, 2, 1], [2, 1, 1], [1.7, 1.7, 1]], [1, 1, 1, 1, 1, 1]),
            "b": ([[0.2, 1, 3], [0.5, 2, 3], [1, 3, 3]], (0, -1.57), [[1, 1, 1], [1, 2, 1]], [1, 0, 1]),
            "c": ([[0.3, 0.7, 2.2]], (0.1,), [[1.7, 1.7, 1]], [0])}
    for k, (sizes, yaws, ratios, use) in sets.items():
        s = np.array(sizes, dtype=np.float32)
        y = np.array(yaws, dtype=np.float32).reshape([-1, 1])      # AnchorGenerator.__init__ :59-70
        r = np.array(ratios, dtype=np.float32)
        cells = [ag.generate_anchors_3d(size, y, r, uy).float().numpy() for size, uy in zip(s, use)]
        out[k + "_sizes"], out[k + "_yaws"], out[k + "_ratios"] = s, np.array(yaws, np.float64), r
        out[k + "_use_yaws"] = np.array(use, np.int64)
        out[k + "_anchors"] = np.stack(cells)
    # RPNHead.__init__ needs none of its module's other imports (box coder, loss, post-processor: compiled extensions)
    for name in ("maskrcnn_benchmark.modeling.box_coder_3d", "maskrcnn_benchmark.modeling.rpn.loss_3d",
                 "maskrcnn_benchmark.modeling.rpn.inference_3d", "maskrcnn_benchmark.modeling.seperate_classifier"):
        sys.modules[name] = _Anything(name)
    mod = _import("maskrcnn_benchmark.modeling.rpn.rpn_sparse3d")
    assert mod.__file__.startswith(REF)
    for k, (C, A) in {"h128": (128, 4), "h32": (32, 2)}.items():
        head = mod.RPNHead(_Cfg(MODEL=_Cfg(SEPARATE_CLASSES=[], SEPARATE_RPN=True)), C, A)
        sd = head.state_dict()
        out[k + "_names"] = np.array(list(sd.keys()))
        out[k + "_shapes"] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], np.int64)
        out[k + "_dims"] = np.array([v.dim() for v in sd.values()], np.int64)
        out[k + "_C_A"] = np.array([C, A], np.int64)
    np.savez_compressed(os.path.join(HERE, "rpn_head_golden.npz"), **out)
    print("wrote rpn_head_golden.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
