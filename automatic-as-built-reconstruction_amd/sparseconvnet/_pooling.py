"""Shared machinery of MaxPooling, AveragePooling and UnPooling (the reference writes each module out in full:
maxPooling.py:14-117, averagePooling.py, unPooling.py:13-97).  What stays the reference's: class names, constructor
arguments, the attributes `dimension / pool_size / pool_stride / nFeaturesToDrop`, the spatial-size arithmetic with its
exact-fit assertion, and the text of `__repr__`.  The modules have no parameters; the kernels are csrc/pool.hip."""
from torch.nn import Module

from .sparseConvNetTensor import SparseConvNetTensor
from .utils import toLongTensor


def _dims(t):
    return ",".join(str(int(i)) for i in t)


class PoolingModule(Module):
    label = None         # the name in __repr__
    function = None      # the autograd Function: apply(features, metadata, in_size, out_size, dimension, size, stride, drop)
    unpool = False       # True: the module goes from the coarse level back to the fine one

    def __init__(self, dimension, pool_size, pool_stride, nFeaturesToDrop=0):
        Module.__init__(self)
        self.dimension = dimension
        self.pool_size = toLongTensor(dimension, pool_size)
        self.pool_stride = toLongTensor(dimension, pool_stride)
        self.nFeaturesToDrop = nFeaturesToDrop

    def _fine(self, coarse):
        return (coarse - 1) * self.pool_stride + self.pool_size

    def _coarse(self, fine):
        """floor division (the reference's `/` on LongTensors under the PyTorch it was written for) + its exact-fit check"""
        coarse = (fine - self.pool_size) // self.pool_stride + 1
        assert (self._fine(coarse) == fine).all(), (fine, coarse, self.pool_size, self.pool_stride)
        return coarse

    def forward(self, input):
        out_size = self._fine(input.spatial_size) if self.unpool else self._coarse(input.spatial_size)
        feats = self.function.apply(input.features, input.metadata, input.spatial_size, out_size, self.dimension,
                                    self.pool_size, self.pool_stride, self.nFeaturesToDrop)
        return SparseConvNetTensor(feats, input.metadata, out_size)

    def input_spatial_size(self, out_size):
        """the input size that gives `out_size` (UnPooling: the inverse of its forward arithmetic, with the exact-fit check
        -- the reference's unPooling.py:79-80 repeats the pooling formula there)"""
        return self._coarse(out_size) if self.unpool else self._fine(out_size)

    def __repr__(self):
        iso = all(int(t.min()) == int(t.max()) for t in (self.pool_size, self.pool_stride))
        if iso:
            s = "%s%d/%d" % (self.label, int(self.pool_size[0]), int(self.pool_stride[0]))
        else:
            s = "%s(%s)/(%s)" % (self.label, _dims(self.pool_size), _dims(self.pool_stride))
        if self.nFeaturesToDrop > 0:
            s += " nFeaturesToDrop = %d" % self.nFeaturesToDrop
        return s
