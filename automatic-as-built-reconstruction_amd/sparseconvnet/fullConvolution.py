"""FullConvolution / TransposeConvolution: the transposed convolution that GROWS the set of active sites -- it writes to every
site a filter can reach from an active input site, out[p * stride + q] += in[p] @ W[q], and returns a tensor with a NEW
Metadata that holds the grown level (reference: SparseConvNet/sparseconvnet/fullConvolution.py:14-158; layer machinery
shared in _sparseConv.py).  `Deconvolution`, by contrast, only writes to the sites an earlier `Convolution` left behind."""
from ._sparseConv import SparseConvModule, SparseConvFunction
from .metadata import Metadata
from .sparseConvNetTensor import SparseConvNetTensor
from .utils import optionalTensor


class FullConvolution(SparseConvModule):
    kind = "full"

    def __init__(self, dimension, nIn, nOut, filter_size, filter_stride, bias, groups=1):
        self._setup(dimension, nIn, nOut, filter_size, filter_stride, bias, groups)

    def forward(self, input):
        assert input.features.nelement() == 0 or input.features.size(1) == self.nIn, (self.nIn, self.nOut, input)
        out_sz = (input.spatial_size - 1) * self.filter_stride + self.filter_size
        out_md = Metadata(self.dimension)       # (takes the input's site order when its level is built)
        feats = SparseConvFunction.apply(input.features, self.weight, optionalTensor(self, "bias"),
                                         (input.metadata, out_md), "full",
                                         (input.spatial_size, out_sz, self.filter_size, self.filter_stride))
        return SparseConvNetTensor(feats, out_md, out_sz)

    def deconvolutionForward(self, input):
        """the layer's weights run as a `Deconvolution` inside the input's own Metadata (fullConvolution.py:53-70)"""
        assert input.features.nelement() == 0 or input.features.size(1) == self.nIn, (self.nIn, self.nOut, input)
        out_sz = (input.spatial_size - 1) * self.filter_stride + self.filter_size
        feats = SparseConvFunction.apply(input.features, self.weight, optionalTensor(self, "bias"), input.metadata,
                                         "deconv", (input.spatial_size, out_sz, self.filter_size, self.filter_stride))
        return SparseConvNetTensor(feats, input.metadata, out_sz)

    def input_spatial_size(self, out_size):
        in_size = (out_size - self.filter_size) // self.filter_stride + 1
        assert ((in_size - 1) * self.filter_stride + self.filter_size == out_size).all(), (
            out_size, self.filter_size, self.filter_stride)
        return in_size


TransposeConvolution = FullConvolution
