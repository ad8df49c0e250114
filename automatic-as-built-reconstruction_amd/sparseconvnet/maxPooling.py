"""MaxPooling: per output site of the coarser grid, the maximum over the active input sites of its window and 0
(reference: SparseConvNet/sparseconvnet/maxPooling.py:14-117; SCN/CPU/MaxPooling.cpp).  The leading `nFeaturesToDrop`
planes of the input are left out of the result."""
from torch.autograd import Function

from . import SCN
from ._pooling import PoolingModule


class MaxPoolingFunction(Function):
    @staticmethod
    def forward(ctx, input_features, input_metadata, input_spatial_size, output_spatial_size, dimension, pool_size,
                pool_stride, nFeaturesToDrop):
        ctx.input_metadata, ctx.nFeaturesToDrop = input_metadata, nFeaturesToDrop
        ctx.geom = (input_spatial_size, output_spatial_size, pool_size, pool_stride)
        output_features = input_features.new()
        SCN.MaxPooling_updateOutput(input_spatial_size, output_spatial_size, pool_size, pool_stride, input_metadata,
                                    input_features, output_features, nFeaturesToDrop)
        ctx.save_for_backward(input_features, output_features)
        return output_features

    @staticmethod
    def backward(ctx, grad_output):
        input_features, output_features = ctx.saved_tensors
        grad_input = grad_output.new()
        SCN.MaxPooling_updateGradInput(*ctx.geom, ctx.input_metadata, input_features, grad_input, output_features,
                                       grad_output.contiguous(), ctx.nFeaturesToDrop)
        return grad_input, None, None, None, None, None, None, None


class MaxPooling(PoolingModule):
    label = "MaxPooling"
    function = MaxPoolingFunction
