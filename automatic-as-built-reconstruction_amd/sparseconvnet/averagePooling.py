"""AveragePooling: per output site of the coarser grid, the sum over the active input sites of its window of x / volume --
inactive cells count as zeros (reference: SparseConvNet/sparseconvnet/averagePooling.py; SCN/CPU/AveragePooling.cpp)."""
from torch.autograd import Function

from . import SCN
from ._pooling import PoolingModule


class AveragePoolingFunction(Function):
    @staticmethod
    def forward(ctx, input_features, input_metadata, input_spatial_size, output_spatial_size, dimension, pool_size,
                pool_stride, nFeaturesToDrop):
        ctx.input_metadata, ctx.nFeaturesToDrop = input_metadata, nFeaturesToDrop
        ctx.geom = (input_spatial_size, output_spatial_size, pool_size, pool_stride)
        ctx.save_for_backward(input_features)
        output_features = input_features.new()
        SCN.AveragePooling_updateOutput(input_spatial_size, output_spatial_size, pool_size, pool_stride, input_metadata,
                                        input_features, output_features, nFeaturesToDrop)
        return output_features

    @staticmethod
    def backward(ctx, grad_output):
        input_features, = ctx.saved_tensors
        grad_input = grad_output.new()
        SCN.AveragePooling_updateGradInput(*ctx.geom, ctx.input_metadata, input_features, grad_input,
                                           grad_output.contiguous(), ctx.nFeaturesToDrop)
        return grad_input, None, None, None, None, None, None, None


class AveragePooling(PoolingModule):
    label = "AveragePooling"
    function = AveragePoolingFunction
