"""UnPooling: from a coarse level back to the fine level the Metadata still holds -- every fine site receives the sum of
the coarse sites whose window covers it (one site when size == stride) (reference:
SparseConvNet/sparseconvnet/unPooling.py:13-97; SCN/CPU/UnPooling.cpp)."""
import torch
from torch.autograd import Function

from . import SCN
from ._pooling import PoolingModule


class UnPoolingFunction(Function):
    @staticmethod
    def forward(ctx, input_features, input_metadata, input_spatial_size, output_spatial_size, dimension, pool_size,
                pool_stride, nFeaturesToDrop):
        ctx.input_metadata, ctx.nFeaturesToDrop = input_metadata, nFeaturesToDrop
        ctx.geom = (input_spatial_size, output_spatial_size, pool_size, pool_stride)
        ctx.input_features_shape = input_features.shape
        output_features = input_features.new()
        SCN.UnPooling_updateOutput(input_spatial_size, output_spatial_size, pool_size, pool_stride, input_metadata,
                                   input_features, output_features, nFeaturesToDrop)
        return output_features

    @staticmethod
    def backward(ctx, grad_output):
        # (the kernel writes every element: nothing to zero first)
        grad_input = torch.empty(ctx.input_features_shape, device=grad_output.device, dtype=grad_output.dtype)
        SCN.UnPooling_updateGradInput(*ctx.geom, ctx.input_metadata, grad_input, grad_output.contiguous(),
                                      ctx.nFeaturesToDrop)
        return grad_input, None, None, None, None, None, None, None


class UnPooling(PoolingModule):
    label = "UnPooling"
    function = UnPoolingFunction
    unpool = True
