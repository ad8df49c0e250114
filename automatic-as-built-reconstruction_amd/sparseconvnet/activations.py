"""Element-wise activations on the feature matrix; grid and spatial size pass through (reference:
SparseConvNet/sparseconvnet/activations.py:16-69).  Plain torch on `.features`."""
import torch
import torch.nn.functional as F
from torch.nn import Module

from .sparseConvNetTensor import SparseConvNetTensor


class _Activation(Module):
    def fn(self, features):
        raise NotImplementedError

    def forward(self, input):
        return SparseConvNetTensor(self.fn(input.features), input.metadata, input.spatial_size)

    def input_spatial_size(self, out_size):
        return out_size


class Sigmoid(_Activation):
    def fn(self, features):
        return torch.sigmoid(features)


class LeakyReLU(_Activation):
    def __init__(self, leak=1 / 3):
        Module.__init__(self)
        self.leak = leak

    def fn(self, features):
        return F.leaky_relu(features, self.leak)


class Tanh(_Activation):
    def fn(self, features):
        return torch.tanh(features)


class ReLU(_Activation):
    def fn(self, features):
        return F.relu(features)


class ELU(_Activation):
    def fn(self, features):
        return F.elu(features)


class SELU(_Activation):
    def fn(self, features):
        return F.selu(features)
