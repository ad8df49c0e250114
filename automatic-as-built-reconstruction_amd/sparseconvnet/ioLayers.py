"""InputLayer / OutputLayer and their batched forms BLInputLayer / BLOutputLayer (reference:
SparseConvNet/sparseconvnet/ioLayers.py:15-160,163-283).

Same constructor, same (coords, features[, batch_size]) input tuple, same modes.  The
reference forces `coords` to the host (`input[0].cpu().long()`, :60) because its hash grid is
a host structure; here the grid is built on the device, so device-resident coordinates are
used as they are and host coordinates are uploaded once."""
import torch
from torch.autograd import Function
from torch.nn import Module

from . import SCN
from .utils import toLongTensor
from .sparseConvNetTensor import SparseConvNetTensor
from .metadata import Metadata


class _InputLayerBase(Module):
    """what InputLayer and BLInputLayer share: constructor, `to`, `site_order` and the ahead-of-time `prepare`; a subclass
    says how its coordinate layout is enqueued (`_enqueue`)"""

    def __init__(self, dimension, spatial_size, mode=3):
        Module.__init__(self)
        self.dimension = dimension
        self.spatial_size = toLongTensor(dimension, spatial_size)
        self.mode = mode
        self.device = None
        # extension (SCN.Metadata_3): "first_seen" = the reference's site numbering (IOLayersRules.h:86-91), "brick" =
        # brick-major rows over brick grids (same sites and features up to a per-sample permutation of the rows)
        self.site_order = "first_seen"

    def to(self, device):
        self.device = device
        return self

    def prepare(self, coords, device=None, stream=None):
        """Optional extension (not in the reference): build the hash grid / site numbering of a
        coordinate list AHEAD of the forward call, e.g. for the next scene on a side stream while
        the current scene trains.  The geometry depends on the coordinates only, so this is the
        device-side analogue of a data-loader prefetch; `forward` picks the prepared Metadata up
        when it is called with the same coordinate tensor."""
        if device is None:
            device = self.device if self.device is not None else coords.device
        md = Metadata(self.dimension, self.site_order)
        side = stream if stream is not None else torch.cuda.current_stream()
        c64 = coords if coords.dtype == torch.int64 else coords.long()   # converted ONCE; forward reuses c64
        with torch.cuda.stream(side):
            # kernels + an asynchronous read-back of the site count; nothing blocks here
            self._enqueue(md, c64, device)
            md.prepared_on = side
        if not hasattr(self, "_prepared"):
            self._prepared = []
        # matched by identity + version of the caller's tensor (held here, so its address cannot be recycled)
        self._prepared.append((coords, coords._version, c64, md))

    def _take_prepared(self, coords):
        """(Metadata, int64 coordinates) of a `prepare(coords)` made for exactly this tensor in this state, handed over
        to the current stream -- or a fresh Metadata and None"""
        prepared = getattr(self, "_prepared", None)
        md, c64 = None, None
        if prepared:
            for i, (src, ver, conv, m) in enumerate(prepared):
                if src is coords and ver == coords._version:
                    md, c64 = m, conv
                    del prepared[i]
                    break
        if md is not None:
            cur = torch.cuda.current_stream()
            if md.prepared_on != cur:
                cur.wait_stream(md.prepared_on)  # tensors were produced on the side stream
                md.hand_over(cur)                # ... and their memory stays theirs until `cur` is done with it
            SCN._reap_handed_over()
        return (md if md is not None else Metadata(self.dimension, self.site_order)), c64


class InputLayer(_InputLayerBase):
    def _enqueue(self, md, c64, device):
        md.inputLayerEnqueue(self.spatial_size, c64, self.mode if self.mode else 3, device)

    def forward(self, input):
        md, c64 = self._take_prepared(input[0])
        output = SparseConvNetTensor(metadata=md, spatial_size=self.spatial_size)
        output.features = InputLayerFunction.apply(
            self.dimension, output.metadata, self.spatial_size, c64 if c64 is not None else input[0].long(),
            input[1].to(self.device) if self.device else input[1], 0 if len(input) == 2 else input[2],
            self.mode)
        return output


class OutputLayer(Module):
    """Used with an InputLayer for 'autoencoder' style networks: SparseConvNetTensor -> float tensor [N, planes],
    N defined by the InputLayer (reference: ioLayers.py:66-87)."""

    def __init__(self, dimension):
        Module.__init__(self)
        self.dimension = dimension

    def forward(self, input):
        return OutputLayerFunction.apply(self.dimension, input.metadata, input.features)


class BLInputLayer(_InputLayerBase):
    """Takes a tuple (coords, features) (reference: ioLayers.py:92-136):
    * coords: integer tensor [batch_size, length, 3]; a row whose x is negative is 'empty' (the reference's test is
      `p[0] >= 0`; -1 in all three is the usual marker).  Device-resident coordinates are read where they lie, host
      coordinates are uploaded once (the reference forces `.cpu()`); nothing is flattened or compacted.
    * features: float32 [batch_size, length, n_feature_planes]

    mode == 0 assumes every row present and unique (checked here: anything else raises)
    mode == 1 use the last item at each spatial location
    mode == 2 keep the first item at each spatial location (the reference fills this mode's rule book for mode 1 only,
              IOLayersRules.h:225-237, so its own mode 2 reads an empty book; the documented meaning is built here)
    mode == 3 sum, mode == 4 average feature vectors sharing one location

    Sites are numbered sample by sample, first-seen inside a sample; the tensor has exactly batch_size samples.
    `site_order` and `prepare` as for InputLayer."""

    def _enqueue(self, md, c64, device):
        if int(self.mode) not in SCN.BL_KERNEL_MODE:
            raise ValueError("BLInputLayer mode must be 0..4, got %r" % (self.mode,))
        md.inputLayerEnqueue(self.spatial_size, c64, SCN.BL_KERNEL_MODE[int(self.mode)], device, bl=True)

    def forward(self, input):
        coords, features = input[0], input[1]
        SCN._bl_check(coords, features, self.mode)
        md, c64 = self._take_prepared(coords)
        output = SparseConvNetTensor(metadata=md, spatial_size=self.spatial_size)
        output.features = BLInputLayerFunction.apply(
            self.dimension, output.metadata, self.spatial_size, c64 if c64 is not None else coords.long(),
            features.to(self.device) if self.device else features, self.mode)
        return output


class BLOutputLayer(Module):
    """Used with a BLInputLayer for 'autoencoder' style networks: SparseConvNetTensor -> float32 [batch_size, length,
    planes], batch_size and length defined by the BLInputLayer (reference: ioLayers.py:139-160).  out[b, l] is the site
    row of every point the BL rule book lists (modes 3 / 4: every point of a site, not averaged; mode 1: a site's last
    point; mode 2: its first; mode 0: all); every other row, empty rows included, is zero."""

    def __init__(self, dimension):
        Module.__init__(self)
        self.dimension = dimension

    def forward(self, input):
        return BLOutputLayerFunction.apply(self.dimension, input.metadata, input.features)


class BLInputLayerFunction(Function):
    @staticmethod
    def forward(ctx, dimension, metadata, spatial_size, coords, input_features, mode):
        output_features = input_features.new()
        ctx.metadata_ = metadata
        ctx.dimension = dimension
        SCN.BLInputLayer_updateOutput(metadata, spatial_size, coords, input_features.contiguous(), output_features, mode)
        return output_features

    @staticmethod
    def backward(ctx, grad_output):
        grad_input = grad_output.new()
        SCN.BLInputLayer_updateGradInput(ctx.metadata_, grad_input, grad_output.contiguous())
        return None, None, None, None, grad_input, None


class BLOutputLayerFunction(Function):
    @staticmethod
    def forward(ctx, dimension, metadata, input_features):
        output_features = input_features.new()
        ctx.metadata_ = metadata
        ctx.dimension = dimension
        SCN.BLOutputLayer_updateOutput(metadata, input_features.contiguous(), output_features)
        return output_features

    @staticmethod
    def backward(ctx, grad_output):
        grad_input = grad_output.new()
        SCN.BLOutputLayer_updateGradInput(ctx.metadata_, grad_input, grad_output.contiguous())
        return None, None, grad_input


class OutputLayerFunction(Function):
    @staticmethod
    def forward(ctx, dimension, metadata, input_features):
        output_features = input_features.new()
        ctx.metadata_ = metadata
        ctx.dimension = dimension
        SCN.OutputLayer_updateOutput(metadata, input_features.contiguous(), output_features)
        return output_features

    @staticmethod
    def backward(ctx, grad_output):
        grad_input = grad_output.new()
        SCN.OutputLayer_updateGradInput(ctx.metadata_, grad_input, grad_output.contiguous())
        return None, None, grad_input


class InputLayerFunction(Function):
    @staticmethod
    def forward(ctx, dimension, metadata, spatial_size, coords, input_features, batch_size, mode):
        output_features = input_features.new()
        ctx.dimension = dimension
        ctx.metadata_ = metadata
        SCN.InputLayer_updateOutput(metadata, spatial_size, coords, input_features.contiguous(), output_features,
                                    batch_size, mode)
        return output_features

    @staticmethod
    def backward(ctx, grad_output):
        grad_input = grad_output.new()
        SCN.InputLayer_updateGradInput(ctx.metadata_, grad_input, grad_output.contiguous())
        return None, None, None, None, grad_input, None, None
