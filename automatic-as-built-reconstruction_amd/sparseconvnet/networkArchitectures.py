"""Network builders: SparseVggNet, SparseResNet, UNet, FullyConvolutionalNet (reference:
SparseConvNet/sparseconvnet/networkArchitectures.py:9-312).  Each returns a composition of this package's modules in the
reference's layer order, so the `state_dict` keys of a checkpoint trained with the reference load.  The reference's
FullConvolutionalNetIntegratedLinear refers to undefined names and is left out."""
import sparseconvnet as scn


def _seq(*layers):
    m = scn.Sequential()
    for layer in layers:
        m.add(layer)
    return m


def _conv_bn(dimension, a, b):
    return [scn.Convolution(dimension, a, b, 3, 2, False), scn.BatchNormReLU(b)]


def _subm_bn(dimension, a, b):
    return [scn.SubmanifoldConvolution(dimension, a, b, 3, False), scn.BatchNormReLU(b)]


def _plus_branch(dimension, nIn, n, depth):
    """the 'Plus' branch that goes `depth` levels down and comes back up: (Convolution 3/2, BNReLU, SubmConv, BNReLU) per
    level down, then (Deconvolution 3/2, BNReLU, SubmConv, BNReLU) per level up, without the last three"""
    layers = []
    for d in range(depth):
        layers += _conv_bn(dimension, nIn if d == 0 else n, n) + _subm_bn(dimension, n, n)
    for d in range(depth):
        layers.append(scn.Deconvolution(dimension, n, n, 3, 2, False))
        if d < depth - 1:
            layers += [scn.BatchNormReLU(n)] + _subm_bn(dimension, n, n)
    return _seq(*layers)


def SparseVggNet(dimension, nInputPlanes, layers):
    """VGG-style nets of submanifold convolutions.  `layers` entries: 'MP' (MaxPooling 3/2), ['MP', size, stride], 'C3/2' and
    ['C3/2', n] (strided Convolution + BNReLU), ['C', n] (SubmConv + BNReLU) and the 'Plus' forms ['C', n, n2[, n3[, n4]]]: a
    ConcatTable of the SubmConv and one branch per extra count that goes 1, 2, 3 levels down and back, joined + BNReLU."""
    nPlanes = nInputPlanes
    m = scn.Sequential()
    for x in layers:
        if x == 'MP':
            m.add(scn.MaxPooling(dimension, 3, 2))
        elif x[0] == 'MP':
            m.add(scn.MaxPooling(dimension, x[1], x[2]))
        elif x == 'C3/2':
            for layer in _conv_bn(dimension, nPlanes, nPlanes):
                m.add(layer)
        elif x[0] == 'C3/2':
            for layer in _conv_bn(dimension, nPlanes, x[1]):
                m.add(layer)
            nPlanes = x[1]
        elif x[0] == 'C' and len(x) == 2:
            for layer in _subm_bn(dimension, nPlanes, x[1]):
                m.add(layer)
            nPlanes = x[1]
        elif x[0] == 'C' and 3 <= len(x) <= 5:
            table = scn.ConcatTable().add(scn.SubmanifoldConvolution(dimension, nPlanes, x[1], 3, False))
            for depth, n in enumerate(x[2:], 1):
                table.add(_plus_branch(dimension, nPlanes, n, depth))
            m.add(table).add(scn.JoinTable())
            nPlanes = sum(x[1:])
            m.add(scn.BatchNormReLU(nPlanes))
    return m


def SparseResNet(dimension, nInputPlanes, layers):
    """pre-activated ResNet; `layers` = [(blockType, n, reps, stride)], blockType 'basic'"""
    nPlanes = nInputPlanes
    m = scn.Sequential()

    def shortcut(nIn, nOut, stride):
        if stride > 1:
            return scn.Convolution(dimension, nIn, nOut, 3, stride, False)
        if nIn != nOut:
            return scn.NetworkInNetwork(nIn, nOut, False)
        return scn.Identity()

    for blockType, n, reps, stride in layers:
        for rep in range(reps):
            if blockType[0] == 'b':
                if rep == 0:     # the block's first unit changes planes / level; its BNReLU feeds both branches
                    m.add(scn.BatchNormReLU(nPlanes))
                    first = scn.SubmanifoldConvolution(dimension, nPlanes, n, 3, False) if stride == 1 else \
                        scn.Convolution(dimension, nPlanes, n, 3, stride, False)
                    m.add(scn.ConcatTable()
                          .add(_seq(first, *([scn.BatchNormReLU(n), scn.SubmanifoldConvolution(dimension, n, n, 3, False)])))
                          .add(shortcut(nPlanes, n, stride)))
                else:
                    m.add(scn.ConcatTable()
                          .add(_seq(scn.BatchNormReLU(nPlanes), scn.SubmanifoldConvolution(dimension, nPlanes, n, 3, False),
                                    scn.BatchNormReLU(n), scn.SubmanifoldConvolution(dimension, n, n, 3, False)))
                          .add(scn.Identity()))
            nPlanes = n
            m.add(scn.AddTable())
    m.add(scn.BatchNormReLU(nPlanes))
    return m


def _block(m, dimension, a, b, residual_blocks, bn):
    """one VGG- or ResNet-style unit a -> b planes appended to `m`; `bn(planes)` makes the normalisation"""
    if residual_blocks:
        m.add(scn.ConcatTable()
              .add(scn.Identity() if a == b else scn.NetworkInNetwork(a, b, False))
              .add(_seq(bn(a), scn.SubmanifoldConvolution(dimension, a, b, 3, False),
                        bn(b), scn.SubmanifoldConvolution(dimension, b, b, 3, False)))
              ).add(scn.AddTable())
    else:
        m.add(_seq(bn(a), scn.SubmanifoldConvolution(dimension, a, b, 3, False)))


def UNet(dimension, reps, nPlanes, residual_blocks=False, downsample=[2, 2], leakiness=0, n_input_planes=-1):
    """U-Net with VGG- or ResNet-style blocks: per level `reps` blocks, then [identity | BN, Convolution down, the deeper
    U, BN, Deconvolution up] joined, then `reps` blocks back to nPlanes[level] planes"""
    def bn(planes):
        return scn.BatchNormLeakyReLU(planes, leakiness=leakiness)

    def U(nPlanes, n_input_planes=-1):
        m = scn.Sequential()
        for _ in range(reps):
            _block(m, dimension, n_input_planes if n_input_planes != -1 else nPlanes[0], nPlanes[0], residual_blocks, bn)
            n_input_planes = -1
        if len(nPlanes) > 1:
            m.add(scn.ConcatTable()
                  .add(scn.Identity())
                  .add(_seq(bn(nPlanes[0]),
                            scn.Convolution(dimension, nPlanes[0], nPlanes[1], downsample[0], downsample[1], False),
                            U(nPlanes[1:]),
                            bn(nPlanes[1]),
                            scn.Deconvolution(dimension, nPlanes[1], nPlanes[0], downsample[0], downsample[1], False))))
            m.add(scn.JoinTable())
            for i in range(reps):
                _block(m, dimension, nPlanes[0] * (2 if i == 0 else 1), nPlanes[0], residual_blocks, bn)
        return m
    return U(nPlanes, n_input_planes)


def FullyConvolutionalNet(dimension, reps, nPlanes, residual_blocks=False, downsample=[2, 2]):
    """fully-convolutional net: per level `reps` blocks, then [identity | BNReLU, Convolution down, the deeper net, UnPooling
    up] joined -- the output carries sum(nPlanes) planes"""
    def U(nPlanes):
        m = scn.Sequential()
        for _ in range(reps):
            _block(m, dimension, nPlanes[0], nPlanes[0], residual_blocks, scn.BatchNormReLU)
        if len(nPlanes) > 1:
            m.add(scn.ConcatTable()
                  .add(scn.Identity())
                  .add(_seq(scn.BatchNormReLU(nPlanes[0]),
                            scn.Convolution(dimension, nPlanes[0], nPlanes[1], downsample[0], downsample[1], False),
                            U(nPlanes[1:]),
                            scn.UnPooling(dimension, downsample[0], downsample[1]))))
            m.add(scn.JoinTable())
        return m
    return U(nPlanes)
