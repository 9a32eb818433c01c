"""ResNetBase and the classification networks ResNet14 / 18 / 34 / 50 / 101; the U-Nets inherit `_make_layer` and
`weight_initialization`.

Mirror of the reference's model/backbone/resnet.py:34-162.  Same attribute names -> same state_dict keys.  The ResFieldNet
classes there (:165-218) need MinkowskiSinusoidal, MinkowskiToSparseTensor and TensorField.cat_slice and are not rebuilt
(DESIGN.md §9).
"""
import torch.nn as nn

from ... import MinkowskiEngine as ME
from ..._lib import SV_ACT_GELU, SV_ACT_RELU


class ResNetBase(nn.Module):
    BLOCK = None
    LAYERS = ()
    INIT_DIM = 64
    PLANES = (64, 128, 256, 512)

    def __init__(self, in_channels, out_channels, D=3):
        nn.Module.__init__(self)
        self.D = D
        assert self.BLOCK is not None
        self.network_initialization(in_channels, out_channels, D)
        self.weight_initialization()

    def network_initialization(self, in_channels, out_channels, D):
        # resnet.py:48-84: k3 s2 stem + InstanceNorm + ReLU + max pooling, four stride-2 stages, k3 s3 conv5 + InstanceNorm
        # + GELU, global max pooling, linear classifier (tensor strides 2, 4, 8, 16, 32, 64, 192)
        self.inplanes = self.INIT_DIM
        self.conv1 = nn.Sequential(
            ME.MinkowskiConvolution(in_channels, self.inplanes, kernel_size=3, stride=2, dimension=D),
            ME.MinkowskiInstanceNorm(self.inplanes),
            ME.MinkowskiReLU(inplace=True),
            ME.MinkowskiMaxPooling(kernel_size=2, stride=2, dimension=D),
        )
        self.layer1 = self._make_layer(self.BLOCK, self.PLANES[0], self.LAYERS[0], stride=2)
        self.layer2 = self._make_layer(self.BLOCK, self.PLANES[1], self.LAYERS[1], stride=2)
        self.layer3 = self._make_layer(self.BLOCK, self.PLANES[2], self.LAYERS[2], stride=2)
        self.layer4 = self._make_layer(self.BLOCK, self.PLANES[3], self.LAYERS[3], stride=2)
        self.conv5 = nn.Sequential(
            ME.MinkowskiDropout(),
            ME.MinkowskiConvolution(self.inplanes, self.inplanes, kernel_size=3, stride=3, dimension=D),
            ME.MinkowskiInstanceNorm(self.inplanes),
            ME.MinkowskiGELU(),
        )
        self.glob_pool = ME.MinkowskiGlobalMaxPooling()
        self.final = ME.MinkowskiLinear(self.inplanes, out_channels, bias=True)

    @staticmethod
    def _run(seq, x):
        """nn.Sequential.forward with InstanceNorm -> ReLU / GELU as ONE call in eval() (sv_instance_norm's fused
        activation); in train() every module runs on its own, as differentiable ops"""
        mods = list(seq)
        i = 0
        while i < len(mods):
            m = mods[i]
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            if isinstance(m, ME.MinkowskiInstanceNorm) and not m.training and isinstance(nxt, (ME.MinkowskiReLU, ME.MinkowskiGELU)):
                x = m.forward_fused(x, act=SV_ACT_RELU if isinstance(nxt, ME.MinkowskiReLU) else SV_ACT_GELU)
                i += 2
            else:
                x = m(x)
                i += 1
        return x

    def forward(self, x):
        # resnet.py:129-137; the result is the [B, out_channels] logits (global pooling gives one row per frame)
        x = self._run(self.conv1, x)
        x = self.layer1(x)
        x = self.layer2(x)
        x = self.layer3(x)
        x = self.layer4(x)
        x = self._run(self.conv5, x)
        x = self.glob_pool(x)
        return self.final(x.F)

    def weight_initialization(self):
        # resnet.py:86-93: kaiming-normal(fan_out, relu) conv kernels, BN gamma = 1, beta = 0
        for m in self.modules():
            if isinstance(m, ME.MinkowskiConvolution):
                ME.utils.kaiming_normal_(m.kernel, mode="fan_out", nonlinearity="relu")
            if isinstance(m, ME.MinkowskiBatchNorm):
                nn.init.constant_(m.bn.weight, 1)
                nn.init.constant_(m.bn.bias, 0)

    def _make_layer(self, block, planes, blocks, stride=1, dilation=1, bn_momentum=0.1):
        # resnet.py:95-127: first block may change width (1x1 conv + BN on the residual path), the rest keep it
        out_planes = planes * block.expansion
        downsample = None
        if stride != 1 or self.inplanes != out_planes:
            downsample = nn.Sequential(
                ME.MinkowskiConvolution(self.inplanes, out_planes, kernel_size=1, stride=stride, dimension=self.D),
                ME.MinkowskiBatchNorm(out_planes),
            )
        layers = [block(self.inplanes, planes, stride=stride, dilation=dilation, downsample=downsample,
                        dimension=self.D)]
        self.inplanes = out_planes
        layers += [block(self.inplanes, planes, stride=1, dilation=dilation, dimension=self.D)
                   for _ in range(1, blocks)]
        return nn.Sequential(*layers)


class ResNet14(ResNetBase):
    BLOCK = ME.BasicBlock
    LAYERS = (1, 1, 1, 1)


class ResNet18(ResNetBase):
    BLOCK = ME.BasicBlock
    LAYERS = (2, 2, 2, 2)


class ResNet34(ResNetBase):
    BLOCK = ME.BasicBlock
    LAYERS = (3, 4, 6, 3)


class ResNet50(ResNetBase):
    BLOCK = ME.Bottleneck
    LAYERS = (3, 4, 6, 3)


class ResNet101(ResNetBase):
    BLOCK = ME.Bottleneck
    LAYERS = (3, 4, 23, 3)
