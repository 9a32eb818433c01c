"""ResNetBase and the classification networks ResNet14 / 18 / 34 / 50 / 101; the U-Nets inherit `_make_layer` and
`weight_initialization`.  ResFieldNetBase and ResFieldNet14 / 18 / 34 / 50 / 101: the same trunk behind two small networks
that run on the POINTS of a TensorField (sinusoidal layer, linear layer, per-voxel mean) before voxelisation.

Mirror of the reference's model/backbone/resnet.py:34-218.  Same attribute names -> same state_dict keys.  In eval() each
field network is one sv_field_stage call.
"""
import torch
import torch.nn as nn

from ... import MinkowskiEngine as ME
from ... import nn as svnn
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


class ResFieldNetBase(ResNetBase):
    FUSE_FIELD = True  # eval(): each field network as ONE sv_field_stage call; False: module by module

    def network_initialization(self, in_channels, out_channels, D):
        # resnet.py:166-188: 3 -> 32 on the points, voxel mean; [32 voxel, 3 point] -> 64 on the points, voxel mean; the trunk
        field_ch = 32
        field_ch2 = 64
        self.field_network = nn.Sequential(
            ME.MinkowskiSinusoidal(in_channels, field_ch),
            ME.MinkowskiBatchNorm(field_ch),
            ME.MinkowskiReLU(inplace=True),
            ME.MinkowskiLinear(field_ch, field_ch),
            ME.MinkowskiBatchNorm(field_ch),
            ME.MinkowskiReLU(inplace=True),
            ME.MinkowskiToSparseTensor(),
        )
        self.field_network2 = nn.Sequential(
            ME.MinkowskiSinusoidal(field_ch + in_channels, field_ch2),
            ME.MinkowskiBatchNorm(field_ch2),
            ME.MinkowskiReLU(inplace=True),
            ME.MinkowskiLinear(field_ch2, field_ch2),
            ME.MinkowskiBatchNorm(field_ch2),
            ME.MinkowskiReLU(inplace=True),
            ME.MinkowskiToSparseTensor(),
        )
        ResNetBase.network_initialization(self, field_ch2, out_channels, D)

    def _run_field(self, seq, field, voxel=None):
        """seq(field), or seq(voxel.cat_slice(field)): fused where seq is exactly the seven-module field network in eval(),
        nothing carries a graph, the field averages and the kernel covers the widths; else module by module"""
        fused = (self.FUSE_FIELD and svnn.is_field_stage(seq)
                 and field.quantization_mode == ME.SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE
                 and not (torch.is_grad_enabled() and (field.F.requires_grad or (voxel is not None and voxel.F.requires_grad))))
        if fused:
            out = svnn.field_stage(seq, field, voxel)
            if out is not None:
                return out
        return seq(field if voxel is None else voxel.cat_slice(field))

    def forward(self, x):
        # resnet.py:190-193
        otensor = self._run_field(self.field_network, x)
        otensor2 = self._run_field(self.field_network2, x, otensor)
        return ResNetBase.forward(self, otensor2)


class ResFieldNet14(ResFieldNetBase):
    BLOCK = ME.BasicBlock
    LAYERS = (1, 1, 1, 1)


class ResFieldNet18(ResFieldNetBase):
    BLOCK = ME.BasicBlock
    LAYERS = (2, 2, 2, 2)


class ResFieldNet34(ResFieldNetBase):
    BLOCK = ME.BasicBlock
    LAYERS = (3, 4, 6, 3)


class ResFieldNet50(ResFieldNetBase):
    BLOCK = ME.Bottleneck
    LAYERS = (3, 4, 6, 3)


class ResFieldNet101(ResFieldNetBase):
    BLOCK = ME.Bottleneck
    LAYERS = (3, 4, 23, 3)
