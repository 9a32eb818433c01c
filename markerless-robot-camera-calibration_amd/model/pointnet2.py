"""PointNet2SSG: the key-point network the reference configures for inference (model/pointnet2.py:9-43,
config/override_inference_test.yaml:97).  SA 1024/256/64/16 centroids (radii .1/.2/.4/.8, 32 neighbours), four feature
propagation stages, 1x1 conv head.
PointNet2MSGEncoder: the pose regressor of STRUCTURE.backbone = pointnet2 with encode_only (model/pointnet2.py:46-77,
train.py:259-263): two multi-scale set abstractions (512 / 128 centroids, three radii each), a group-all one, three
fully connected layers.  Same attribute names as the reference -> same state_dict keys.
set_training_path(model, "hip") (re-exported from pointnet2_utils): train() on the HIP kernels."""
import torch.nn as nn
import torch.nn.functional as F

from .. import nn as svnn
from .._lib import SV_ACT_NONE, SV_ACT_RELU
from .pointnet2_utils import (FoldCache, PointNetFeaturePropagation, PointNetSetAbstraction,  # noqa: F401
                              PointNetSetAbstractionMsg, _fold_conv_bn, _hip_train, bn_rows_train, conv_rows_train,
                              set_training_path)


class PointNet2SSG(FoldCache):
    _hip_trainable = True  # set_training_path: the conv1 / bn1 / conv2 head

    def __init__(self, num_classes=10, in_channels=3):
        super().__init__()
        self.sa1 = PointNetSetAbstraction(1024, 0.1, 32, in_channels + 3, [32, 32, 64], False)
        self.sa2 = PointNetSetAbstraction(256, 0.2, 32, 64 + 3, [64, 64, 128], False)
        self.sa3 = PointNetSetAbstraction(64, 0.4, 32, 128 + 3, [128, 128, 256], False)
        self.sa4 = PointNetSetAbstraction(16, 0.8, 32, 256 + 3, [256, 256, 512], False)
        self.fp4 = PointNetFeaturePropagation(768, [256, 256])
        self.fp3 = PointNetFeaturePropagation(384, [256, 256])
        self.fp2 = PointNetFeaturePropagation(320, [256, 128])
        self.fp1 = PointNetFeaturePropagation(128, [128, 128, 128])
        self.conv1 = nn.Conv1d(128, 128, 1)
        self.bn1 = nn.BatchNorm1d(128)
        self.drop1 = nn.Dropout(0.5)
        self.conv2 = nn.Conv1d(128, num_classes, 1)

    def _head(self, l0_points):
        """eval head on libsvhip: conv1 + bn1 + relu as one folded layer, conv2 with its bias as the shift (Dropout is the
        identity in eval) -> [B, N, classes]"""
        def build():
            w1, s1, h1 = _fold_conv_bn(self.conv1, self.bn1)
            w2 = self.conv2.weight.detach().reshape(self.conv2.out_channels, -1).t().contiguous().unsqueeze(0)
            b2 = self.conv2.bias.detach().float().contiguous() if self.conv2.bias is not None else None
            return w1, s1, h1, w2, b2

        w1, s1, h1, w2, b2 = self._fold_get(build, (self.conv1, self.bn1, self.conv2))  # keyed on the head alone
        B, C, N = l0_points.shape
        rows = l0_points.permute(0, 2, 1).reshape(B * N, C)
        x = svnn.conv_forward(rows, w1, None, B * N, s1, h1, None, SV_ACT_RELU)
        x = svnn.conv_forward(x, w2, None, B * N, None, b2, None, SV_ACT_NONE)
        return x.view(B, N, -1)

    def _head_train(self, l0_points):
        """train() head on the HIP path, rows [B*N, C]: conv1 / conv2 on sv_conv_fwd, bn1 as F.batch_norm -> [B, N, classes]"""
        B, C, N = l0_points.shape
        rows = l0_points.permute(0, 2, 1).reshape(B * N, C)
        x = self.drop1(F.relu(bn_rows_train(self.bn1, conv_rows_train(rows, self.conv1))))
        return conv_rows_train(x, self.conv2).view(B, N, -1)

    def forward(self, xyz, fps_starts=None):
        """xyz [B, in_channels, N] with the coordinates in the first three channels -> ([B, N, classes], l4 features).
        fps_starts int64 [4, B]: the first farthest-point centroid of every set abstraction (None: drawn as the reference
        draws them)."""
        st = [None] * 4 if fps_starts is None else [fps_starts[i] for i in range(4)]
        l0_xyz = xyz[:, :3, :]
        l1_xyz, l1_points = self.sa1(l0_xyz, xyz, fps_start=st[0])
        l2_xyz, l2_points = self.sa2(l1_xyz, l1_points, fps_start=st[1])
        l3_xyz, l3_points = self.sa3(l2_xyz, l2_points, fps_start=st[2])
        l4_xyz, l4_points = self.sa4(l3_xyz, l3_points, fps_start=st[3])
        l3_points = self.fp4(l3_xyz, l4_xyz, l3_points, l4_points)
        l2_points = self.fp3(l2_xyz, l3_xyz, l2_points, l3_points)
        l1_points = self.fp2(l1_xyz, l2_xyz, l1_points, l2_points)
        l0_points = self.fp1(l0_xyz, l1_xyz, None, l1_points)
        if not self.training and l0_points.is_cuda:
            return self._head(l0_points), l4_points
        if _hip_train(self):
            return self._head_train(l0_points), l4_points
        x = self.drop1(F.relu(self.bn1(self.conv1(l0_points))))
        x = self.conv2(x)
        return x.permute(0, 2, 1), l4_points


class PointNet2MSGEncoder(FoldCache):
    _hip_trainable = True  # set_training_path: the fc1 / fc2 / fc3 head

    def __init__(self, num_class, normal_channel=True):
        super().__init__()
        in_channel = 3 if normal_channel else 0
        self.normal_channel = normal_channel
        self.sa1 = PointNetSetAbstractionMsg(512, [0.1, 0.2, 0.4], [16, 32, 128], in_channel,
                                             [[32, 32, 64], [64, 64, 128], [64, 96, 128]])
        self.sa2 = PointNetSetAbstractionMsg(128, [0.2, 0.4, 0.8], [32, 64, 128], 320,
                                             [[64, 64, 128], [128, 128, 256], [128, 128, 256]])
        # group-all over 128 centroids, 643 -> 256 -> 512 -> 1024: dense rows (its rows do not fit the fused kernel's LDS)
        self.sa3 = PointNetSetAbstraction(None, None, None, 640 + 3, [256, 512, 1024], True)
        self.fc1 = nn.Linear(1024, 512)
        self.bn1 = nn.BatchNorm1d(512)
        self.drop1 = nn.Dropout(0.4)
        self.fc2 = nn.Linear(512, 256)
        self.bn2 = nn.BatchNorm1d(256)
        self.drop2 = nn.Dropout(0.5)
        self.fc3 = nn.Linear(256, num_class)

    def _head(self, x):
        """eval head on libsvhip: fc1 + bn1 + relu and fc2 + bn2 + relu as folded layers, fc3 with its bias as the shift
        (Dropout is the identity in eval) -> [B, num_class]"""
        def build():
            w3 = self.fc3.weight.detach().t().contiguous().unsqueeze(0)
            b3 = self.fc3.bias.detach().float().contiguous() if self.fc3.bias is not None else None
            return _fold_conv_bn(self.fc1, self.bn1), _fold_conv_bn(self.fc2, self.bn2), (w3, b3)

        (w1, s1, h1), (w2, s2, h2), (w3, b3) = self._fold_get(build, (self.fc1, self.bn1, self.fc2, self.bn2, self.fc3))
        B = x.shape[0]
        x = svnn.conv_forward(x.contiguous(), w1, None, B, s1, h1, None, SV_ACT_RELU)
        x = svnn.conv_forward(x, w2, None, B, s2, h2, None, SV_ACT_RELU)
        return svnn.conv_forward(x, w3, None, B, None, b3, None, SV_ACT_NONE)

    def _head_train(self, x):
        """train() head on the HIP path: fc1 / fc2 / fc3 on sv_conv_fwd, bn1 / bn2 as F.batch_norm -> [B, num_class]"""
        x = self.drop1(F.relu(bn_rows_train(self.bn1, conv_rows_train(x, self.fc1))))
        x = self.drop2(F.relu(bn_rows_train(self.bn2, conv_rows_train(x, self.fc2))))
        return conv_rows_train(x, self.fc3)

    def forward(self, xyz, fps_starts=None):
        """xyz [B, 6, N] (coordinates, then normals; [B, 3, N] with normal_channel False) -> (x [B, num_class],
        l3_points [B, 1024, 1]).  fps_starts int64 [2, B]: the first farthest-point centroid of sa1 and sa2 (None: drawn
        as the reference draws them)."""
        want = 6 if self.normal_channel else 3
        if xyz.dim() != 3 or xyz.shape[1] != want:
            raise ValueError(f"PointNet2MSGEncoder(normal_channel={self.normal_channel}) expects [B, {want}, N] input, "
                             f"got {tuple(xyz.shape)}")
        B = xyz.shape[0]
        st = [None, None] if fps_starts is None else [fps_starts[0], fps_starts[1]]
        norm = xyz[:, 3:, :] if self.normal_channel else None
        xyz = xyz[:, :3, :]
        l1_xyz, l1_points = self.sa1(xyz, norm, fps_start=st[0])
        l2_xyz, l2_points = self.sa2(l1_xyz, l1_points, fps_start=st[1])
        _, l3_points = self.sa3(l2_xyz, l2_points)
        x = l3_points.reshape(B, 1024)
        if not self.training and x.is_cuda:
            return self._head(x), l3_points
        if _hip_train(self):
            return self._head_train(x), l3_points
        x = self.drop1(F.relu(self.bn1(self.fc1(x))))
        x = self.drop2(F.relu(self.bn2(self.fc2(x))))
        return self.fc3(x), l3_points
