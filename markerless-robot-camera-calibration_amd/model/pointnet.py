"""PointNet (model/pointnet.py:8-36 in the reference): the key-points-to-pose regressor of train_kp_to_pose.py:286-291.

Input [B, in_channel, K] with K = 6 key points per sample: five shared 1x1 convolutions with BatchNorm and ReLU, a max over
the points, two linear layers -> [B, out_channel].  A few thousand multiply-adds per sample: plain torch modules, no HIP
path.  Module names and so the state_dict keys (conv1..5, bn1..6, linear1, linear2) are the reference's.
"""
import torch.nn as nn
import torch.nn.functional as F

WIDTHS = (64, 64, 64, 128)  # conv1 .. conv4; conv5 widens to embedding_channel


class PointNet(nn.Module):
    def __init__(self, in_channel, out_channel, embedding_channel=1024):
        super().__init__()
        widths = (in_channel,) + WIDTHS + (embedding_channel,)
        for k in range(1, 6):
            setattr(self, f"conv{k}", nn.Conv1d(widths[k - 1], widths[k], kernel_size=1, bias=False))
        for k in range(1, 6):
            setattr(self, f"bn{k}", nn.BatchNorm1d(widths[k]))
        self.linear1 = nn.Linear(embedding_channel, 512, bias=False)
        self.bn6 = nn.BatchNorm1d(512)
        self.dp1 = nn.Dropout()
        self.linear2 = nn.Linear(512, out_channel, bias=True)

    def forward(self, x):
        for k in range(1, 6):
            x = F.relu(getattr(self, f"bn{k}")(getattr(self, f"conv{k}")(x)))
        # the reference's squeeze() takes every unit dimension: a batch of one arrives at bn6 as [embedding_channel], which
        # BatchNorm1d refuses - the reference's behaviour at B = 1, kept
        x = F.adaptive_max_pool1d(x, 1).squeeze()
        x = self.dp1(F.relu(self.bn6(self.linear1(x))))
        return self.linear2(x)
