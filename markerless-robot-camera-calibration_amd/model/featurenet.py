"""FeatureNet (model/featurenet.py:14-34 in the reference): one embedding per frame for metric learning.

MinkUNet34A(out_channels) -> BatchNorm -> LeakyReLU -> global average pooling: a [B, out_channels] PooledTensor whose
`.features` the feature-extractor trainers hand to their criterion.  Attribute names (`global_pool`, `leaky_relu`,
`final_bn`) and so the state_dict keys (MinkUNet34A's plus `final_bn.bn.*`) are the reference's.  The criterion is
utils/metric_learning.py: the two pytorch_metric_learning classes the reference builds here, on the N10 HIP entries.
"""
from .. import MinkowskiEngine as ME
from .backbone.minkunet import MinkUNet34A as UNet


class FeatureNet(UNet):
    name = "featurenet"

    def __init__(self, in_channels, out_channels, D=3):
        UNet.__init__(self, in_channels, out_channels, D)
        self.global_pool = ME.MinkowskiGlobalAvgPooling()
        self.leaky_relu = ME.MinkowskiLeakyReLU(inplace=True)
        self.final_bn = ME.MinkowskiBatchNorm(out_channels)

    def forward(self, x):
        out = UNet.forward(self, x)
        return self.global_pool(self.leaky_relu(self.final_bn(out)))


def get_criterion(device="cuda"):
    """featurenet.py:30-34: (loss_func, miner) with the library's defaults.  The trainer's whole step - mine, truncate,
    loss - is utils.metric_learning.mined_triplet_loss, which waits for nothing."""
    from ..utils.metric_learning import MultiSimilarityMiner, TripletMarginLoss

    return TripletMarginLoss(), MultiSimilarityMiner()
