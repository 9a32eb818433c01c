"""RobotNetVote (model/robotnet_vote.py:36-71 in the reference): same head as RobotNetSegmentation, 2 or 4 classes."""
import torch

from ..utils import config
from .robotnet_segmentation import make_robotnet_vote

RobotNetVote = make_robotnet_vote()


def get_criterion(fused=False):
    """robotnet_vote.py:74-79.  fused=True: the same configuration as utils.loss.SegmentationCriterion (one HIP pass for
    loss, gradient and the step's confusion counts); the default stays torch's module."""
    cfg = config.Config()
    if fused:
        from ..utils.loss import SegmentationCriterion

        return SegmentationCriterion(ignore_index=cfg.DATA.ignore_label,
                                     reduction=cfg().get("TRAIN", {}).get("loss_reduction", "mean"))
    return torch.nn.CrossEntropyLoss(reduction=cfg().get("TRAIN", {}).get("loss_reduction", "mean"),
                                     ignore_index=cfg.DATA.ignore_label)
