"""Loss identifiers (mirrors pldepth/losses/losses_meta.py:1-5). ``RANKING`` names the pairwise
ranking loss (losses/ranking_loss.py), which the reference's enum has no member for."""
from ..models.models_meta import StringEnum


class DepthLossType(StringEnum):
    NLL = "NLL"
    RANKING = "RANKING"
