"""Lightning-free Stage1 / Stage2 / Stage3 / ExpFCN trainers over the HIP modules (reference
trainers/ and scripts/train_fcn.py)."""
from .fcn import ExpFCN
from .stage1 import Stage1
from .stage2 import Stage2
from .stage3 import Stage3

__all__ = ["ExpFCN", "Stage1", "Stage2", "Stage3"]
