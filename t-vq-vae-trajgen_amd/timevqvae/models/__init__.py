"""Model modules with the reference's names and state_dict keys, run on the HIP kernels.
FCNBaseline (the evaluation feature extractor) runs its eval forward there (tvq_fcn.hip) and
its training step through `FCNBaseline.loss` (tvq_fcn_train.hip, trainers.ExpFCN)."""
from .vq import VectorQuantize
from .vq_vae import VQVAEDecoder, VQVAEEncoder
from .bidirectional_transformer import BidirectionalTransformer
from .maskgit import MaskGIT
from .fidelity_enhancer import FidelityEnhancer, Unet1D
from .fcn import FCNBaseline

__all__ = ["VectorQuantize", "VQVAEEncoder", "VQVAEDecoder", "BidirectionalTransformer", "MaskGIT", "FidelityEnhancer", "Unet1D", "FCNBaseline"]
