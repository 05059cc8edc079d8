"""Sampling from trained models (reference generation/): TrainedModelSampler, its sampling
half and its ROCKET evaluation half."""
from .sampler import TrainedModelSampler

__all__ = ["TrainedModelSampler"]
