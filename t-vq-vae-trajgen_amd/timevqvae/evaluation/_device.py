"""Which device an evaluation function runs on."""
import torch


def resolve_device(device, tensors=()):
    """The explicit `device` if one is given, otherwise the device of the first CUDA tensor
    among `tensors`, otherwise the current CUDA device."""
    if device is not None:
        return torch.device(device)
    for t in tensors:
        if t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device())
