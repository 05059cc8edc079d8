"""ExpFCN -- the reference's supervised FCN trainer (scripts/train_fcn.py:101-186) without
Lightning, mlflow or sklearn: the stage that writes the `fcn.ckpt` the FID / IS evaluation
loads (evaluation.load_pretrained_FCN).

  training_step (train_fcn.py:118-138): CrossEntropyLoss(fcn(x), y) in training mode through
    FCNBaseline.loss (one autograd Function over the HIP training kernels); the scheduler is
    stepped inside, as the reference does.  Returns {"loss": with grad_fn, "acc": 0-dim device
    tensor}: the reference computes `acc` on the host with sklearn's accuracy_score and returns
    a Python float; here it stays on the device so that the step never synchronises.
  validation_step / test_step (train_fcn.py:140-186): the same two numbers through the eval
    forward (running statistics), no gradient.
  configure_optimizers (train_fcn.py:158-168): AdamW(lr = exp_params.LR, weight_decay =
    exp_params.weight_decay) as FusedAdamW + CosineAnnealingLR(T_max).
"""
import math

import torch
import torch.nn as nn
from torch.optim.lr_scheduler import CosineAnnealingLR

from ..hip.optim import FusedAdamW
from ..models import FCNBaseline


def _accuracy(logits, y):
    return (logits.argmax(dim=-1) == y.reshape(-1)).float().mean()


class ExpFCN(nn.Module):
    def __init__(self, config: dict, n_train_samples: int, n_classes: int):
        super().__init__()
        self.config = config
        self.T_max = config["trainer_params"]["max_epochs"] * (
            math.ceil(n_train_samples / config["dataset"]["batch_size"]) + 1)
        self.fcn = FCNBaseline(config["dataset"]["in_channels"], n_classes)
        self._opt = None
        self._sched = None

    def training_step(self, batch, batch_idx=0):
        x, y = batch
        self.fcn.train()
        loss, logits = self.fcn.loss(x.float(), y)
        if self._sched is not None:
            self._sched.step()
        return {"loss": loss, "acc": _accuracy(logits, y.to(logits.device))}

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0):
        x, y = batch
        self.fcn.eval()
        logits = self.fcn(x.float())
        y = y.reshape(-1).to(device=logits.device, dtype=torch.int64)
        return {"loss": torch.nn.functional.cross_entropy(logits, y), "acc": _accuracy(logits, y)}

    test_step = validation_step

    def configure_optimizers(self):
        opt = FusedAdamW(self.fcn.parameters(), lr=self.config["exp_params"]["LR"],
                         weight_decay=self.config["exp_params"]["weight_decay"])
        sch = CosineAnnealingLR(opt, self.T_max)
        self._opt, self._sched = opt, sch
        return {"optimizer": opt, "lr_scheduler": sch}

    def fit(self, train_loader, max_steps: int, val_loader=None):
        """zero_grad / training_step / backward / step over `train_loader` (re-iterated as
        epochs) until `max_steps` optimizer steps; after each epoch one pass of validation_step
        over `val_loader` when given.  Batches are moved to the FCN's device.  Returns the list
        of per-step training losses (device tensors) and the list of per-epoch mean validation
        losses."""
        if self._opt is None:
            self.configure_optimizers()
        dev = next(self.fcn.parameters()).device
        losses, val, step = [], [], 0
        while step < max_steps:
            seen = 0
            for i, (x, y) in enumerate(train_loader):
                if step >= max_steps:
                    break
                self._opt.zero_grad()
                out = self.training_step((x.to(dev), y.to(dev)), i)
                out["loss"].backward()
                self._opt.step()
                losses.append(out["loss"].detach())
                step += 1
                seen += 1
            if seen == 0:
                raise ValueError("ExpFCN.fit: the training loader gave no batch")
            if val_loader is not None:
                v = [self.validation_step((x.to(dev), y.to(dev)), i)["loss"]
                     for i, (x, y) in enumerate(val_loader)]
                if v:
                    val.append(torch.stack(v).mean())
        return losses, val

    def save(self, path):
        """torch.save(fcn.state_dict()) on the CPU: the reference's 23 keys, loadable by
        load_pretrained_FCN (weights_only) and by the reference's FCNBaseline."""
        torch.save({k: v.detach().cpu().clone() for k, v in self.fcn.state_dict().items()}, path)
