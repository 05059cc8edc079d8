"""trainers.ExpFCN (reference scripts/train_fcn.py ExpFCN without Lightning): the schedule
constant, four optimizer steps against a float64 torch loop, the eval features after training
(the eval path's fold cache must not be stale) and the checkpoint round trip.

Bound of the multi-step losses: |d| <= 1e-4 (1 + |ref|) (tests/test_stage3.py);
`test_torch_fp32_loop_is_inside_the_bound` shows torch fp32 on the CPU inside it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.optim.lr_scheduler import CosineAnnealingLR

from fcn_train_ref import STEP_REL, close, conv_bias_keys, ref_fcn
from make_golden_fcn import fcn_input, fcn_state

CIN, CLASSES, WSEED, SHAPE, ROUNDS = 3, 3, 201, (6, 3, 40), 4
CONFIG = {"dataset": {"in_channels": CIN, "batch_size": 6},
          "exp_params": {"LR": 1e-3, "weight_decay": 1e-5},
          "trainer_params": {"max_epochs": 2}}
N_TRAIN = 12  # T_max = 2 * (ceil(12 / 6) + 1) = 6: the cosine moves visibly in four steps


def _batches():
    rng = np.random.default_rng(77)
    out = []
    for r in range(ROUNDS):
        y = rng.integers(0, CLASSES, SHAPE[0]).astype(np.int64)
        y[0], y[-1] = 0, CLASSES - 1
        out.append((torch.from_numpy(fcn_input(300 + r, SHAPE)), torch.from_numpy(y).reshape(-1, 1)))
    return out


def _torch_loop(dtype):
    """the reference's loop in plain torch on the CPU, conv biases frozen: training_step
    (loss, scheduler step), backward, AdamW step; the losses and the lr each step used"""
    m = ref_fcn(fcn_state(CIN, CLASSES, WSEED), CIN, CLASSES, dtype)
    for k, p in m.named_parameters():
        p.requires_grad_(k not in conv_bias_keys())
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad],
                            lr=CONFIG["exp_params"]["LR"], weight_decay=CONFIG["exp_params"]["weight_decay"])
    sch = CosineAnnealingLR(opt, 6)
    losses, lrs = [], []
    for x, y in _batches():
        opt.zero_grad()
        loss = F.cross_entropy(m(x.to(dtype)), y.squeeze())
        sch.step()
        loss.backward()
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        losses.append(float(loss.detach()))
    return losses, lrs


# ------------------------------------------------------------------------------------ CPU
def test_t_max_and_export():
    from timevqvae import trainers
    from timevqvae.models import FCNBaseline
    assert "ExpFCN" in trainers.__all__
    exp = trainers.ExpFCN(CONFIG, N_TRAIN, CLASSES)
    assert exp.T_max == 6
    cfg = {"dataset": {"in_channels": 4, "batch_size": 256}, "exp_params": {"LR": 1e-3, "weight_decay": 1e-5},
           "trainer_params": {"max_epochs": 1000}}
    assert trainers.ExpFCN(cfg, 1000, 7).T_max == 1000 * (4 + 1)
    assert trainers.ExpFCN(cfg, 1024, 7).T_max == 1000 * (4 + 1)
    assert trainers.ExpFCN(cfg, 1025, 7).T_max == 1000 * (5 + 1)
    assert isinstance(exp.fcn, FCNBaseline) and exp.fcn.final.out_features == CLASSES
    assert len(exp.fcn.state_dict()) == 23


def test_torch_fp32_loop_is_inside_the_bound():
    l64, lr64 = _torch_loop(torch.float64)
    l32, lr32 = _torch_loop(torch.float32)
    assert lr32 == lr64
    for a, b in zip(l32, l64):
        print(f"loss fp32 {a:.7f} fp64 {b:.7f}: {abs(a - b) / (1 + abs(b)):.2e}")
        assert abs(a - b) <= STEP_REL * (1 + abs(b))


# ------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def trained(cuda, tmp_path_factory):
    from timevqvae.trainers import ExpFCN
    exp = ExpFCN(CONFIG, N_TRAIN, CLASSES)
    exp.fcn.load_state_dict(fcn_state(CIN, CLASSES, WSEED), strict=True)
    exp.to(cuda)
    for k, p in exp.fcn.named_parameters():
        p.requires_grad_(k not in conv_bias_keys())
    opt = exp.configure_optimizers()["optimizer"]
    probe = _batches()[0][0].to(cuda)
    # fills the eval fold cache, after the optimizer has moved the parameters into its flat
    # buffer: from here on neither data_ptr nor _version of any tensor changes
    before = exp.fcn.eval()(probe, return_feature_vector=True).cpu()
    outs, lrs = [], []
    for i, (x, y) in enumerate(_batches()):
        opt.zero_grad()
        out = exp.training_step((x.to(cuda), y.to(cuda)), i)
        assert out["loss"].grad_fn is not None and out["loss"].is_cuda
        assert out["acc"].dim() == 0 and out["acc"].is_cuda
        out["loss"].backward()
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        outs.append(out)
    path = tmp_path_factory.mktemp("fcn") / "fcn.ckpt"
    exp.save(str(path))
    return {"exp": exp, "outs": outs, "lrs": lrs, "before": before, "probe": probe, "path": str(path)}


@pytest.mark.gpu
def test_four_steps_follow_the_float64_loop(trained):
    """Losses, the lr sequence and num_batches_tracked of four training_step / backward / step
    rounds.  The parameters after the steps are not compared: AdamW normalises each gradient
    by its own running magnitude, so it turns the conv-bias gradients -- pure rounding noise
    in front of a training BatchNorm, in torch as well -- into +-lr steps of random sign; the
    conv biases are frozen on both sides for that reason, and what the updated parameters
    compute is checked through the losses of the later steps and the eval features."""
    ref_losses, ref_lrs = _torch_loop(torch.float64)
    assert trained["lrs"] == ref_lrs
    for out, ref in zip(trained["outs"], ref_losses):
        got = float(out["loss"])
        print(f"loss {got:.7f} ref {ref:.7f}: {abs(got - ref) / (1 + abs(ref)):.2e}; acc {float(out['acc']):.3f}")
        assert abs(got - ref) <= STEP_REL * (1 + abs(ref))
        assert 0.0 <= float(out["acc"]) <= 1.0
    sd = trained["exp"].fcn.state_dict()
    assert all(int(sd[f"layers.{i}.layers.1.num_batches_tracked"]) == 100 + ROUNDS for i in range(3))


@pytest.mark.gpu
def test_eval_after_training_uses_the_updated_statistics(trained):
    """the eval path folds BatchNorm into a cached scale / shift keyed by data_ptr and
    _version, which neither the training kernels nor FusedAdamW.step move: a stale cache would
    give the features of the untrained network"""
    exp = trained["exp"]
    after = exp.fcn.eval()(trained["probe"], return_feature_vector=True)
    sd = {k: v.detach().cpu() for k, v in exp.fcn.state_dict().items()}
    ref = ref_fcn(sd, CIN, CLASSES).eval()
    with torch.no_grad():
        want = ref(trained["probe"].cpu().double(), return_feature_vector=True)
    close(after, want, "features after training")
    assert not torch.equal(after.cpu(), trained["before"])
    val = exp.validation_step(tuple(t.to(after.device) for t in _batches()[1]))
    assert val["loss"].dim() == 0 and 0.0 <= float(val["acc"]) <= 1.0
    exp.fcn.train()


@pytest.mark.gpu
def test_checkpoint_round_trips(trained):
    from timevqvae.evaluation import load_pretrained_FCN
    sd = trained["exp"].fcn.state_dict()
    fcn = load_pretrained_FCN(trained["path"], CIN, CLASSES)
    got = fcn.state_dict()
    assert len(got) == 23 and list(got) == list(sd)
    assert all(torch.equal(got[k], sd[k].cpu()) for k in sd)
    ref = ref_fcn(torch.load(trained["path"], weights_only=True), CIN, CLASSES)  # the reference's keys
    assert list(ref.state_dict()) == list(sd)
