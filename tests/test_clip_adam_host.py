"""optim.ClipAdam / ClipAdamW, the part that needs no GPU: constructor checks, defaults and param_group keys (torch's),
scale_loss, the trainers' choice of optimiser on the CPU, and the two entry points in include/tdx.h and the ctypes table."""

import ctypes as C
import re
import sys
from pathlib import Path

import pytest
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
sys.path.insert(0, str(HERE))


def _p():
    return [torch.nn.Parameter(torch.zeros(3))]


def test_constructor_checks():
    from turbdiff_amd.optim import ClipAdam, ClipAdamW

    for cls in (ClipAdam, ClipAdamW):
        with pytest.raises(ValueError, match="amsgrad"):
            cls(_p(), amsgrad=True)
        with pytest.raises(ValueError, match="maximize"):
            cls(_p(), maximize=True)
        with pytest.raises(ValueError, match="weight_decay"):
            cls(_p(), weight_decay=-1e-3)
        with pytest.raises(ValueError, match="power of two"):
            cls(_p(), loss_scale=1000.0)
        with pytest.raises(ValueError, match="learning rate"):
            cls(_p(), lr=-1.0)
        with pytest.raises(ValueError, match="betas"):
            cls(_p(), betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="decoupled"):
        ClipAdamW(_p(), decoupled_weight_decay=False)


def test_defaults_and_param_groups_are_torchs():
    from turbdiff_amd.optim import ClipAdam, ClipAdamW, ClipRAdam, _ClipOptimizer

    for cls, ref, wd, dec in ((ClipAdam, torch.optim.Adam, 0.0, False), (ClipAdamW, torch.optim.AdamW, 1e-2, True)):
        opt, tor = cls(_p()), ref(_p())
        assert isinstance(opt, torch.optim.Optimizer) and isinstance(opt, _ClipOptimizer)
        group = opt.param_groups[0]
        assert set(group) == {"params", "lr", "betas", "eps", "weight_decay", "decoupled_weight_decay"}
        assert set(group) <= set(tor.param_groups[0])
        for k in ("lr", "betas", "eps", "weight_decay", "decoupled_weight_decay"):
            assert group[k] == tor.param_groups[0][k] == opt.defaults[k], k
        assert (group["weight_decay"], group["decoupled_weight_decay"]) == (wd, dec)
        assert opt.max_norm is None and opt.loss_scale is None and opt.write_clipped_grads is False
    assert issubclass(ClipAdamW, ClipAdam) and issubclass(ClipRAdam, _ClipOptimizer)
    assert ClipAdam(_p(), weight_decay=0.1, decoupled_weight_decay=True).param_groups[0]["decoupled_weight_decay"] is True
    # ClipRAdam keeps its layout
    assert set(ClipRAdam(_p()).param_groups[0]) == {"params", "lr", "betas", "eps", "weight_decay"}


def test_scale_loss():
    from turbdiff_amd.optim import ClipAdam, ClipAdamW

    for cls in (ClipAdam, ClipAdamW):
        assert cls(_p(), loss_scale=2.0**10).scale_loss(torch.tensor(1.5)).item() == 1536.0
        assert cls(_p()).scale_loss(torch.tensor(1.5)).item() == 1.5


def test_cpu_trainers_return_the_stock_classes():
    from test_dilresnet_host import _task
    from turbdiff_amd.training import DiffusionTrainer

    cfg = {**DiffusionTrainer.SHIPPED_CONFIG, "dim": 8, "timesteps": 10}
    for name, cls in (("adam", torch.optim.Adam), ("adamw", torch.optim.AdamW), ("radam", torch.optim.RAdam)):
        task = DiffusionTrainer(**{**cfg, "optimizer": name}, u_net_levels=2)
        assert task.fused_optimizer is True
        opt, sched = task.configure_optimizers()
        assert type(opt) is cls and sched is not None
        half = DiffusionTrainer(**{**cfg, "optimizer": name}, u_net_levels=2, compute_mode="fp16")
        with pytest.raises(RuntimeError, match="fp16 training needs the loss-scaling optimiser"):
            half.configure_optimizers()
    t = _task()
    assert isinstance(t.fused_optimizer, bool)
    for fused in (True, False):
        t.fused_optimizer = fused
        opt, sched = t.configure_optimizers()
        assert type(opt) is torch.optim.Adam and isinstance(sched, torch.optim.lr_scheduler.LambdaLR)


def test_adam_entry_points_are_declared_and_bound():
    from turbdiff_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tdx.h").read_text(), flags=re.S)
    tail = [C.c_int64] + [C.c_double] * 5 + [C.c_int, C.c_int, C.c_void_p]
    for name in ("tdx_adam_step", "tdx_adam_step_scaled"):
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/tdx.h"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == 14 and [a.split()[-1] for a in args[5:]] == [
            "step", "lr", "beta1", "beta2", "eps", "weight_decay", "decoupled", "write_grad", "stream"]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is C.c_int and argtypes[:5] == [C.c_void_p] * 3 + [C.c_int, C.c_void_p] and argtypes[5:] == tail
        assert hasattr(_lib.load(), name), f"{name} not exported by libtdx_hip.so"
