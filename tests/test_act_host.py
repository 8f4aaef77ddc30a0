"""Host side of the activation codes: which modules the kernels evaluate (ops.act_code), which ResnetBlocks are fused for them,
and the FUSE_ACTFNS switch that restores the SiLU-only route.  No kernel is launched."""

import pytest
import torch
from torch import nn

SUPPORTED = [(nn.SiLU, 1), (nn.GELU, 2), (nn.ReLU, 3), (nn.Softplus, 4), (nn.Tanh, 5)]
UNSUPPORTED = [lambda: nn.GELU(approximate="tanh"), lambda: nn.Softplus(beta=2), nn.LeakyReLU]


def test_codes_are_the_headers():
    import re
    from pathlib import Path

    from turbdiff_amd import _lib as L
    from turbdiff_amd import ops

    text = (Path(__file__).resolve().parent.parent / "include" / "tdx.h").read_text()
    header = {k: int(v) for k, v in re.findall(r"#define TDX_ACT_([A-Z]+) (\d+)", text)}
    assert header == dict(NONE=0, SILU=1, GELU=2, RELU=3, SOFTPLUS=4, TANH=5)
    for name, code in header.items():
        assert getattr(L, f"ACT_{name}") == code and getattr(ops, f"ACT_{name}") == code


@pytest.mark.parametrize("klass,code", SUPPORTED, ids=[k.__name__ for k, _ in SUPPORTED])
def test_act_code_of_the_five_modules(klass, code):
    from turbdiff_amd import ops
    from turbdiff_amd.training import ACTFNS

    assert ops.act_code(klass()) == code
    assert klass in ACTFNS.values()  # what DiffusionTrainer accepts is what the kernels evaluate


@pytest.mark.parametrize("make", UNSUPPORTED, ids=["gelu_tanh", "softplus_beta2", "leaky_relu"])
def test_act_code_of_anything_else_is_none(make):
    from turbdiff_amd import ops

    assert ops.act_code(make()) is None


def test_act_code_of_other_arguments_and_subclasses():
    from turbdiff_amd import ops

    class MySiLU(nn.SiLU):
        def forward(self, x):
            return 2 * x

    assert ops.act_code(nn.Softplus(threshold=10)) is None
    assert ops.act_code(MySiLU()) is None and ops.act_code(nn.Identity()) is None
    assert ops.act_code(nn.ReLU(inplace=True)) == 3  # the same function


def _block(actfn, dim_in=16, dim_out=16):
    from turbdiff_amd.models.ddpm import ResnetBlock

    return ResnetBlock(dim_in, dim_out, c_dim=8, actfn=actfn, norm_klass=lambda ch: nn.GroupNorm(8, ch))


@pytest.mark.parametrize("klass,code", SUPPORTED, ids=[k.__name__ for k, _ in SUPPORTED])
def test_resnet_block_is_fused_for_the_five(klass, code, monkeypatch):
    from turbdiff_amd.models import ddpm as D

    for dims in ((16, 16), (16, 32)):
        blk = _block(klass, *dims)
        assert blk.fused() and blk.block1.fused_act() == code and blk.block2.fused_act() == code
        monkeypatch.setattr(D, "FUSE_ACTFNS", False)  # read per call: the same module, the route of before
        assert blk.fused() == (klass is nn.SiLU)
        assert blk.block1.fused_act() == (1 if klass is nn.SiLU else None)
        monkeypatch.setattr(D, "FUSE_ACTFNS", True)
        assert blk.fused()
    monkeypatch.setattr(D, "FUSE_BLOCKS", False)
    assert not _block(klass).fused()


@pytest.mark.parametrize("make", UNSUPPORTED, ids=["gelu_tanh", "softplus_beta2", "leaky_relu"])
def test_resnet_block_of_anything_else_is_not_fused(make):
    blk = _block(make)
    assert not blk.fused() and blk.block1.fused_act() is None


def test_identity_skip_of_two_tensors_stays_unfused():
    x2 = torch.zeros(1)
    assert not _block(nn.GELU, 16, 16).fused(x2) and _block(nn.GELU, 16, 32).fused(x2)


def test_model_routes_follow_the_switch(monkeypatch):
    """compose_first_conv and the cached conditioning conv ask `first.fused()`: with a GELU model they are on with
    FUSE_ACTFNS and off without it."""
    from turbdiff_amd.models import ddpm as D

    net = D.DenoisingModel(in_features=4, out_features=4, c_local_features=4, c_global_features=0, timesteps=10, dim=8,
                           u_net_levels=2, norm_type="group", actfn=nn.GELU)
    blocks = [m for m in net.modules() if isinstance(m, D.ResnetBlock)]
    assert len(blocks) == 7 and all(b.fused() for b in blocks)
    monkeypatch.setattr(D, "FUSE_ACTFNS", False)
    assert not any(b.fused() for b in blocks)
    x, c = torch.zeros(1, 4, 4, 4, 4), torch.zeros(4, 4, 4, 4)
    assert net.compose_first_conv(x, c) is None  # before any device work: the route is off


def test_resnet_block_rejects_a_code_it_cannot_run():
    from turbdiff_amd import ops

    with pytest.raises(ValueError, match="TDX_ACT"):
        ops.resnet_block(None, None, None, None, None, None, None, None, None, 8, act=0)
    with pytest.raises(ValueError, match="TDX_ACT"):
        ops.resnet_block(None, None, None, None, None, None, None, None, None, 8, act=None)
