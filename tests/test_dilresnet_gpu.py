"""DilResNet regression baseline on the GPU: the task against the reference's golden vectors (f32 and bf16 paths), the fused
bf16 chain against the same network composed from ops.conv3d and torch elementwise ops, every epilogue / fold option of
tdx_convg_apply_fused / tdx_convg_fold_fused against an fp32 composition, the rollout's invariants, and the full-size
shapes-dataset configuration."""

import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE / "golden"))

from conftest import rel_l2  # noqa: E402
from make_golden_dilresnet import golden_weights  # noqa: E402
from test_dilresnet_host import TASK_CFG, _stats  # noqa: E402

pytestmark = pytest.mark.gpu
G = np.load(HERE / "golden" / "dilresnet.npz")
DEV = "cuda:0"

# bf16 against the fp32 reference.  Forward output, d c_enc and the encode / decode gradients of the bf16 chain are within
# 0.5 % of fp32 (measured 3-4e-3: operands rounded to bf16, unit roundoff 2^-9, at each of the 2 + 7 N convs).  The weight
# gradients INSIDE the blocks are not: they are sums over every voxel of small activations times a data gradient dominated
# by the residual stream, with heavy cancellation, and bf16 moves them by 5-15 % rel-L2 -- the unfused bf16 composition
# (ops.conv3d + torch ReLU / adds) as much as the fused chain (both measured at 194 x 50 x 50 and 23 x 17 x 13).  So the
# fused chain is held to the unfused composition's error against the same fp32 values: per parameter within 2.5x + 5e-3,
# and over all parameters (root mean square) within 1.3x.  A wrong tap, mask, addend or fold gives O(1) errors.
BF16_WELL = 1e-2
F32_TOL = 2e-5  # fp32 reordering (27 taps x channels summed in another order than the CPU's)


def _batch(dev=DEV):
    import h5fake
    from turbdiff_amd.data.ofles import OpenFOAMBatch, OpenFOAMData, OpenFOAMDataRepository, Variable
    from turbdiff_amd.data.ofles_seq import OpenFOAMSequenceDataset

    files = h5fake.install_cases()
    ds = OpenFOAMSequenceDataset(OpenFOAMDataRepository(files["train"], (Variable.U, Variable.P), opener=h5fake.File), _stats(),
                                 sequence_length=2, stride=1)
    b = ds[[int(i) for i in G["batch/idx"]]]
    d = b.data
    return OpenFOAMBatch(OpenFOAMData(d.metadata.to(dev), d.t.to(dev), {v: s.to(dev) for v, s in d.samples.items()}),
                         b.stats.to(dev))


def _task(mode, **over):
    from turbdiff_amd.data.ofles import Variable
    from turbdiff_amd.regression import DilResNetTrainer

    t = DilResNetTrainer(variables=(Variable.U, Variable.P), compute_mode=mode, **{**TASK_CFG, **over})
    golden_weights(t, salt=1 if over.get("cell_pos_features") else 0)
    return t.to(DEV)


def _noise(i):
    return torch.from_numpy(G[f"noise/{i}"]).to(DEV)


def _no_worse_than_unfused(fused: dict, unfused: dict, ref: dict):
    """Per key: err(fused) <= 2.5 err(unfused) + 5e-3, and the rms of the errors within 1.3x (see BF16_WELL)."""
    ef = {k: rel_l2(fused[k], ref[k]) for k in ref}
    eu = {k: rel_l2(unfused[k], ref[k]) for k in ref}
    for k in ref:
        assert ef[k] <= 2.5 * eu[k] + 5e-3, (k, ef[k], eu[k])
    rms = lambda e: (sum(v * v for v in e.values()) / len(e)) ** 0.5
    assert rms(ef) <= 1.3 * rms(eu), (rms(ef), rms(eu))


def _bf16_task_grads(batch, unfused: bool):
    """Loss, conditioning gradient and parameter gradients of one bf16 training step; `unfused` routes the network through
    the ops.conv3d + torch composition instead of the fused chain (the yardstick of _no_worse_than_unfused)."""
    t = _task("bf16")
    if unfused:
        t.model.forward_nvc = t.model.forward_unfused
    seen = {}
    orig = t._model_input

    def model_input(b):
        xx, CC = orig(b)
        for v in CC.values():
            v.retain_grad()
        seen.update(CC)
        return xx, CC

    t._model_input = model_input
    loss = t.training_step(batch, _noise(0))
    loss.backward()
    grads = {f"grad/{k}": p.grad.detach().cpu() for k, p in t.named_parameters()}
    grads["dC"] = next(iter(seen.values())).grad.detach().cpu()
    return loss.item(), grads


def test_golden_f32_forward_gradients_training_unroll():
    batch = _batch()
    t = _task("f32")
    x, C = t._model_input(batch)
    assert rel_l2(x[:, 0].cpu(), torch.from_numpy(G["fwd/x0"])) < 1e-6
    y = t.model(x[:, 0], C)
    assert rel_l2(y.detach().cpu(), torch.from_numpy(G["fwd/y"])) < F32_TOL

    # the training loss's gradients, the conditioning's included
    seen = {}
    orig = t._model_input

    def model_input(b):
        xx, CC = orig(b)
        for v in CC.values():
            v.retain_grad()
        seen.update(CC)
        return xx, CC

    t._model_input = model_input
    loss = t.training_step(batch, _noise(0))
    loss.backward()
    assert abs(loss.item() - float(G["loss0"])) / float(G["loss0"]) < F32_TOL
    dC = next(iter(seen.values())).grad
    assert rel_l2(dC.cpu(), torch.from_numpy(G["dC"])) < F32_TOL
    for k, p in t.named_parameters():
        assert rel_l2(p.grad.cpu(), torch.from_numpy(G[f"grad/{k}"])) < F32_TOL, k
    np.testing.assert_allclose(t.dx_mean.cpu().numpy(), G["after0/dx_mean"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(t.dx_var.cpu().numpy(), G["after0/dx_var"], rtol=1e-5)

    # 3 optimiser steps with clipping; then the 5-step unroll in blocks of 2
    t = _task("f32")
    t.gradient_clip_val = 0.1
    losses = [t.fit_step(batch, _noise(i)).item() for i in (1, 2, 3)]
    np.testing.assert_allclose(losses, G["train/losses"], rtol=F32_TOL)
    sd, sd0 = t.state_dict(), _task("f32").state_dict()
    for k in G.files:
        if k.startswith("train/sd/"):
            name = k[len("train/sd/"):]
            ref = torch.from_numpy(G[k])
            if ref.dtype == torch.int64:
                assert int(sd[name]) == int(ref), name
            else:
                # Adam's first steps move every weight by ~lr whatever the gradient's size: compare the update, not the weight
                w0 = sd0[name].cpu()
                assert rel_l2(sd[name].cpu() - w0, ref - w0) < 1e-4, name
    t.eval()
    xs = t.unroll_samples(batch, [0, 1, 2, 3, 4], block_size=2)
    assert rel_l2(xs.cpu(), torch.from_numpy(G["unroll/x"])) < 1e-5


def test_golden_bf16_forward_gradients_training():
    """The bf16 task against the reference's fp32 values: forward and loss within BF16_WELL, the gradients no farther from
    them than the unfused bf16 composition's.  Training: the losses of 3 clipped Adam steps.  The weights after them are not
    compared: Adam divides by the gradient's rms, so the bf16 noise of the block-internal gradients becomes an O(1) change of
    their first updates (measured: 0.7 rel-L2 for the unfused composition too)."""
    batch = _batch()
    t = _task("bf16")
    x, C = t._model_input(batch)
    y = t.model(x[:, 0].to(torch.bfloat16), C)
    assert rel_l2(y.detach().cpu(), torch.from_numpy(G["fwd/y"])) < BF16_WELL
    loss_f, gf = _bf16_task_grads(batch, unfused=False)
    _, gu = _bf16_task_grads(batch, unfused=True)
    assert abs(loss_f - float(G["loss0"])) / float(G["loss0"]) < 1e-3
    ref = {k: torch.from_numpy(G[k]) for k in gf}
    _no_worse_than_unfused(gf, gu, ref)
    for k in ("grad/model.encode.weight", "grad/model.decode.weight", "grad/model.encode_c_local.weight", "dC"):
        assert rel_l2(gf[k], ref[k]) < BF16_WELL, k
    t = _task("bf16")
    t.gradient_clip_val = 0.1
    losses = [t.fit_step(batch, _noise(i)).item() for i in (1, 2, 3)]
    np.testing.assert_allclose(losses, G["train/losses"], rtol=1e-3)
    assert int(t.n_train_batches_tracked) == 3


def test_golden_conditioning_width_11():
    batch = _batch()
    for mode, tol in (("f32", F32_TOL), ("bf16", BF16_WELL)):
        t = _task(mode, cell_pos_features=True)
        x, C = t._model_input(batch)
        y = t.model(x[:, 0].to(t.compute_dtype), C)
        assert rel_l2(y.detach().cpu(), torch.from_numpy(G["c11/y"])) < tol
        y.backward(torch.from_numpy(G["c11/gy"]).to(DEV))
        assert rel_l2(t.model.encode_c_local.weight.grad.cpu(), torch.from_numpy(G["c11/grad_encode_c_local"])) < tol
        assert rel_l2(t.model.encode.weight.grad.cpu(), torch.from_numpy(G["c11/grad_encode"])) < tol


# ----------------------------------------------------------------------------------------------- fused vs unfused


def _net(H=48, N=4, cc=8, seed=0):
    from turbdiff_amd.models.dilresnet import DilResNet

    torch.manual_seed(seed)
    return DilResNet(4, cc, 0, N=N, hidden_dim=H).to(DEV)


def _three_way(net, x, c, gy):
    """Output, d c_enc and every parameter gradient of net on NDHWC inputs: fp32 composition, fused bf16 chain, unfused bf16
    composition on the same bf16-rounded operands."""
    res = {}
    for name, fn, dt in (("f32", net.forward_unfused, torch.float32), ("fused", net.forward_nvc, torch.bfloat16),
                         ("unfused", net.forward_unfused, torch.bfloat16)):
        net.zero_grad(set_to_none=True)
        cl = c.to(torch.bfloat16).to(dt).requires_grad_()
        y = fn(x.to(torch.bfloat16).to(dt), cl)
        (y * gy).sum().backward()
        res[name] = {"out": y.detach().float().cpu(), "dc": cl.grad.float().cpu(),
                     **{k: p.grad.detach().cpu() for k, p in net.named_parameters() if p.grad is not None}}
        del y
    return res


def _check_three_way(res, n_blocks):
    f, u, r = res["fused"], res["unfused"], res["f32"]
    assert set(f) == set(u) == set(r) and len(f) == 2 + 2 * (2 + 7 * n_blocks)  # encode_c_local is not part of forward_nvc
    for k in ("out", "dc", "encode.weight", "encode.bias", "decode.weight"):
        assert rel_l2(f[k], r[k]) < BF16_WELL, k
        assert rel_l2(f[k], u[k]) < BF16_WELL, k
    _no_worse_than_unfused(f, u, r)


def test_fused_chain_matches_unfused_bf16():
    """Same bf16 operands, same network, a ragged grid: the fused chain against ops.conv3d + torch ReLU / adds and both against
    fp32.  The two bf16 paths round at different places (the fused epilogue adds in fp32 and rounds once, the composition
    rounds after each op), so they are compared through their distance to fp32 (BF16_WELL)."""
    net = _net()
    g = torch.Generator(device=DEV).manual_seed(1)
    B, X, Y, Z = 2, 23, 17, 13
    x = torch.randn(B, X, Y, Z, 8, device=DEV, generator=g)
    x[..., 4:] = 0
    c = 0.3 * torch.randn(1, X, Y, Z, 48, device=DEV, generator=g)
    gy = torch.randn(B, X, Y, Z, 8, device=DEV, generator=g)
    gy[..., 4:] = 0
    _check_three_way(_three_way(net, x, c, gy), 4)


def _ref_conv(x, w, b, d):
    """fp32 composition of a bf16 conv: bf16 operands, fp32 arithmetic (stock PyTorch on the GPU)."""
    xp = F.pad(x.float().movedim(-1, 1), (d,) * 6, mode="replicate")
    return F.conv3d(xp, w.to(torch.bfloat16).float(), b, dilation=d).movedim(1, -1)


@pytest.mark.parametrize("cout", [8, 48, 64])
@pytest.mark.parametrize("dil", [1, 2, 3, 8])
@pytest.mark.parametrize("relu,n_add,with_h,f32", [(False, 0, False, False), (True, 0, False, False), (True, 1, True, False),
                                                   (True, 2, True, False), (False, 1, False, True), (False, 2, False, True)])
def test_kernel_epilogue_options(cout, dil, relu, n_add, with_h, f32):
    from turbdiff_amd import ops
    from turbdiff_amd.models.dilresnet import conv_fused

    g = torch.Generator(device=DEV).manual_seed(cout * 100 + dil)
    B, X, Y, Z, cin = 2, 11, 6, 19, 16
    x = torch.randn(B, X, Y, Z, cin, device=DEV, generator=g).to(torch.bfloat16)
    w = torch.randn(cout, cin, 3, 3, 3, device=DEV, generator=g) * 0.1
    b = torch.randn(cout, device=DEV, generator=g)
    adds = [torch.randn(B if i == 0 else 1, X, Y, Z, cout, device=DEV, generator=g).to(torch.bfloat16) for i in range(n_add)]
    h = torch.empty(B, X, Y, Z, cout, device=DEV, dtype=torch.bfloat16) if with_h else None
    out = conv_fused(x, ops._taps_first(w, 1, 0), b, cout, dil, relu=relu, add0=adds[0] if n_add > 0 else None,
                     add1=adds[1] if n_add > 1 else None, h=h, out_f32=f32)
    z = _ref_conv(x, w, b, dil)
    r = torch.relu(z) if relu else z
    ref = r + sum(a.float() for a in adds) if adds else r
    assert out.dtype == (torch.float32 if f32 else torch.bfloat16)
    tol = 1e-5 if f32 else 8e-3  # fp32 store: reordering only; bf16 store: one rounding (2^-9 relative)
    assert (out.float() - ref).abs().max().item() <= tol * ref.abs().max().item() + 1e-4
    if with_h:
        assert (h.float() - r).abs().max().item() <= 8e-3 * r.abs().max().item()


@pytest.mark.parametrize("dil", [1, 4, 8])
def test_kernel_rollout_mode(dil):
    from turbdiff_amd import ops
    from turbdiff_amd.models.dilresnet import conv_fused

    g = torch.Generator(device=DEV).manual_seed(dil)
    B, X, Y, Z, cin, Fn = 3, 9, 7, 12, 48, 4
    u = torch.randn(B, X, Y, Z, cin, device=DEV, generator=g).to(torch.bfloat16)
    w = torch.randn(8, cin, 3, 3, 3, device=DEV, generator=g) * 0.05
    w[Fn:] = 0
    b = torch.randn(8, device=DEV, generator=g)
    b[Fn:] = 0
    xs = torch.randn(B, X, Y, Z, Fn, device=DEV, generator=g)
    inside = (torch.rand(X, Y, Z, device=DEV, generator=g) > 0.3).to(torch.uint8)
    mean, std = torch.randn(Fn, device=DEV, generator=g), torch.rand(Fn, device=DEV, generator=g) + 0.5
    xn = torch.empty_like(xs)
    xb = torch.full((B, X, Y, Z, 8), 7.0, device=DEV, dtype=torch.bfloat16)
    conv_fused(u, ops._taps_first(w, 1, 0), b, 8, dil, out=xb, rollout=(xs, xn, inside, mean, std))
    z = _ref_conv(u, w, b, dil)[..., :Fn]
    ref = torch.where(inside[..., None].bool(), xs + (mean + std * z), xs)
    out_m = ~inside.bool()
    assert torch.equal(xn[:, out_m], xs[:, out_m])  # outside: bit-identical
    assert (xn - ref).abs().max().item() < 1e-4 * ref.abs().max().item() + 1e-5
    assert torch.equal(xb[..., :Fn], xn.to(torch.bfloat16)) and torch.equal(xb[..., Fn:], torch.zeros_like(xb[..., Fn:]))


@pytest.mark.parametrize("pad", [1, 8])
def test_kernel_fold_options(pad):
    from turbdiff_amd import _lib as L
    from turbdiff_amd.models.dilresnet import fold_fused

    g = torch.Generator(device=DEV).manual_seed(pad)
    B, X, Y, Z, C = 3, 5, 9, 4, 48
    dpad = torch.randn(B, X + 2 * pad, Y + 2 * pad, Z + 2 * pad, C, device=DEV, generator=g).to(torch.bfloat16)
    res = torch.randn(B, X, Y, Z, C, device=DEV, generator=g).to(torch.bfloat16)
    msrc = torch.randn(B, X, Y, Z, C, device=DEV, generator=g).to(torch.bfloat16)
    folded = torch.empty(B, X, Y, Z, C, device=DEV, dtype=torch.float32)
    L.call("tdx_convg_fold_clamp", L.ptr(dpad.float().contiguous()), L.ptr(folded), B, X, Y, Z, pad, C, L.F32, L.stream())
    acc0 = torch.randn(X, Y, Z, C, device=DEV, generator=g)
    for use_res in (False, True):
        for use_mask in (False, True):
            dx = torch.empty_like(res)
            dm = torch.empty_like(res) if use_mask else None
            acc = acc0.clone()
            fold_fused(dpad, (X, Y, Z), pad, res=res if use_res else None, mask_src=msrc if use_mask else None, dx=dx,
                       dx_masked=dm, acc=acc)
            t = folded + (res.float() if use_res else 0)
            assert (dx.float() - t).abs().max().item() <= 8e-3 * t.abs().max().item()
            assert (acc - (acc0 + t.sum(0))).abs().max().item() < 1e-4 * t.abs().max().item() * B
            if use_mask:
                assert torch.equal(dm, torch.where(msrc > 0, dx, torch.zeros_like(dx)))


# ----------------------------------------------------------------------------------------------- rollout invariants


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_rollout_outside_frozen_and_conditioning_once(mode):
    batch = _batch()
    t = _task(mode)
    with torch.no_grad():
        t.dx_mean.fill_(0.1)
        t.dx_var.fill_(4.0)
    t.eval()
    x, _ = t._model_input(batch)
    calls = t.model.encode_c_local_calls
    xs = t.unroll_samples(batch, [0, 1, 2, 3, 4, 5, 6], block_size=3)
    assert t.model.encode_c_local_calls == calls + 1  # once per batch, not per block or step
    x0 = t.normalization.denormalize_grid(x[:, 0], batch.stats)
    outside = ~batch.data.metadata.inside_mask
    for s in range(xs.shape[1]):
        assert torch.equal(xs[:, s][..., outside], x0[..., outside])
    assert torch.isfinite(xs).all() and not torch.equal(xs[:, -1], xs[:, 0])
    if mode == "bf16":  # the fused rollout against the same network run step by step through the unfused composition
        ref = _task("f32")
        ref.load_state_dict(t.state_dict())
        ref.eval()
        xr = ref.unroll_samples(batch, [0, 1, 2, 3, 4, 5, 6], block_size=3)
        assert rel_l2(xs, xr) < 2e-2


# ----------------------------------------------------------------------------------------------- full size


def test_full_size_bf16_against_f32_and_rollout():
    """B = 3 on the shapes grid 194 x 50 x 50, hidden 48, N 4: the fused bf16 chain and the unfused bf16 composition against
    the f32 path (BF16_WELL).  Then a 2-step fused rollout at B = 8."""
    from turbdiff_amd.models.conditioning import Conditioning

    net = _net(seed=3)
    g = torch.Generator(device=DEV).manual_seed(5)
    B, X, Y, Z = 3, 194, 50, 50
    x = torch.randn(B, X, Y, Z, 8, device=DEV, generator=g)
    x[..., 4:] = 0
    C = {Conditioning.Type.CELL_TYPE: torch.randn(8, X, Y, Z, device=DEV, generator=g)}
    c = net.encode_conditioning(C, torch.float32).detach()
    gy = torch.randn(B, X, Y, Z, 8, device=DEV, generator=g)
    gy[..., 4:] = 0
    _check_three_way(_three_way(net, x, c, gy), 4)

    xb = torch.randn(8, 4, X, Y, Z, device=DEV, generator=g)
    inside = torch.rand(X, Y, Z, device=DEV, generator=g) > 0.2
    out = net.unroll(xb, C, inside, torch.zeros(4, device=DEV), torch.ones(4, device=DEV) * 0.01, 2, dtype=torch.bfloat16)
    assert out.shape == (8, 2, 4, X, Y, Z) and torch.isfinite(out).all()
    assert torch.equal(out[:, 1][..., ~inside], xb[..., ~inside])
    ref = net.unroll(xb, C, inside, torch.zeros(4, device=DEV), torch.ones(4, device=DEV) * 0.01, 2, dtype=torch.float32)
    assert rel_l2(out, ref) < 1e-3  # the update is 1 % of the state: bf16's error on it is ~1e-2 of 1e-2
