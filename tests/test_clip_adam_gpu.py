"""optim.ClipAdam / ClipAdamW (tdx_grad_norm + tdx_adam_step, csrc/tdx_optim.hip) on the GPU against clip_grad_norm_ +
torch.optim.Adam / AdamW: the update over odd tensor sizes and several chunks, 4-byte-aligned gradient views (the scalar
path of the update skeleton), per-parameter step counts, loss scaling, state_dict interchange, and the two trainers that
route to the fused classes.  The tolerances are those of the ClipRAdam tests (tests/test_hip_ops.py): the fused kernel
rounds where torch's foreach kernels round, up to the order of fused multiply-adds inside one element's update."""

import io
import sys
from pathlib import Path

import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

pytestmark = pytest.mark.gpu

P_TOL = dict(rtol=2e-6, atol=1e-7)      # parameters
G_TOL = dict(rtol=1e-6, atol=1e-9)      # stored (clipped) gradients
V_TOL = dict(rtol=1e-4, atol=1e-12)     # exp_avg_sq

RULES = [("adam", 0.0), ("adam", 0.1), ("adamw", 1e-2), ("adamw", 0.1)]


def _pair(rule, wd, pa, pb, lr=1e-2, **kw):
    """(torch optimiser on pa, fused optimiser on pb) of one rule and weight decay"""
    from turbdiff_amd.optim import ClipAdam, ClipAdamW

    if rule == "adam":
        return torch.optim.Adam(pa, lr=lr, weight_decay=wd), ClipAdam(pb, lr=lr, weight_decay=wd, **kw)
    return torch.optim.AdamW(pa, lr=lr, weight_decay=wd), ClipAdamW(pb, lr=lr, weight_decay=wd, **kw)


def _twins(shapes, d, seed):
    torch.manual_seed(seed)
    pa = [torch.randn(s, device=d).requires_grad_() for s in shapes]
    return pa, [p.detach().clone().requires_grad_() for p in pa]


@pytest.mark.parametrize("max_norm", [0.1, None])
@pytest.mark.parametrize("rule,wd", RULES)
def test_clip_adam_matches_torch(rule, wd, max_norm):
    """8 steps; (40000,) spans three 16384-element chunks with a ragged tail, parameter 3 never gets a gradient, gradients
    alternate between x3.0 and x0.01, the LR changes at step 4."""
    d = torch.device("cuda:0")
    shapes = [(3,), (17, 5), (64, 64, 3, 3, 3), (1,), (40000,), (33, 7, 2)]
    pa, pb = _twins(shapes, d, 0)
    oa, ob = _pair(rule, wd, pa, pb, max_norm=max_norm, write_clipped_grads=True)
    for step in range(8):
        gs = [torch.randn(s, device=d) * (3.0 if step % 2 else 0.01) for s in shapes]
        for k, (a, b, g) in enumerate(zip(pa, pb, gs)):
            a.grad, b.grad = (None, None) if k == 3 else (g.clone(), g.clone())
        if step == 4:
            oa.param_groups[0]["lr"] = ob.param_groups[0]["lr"] = 3e-3
        if max_norm:
            ref_norm = torch.nn.utils.clip_grad_norm_(pa, max_norm)
        versions = [b._version for b in pb]
        oa.step()
        ob.step()
        assert all((b._version > v) == (k != 3) for k, (b, v) in enumerate(zip(pb, versions)))
        if max_norm:
            assert abs(ob.last_grad_norm.item() - ref_norm.item()) < 1e-5 * ref_norm.item()
        for k, (a, b) in enumerate(zip(pa, pb)):
            worst = ((a - b).abs() / (P_TOL["atol"] + P_TOL["rtol"] * b.abs())).max().item()
            print(f"{rule} wd {wd} clip {max_norm} step {step} tensor {k}: max |diff| / bound = {worst:.3f}")
            assert torch.allclose(a, b, **P_TOL), (step, k, (a - b).abs().max().item())
            if k != 3:
                assert torch.allclose(a.grad, b.grad, **G_TOL), (step, k)
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    for k in sa:  # (torch holds no state for the parameter that never had a gradient)
        assert float(sa[k]["step"]) == float(sb[k]["step"])
        assert torch.allclose(sa[k]["exp_avg_sq"], sb[k]["exp_avg_sq"], **V_TOL)


@pytest.mark.parametrize("rule,wd", [("adam", 0.1), ("adamw", 1e-2)])
def test_clip_adam_with_unaligned_gradient_views(rule, wd):
    """Gradients that are views into one flat fp32 buffer at an odd element offset are 4-byte but not 16-byte aligned: the
    scalar path of the update skeleton (and of the norm kernel)."""
    d = torch.device("cuda:0")
    shapes = [(5,), (7, 3), (1001,), (64, 3, 3), (20000,)]
    pa, pb = _twins(shapes, d, 1)
    oa, ob = _pair(rule, wd, pa, pb, max_norm=0.5)
    for step in range(3):
        flat = torch.randn(1 + sum(p.numel() for p in pa), device=d)
        off = 1
        for a, b in zip(pa, pb):
            n = a.numel()
            a.grad = flat[off : off + n].view_as(a).clone()
            b.grad = flat[off : off + n].view_as(b)
            off += n
        assert any(b.grad.data_ptr() % 16 for b in pb)
        torch.nn.utils.clip_grad_norm_(pa, 0.5)
        oa.step()
        ob.step()
        for k, (a, b) in enumerate(zip(pa, pb)):
            assert torch.allclose(a, b, **P_TOL), (step, k, (a - b).abs().max().item())


def test_clip_adam_parameters_at_different_step_counts():
    """Parameter 1 gets gradients every other step, parameter 3 joins late: torch keeps a step count per parameter, the fused
    optimiser follows with one launch per distinct count."""
    from turbdiff_amd.optim import ClipAdam

    d = torch.device("cuda:0")
    shapes = [(9,), (33, 5), (20000,), (7, 3)]
    pa, pb = _twins(shapes, d, 2)
    oa, ob = torch.optim.Adam(pa, lr=1e-2), ClipAdam(pb, lr=1e-2, max_norm=None)
    for step in range(9):
        for k, (a, b) in enumerate(zip(pa, pb)):
            skip = (k == 1 and step % 2 == 1) or (k == 3 and step < 4)
            g = torch.randn(a.shape, device=d)
            a.grad, b.grad = (None, None) if skip else (g.clone(), g.clone())
        oa.step()
        ob.step()
        for k, (a, b) in enumerate(zip(pa, pb)):
            assert torch.allclose(a, b, **P_TOL), (step, k)
    assert [int(oa.state[p]["step"]) for p in pa] == [int(ob.state[p]["step"]) for p in pb] == [9, 5, 9, 5]


# ---- loss scaling: the synthetic schedule of the ClipRAdam tests (helpers copied from tests/test_hip_ops.py)
_LS_SHAPES = [(5,), (17, 3), (40000,), (9, 2)]
_LS_BAD = {3: float("inf"), 4: float("nan")}  # the overflow steps of the 12-step schedule


def _ls_schedule(d):
    """12 steps of unscaled gradients, alternately large and small."""
    gen = torch.Generator().manual_seed(9)
    return [[(torch.randn(s, generator=gen) * (2.0 if step % 2 else 0.02)).to(d) for s in _LS_SHAPES] for step in range(12)]


def _ls_scaled_step(opt, params, grads, step):
    """One step of the loss-scaling optimiser: gradients S times too large, parameter 3 only on even steps, an overflow in
    parameter 2 on the bad steps."""
    S = opt.loss_scale
    for k, (p, g) in enumerate(zip(params, grads[step])):
        p.grad = None if (k == 3 and step % 2 == 1) else g * S
    if step in _LS_BAD:
        params[2].grad[123] = _LS_BAD[step]
    opt.step()


def _ls_reference_step(opt, params, grads, step):
    """The reference: clip_grad_norm_ + the torch optimiser on the unscaled gradients; an overflow step does not happen."""
    if step in _LS_BAD:
        return
    for k, (p, g) in enumerate(zip(params, grads[step])):
        p.grad = None if (k == 3 and step % 2 == 1) else g.clone()
    torch.nn.utils.clip_grad_norm_(params, 0.5)
    opt.step()


def _ls_params(d):
    gen = torch.Generator().manual_seed(4)
    return [torch.randn(s, generator=gen).to(d).requires_grad_() for s in _LS_SHAPES]


def _through_a_file(sd):
    """What a checkpoint does to a state_dict: torch.save / torch.load (no tensor shared with the live optimiser)."""
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf)


@pytest.mark.parametrize("rule,wd", [("adam", 0.0), ("adamw", 1e-2)])
def test_clip_adam_loss_scaling_unscales_skips_and_adapts(rule, wd):
    """Gradients stored 2^12 times too large give the unscaled reference's updates and norm; a step with a non-finite gradient
    changes nothing and halves the scale; `scale_growth_interval` clean steps double it; after settle() the step counts are
    torch's -- with every step waiting for its own flag (sync_flags) and with the default two-step lag."""
    d = torch.device("cuda:0")
    grads = _ls_schedule(d)
    for sync in (True, False):
        pa, pb = _ls_params(d), _ls_params(d)
        oa, ob = _pair(rule, wd, pa, pb, max_norm=0.5, loss_scale=2.0**12, scale_growth_interval=4, sync_flags=sync)
        assert ob.scale_loss(torch.tensor(1.5, device=d)).item() == 1.5 * 2.0**12
        for step in range(12):
            before = [b.detach().clone() for b in pb]
            scale = ob.loss_scale
            _ls_reference_step(oa, pa, grads, step)
            _ls_scaled_step(ob, pb, grads, step)
            if step in _LS_BAD:
                assert all(torch.equal(b, v) for b, v in zip(pb, before)), "a skipped step must not touch the parameters"
                if sync:
                    assert ob.loss_scale == scale / 2
                continue
            if sync:  # (lazy flags: the steps right behind an overflow run on a step count one or two too high)
                ref_norm = (sum(float(g.norm() ** 2) for k, g in enumerate(grads[step]) if not (k == 3 and step % 2 == 1))) ** 0.5
                assert abs(ob.last_grad_norm.item() - ref_norm) < 1e-5 * ref_norm
                for k, (a, b) in enumerate(zip(pa, pb)):
                    assert torch.allclose(a, b, rtol=3e-6, atol=2e-7), (step, k, (a - b).abs().max().item())
        ob.settle()
        # flags 0-2 clean, 3 and 4 skipped (2^12 -> 2^10), then 7 clean steps = one doubling after 4 (-> 2^11)
        assert ob.skipped_steps == 2 and ob.loss_scale == 2.0**11 and ob._clean_steps == 3
        sa, sb = oa.state_dict(), ob.state_dict()
        assert sb["loss_scaling"] == {"loss_scale": 2.0**11, "clean_steps": 3, "skipped_steps": 2, "step_index": 12}
        for k in sa["state"]:
            assert float(sa["state"][k]["step"]) == float(sb["state"][k]["step"]) == [10, 10, 10, 5][k]
            if sync:
                assert torch.allclose(sa["state"][k]["exp_avg_sq"], sb["state"][k]["exp_avg_sq"], **V_TOL)


@pytest.mark.parametrize("rule,wd", [("adam", 0.1), ("adamw", 1e-2)])
def test_clip_adam_state_dicts_interchange_with_torch(rule, wd):
    """After 4 steps a ClipAdam(W) state_dict goes through torch.save / torch.load into torch.optim.Adam(W), and torch's into
    a fresh ClipAdam(W); all four optimisers continue for 3 steps and stay together."""
    d = torch.device("cuda:0")
    shapes = [(5,), (17, 3), (40000,), (9, 2)]
    pa, pb = _twins(shapes, d, 6)
    oa, ob = _pair(rule, wd, pa, pb, max_norm=0.5)
    gen = torch.Generator().manual_seed(7)
    grads = [[torch.randn(s, generator=gen).to(d) for s in shapes] for _ in range(7)]

    def step(opt, params, i, fused):
        for p, g in zip(params, grads[i]):
            p.grad = g.clone()
        if not fused:
            torch.nn.utils.clip_grad_norm_(params, 0.5)
        opt.step()

    for i in range(4):
        step(oa, pa, i, False)
        step(ob, pb, i, True)
    from_torch, from_clip = _through_a_file(oa.state_dict()), _through_a_file(ob.state_dict())
    assert set(from_clip) == {"state", "param_groups"}
    assert {"weight_decay", "decoupled_weight_decay"} <= set(from_clip["param_groups"][0])
    assert set(from_clip["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    pc, pd = [p.detach().clone().requires_grad_() for p in pb], [p.detach().clone().requires_grad_() for p in pa]
    oc, od = _pair(rule, wd, pc, pd, max_norm=0.5)  # oc: torch continuing the fused run; od: fused continuing torch's
    oc.load_state_dict(from_clip)
    od.load_state_dict(from_torch)
    for i in range(4, 7):
        step(oa, pa, i, False)
        step(ob, pb, i, True)
        step(oc, pc, i, False)
        step(od, pd, i, True)
        for k, a in enumerate(pa):
            for name, other in (("fused", pb), ("clip->torch", pc), ("torch->clip", pd)):
                assert torch.allclose(a, other[k], **P_TOL), (name, i, k, (a - other[k]).abs().max().item())
    assert [float(od.state[p]["step"]) for p in pd] == [float(oc.state[p]["step"]) for p in pc] == [7.0] * 4


# ---- trainers
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("optimizer", ["adam", "adamw"])
def test_diffusion_trainer_trains_with_fused_adam(golden, optimizer, mode):
    """DiffusionTrainer(optimizer="adam" | "adamw") on a GPU routes to ClipAdam / ClipAdamW -- in fp16 too, under the loss
    scale -- and trains: finite losses, moving parameters, no skipped step."""
    from test_hip_model import _dense_batch
    from turbdiff_amd import optim
    from turbdiff_amd.training import DiffusionTrainer

    g = golden("model_cfg1")
    d = torch.device("cuda:0")
    batch = _dense_batch(g, d)
    torch.manual_seed(3)
    cfg = {**DiffusionTrainer.SHIPPED_CONFIG, "dim": 8, "timesteps": 10, "optimizer": optimizer}
    task = DiffusionTrainer(**cfg, u_net_levels=2, max_train_steps=20, compute_mode=mode).to(d)
    task.model.model.load_state_dict(g.sub("sd/"))
    opt, sched = task.configure_optimizers()
    want = {"adam": optim.ClipAdam, "adamw": optim.ClipAdamW}[optimizer]
    assert type(opt) is want and opt.max_norm == 0.1 and sched is not None
    assert (opt.loss_scale is not None) == (mode == "fp16")
    assert opt.param_groups[0]["weight_decay"] == (1e-2 if optimizer == "adamw" else 0.0)
    task.fused_optimizer = False
    if mode == "fp16":
        with pytest.raises(RuntimeError, match="loss-scaling optimiser"):
            task.configure_optimizers()
    else:
        assert type(task.configure_optimizers()[0]) is {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW}[optimizer]
    task.fused_optimizer = True
    before = {k: v.detach().clone() for k, v in task.model.model.named_parameters()}
    losses = [task.fit_step(batch) for _ in range(3)]
    assert type(task._opt) is want
    assert all(torch.isfinite(l) for l in losses)
    after = dict(task.model.model.named_parameters())
    assert sum(not torch.equal(before[k], after[k].detach()) for k in before) > len(before) // 2
    if mode == "fp16":
        task._opt.settle()
        assert task._opt.skipped_steps == 0
    assert float(task._opt.state[after["encode_x.weight"]]["step"]) == 3.0


def test_dilresnet_trainer_fused_adam_equals_the_torch_pair():
    """DilResNetTrainer (f32) on a GPU: ClipAdam under the LambdaLR, or torch.optim.Adam with fused_optimizer = False; three
    clipped fit_steps of the two from the same weights and noise give the same losses."""
    from test_dilresnet_gpu import _batch, _noise, _task
    from turbdiff_amd.optim import ClipAdam

    batch = _batch()
    losses = {}
    for fused in (True, False):
        t = _task("f32")
        t.fused_optimizer = fused
        t.gradient_clip_val = 0.1
        opt, sched = t.configure_optimizers()
        assert type(opt) is (ClipAdam if fused else torch.optim.Adam)
        assert isinstance(sched, torch.optim.lr_scheduler.LambdaLR) and sched.optimizer is opt
        if fused:
            assert opt.max_norm == 0.1 and opt.param_groups[0]["lr"] == t.learning_rate
        losses[fused] = [t.fit_step(batch, _noise(i)).item() for i in (1, 2, 3)]
        assert type(t._opt) is type(opt)
        assert t._sched.last_epoch == 3
    torch.testing.assert_close(losses[True], losses[False], rtol=1e-5, atol=0.0)
