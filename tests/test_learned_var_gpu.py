"""Learned variances on the HIP path: `ops.p_sample_step_lv` against an fp64 restatement, `ops.p_sample_step_lv_rng` bit for
bit against separate draws, `ops.elbo_loss` (value and gradient) against the kept torch formulation in fp64, the golden
`learned_var` loss through the fused op eagerly and in the captured training step, and the captured sampler against the
eager loops on the golden `learned_var_noelbo` model."""

from types import SimpleNamespace

import pytest
import torch

from conftest import assert_grad_close, rel_l2
from step_inputs import _loss_inputs, _mask_idx, _tables, rnd  # the seeded inputs, shared with reverse_step_cases.py

pytestmark = pytest.mark.gpu

STEP_T = {"linear": 1000, "log-linear": 50, "log-snr-linear": 10, "cosine": 1000, "sigmoid": 1000}  # T per schedule


def dev():
    return torch.device("cuda:0")


def _bits(x):
    return x.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the update against the restatement
def lv_step_f64(tab, t, x_t, out, z, z2, x_bcs, inside, noise_bcs, clip):
    """model_predictions (ddpm.py:680-693) + the loop body of _general_sample (+ its closing BC fix at t == 0) in float64,
    reading the float32 tables.  inside: bool, broadcastable to x_t."""
    F = x_t.shape[1]
    c = lambda name: float(tab[name][t].double())
    x_t, out, z, z2, x_bcs = (v.double() for v in (x_t, out, z, z2, x_bcs))
    eps, w = out[:, :F], out[:, F:]
    lb, plv = c("log_betas"), c("posterior_log_var")
    log_var = lb + torch.sigmoid(w) * (plv - lb)
    x0 = c("sqrt_recip_alphas_cumprod") * x_t - c("sqrt_recipm1_alphas_cumprod") * eps
    if not noise_bcs:
        x0 = torch.where(inside, x0, x_t)
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    mean = c("posterior_mean_coef1") * x0 + c("posterior_mean_coef2") * x_t
    if t == 0:
        return torch.where(inside, mean, x_bcs)
    noise = z if noise_bcs else torch.where(inside, z, torch.zeros_like(z))
    x = mean + (log_var / 2).exp() * noise
    if noise_bcs:
        x = torch.where(inside, x, c("sqrt_alphas_cumprod") * x_bcs + c("sqrt_one_minus_alphas_cumprod") * z2)
    return x


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("noise_bcs", [True, False])
@pytest.mark.parametrize("shape", [(2, 4, 6, 5, 4), (1, 4, 3, 3, 3)])  # the second: V = 27, every lane works alone
def test_lv_step_matches_fp64_restatement(shape, noise_bcs, clip):
    """Bound per element, as for `test_ddim_step_matches_fp64_restatement`: |out - ref| <= 8 * 2^-24 * scale, scale =
    recip |x_t| + recipm1 |eps| + |x_bcs| + |z| + |z2| + 1.  The terms of the update are products of table entries <= 1
    (coef1, coef2, sqrt_ac, sqrt_1mac) and of sigma = exp(log_var / 2) <= 1 (log_var lies between two logarithms of numbers
    below 1) with x0, x_t, z, z2 or x_bcs.  Every schedule, t in {T - 1, T / 2, 1, 0}."""
    from turbdiff_amd import ops, schedules

    d = dev()
    F, V = shape[1], shape[2] * shape[3] * shape[4]
    x_t, z, z2, xb = (rnd(*shape, seed=s) for s in range(4))
    out = rnd(shape[0], 2 * F, *shape[2:], seed=4)
    idx = _mask_idx(V)
    inside = torch.zeros(V, dtype=torch.bool)
    inside[idx] = True
    inside = inside.view(shape[2:])
    mask = ops.cell_mask(idx.to(d), V)
    assert int(mask.sum()) == idx.numel() and 0 < idx.numel() < V
    dx, do, dz, dz2, dxb = (v.to(d) for v in (x_t, out, z, z2, xb))
    worst = 0.0
    assert set(STEP_T) == set(schedules.SCHEDULES)
    for name, T in STEP_T.items():
        tab, packed = _tables(name, T)
        packed_d, plv_d = packed.to(d), tab["posterior_log_var"].to(d)
        for t in (T - 1, T // 2, 1, 0):
            t_d = torch.tensor([t], device=d)
            got = ops.p_sample_step_lv(dx, do, dz, dz2 if noise_bcs else None, dxb, mask, packed_d, plv_d, T, t_d, noise_bcs,
                                       clip).cpu().double()
            ref = lv_step_f64(tab, t, x_t, out, z, z2, xb, inside, noise_bcs, clip)
            recip, recipm1 = float(tab["sqrt_recip_alphas_cumprod"][t]), float(tab["sqrt_recipm1_alphas_cumprod"][t])
            scale = (recip * x_t.abs() + recipm1 * out[:, :F].abs() + xb.abs() + z.abs() + z2.abs() + 1).double()
            ratio = ((got - ref).abs() / (2.0**-24 * scale)).max().item()
            print(f"{name} T={T} t={t} noise_bcs={noise_bcs} clip={clip}: worst |err| = {ratio:.2f} x 2^-24 scale")
            worst = max(worst, ratio)
            assert int(t_d) == t  # the plain entry leaves the scalar alone
    assert worst <= 8.0, worst


# ---------------------------------------------------------------------------------------------------------------------
# 2. noise drawn in the kernel == separate draws, bit for bit
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("noise_bcs", [True, False])
@pytest.mark.parametrize("shape", [(3, 4, 6, 5, 4), (1, 4, 2, 2, 1), (2, 4, 40, 33, 28), (1, 4, 48, 48, 32)])
def test_lv_step_rng_matches_separate_draws_bitwise(shape, noise_bcs, clip):
    """tdx_p_sample_step_lv_rng == tdx_randn_batched(z); [tdx_randn_batched(z2);] tdx_p_sample_step_lv, bit for bit, out of
    place and in place; afterwards the offset has advanced by (2 if noise_bcs else 1) F V / 4 (F = the state's planes) and t
    is t - 1, at t == 0 too -- exactly what tdx_p_sample_step_rng does there."""
    from turbdiff_amd import ops

    d = dev()
    T = 10
    tab, packed = _tables("log-snr-linear", T)
    packed_d, plv_d = packed.to(d), tab["posterior_log_var"].to(d)
    F, V = shape[1], shape[2] * shape[3] * shape[4]
    x_t, xb = (rnd(*shape, seed=s).to(d) for s in range(2))
    mo = rnd(shape[0], 2 * F, *shape[2:], seed=2).to(d)
    mask = ops.cell_mask(_mask_idx(V).to(d), V)
    inside = mask.view(shape[2:]).bool()
    sids = torch.tensor([(5 << 32) | 7, (9 << 32) | 11, (1 << 32) | 2][: shape[0]], dtype=torch.int64, device=d)
    seed, off0 = 1234, 4096
    assert ops.p_sample_step_rng_supported(x_t)
    for t in (T - 1, T // 2, 1, 0):
        off = torch.full((1,), off0, dtype=torch.int64, device=d)
        z = ops.randn_philox_batched(torch.empty_like(x_t), seed, sids, off)
        z2 = ops.randn_philox_batched(torch.empty_like(x_t), seed, sids, off) if noise_bcs else None
        t_d = torch.tensor([t], device=d)
        ref = ops.p_sample_step_lv(x_t, mo, z, z2, xb, mask, packed_d, plv_d, T, t_d, noise_bcs, clip)
        t_d.sub_(1)  # the separate route's own decrement (GraphSampler._lv_update)

        off_f = torch.full((1,), off0, dtype=torch.int64, device=d)
        t_f = torch.tensor([t], device=d)
        out = ops.p_sample_step_lv_rng(x_t, mo, xb, mask, packed_d, plv_d, T, t_f, noise_bcs, clip, seed, sids, off_f)
        assert torch.equal(_bits(out), _bits(ref)), t
        assert int(off_f) == int(off) == off0 + (2 if noise_bcs else 1) * (F * V // 4)
        assert int(t_f) == int(t_d) == t - 1
        # in place, as the sampler calls it
        x_in = x_t.clone()
        off_f.fill_(off0); t_f.fill_(t)
        ops.p_sample_step_lv_rng(x_in, mo, xb, mask, packed_d, plv_d, T, t_f, noise_bcs, clip, seed, sids, off_f, out=x_in)
        assert torch.equal(_bits(x_in), _bits(ref)), t
        # another seed: the noise reaches the interior at t > 0 and nothing at t == 0
        off_f.fill_(off0); t_f.fill_(t)
        other = ops.p_sample_step_lv_rng(x_t, mo, xb, mask, packed_d, plv_d, T, t_f, noise_bcs, clip, seed + 1, sids, off_f)
        assert torch.equal(_bits(other), _bits(out)) == (t == 0), t
        if t > 0:
            assert not torch.equal(other[..., inside], out[..., inside])
        else:
            # t == 0 consumes what tdx_p_sample_step_rng consumes there, no more
            off_p, t_p = torch.full((1,), off0, dtype=torch.int64, device=d), torch.tensor([0], device=d)
            ops.p_sample_step_rng(x_t, mo[:, :F].contiguous(), xb, mask, packed_d, T, t_p, noise_bcs, clip, seed, sids, off_p)
            assert int(off_p) == int(off_f) and int(t_p) == int(t_f) == -1


def test_lv_step_checks_the_model_output_shape():
    from turbdiff_amd import ops

    d = dev()
    x = torch.zeros(1, 4, 2, 2, 2, device=d)
    tab, packed = _tables("log-snr-linear", 10)
    with pytest.raises(ValueError, match="eps_hat"):
        ops.p_sample_step_lv(x, x, x, x, x, torch.ones(8, dtype=torch.uint8, device=d), packed.to(d), tab["posterior_log_var"].to(d),
                             10, torch.zeros(1, dtype=torch.int64, device=d), True, False)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the loss kernel, value and gradient
def _diffusion(l1, clip, detach_mean, ew=0.1, T=10):
    from turbdiff_amd.models.ddpm import GaussianDiffusion

    return GaussianDiffusion(torch.nn.Identity(), timesteps=T, beta_schedule="log-snr-linear", loss_type="l1" if l1 else "l2",
                             noise_bcs=True, clip_denoised=clip, learned_variances=True, elbo_weight=ew, detach_elbo_mean=detach_mean)


def _ulp32(v: float) -> float:
    a = torch.tensor(abs(v), dtype=torch.float32)
    return (torch.nextafter(a, torch.tensor(float("inf"))) - a).item()


@pytest.mark.parametrize("detach_mean", [True, False])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("l1", [False, True])
@pytest.mark.parametrize("shape", [(2, 4, 6, 5, 4), (2, 4, 7, 5, 3), (2, 4, 40, 33, 28)])  # vector, scalar (V = 105), multi-block
def test_elbo_loss_matches_fp64(shape, l1, clip, detach_mean):
    """Reference: the kept torch formulation (`_p_losses_elbo_torch`) in float64 on the CPU, cell_idx gathers and autograd.
    Yardstick: the same formulation in float32 on the GPU -- the code the kernel replaced.  The kernel's error against fp64
    may be at most 2x the yardstick's, plus one fp32 ulp of the largest gradient entry (gradient, element-wise over the
    in-domain cells) or of the loss entry itself (the three losses are stored as float32: half an ulp is the format's own
    rounding, and the yardstick's error can fall below that by chance).  t = [6, 0]: both branches in one launch, sample b
    reads t[b]; [0, 0]; [T - 1, 1].  n_cells as an int and as a device scalar give the same bits.

    Measured on the MI355X over all cases, worst error relative to the value as (kernel, fp32 torch): total 5.8e-8 / 5.8e-8,
    simple 2.2e-8 / 2.2e-8, ELBO 4.9e-8 / 5.7e-8 (all at float32's own rounding: the kernel evaluates the ELBO term in
    double), gradient relative to its largest entry 1.1e-7 / 4.2e-7.  The case that the float evaluation of the ELBO term
    missed -- (7, 5, 3), l2, t = [6, 0], total 0.0616 = 0.240 - 0.1 * 1.78, kernel 2.2e-8 against fp32 torch 4.0e-9 -- is why
    it is in double.
    The test prints every pair (kernel, fp32 torch) before it asserts."""
    from turbdiff_amd import ops

    d = dev()
    B, F = shape[:2]
    V = shape[2] * shape[3] * shape[4]
    T, ew = 10, 0.1
    tab, packed = _tables("log-snr-linear", T)
    idx = _mask_idx(V)
    inside = torch.zeros(V, dtype=torch.bool)
    inside[idx] = True
    mask = ops.cell_mask(idx.to(d), V)
    diff32 = _diffusion(l1, clip, detach_mean, ew, T).to(d)
    diff64 = _diffusion(l1, clip, detach_mean, ew, T).double()
    n_dev = torch.tensor([idx.numel()], dtype=torch.int64, device=d)
    for tt in ([6, 0], [0, 0], [T - 1, 1]):
        t = torch.tensor(tt)
        out, noise, x_start, x_t = _loss_inputs(shape, t, clip, tab)
        if clip:
            raw = (tab["sqrt_recip_alphas_cumprod"][t].view(B, 1, 1, 1, 1) * x_t
                   - tab["sqrt_recipm1_alphas_cumprod"][t].view(B, 1, 1, 1, 1) * out[:, :F])
            frac = (raw.abs() > 1).float().mean().item()
            assert 0.2 < frac < 0.8, frac
        # fp64 reference
        o64 = out.double().requires_grad_()
        ref = diff64._p_losses_elbo_torch(o64, x_start.double(), x_t.double(), t, noise.double(), inside.to(torch.uint8),
                                          idx.numel(), idx, parts=True)
        ref[0].backward()
        ref_loss, ref_grad = torch.stack([v.detach() for v in ref]), o64.grad
        # yardstick: fp32 torch on the GPU
        o32 = out.to(d).requires_grad_()
        dn, dxs, dxt, dt = noise.to(d), x_start.to(d), x_t.to(d), t.to(d)
        yard = diff32._p_losses_elbo_torch(o32, dxs, dxt, dt, dn, mask, idx.numel(), idx.to(d), parts=True)
        yard[0].backward()
        yard_loss, yard_grad = torch.stack([v.detach() for v in yard]).cpu().double(), o32.grad.cpu().double()
        # the kernel
        ok = out.to(d).requires_grad_()
        total, parts = ops.elbo_loss(ok, dn, dxs, dxt, mask, idx.numel(), dt, diff32.step_tables, diff32.posterior_log_var,
                                     l1=l1, clip=clip, detach_mean=detach_mean, elbo_weight=ew, parts=True)
        total.backward()
        got_loss, got_grad = torch.cat([total.detach().view(1), parts]).cpu().double(), ok.grad.cpu().double()
        ok2 = out.to(d).requires_grad_()
        total2, parts2 = ops.elbo_loss(ok2, dn, dxs, dxt, mask, n_dev, dt, diff32.step_tables, diff32.posterior_log_var,
                                       l1=l1, clip=clip, detach_mean=detach_mean, elbo_weight=ew, parts=True)
        total2.backward()
        assert torch.equal(total2, total) and torch.equal(parts2, parts) and torch.equal(_bits(ok2.grad), _bits(ok.grad))

        for k, what in enumerate(("total", "simple", "elbo")):
            e_k, e_y = abs(got_loss[k] - ref_loss[k]).item(), abs(yard_loss[k] - ref_loss[k]).item()
            print(f"t={tt} {what}: kernel {e_k:.3e} fp32-torch {e_y:.3e} (value {ref_loss[k].item():.6f})")
            assert e_k <= 2 * e_y + _ulp32(ref_loss[k].item()), (tt, what, e_k, e_y)
        sel = inside.view(shape[2:])
        e_k = (got_grad - ref_grad)[..., sel].abs().max().item()
        e_y = (yard_grad - ref_grad)[..., sel].abs().max().item()
        gmax = ref_grad.abs().max().item()
        print(f"t={tt} grad: kernel {e_k:.3e} fp32-torch {e_y:.3e} (largest entry {gmax:.3e})")
        assert e_k <= 2 * e_y + _ulp32(gmax), (tt, e_k, e_y)
        assert got_grad[..., ~sel].abs().max().item() == 0.0
        assert got_grad[:, F:][..., sel].abs().max().item() > 0.0
        if detach_mean:
            e = out[:, :F].contiguous().to(d).requires_grad_()
            ops.masked_loss(e, dn, mask, idx.numel(), l1=l1).backward()
            assert torch.equal(_bits(ok.grad[:, :F]), _bits(e.grad))


# ---------------------------------------------------------------------------------------------------------------------
# 4. TDX_DETERMINISTIC=1
def test_elbo_loss_is_reproducible_under_the_deterministic_switch(monkeypatch):
    """The library reads TDX_DETERMINISTIC per call: with it the block partials are added on a 2^-20 grid, where float64
    additions are exact, so two launches on the same inputs (296 blocks, any order) give the same bits."""
    from turbdiff_amd import ops

    monkeypatch.setenv("TDX_DETERMINISTIC", "1")
    d = dev()
    shape = (2, 4, 40, 33, 28)
    V = shape[2] * shape[3] * shape[4]
    tab, packed = _tables("log-snr-linear", 10)
    t = torch.tensor([6, 0])
    out, noise, x_start, x_t = (v.to(d) for v in _loss_inputs(shape, t, False, tab))
    idx = _mask_idx(V)
    mask = ops.cell_mask(idx.to(d), V)
    runs = []
    for _ in range(2):
        o = out.clone().requires_grad_()
        total, parts = ops.elbo_loss(o, noise, x_start, x_t, mask, idx.numel(), t.to(d), packed.to(d), tab["posterior_log_var"].to(d),
                                     detach_mean=False, elbo_weight=0.1, parts=True)
        total.backward()
        runs.append((total.detach().clone(), parts.clone(), o.grad.clone()))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*runs))
    assert torch.isfinite(runs[0][0]) and runs[0][2].abs().sum() > 0


# ---------------------------------------------------------------------------------------------------------------------
# the golden learned-variance models (tests/golden/options.npz; built as tests/test_hip_model.py builds them)
def build_golden(golden, tag, noise_bcs=True):
    from turbdiff_amd.models.ddpm import DenoisingModel, GaussianDiffusion

    gd_kw = {"learned_var": dict(learned_variances=True, elbo_weight=0.001), "learned_var_noelbo": dict(learned_variances=True)}[tag]
    net = DenoisingModel(in_features=4, out_features=8, c_local_features=4, c_global_features=0, timesteps=10, dim=8, u_net_levels=2,
                         norm_type="group")
    sd = dict(golden("model_cfg1").sub("sd/"))
    sd.update(golden("options").sub("learned_var/sd/"))
    net.load_state_dict(sd, strict=True)
    return GaussianDiffusion(net, timesteps=10, beta_schedule="log-snr-linear", loss_type="l2", noise_bcs=noise_bcs, **gd_kw).to(dev())


def golden_inputs(golden):
    from turbdiff_amd.models.conditioning import Conditioning

    g = golden("options")
    return g["x"].to(dev()), {Conditioning.Type.CELL_TYPE: g["c_local"].to(dev())}, g["cell_idx"].to(dev()), g["t"].to(dev())


# 5. golden, eager
def test_golden_learned_var_loss_runs_on_the_fused_op(golden, monkeypatch):
    from turbdiff_amd import ops

    g = golden("options")
    tag = "learned_var"
    diff = build_golden(golden, tag)
    x, C, cidx, t = golden_inputs(golden)
    assert t.tolist() == [6, 0]
    calls = []
    fused = ops.elbo_loss
    monkeypatch.setattr(ops, "elbo_loss", lambda *a, **kw: (calls.append(kw), fused(*a, **kw))[1])
    loss, _ = diff.p_losses(x, t, C, SimpleNamespace(cell_idx=cidx), None, noise=g[f"{tag}/noise"].to(dev()))
    assert len(calls) == 1 and calls[0]["elbo_weight"] == 0.001 and calls[0]["detach_mean"] is True
    loss.backward()
    assert abs(loss.item() - g[f"{tag}/loss"].item()) < 1e-4 * abs(g[f"{tag}/loss"].item())
    for name, p in diff.model.named_parameters():
        ref = g[f"{tag}/gnorm/{name}"].item()
        got = p.grad.norm().item()
        assert abs(got - ref) < 2e-3 * ref + 2e-6, (name, got, ref)
        if f"{tag}/grad/{name}" in g.z.files:
            assert_grad_close(name, p.grad.cpu(), g[f"{tag}/grad/{name}"], 2e-3)


# 6. the captured training step
class _GraphTask:
    """What training.GraphedTrainingStep asks of a task, around a bare GaussianDiffusion and dense inputs."""

    def __init__(self, diff):
        self.model, self.ddp, self._opt = diff, None, None

    def _model_input(self, b):
        return b.x, b.C

    def _cell_idx(self, b):
        return b.cell_idx

    def parameters(self):
        return self.model.parameters()


def test_captured_training_step_runs_the_elbo_loss(golden):
    """GraphedTrainingStep on the `learned_var` configuration: loss and parameter gradients of a replay equal the eager
    fused step's (the tolerances of test_graphed_training_step_equals_the_eager_step_and_serves_other_geometries: the same
    kernels, merged by atomics), and a second geometry of the same grid -- another mask, another n_cells, read on the device
    by tdx_elbo_loss_dyn -- replays the same graph and matches its own eager step."""
    from turbdiff_amd.training import GraphedTrainingStep

    g = golden("options")
    diff = build_golden(golden, "learned_var")
    x, C, cidx, t = golden_inputs(golden)
    noise = g["learned_var/noise"].to(dev())
    geometries = [cidx, cidx[::2].contiguous()]
    gs = GraphedTrainingStep(_GraphTask(diff), inject=True)
    for i, idx in enumerate(geometries):
        diff.zero_grad(set_to_none=True)
        loss, _ = diff.p_losses(x, t, C, SimpleNamespace(cell_idx=idx), None, noise=noise)
        loss.backward()
        want = {n: p.grad.clone() for n, p in diff.named_parameters() if p.grad is not None}
        want_loss = loss.item()
        del loss  # no eager autograd graph may be alive when the step is captured
        diff.zero_grad(set_to_none=True)
        gs.set_draws(t, noise)
        got = gs(SimpleNamespace(x=x, C=C, cell_idx=idx))
        assert len(gs.slots) == 1, "both geometries must replay one graph"
        assert abs(got.item() - want_loss) < 1e-5 * abs(want_loss), (i, got.item(), want_loss)
        assert want
        for n, p in diff.named_parameters():
            if n in want:
                assert p.grad is not None, n
                dd = (p.grad - want[n]).norm().item()
                assert dd <= 1e-4 * want[n].norm().item() + 1e-9, (i, n, dd)
    assert abs(want_loss - g["learned_var/loss"].item()) > 1e-4 * abs(want_loss)  # the second geometry is another problem


# 7. the captured sampler
@pytest.mark.parametrize("nb", [True, False])
def test_graph_sampler_equals_the_eager_loops_with_learned_variances(golden, nb, monkeypatch):
    """The captured step (tdx_p_sample_step_lv_rng) against (a) the same sampler issued eagerly, (b) separate draws +
    tdx_p_sample_step_lv, (c) `_general_sample` -- torch ops, untouched -- fed the very same Philox normals in the
    reference's drawing order; rel-L2 1e-5 as tests/test_ddim_gpu.py uses for the same three-way comparison."""
    from turbdiff_amd import sampling
    from turbdiff_amd.sampling import GraphSampler

    diff = build_golden(golden, "learned_var_noelbo", noise_bcs=nb)
    x_bcs, C, cidx, _ = golden_inputs(golden)
    gs = GraphSampler(diff, x_bcs, C, cidx, seed=42, trajectory_ids=[5, 9])
    assert gs.fused_noise and gs.z is None and gs.steps_left == 10 and int(gs.t) == 9
    out_graph = gs.sample()
    assert gs.graph is not None and torch.isfinite(out_graph).all() and gs.steps_left == 0 and int(gs.t) == -1
    # (a)
    eager = GraphSampler(diff, x_bcs, C, cidx, seed=42, trajectory_ids=[5, 9], use_graph=False)
    assert rel_l2(eager.sample(), out_graph) < 1e-5 and eager.graph is None
    # (c) the same normals as tensors: x_T, then per step t > 0 z [and z2]
    stream = gs.noise_stream()
    out_general = diff.p_sample_loop(x_bcs, C, cidx, noise_fn=lambda like: next(stream))
    err = rel_l2(out_graph, out_general)
    print(f"nb={nb}: captured vs _general_sample rel-L2 {err:.2e}")
    assert err < 1e-5
    assert rel_l2(gs.sample(), out_graph) < 1e-5
    # sharding independence: trajectory 9 alone gives row 1
    solo = GraphSampler(diff, x_bcs[1:], C, cidx, seed=42, trajectory_ids=[9], use_graph=False)
    assert rel_l2(solo.sample()[0], out_graph[1]) < 1e-5
    # BC cells hold the boundary values exactly
    inside = torch.zeros(out_graph[0, 0].numel(), dtype=torch.bool, device=dev())
    inside[cidx] = True
    assert torch.equal(out_graph.flatten(-3)[..., ~inside], x_bcs.flatten(-3)[..., ~inside])
    # start_from
    assert rel_l2(gs.sample(start_from=6), eager.sample(start_from=6)) < 1e-5
    # another geometry and back
    x2, idx2 = x_bcs.flip(0).contiguous(), cidx[::2].contiguous()
    other = gs.rebind(x2, C, idx2).sample()
    ref2 = GraphSampler(diff, x2, C, idx2, seed=42, trajectory_ids=[5, 9], use_graph=False).sample()
    assert rel_l2(other, ref2) < 1e-5 and rel_l2(other, out_graph) > 1e-2
    assert rel_l2(gs.rebind(x_bcs, C, cidx).sample(), out_graph) < 1e-5
    # (b)
    monkeypatch.setattr(sampling, "FUSED_STEP_NOISE", False)
    plain = GraphSampler(diff, x_bcs, C, cidx, seed=42, trajectory_ids=[5, 9])
    assert not plain.fused_noise and plain.z is not None and (plain.z2 is not None) == nb
    assert rel_l2(plain.sample(), out_graph) < 1e-5 and int(plain.t) == -1


# 8. the public default path
def test_default_sampling_path_with_learned_variances(golden, monkeypatch):
    from turbdiff_amd.models import ddpm

    g = golden("options")
    tag = "learned_var_noelbo"
    diff = build_golden(golden, tag)
    x, C, cidx, _ = golden_inputs(golden)
    a = diff.p_sample_loop(x, C, cidx, seed=3)
    assert len(diff.graph_samplers()) == 1
    (gs,) = diff.graph_samplers().values()
    assert gs.signature()[-2:] == ("learned-variances", 0.0) and gs.graph is not None
    assert torch.equal(diff.p_sample_loop(x, C, cidx, seed=3), a)
    assert rel_l2(diff.p_sample_loop(x, C, cidx, seed=4), a) > 1e-2
    assert len(diff.graph_samplers()) == 1
    # a weight update re-captures
    graph = gs.graph
    with torch.no_grad():
        next(diff.model.parameters()).mul_(1.0)
    diff.p_sample_loop(x, C, cidx, seed=3)
    assert gs.graph is not graph
    with pytest.raises(ValueError, match="learned_variances"):
        diff.p_sample_loop(x, C, cidx, sampling_timesteps=4)
    # noise_fn= and GRAPH_SAMPLER off: the eager torch loop, no sampler, the golden sample
    noises = [g[f"{tag}/sample_noise/{i}"].to(dev()) for i in range(int(g[f"{tag}/n_noise"]))]
    for off in (False, True):
        fresh = build_golden(golden, tag)
        if off:
            monkeypatch.setattr(ddpm, "GRAPH_SAMPLER", False)
            torch.manual_seed(5)
            assert torch.isfinite(fresh.p_sample_loop(x, C, cidx)).all()
        it = iter(noises)
        out = fresh.p_sample_loop(x, C, cidx, noise_fn=lambda like: next(it))
        assert next(it, None) is None and not fresh.graph_samplers()
        assert rel_l2(out.cpu(), g[f"{tag}/sample"]) < 1e-4
