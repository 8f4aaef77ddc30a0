"""The DDIM sampler on the GPU: `ops.ddim_step` against an fp64 restatement, `ops.ddim_step_rng` bit for bit against separate
draws, recovery of a point mass under the exact denoiser, the captured loop against the eager one on the cfg1 model, and
the default (ancestral) path left as it was."""

from types import SimpleNamespace

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

SCHEDULES = {"logsnr10": ("log-snr-linear", 10, 4), "sigmoid1000": ("sigmoid", 1000, 7)}  # name, T, S


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _mask_idx(V, seed=0):
    """two thirds of the cells, scattered: about a third of every quad is outside the domain"""
    g = torch.Generator().manual_seed(seed)
    return torch.sort(torch.randperm(V, generator=g)[: (2 * V) // 3]).values


def _tables(sched, eta, start_from=None):
    from turbdiff_amd import schedules

    name, T, S = SCHEDULES[sched]
    taus = schedules.ddim_timesteps(T, S, start_from)
    return schedules.ddim_tables(name, T, taus, eta), taus


def ddim_step_f64(tab, k, x_t, eps, z, z2, x_bcs, inside, noise_bcs, clip):
    """The step of include/tdx.h in float64, reading the float32 table.  inside: bool, broadcastable to x_t."""
    recip, recipm1, sp, dirc, sigma, sbp = (float(v) for v in tab[:, k].double())
    x_t, eps, z, z2, x_bcs = (v.double() for v in (x_t, eps, z, z2, x_bcs))
    raw = recip * x_t - recipm1 * eps
    x0 = raw if noise_bcs else torch.where(inside, raw, x_t)
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    e = torch.where(x0 == raw, eps, (recip * x_t - x0) / recipm1)
    r = sp * x0 + dirc * e
    if k == 0:
        return torch.where(inside, r, x_bcs)
    outside = sp * x_bcs + sbp * z2 if noise_bcs else r
    return torch.where(inside, r + sigma * z, outside)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the update against the restatement
#
# Bound per element: |out - ref| <= 8 * 2^-24 * scale, scale = recip |x_t| + recipm1 |eps| + |x_bcs| + |z| + |z2| + 1.
# Every term of the update is a product of table entries <= 1 (sp, dir, sigma, sbp) with x0, e, z, z2 or x_bcs; x0 is one
# rounding of recip x_t and one of recipm1 eps away from exact, hence the first two terms of the scale.  Where the clip or
# the BC rule changed x0, e = (recip x_t - x0) / recipm1 divides an error of that size by recipm1 < 1, but enters through
# dir, and dir / recipm1 = sqrt((1 - p - sigma^2) a / (1 - a)) <= sqrt(a) < 1 because p = abar[tau_{k-1}] > a: the
# division never amplifies.  An fp32 torch restatement on the CPU (no FMA contraction) has a worst ratio of 1.30 in units
# of 2^-24 * scale over these cases and 1.9-2.13 with every step of cosine T = 1000, S = 50 added (two input draws); the
# factor 8 leaves about 4x for fused multiply-adds on the device (each removes a rounding, but moves the result relative to
# the unfused fp32 evaluation).  Measured on the MI355X over these cases: at most 1.34.
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("noise_bcs", [True, False])
@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("shape", [(2, 4, 6, 5, 4), (1, 4, 3, 3, 3)])  # the second: V = 27, every lane works alone
def test_ddim_step_matches_fp64_restatement(shape, sched, noise_bcs, clip):
    from turbdiff_amd import ops

    d = dev()
    S = SCHEDULES[sched][2]
    V = shape[2] * shape[3] * shape[4]
    x_t, eps, z, z2, xb = (rnd(*shape, seed=s) for s in range(5))
    idx = _mask_idx(V)
    inside = torch.zeros(V, dtype=torch.bool)
    inside[idx] = True
    inside = inside.view(shape[2:])
    mask = ops.cell_mask(idx.to(d), V)
    assert int(mask.sum()) == idx.numel() and 0 < idx.numel() < V
    dx, de, dz, dz2, dxb = (v.to(d) for v in (x_t, eps, z, z2, xb))
    worst = 0.0
    for eta in (0.0, 0.5, 1.0):
        tab, taus = _tables(sched, eta)
        tab_d, tau_d = tab.to(d), torch.tensor(taus, device=d)
        for k in (0, 1, S - 1):
            k_d, t_d = torch.tensor([k], device=d), torch.tensor([taus[k]], device=d)
            out = ops.ddim_step(dx, de, dz, dz2, dxb, mask, tab_d, k_d, tau_d, t_d, noise_bcs, clip).cpu().double()
            ref = ddim_step_f64(tab, k, x_t, eps, z, z2, xb, inside, noise_bcs, clip)
            recip, recipm1 = float(tab[0, k]), float(tab[1, k])
            scale = (recip * x_t.abs() + recipm1 * eps.abs() + xb.abs() + z.abs() + z2.abs() + 1).double()
            ratio = ((out - ref).abs() / (2.0**-24 * scale)).max().item()
            print(f"{sched} eta={eta} k={k} noise_bcs={noise_bcs} clip={clip}: worst |err| = {ratio:.2f} x 2^-24 scale")
            worst = max(worst, ratio)
            assert int(k_d) == k and int(t_d) == taus[k]  # the plain entry leaves the scalars alone
    assert worst <= 8.0, worst


def test_ddim_step_writes_nothing_for_a_finished_trajectory():
    """An index outside the tables -- k outside [0, S) for the DDIM step, t outside [0, T) for the two ancestral ones -- has
    no column: no step may read one (nor write), through either entry.  The entry that draws its noise still advances the
    offset and the index."""
    from turbdiff_amd import ops, schedules

    d = dev()
    shape = (1, 4, 2, 2, 2)
    tab, taus = _tables("logsnr10", 1.0)
    x, e, xb = (rnd(*shape, seed=s).to(d) for s in range(3))
    mo = rnd(1, 8, 2, 2, 2, seed=3).to(d)
    mask = torch.ones(8, dtype=torch.uint8, device=d)
    tab_d, tau_d, t_d = tab.to(d), torch.tensor(taus, device=d), torch.tensor([0], device=d)
    tables = schedules.diffusion_tables("log-snr-linear", 10)
    sched, plv = schedules.pack_step_tables(tables).to(d), tables["posterior_log_var"].to(d)
    sids, off = torch.tensor([3], dtype=torch.int64, device=d), torch.zeros(1, dtype=torch.int64, device=d)
    rng = (1, sids, off)
    rules = {  # number of columns, the entry on noise tensors, the entry that draws its noise
        "ddim": (4, lambda i, out: ops.ddim_step(x, e, x, x, xb, mask, tab_d, i, tau_d, t_d, True, False, out=out),
                 lambda i, out: ops.ddim_step_rng(x, e, xb, mask, tab_d, i, tau_d, t_d, True, False, *rng, out=out)),
        "ancestral": (10, lambda i, out: ops.p_sample_step(x, e, x, x, xb, mask, sched, 10, i, True, False, out=out),
                      lambda i, out: ops.p_sample_step_rng(x, e, xb, mask, sched, 10, i, True, False, *rng, out=out)),
        "lv": (10, lambda i, out: ops.p_sample_step_lv(x, mo, x, x, xb, mask, sched, plv, 10, i, True, False, out=out),
               lambda i, out: ops.p_sample_step_lv_rng(x, mo, xb, mask, sched, plv, 10, i, True, False, *rng, out=out)),
    }
    for rule, (n, plain, fused) in rules.items():
        for k in (-1, n):
            out = torch.full(shape, 7.0, device=d)
            plain(torch.tensor([k], device=d), out)
            assert torch.equal(out, torch.full(shape, 7.0, device=d)), rule
            k_d, off0 = torch.tensor([k], device=d), int(off)
            fused(k_d, out)
            assert torch.equal(out, torch.full(shape, 7.0, device=d)) and int(k_d) == k - 1, rule
            assert int(off) == off0 + 2 * (4 * 8 // 4), rule  # noise_bcs: 2 F V / 4 counters, drawn or not


# ---------------------------------------------------------------------------------------------------------------------
# 2. noise drawn in the kernel == separate draws, bit for bit
def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("noise_bcs", [True, False])
@pytest.mark.parametrize("shape", [(3, 4, 6, 5, 4), (1, 4, 2, 2, 1), (2, 4, 40, 33, 28), (1, 4, 48, 48, 32)])
def test_ddim_step_rng_matches_separate_draws_bitwise(shape, noise_bcs, clip):
    """tdx_ddim_step_rng == tdx_randn_batched(z); [tdx_randn_batched(z2);] tdx_ddim_step, bit for bit, out of place and in
    place; afterwards the offset has advanced by (2 if noise_bcs else 1) F V / 4 whatever eta is, k is k - 1 and t is
    tau[k - 1] (untouched after the last step)."""
    from turbdiff_amd import ops

    d = dev()
    S = SCHEDULES["logsnr10"][2]
    F, V = shape[1], shape[2] * shape[3] * shape[4]
    x_t, eps, xb = (rnd(*shape, seed=s).to(d) for s in range(3))
    mask = ops.cell_mask(_mask_idx(V).to(d), V)
    inside = mask.view(shape[2:]).bool()
    sids = torch.tensor([(5 << 32) | 7, (9 << 32) | 11, (1 << 32) | 2][: shape[0]], dtype=torch.int64, device=d)
    seed, off0, untouched = 1234, 4096, 77
    assert ops.p_sample_step_rng_supported(x_t)
    for eta in (0.0, 0.5, 1.0):
        tab, taus = _tables("logsnr10", eta)
        tab_d, tau_d = tab.to(d), torch.tensor(taus, device=d)
        for k in (0, 1, S - 1):
            off = torch.full((1,), off0, dtype=torch.int64, device=d)
            z = ops.randn_philox_batched(torch.empty_like(x_t), seed, sids, off)
            z2 = ops.randn_philox_batched(torch.empty_like(x_t), seed, sids, off) if noise_bcs else None
            k_d, t_d = torch.tensor([k], device=d), torch.tensor([untouched], device=d)
            ref = ops.ddim_step(x_t, eps, z, z2, xb, mask, tab_d, k_d, tau_d, t_d, noise_bcs, clip)

            off_f = torch.full((1,), off0, dtype=torch.int64, device=d)
            out = ops.ddim_step_rng(x_t, eps, xb, mask, tab_d, k_d, tau_d, t_d, noise_bcs, clip, seed, sids, off_f)
            assert torch.equal(_bits(out), _bits(ref)), (eta, k)
            assert int(off_f) == int(off) == off0 + (2 if noise_bcs else 1) * (F * V // 4)
            assert int(k_d) == k - 1
            assert int(t_d) == (taus[k - 1] if k > 0 else untouched)
            # in place, as the sampler calls it
            x_in = x_t.clone()
            off_f.fill_(off0); k_d.fill_(k)
            ops.ddim_step_rng(x_in, eps, xb, mask, tab_d, k_d, tau_d, t_d, noise_bcs, clip, seed, sids, off_f, out=x_in)
            assert torch.equal(_bits(x_in), _bits(ref)), (eta, k)
            if k > 0:
                # another seed: at eta = 0 the interior does not depend on z at all; with noise it does
                off_f.fill_(off0); k_d.fill_(k)
                other = ops.ddim_step_rng(x_t, eps, xb, mask, tab_d, k_d, tau_d, t_d, noise_bcs, clip, seed + 1, sids, off_f)
                same_inside = torch.equal(_bits(other[..., inside]), _bits(out[..., inside]))
                assert same_inside == (eta == 0.0), (eta, k)
                if noise_bcs:
                    assert not torch.equal(other[..., ~inside], out[..., ~inside])


def test_ddim_step_rng_shares_the_layout_predicate():
    from turbdiff_amd import ops

    assert not ops.p_sample_step_rng_supported(torch.zeros(1, 4, 3, 3, 3, device=dev()))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the exact denoiser of a point mass: S steps from x_T ~ N(0, I) land on it
#
# Independent of the restatement above: if the data distribution is a point mass at x*, eps = (x_t - sqrt(a) x*) /
# sqrt(1 - a) is the exact noise prediction, x0 = x* at every step and the last step returns it -- for any eta, since the
# re-derived state is again x* plus noise at the new level.  A wrong row or column of the table breaks this at once.
# Bound: atol 2e-6.  An fp32 torch restatement on the CPU gives 2.4e-7 (one ulp of |x*| in [2, 4)) in all four cases: an
# error d of x_t cancels in x0 (recip d - recipm1 d / sqrt(1 - a) = 0) and is damped in the direction term, so only the
# last steps' roundings survive; 8x that is 1.9e-6, rounded up.
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_exact_denoiser_recovers_the_point_mass(sched, eta):
    from turbdiff_amd import ops, schedules

    d = dev()
    name, T, S = SCHEDULES[sched]
    shape = (2, 4, 6, 5, 4)
    V = shape[2] * shape[3] * shape[4]
    tab, taus = _tables(sched, eta)
    abar = torch.cumprod(1.0 - schedules.betas_for(name, T).double(), dim=0)[taus]
    sa, sb = abar.sqrt().float().to(d), (1.0 - abar).sqrt().float().to(d)
    x_star = rnd(*shape, seed=21).to(d)
    mask = torch.ones(V, dtype=torch.uint8, device=d)
    sids = torch.tensor([(3 << 32) | 1, (3 << 32) | 2], dtype=torch.int64, device=d)
    off = torch.full((1,), 64, dtype=torch.int64, device=d)
    x = ops.randn_philox_batched(torch.empty_like(x_star), 99, sids, off)
    tab_d, tau_d = tab.to(d), torch.tensor(taus, device=d)
    k_d, t_d = torch.tensor([S - 1], device=d), torch.tensor([taus[-1]], device=d)
    for k in reversed(range(S)):
        assert int(k_d) == k and int(t_d) == taus[k]
        eps = (x - sa[k] * x_star) / sb[k]
        ops.ddim_step_rng(x, eps, x_star, mask, tab_d, k_d, tau_d, t_d, False, False, 99, sids, off, out=x)
    err = (x - x_star).abs().max().item()
    print(f"{sched} eta={eta}: max |x_0 - x*| = {err:.2e}")
    assert err <= 2e-6, err


# ---------------------------------------------------------------------------------------------------------------------
# 4. the loop on the cfg1 model (48 x 32 x 32 golden grid, 2 levels, T = 10)
def build_cfg1(golden, noise_bcs=True):
    from turbdiff_amd.models.ddpm import DenoisingModel, GaussianDiffusion

    net = DenoisingModel(in_features=4, out_features=4, c_local_features=4, c_global_features=0, timesteps=10, dim=8,
                         u_net_levels=2, norm_type="group")
    net.load_state_dict(golden("model_cfg1").sub("sd/"), strict=True)
    net.set_compute_dtype(torch.float32)
    return GaussianDiffusion(net, timesteps=10, beta_schedule="log-snr-linear", loss_type="l2", noise_bcs=noise_bcs).to(dev())


def cfg1_inputs(golden):
    from turbdiff_amd.models.conditioning import Conditioning

    g = golden("sample_cfg1")
    return g["x_bcs"].to(dev()), {Conditioning.Type.CELL_TYPE: g["c_local"].to(dev())}, g["cell_idx"].to(dev())


@pytest.mark.parametrize("nb", [True, False])
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_graph_ddim_sampler_equals_eager_loop(golden, eta, nb):
    """The captured DDIM sampler (device-side k, tau, t; Philox noise) reproduces the eager loop over `ops.ddim_step` fed
    with the very same noise tensors; rel-L2 1e-5 as for the ancestral twin of this test (the GroupNorm statistics merge
    per-block partials with f64 atomics, so runs agree to rounding, not bitwise)."""
    from turbdiff_amd import schedules
    from turbdiff_amd.sampling import GraphSampler

    diff = build_cfg1(golden, noise_bcs=nb)
    x_bcs, C, cidx = cfg1_inputs(golden)
    taus = schedules.ddim_timesteps(10, 4)
    gs = GraphSampler(diff, x_bcs, C, cidx, seed=42, trajectory_ids=[5, 9], sampling_timesteps=4, eta=eta)
    assert gs.steps_left == 4 and int(gs.k) == 3 and int(gs.t) == taus[-1] and gs.tau.tolist() == taus
    out_graph = gs.sample()
    assert gs.graph is not None and torch.isfinite(out_graph).all()
    assert gs.steps_left == 0 and int(gs.t) == taus[0] and int(gs.k) == -1
    stream = gs.noise_stream()
    out_eager = diff.p_sample_loop(x_bcs, C, cidx, noise_fn=lambda like: next(stream), sampling_timesteps=4, eta=eta)
    assert rel_l2(out_graph, out_eager) < 1e-5
    assert rel_l2(gs.sample(), out_graph) < 1e-5
    # sharding invariance: trajectory 9 alone, eagerly, gives row 1
    solo = GraphSampler(diff, x_bcs[1:], C, cidx, seed=42, trajectory_ids=[9], use_graph=False, sampling_timesteps=4, eta=eta)
    assert rel_l2(solo.sample()[0], out_graph[1]) < 1e-5
    # BC cells hold the boundary values exactly
    inside = torch.zeros(out_graph[0, 0].numel(), dtype=torch.bool, device=dev())
    inside[cidx] = True
    assert torch.equal(out_graph.flatten(-3)[..., ~inside], x_bcs.flatten(-3)[..., ~inside])
    assert torch.equal(out_eager.flatten(-3)[..., ~inside], x_bcs.flatten(-3)[..., ~inside])
    # the public route: same sampler class behind p_sample_loop, cached under a signature that carries S and eta
    pub = diff.p_sample_loop(x_bcs, C, cidx, seed=42, trajectory_ids=[5, 9], sampling_timesteps=4, eta=eta)
    (cached,) = diff.graph_samplers().values()
    assert cached.sampling_timesteps == 4 and cached.eta == eta and cached.signature()[-2:] == (4, eta)
    ref = GraphSampler(diff, x_bcs, C, cidx, seed=0, trajectory_ids=[5, 9], nonce=42, use_graph=False, sampling_timesteps=4, eta=eta)
    assert rel_l2(pub, ref.sample()) < 1e-5


def test_ddim_loops_visit_the_subsequence_and_separate_draws_agree(golden, monkeypatch):
    """start_from = 6 with 3 steps runs the model at t = 5, 3, 0 (eager route, recorded at the model's forward), the captured
    route started there agrees with it, and so does the sampler on separate draws + tdx_ddim_step (the route for layouts the
    fused kernel does not take)."""
    from turbdiff_amd import sampling
    from turbdiff_amd.sampling import GraphSampler

    diff = build_cfg1(golden, noise_bcs=True)
    x_bcs, C, cidx = cfg1_inputs(golden)
    gs = GraphSampler(diff, x_bcs, C, cidx, seed=7, trajectory_ids=[0, 1], sampling_timesteps=3, eta=1.0)
    full = gs.sample()  # tau = [0, 5, 9]
    assert gs.tau.tolist() == [0, 5, 9]
    out = gs.sample(start_from=6)  # same graph, tau and table refilled
    assert gs.tau.tolist() == [0, 3, 5] and gs.steps_left == 0 and int(gs.t) == 0
    seen = []
    fwd = diff.model.forward
    monkeypatch.setattr(diff.model, "forward", lambda x, t, *a, **kw: (seen.append(t.tolist()), fwd(x, t, *a, **kw))[1])
    stream = gs.noise_stream()
    eager = diff.p_sample_loop(x_bcs, C, cidx, start_from=6, noise_fn=lambda like: next(stream), sampling_timesteps=3, eta=1.0)
    monkeypatch.undo()
    assert seen == [[5, 5], [3, 3], [0, 0]]
    assert rel_l2(out, eager) < 1e-5
    assert rel_l2(gs.sample(), full) < 1e-5  # and back
    monkeypatch.setattr(sampling, "FUSED_STEP_NOISE", False)
    plain = GraphSampler(diff, x_bcs, C, cidx, seed=7, trajectory_ids=[0, 1], sampling_timesteps=3, eta=1.0)
    assert not plain.fused_noise and plain.z is not None
    assert rel_l2(plain.sample(start_from=6), out) < 1e-5
    assert plain.steps_left == 0 and int(plain.t) == 0 and int(plain.k) == -1


def test_trainer_samples_with_its_ddim_attributes(golden):
    """DiffusionTrainer.sample: the keyword override and the `sampling_timesteps` / `sampling_eta` attributes reach the same
    captured DDIM sampler; the denormalised output keeps the data values outside the domain."""
    from turbdiff_amd.training import DiffusionTrainer

    g = golden("model_cfg1")
    d = dev()
    torch.manual_seed(3)
    task = DiffusionTrainer(**{**DiffusionTrainer.SHIPPED_CONFIG, "dim": 8, "timesteps": 10}, u_net_levels=2, max_train_steps=20).to(d)
    task.model.model.load_state_dict(g.sub("sd/"))
    assert task.sampling_timesteps is None and task.sampling_eta == 0.0
    X, Y, Z = g["x"].shape[-3:]
    cell_types = torch.randint(0, 6, (X, Y, Z), generator=torch.Generator().manual_seed(11))
    mean, std = torch.tensor([0.3, -0.1, 0.2, 1.0]), torch.tensor([2.0, 1.5, 0.7, 3.0])
    raw = g["x"] * std.view(4, 1, 1, 1) + mean.view(4, 1, 1, 1)
    batch = SimpleNamespace(x=raw.to(d), cell_idx=g["cell_idx"].to(d), cell_types=cell_types.to(d), mean=mean.to(d), std=std.to(d))
    torch.manual_seed(5)
    a = task.sample(batch, sampling_timesteps=4, eta=0.5)
    (gs,) = task.model.graph_samplers().values()
    assert gs.sampling_timesteps == 4 and gs.eta == 0.5 and gs.steps_left == 0
    task.sampling_timesteps, task.sampling_eta = 4, 0.5
    torch.manual_seed(5)
    b = task.sample(batch)
    assert len(task.model.graph_samplers()) == 1 and rel_l2(b, a) < 1e-5
    inside = torch.zeros(X * Y * Z, dtype=torch.bool)
    inside[g["cell_idx"]] = True
    assert rel_l2(a.cpu().flatten(-3)[..., ~inside], raw.flatten(-3)[..., ~inside]) < 1e-5
    assert task.measure_sample_time(batch) > 0 and len(task.model.graph_samplers()) == 1


# ---------------------------------------------------------------------------------------------------------------------
# 5. the default path is untouched
def test_default_path_is_the_ancestral_one(golden):
    from turbdiff_amd import _lib as L
    from turbdiff_amd.sampling import GraphSampler

    g = golden("sample_cfg1")
    diff = build_cfg1(golden, noise_bcs=True)
    x_bcs, C, cidx = cfg1_inputs(golden)
    sig = GraphSampler.signature_of(diff, x_bcs, C)
    c = tuple(sorted((str(k), tuple(v.shape), str(v.dtype)) for k, v in C.items()))
    assert sig[:-2] == (tuple(x_bcs.shape), str(x_bcs.device), c, getattr(diff.model, "compute_dtype", None), getattr(diff.model, "conv_impl", None), L.conv_impl(),
                        True, False, 10)
    assert sig[-2:] == (None, 0.0)
    noises = [g[f"nb1/noise/{i}"].to(dev()) for i in range(int(g["nb1/n_noise"]))]
    it = iter(noises)
    out = diff.p_sample_loop(x_bcs, C, cidx, noise_fn=lambda like: next(it))
    assert next(it, None) is None
    assert rel_l2(out.cpu(), g["nb1/out"]) < 1e-4
    gs = GraphSampler(diff, x_bcs, C, cidx, seed=1)
    assert gs.sampling_timesteps is None and gs.k is None and gs.tau is None and gs.ddim_table is None and gs.steps_left == 10


def test_ddim_arguments_are_checked(golden):
    diff = build_cfg1(golden)
    x_bcs, C, cidx = cfg1_inputs(golden)
    for kw in ({"sampling_timesteps": 0}, {"sampling_timesteps": 11}, {"sampling_timesteps": 7, "start_from": 6},
               {"sampling_timesteps": 4, "eta": -0.1}, {"sampling_timesteps": 4, "eta": 1.01}):
        with pytest.raises(ValueError):
            diff.p_sample_loop(x_bcs, C, cidx, **kw)
    assert not diff.graph_samplers()
    diff.learned_variances = True
    with pytest.raises(ValueError, match="learned_variances"):
        diff.p_sample_loop(x_bcs, C, cidx, sampling_timesteps=4)
