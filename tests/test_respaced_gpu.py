"""A learned-variance model over S of T steps on the GPU: `ops.p_sample_step_lv_respaced` against an fp64 restatement and
bit for bit against `ops.p_sample_step_lv` on the training chain's own columns, `ops.ddim_step_lv` bit for bit against
`ops.ddim_step` with NaN in the w half, the `_rng` entries bit for bit against separate draws, recovery of a point mass under
the exact denoiser, the captured samplers against the eager loops on the golden learned-variance model, the trainer, and the
default calls left as they were."""

from types import SimpleNamespace

import pytest
import torch

from conftest import rel_l2
from respaced_reference import respaced_step_f64
from step_inputs import _mask_idx, _tables, rnd
from test_learned_var_gpu import STEP_T, build_golden, golden_inputs

pytestmark = pytest.mark.gpu

S_OF = {"linear": 7, "log-linear": 7, "log-snr-linear": 4, "cosine": 7, "sigmoid": 7}  # steps per schedule (T: STEP_T)


def dev():
    return torch.device("cuda:0")


def _bits(x):
    return x.contiguous().view(torch.int32)


def _respaced(name, start_from=None):
    from turbdiff_amd import schedules

    T = STEP_T[name]
    taus = schedules.ddim_timesteps(T, S_OF[name], start_from)
    return schedules.respaced_tables(name, T, taus), taus


def _ddim(eta, name="log-snr-linear"):
    from turbdiff_amd import schedules

    T = STEP_T[name]
    taus = schedules.ddim_timesteps(T, S_OF[name])
    return schedules.ddim_tables(name, T, taus, eta), taus


# ---------------------------------------------------------------------------------------------------------------------
# 1. the respaced update against the restatement
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("noise_bcs", [True, False])
@pytest.mark.parametrize("shape", [(2, 4, 6, 5, 4), (1, 4, 3, 3, 3)])  # the second: V = 27, every lane works alone
def test_respaced_step_matches_fp64_restatement(shape, noise_bcs, clip):
    """Bound per element, that of `test_lv_step_matches_fp64_restatement`: |out - ref| <= 8 * 2^-24 * scale, scale =
    recip |x_t| + recipm1 |eps| + |x_bcs| + |z| + |z2| + 1.  Its premise -- coef1, coef2, sqrt_p, sqrt_one_minus_p and
    sigma = exp(log_var / 2) all <= 1, log_var between two logarithms of numbers below 1 -- is what
    tests/test_respaced_host.py::test_subsequence_tables checks of the table.  Every schedule, k in {0, 1, S / 2, S - 1}."""
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
    for name in STEP_T:
        tab, taus = _respaced(name)
        S = len(taus)
        tab_d, tau_d = tab.to(d), torch.tensor(taus, device=d)
        for k in (0, 1, S // 2, S - 1):
            k_d, t_d = torch.tensor([k], device=d), torch.tensor([taus[k]], device=d)
            got = ops.p_sample_step_lv_respaced(dx, do, dz, dz2 if noise_bcs else None, dxb, mask, tab_d, k_d, tau_d, t_d,
                                                noise_bcs, clip).cpu().double()
            ref = respaced_step_f64(tab, k, x_t, out, z, z2, xb, inside, noise_bcs, clip)
            recip, recipm1 = float(tab[0, k]), float(tab[1, k])
            scale = (recip * x_t.abs() + recipm1 * out[:, :F].abs() + xb.abs() + z.abs() + z2.abs() + 1).double()
            ratio = ((got - ref).abs() / (2.0**-24 * scale)).max().item()
            print(f"{name} T={STEP_T[name]} S={S} k={k} noise_bcs={noise_bcs} clip={clip}: worst |err| = {ratio:.2f} x 2^-24 scale")
            worst = max(worst, ratio)
            assert int(k_d) == k and int(t_d) == taus[k]  # the plain entry leaves the scalars alone
    assert worst <= 8.0, worst


# ---------------------------------------------------------------------------------------------------------------------
# 2. one element function: the training chain's columns give the training chain's bits
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("noise_bcs", [True, False])
@pytest.mark.parametrize("shape", [(2, 4, 6, 5, 4), (1, 4, 3, 3, 3)])
def test_respaced_step_on_the_training_columns_is_the_lv_step_bitwise(shape, noise_bcs, clip):
    """An [8, T] table assembled from the diffusion's own float32 columns, tau = range(T): the respaced entry at k = t
    equals `ops.p_sample_step_lv` at t in every cell, bit for bit -- the rule calls LvRule's element function, it does not
    restate it."""
    from turbdiff_amd import ops, schedules

    d = dev()
    F, V = shape[1], shape[2] * shape[3] * shape[4]
    x_t, z, z2, xb = (rnd(*shape, seed=s).to(d) for s in range(4))
    mo = rnd(shape[0], 2 * F, *shape[2:], seed=4).to(d)
    mask = ops.cell_mask(_mask_idx(V).to(d), V)
    for name, T in STEP_T.items():
        tab, packed = _tables(name, T)
        rows = [tab[n] for n in schedules.PACKED_ORDER[:5]] + [tab["posterior_log_var"], tab["sqrt_alphas_cumprod"],
                                                               tab["sqrt_one_minus_alphas_cumprod"]]
        tab8 = torch.stack(rows).contiguous().to(d)
        assert schedules.PACKED_ORDER[5:] == ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod") and tab8.shape == (8, T)
        packed_d, plv_d, tau_d = packed.to(d), tab["posterior_log_var"].to(d), torch.arange(T, device=d)
        for t in (T - 1, T // 2, 1, 0):
            t_d = torch.tensor([t], device=d)
            want = ops.p_sample_step_lv(x_t, mo, z, z2 if noise_bcs else None, xb, mask, packed_d, plv_d, T, t_d, noise_bcs, clip)
            got = ops.p_sample_step_lv_respaced(x_t, mo, z, z2 if noise_bcs else None, xb, mask, tab8, t_d.clone(), tau_d, t_d,
                                                noise_bcs, clip)
            assert torch.equal(_bits(got), _bits(want)), (name, t)


# ---------------------------------------------------------------------------------------------------------------------
# 3. noise drawn in the kernel == separate draws, bit for bit (both new pairs)
def _pair(which, eta=None):
    from turbdiff_amd import ops

    if which == "respaced":
        tab, taus = _respaced("log-snr-linear")
        return ops.p_sample_step_lv_respaced, ops.p_sample_step_lv_respaced_rng, tab, taus
    tab, taus = _ddim(eta)
    return ops.ddim_step_lv, ops.ddim_step_lv_rng, tab, taus


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("noise_bcs", [True, False])
@pytest.mark.parametrize("shape", [(3, 4, 6, 5, 4), (1, 4, 2, 2, 1), (2, 4, 40, 33, 28), (1, 4, 48, 48, 32)])
@pytest.mark.parametrize("which,eta", [("respaced", None), ("ddim", 0.0), ("ddim", 1.0)])
def test_rng_entries_match_separate_draws_bitwise(which, eta, shape, noise_bcs, clip):
    """<entry>_rng == tdx_randn_batched(z); [tdx_randn_batched(z2);] <entry>, bit for bit, out of place and in place;
    afterwards the offset has advanced by (2 if noise_bcs else 1) F V / 4 (F = the state's planes), k is k - 1 and t is
    tau[k - 1] (untouched after the last step)."""
    from turbdiff_amd import ops

    d = dev()
    plain, fused, tab, taus = _pair(which, eta)
    S = len(taus)
    F, V = shape[1], shape[2] * shape[3] * shape[4]
    x_t, xb = (rnd(*shape, seed=s).to(d) for s in range(2))
    mo = rnd(shape[0], 2 * F, *shape[2:], seed=2).to(d)
    mask = ops.cell_mask(_mask_idx(V).to(d), V)
    inside = mask.view(shape[2:]).bool()
    sids = torch.tensor([(5 << 32) | 7, (9 << 32) | 11, (1 << 32) | 2][: shape[0]], dtype=torch.int64, device=d)
    seed, off0, untouched = 1234, 4096, 77
    assert ops.p_sample_step_rng_supported(x_t)
    tab_d, tau_d = tab.to(d), torch.tensor(taus, device=d)
    for k in (0, 1, S - 1):
        off = torch.full((1,), off0, dtype=torch.int64, device=d)
        z = ops.randn_philox_batched(torch.empty_like(x_t), seed, sids, off)
        z2 = ops.randn_philox_batched(torch.empty_like(x_t), seed, sids, off) if noise_bcs else None
        k_d, t_d = torch.tensor([k], device=d), torch.tensor([untouched], device=d)
        ref = plain(x_t, mo, z, z2, xb, mask, tab_d, k_d, tau_d, t_d, noise_bcs, clip)
        assert int(k_d) == k and int(t_d) == untouched

        off_f = torch.full((1,), off0, dtype=torch.int64, device=d)
        out = fused(x_t, mo, xb, mask, tab_d, k_d, tau_d, t_d, noise_bcs, clip, seed, sids, off_f)
        assert torch.equal(_bits(out), _bits(ref)), k
        assert int(off_f) == int(off) == off0 + (2 if noise_bcs else 1) * (F * V // 4)
        assert int(k_d) == k - 1
        assert int(t_d) == (taus[k - 1] if k > 0 else untouched)
        # in place, as the sampler calls it
        x_in = x_t.clone()
        off_f.fill_(off0); k_d.fill_(k)
        fused(x_in, mo, xb, mask, tab_d, k_d, tau_d, t_d, noise_bcs, clip, seed, sids, off_f, out=x_in)
        assert torch.equal(_bits(x_in), _bits(ref)), k
        if k > 0:
            # another seed reaches the interior wherever the step adds noise there
            off_f.fill_(off0); k_d.fill_(k)
            other = fused(x_t, mo, xb, mask, tab_d, k_d, tau_d, t_d, noise_bcs, clip, seed + 1, sids, off_f)
            same_inside = torch.equal(_bits(other[..., inside]), _bits(out[..., inside]))
            assert same_inside == (which == "ddim" and eta == 0.0), k
            if noise_bcs:
                assert not torch.equal(other[..., ~inside], out[..., ~inside])


# ---------------------------------------------------------------------------------------------------------------------
# 4. DDIM on the eps_hat half never loads w
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("noise_bcs", [True, False])
@pytest.mark.parametrize("shape", [(2, 4, 6, 5, 4), (1, 4, 3, 3, 3)])
def test_ddim_lv_step_is_the_ddim_step_and_never_loads_w(shape, noise_bcs, clip):
    """`ops.ddim_step_lv(x, [eps_hat | NaN])` == `ops.ddim_step(x, eps_hat)` bit for bit and finite, eta in {0, 0.5, 1}, k in
    {0, 1, S - 1}; the `_rng` pair likewise (on the layout it takes), scalars included."""
    from turbdiff_amd import ops

    d = dev()
    F, V = shape[1], shape[2] * shape[3] * shape[4]
    x_t, eps, z, z2, xb = (rnd(*shape, seed=s).to(d) for s in range(5))
    mo = torch.cat([eps, torch.full_like(eps, float("nan"))], dim=1).contiguous()
    mask = ops.cell_mask(_mask_idx(V).to(d), V)
    sids = torch.tensor([(5 << 32) | 7, (9 << 32) | 11][: shape[0]], dtype=torch.int64, device=d)
    for eta in (0.0, 0.5, 1.0):
        tab, taus = _ddim(eta)
        S = len(taus)
        tab_d, tau_d = tab.to(d), torch.tensor(taus, device=d)
        for k in (0, 1, S - 1):
            k_d, t_d = torch.tensor([k], device=d), torch.tensor([taus[k]], device=d)
            zz2 = z2 if noise_bcs else None
            want = ops.ddim_step(x_t, eps, z, zz2, xb, mask, tab_d, k_d, tau_d, t_d, noise_bcs, clip)
            got = ops.ddim_step_lv(x_t, mo, z, zz2, xb, mask, tab_d, k_d, tau_d, t_d, noise_bcs, clip)
            assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want)), (eta, k)
            if ops.p_sample_step_rng_supported(x_t):
                offs = [torch.full((1,), 4096, dtype=torch.int64, device=d) for _ in range(2)]
                ks = [k_d.clone() for _ in range(2)]
                want = ops.ddim_step_rng(x_t, eps, xb, mask, tab_d, ks[0], tau_d, t_d.clone(), noise_bcs, clip, 1234, sids, offs[0])
                got = ops.ddim_step_lv_rng(x_t, mo, xb, mask, tab_d, ks[1], tau_d, t_d.clone(), noise_bcs, clip, 1234, sids, offs[1])
                assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want)), (eta, k)
                assert int(offs[0]) == int(offs[1]) and int(ks[0]) == int(ks[1]) == k - 1


# ---------------------------------------------------------------------------------------------------------------------
# 5. a finished trajectory
def test_new_entries_write_nothing_for_a_finished_trajectory():
    """k outside [0, S) has no column: neither new rule may read one (nor write), through either entry.  The entries that
    draw their noise still advance the offset and the index."""
    from turbdiff_amd import ops

    d = dev()
    shape = (1, 4, 2, 2, 2)
    x, xb = (rnd(*shape, seed=s).to(d) for s in range(2))
    mo = rnd(1, 8, 2, 2, 2, seed=3).to(d)
    mask = torch.ones(8, dtype=torch.uint8, device=d)
    sids, off = torch.tensor([3], dtype=torch.int64, device=d), torch.zeros(1, dtype=torch.int64, device=d)
    for which, eta in (("respaced", None), ("ddim", 1.0)):
        plain, fused, tab, taus = _pair(which, eta)
        tab_d, tau_d, t_d = tab.to(d), torch.tensor(taus, device=d), torch.tensor([0], device=d)
        for k in (-1, len(taus)):
            out = torch.full(shape, 7.0, device=d)
            plain(x, mo, x, x, xb, mask, tab_d, torch.tensor([k], device=d), tau_d, t_d, True, False, out=out)
            assert torch.equal(out, torch.full(shape, 7.0, device=d)), which
            k_d, off0 = torch.tensor([k], device=d), int(off)
            fused(x, mo, xb, mask, tab_d, k_d, tau_d, t_d, True, False, 1, sids, off, out=out)
            assert torch.equal(out, torch.full(shape, 7.0, device=d)) and int(k_d) == k - 1, which
            assert int(off) == off0 + 2 * (4 * 8 // 4), which  # noise_bcs: 2 F V / 4 counters, drawn or not


# ---------------------------------------------------------------------------------------------------------------------
# 6. the exact denoiser of a point mass: the respaced chain lands on it
#
# Construction and bound of tests/test_ddim_gpu.py::test_exact_denoiser_recovers_the_point_mass (atol 2e-6: an error d of x_t
# cancels in x0 = recip x_t - recipm1 eps(x_t) and is damped by coef2 < 1 in the mean, so only the last steps' roundings
# survive).  The ancestral mean has the same property, whatever the variance: w is arbitrary finite.
@pytest.mark.parametrize("name", list(STEP_T))
def test_exact_denoiser_recovers_the_point_mass(name):
    from turbdiff_amd import ops, schedules

    d = dev()
    T = STEP_T[name]
    shape = (2, 4, 6, 5, 4)
    V = shape[2] * shape[3] * shape[4]
    tab, taus = _respaced(name)
    S = len(taus)
    abar = torch.cumprod(1.0 - schedules.betas_for(name, T).double(), dim=0)[taus]
    sa, sb = abar.sqrt().float().to(d), (1.0 - abar).sqrt().float().to(d)
    x_star = rnd(*shape, seed=21).to(d)
    w = (3.0 * rnd(*shape, seed=22)).to(d)
    mask = torch.ones(V, dtype=torch.uint8, device=d)
    sids = torch.tensor([(3 << 32) | 1, (3 << 32) | 2], dtype=torch.int64, device=d)
    off = torch.full((1,), 64, dtype=torch.int64, device=d)
    x = ops.randn_philox_batched(torch.empty_like(x_star), 99, sids, off)
    tab_d, tau_d = tab.to(d), torch.tensor(taus, device=d)
    k_d, t_d = torch.tensor([S - 1], device=d), torch.tensor([taus[-1]], device=d)
    for k in reversed(range(S)):
        assert int(k_d) == k and int(t_d) == taus[k]
        mo = torch.cat([(x - sa[k] * x_star) / sb[k], w], dim=1).contiguous()
        ops.p_sample_step_lv_respaced_rng(x, mo, x_star, mask, tab_d, k_d, tau_d, t_d, False, False, 99, sids, off, out=x)
    err = (x - x_star).abs().max().item()
    print(f"{name} T={T} S={S}: max |x_0 - x*| = {err:.2e}")
    assert err <= 2e-6, err


# ---------------------------------------------------------------------------------------------------------------------
# 7. a model output with F planes
def test_new_entries_check_the_model_output_shape():
    from turbdiff_amd import ops

    d = dev()
    x = torch.zeros(1, 4, 2, 2, 2, device=d)
    mask = torch.ones(8, dtype=torch.uint8, device=d)
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64, device=d)
    sentinel = torch.full_like(x, 7.0)
    for which, eta in (("respaced", None), ("ddim", 0.0)):
        plain, fused, tab, taus = _pair(which, eta)
        tab_d, tau_d = tab.to(d), i64(*taus)
        with pytest.raises(ValueError, match="eps_hat"):
            plain(x, x, x, x, x, mask, tab_d, i64(1), tau_d, i64(taus[1]), True, False, out=sentinel)
        with pytest.raises(ValueError, match="eps_hat"):
            fused(x, x, x, mask, tab_d, i64(1), tau_d, i64(taus[1]), True, False, 1, i64(3), i64(0), out=sentinel)
        mo = torch.zeros(1, 8, 2, 2, 2, device=d)
        with pytest.raises(ValueError, match="do not fit"):  # and the wrong table
            plain(x, mo, x, x, x, mask, tab_d[:5].contiguous(), i64(1), tau_d, i64(taus[1]), True, False, out=sentinel)
    assert torch.equal(sentinel, torch.full_like(x, 7.0))  # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------
# 8. the captured samplers against the eager loops on the golden learned-variance model (T = 10)
@pytest.mark.parametrize("nb", [True, False])
@pytest.mark.parametrize("method,eta", [("respaced", 0.0), ("ddim", 0.0), ("ddim", 1.0)])
def test_captured_sampler_equals_the_eager_loop(golden, method, eta, nb):
    """The captured step (device-side k, tau, t; Philox noise drawn in the kernel) reproduces the eager loop over the plain
    entry fed the very same Philox tensors; rel-L2 1e-5 as for the DDIM and the learned-variance twin of this test (the
    GroupNorm statistics merge per-block partials with f64 atomics, so runs agree to rounding, not bitwise)."""
    from turbdiff_amd import schedules
    from turbdiff_amd.sampling import GraphSampler

    diff = build_golden(golden, "learned_var_noelbo", noise_bcs=nb)
    x_bcs, C, cidx, _ = golden_inputs(golden)
    taus = schedules.ddim_timesteps(10, 4)
    kw = dict(sampling_timesteps=4, eta=eta, sampling_method=method)
    gs = GraphSampler(diff, x_bcs, C, cidx, seed=42, trajectory_ids=[5, 9], **kw)
    assert gs.fused_noise and gs.steps_left == 4 and int(gs.k) == 3 and int(gs.t) == taus[-1] and gs.tau.tolist() == taus
    assert gs.ddim_table.shape == ((8 if method == "respaced" else 6), 4)
    out_graph = gs.sample()
    assert gs.graph is not None and torch.isfinite(out_graph).all()
    assert gs.steps_left == 0 and int(gs.t) == taus[0] and int(gs.k) == -1
    stream = gs.noise_stream()
    out_eager = diff.p_sample_loop(x_bcs, C, cidx, noise_fn=lambda like: next(stream), **kw)
    err = rel_l2(out_graph, out_eager)
    print(f"{method} eta={eta} nb={nb}: captured vs eager rel-L2 {err:.2e}")
    assert err < 1e-5
    assert not diff.graph_samplers()  # noise_fn= took the eager loop
    assert rel_l2(gs.sample(), out_graph) < 1e-5
    # sharding invariance: trajectory 9 alone, eagerly, gives row 1
    solo = GraphSampler(diff, x_bcs[1:], C, cidx, seed=42, trajectory_ids=[9], use_graph=False, **kw)
    assert rel_l2(solo.sample()[0], out_graph[1]) < 1e-5
    # BC cells hold the boundary values exactly
    inside = torch.zeros(out_graph[0, 0].numel(), dtype=torch.bool, device=dev())
    inside[cidx] = True
    assert torch.equal(out_graph.flatten(-3)[..., ~inside], x_bcs.flatten(-3)[..., ~inside])
    assert torch.equal(out_eager.flatten(-3)[..., ~inside], x_bcs.flatten(-3)[..., ~inside])
    # the public route: the same sampler class behind p_sample_loop, cached under a signature that names method and S
    pub = diff.p_sample_loop(x_bcs, C, cidx, seed=42, trajectory_ids=[5, 9], **kw)
    (cached,) = diff.graph_samplers().values()
    assert cached.sampling_method == method and cached.signature()[-2:] == (("learned-variances", method, 4), eta)
    ref = GraphSampler(diff, x_bcs, C, cidx, seed=0, trajectory_ids=[5, 9], nonce=42, use_graph=False, **kw)
    assert rel_l2(pub, ref.sample()) < 1e-5
    # the samplers differ from each other and from the T-step chain
    assert rel_l2(out_graph, GraphSampler(diff, x_bcs, C, cidx, seed=42, trajectory_ids=[5, 9], use_graph=False).sample()) > 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# 9. subsequence, separate draws, rebind, re-capture
@pytest.mark.parametrize("method", ["respaced", "ddim"])
def test_loops_visit_the_subsequence_and_the_graph_is_reused(golden, method, monkeypatch):
    """start_from = 6 with 3 steps runs the model at t = 5, 3, 0 on both routes (recorded at the model's forward), the
    captured route started there agrees with the eager one, and so does the sampler on separate draws + the plain entry.  A
    second public call with another seed re-uses the graph; a weight update re-captures."""
    from turbdiff_amd import sampling
    from turbdiff_amd.sampling import GraphSampler

    diff = build_golden(golden, "learned_var_noelbo", noise_bcs=True)
    x_bcs, C, cidx, _ = golden_inputs(golden)
    kw = dict(sampling_timesteps=3, eta=0.0, sampling_method=method)
    gs = GraphSampler(diff, x_bcs, C, cidx, seed=7, trajectory_ids=[0, 1], use_graph=False, **kw)
    seen = []
    fwd = diff.model.forward
    monkeypatch.setattr(diff.model, "forward", lambda x, t, *a, **k: (seen.append(t.tolist()), fwd(x, t, *a, **k))[1])
    out = gs.sample(start_from=6)  # issued eagerly: the forward is called per step
    assert gs.tau.tolist() == [0, 3, 5] and gs.steps_left == 0 and int(gs.t) == 0 and int(gs.k) == -1
    assert seen == [[5, 5], [3, 3], [0, 0]]
    del seen[:]
    stream = gs.noise_stream()
    eager = diff.p_sample_loop(x_bcs, C, cidx, start_from=6, noise_fn=lambda like: next(stream), **kw)
    monkeypatch.undo()
    assert seen == [[5, 5], [3, 3], [0, 0]]
    assert rel_l2(out, eager) < 1e-5
    captured = GraphSampler(diff, x_bcs, C, cidx, seed=7, trajectory_ids=[0, 1], **kw)
    full = captured.sample()
    assert captured.tau.tolist() == [0, 5, 9] and captured.graph is not None
    graph = captured.graph
    assert rel_l2(captured.sample(start_from=6), out) < 1e-5 and captured.graph is graph  # same graph, tau and table refilled
    assert captured.tau.tolist() == [0, 3, 5]
    assert rel_l2(captured.sample(), full) < 1e-5  # and back
    monkeypatch.setattr(sampling, "FUSED_STEP_NOISE", False)
    plain = GraphSampler(diff, x_bcs, C, cidx, seed=7, trajectory_ids=[0, 1], **kw)
    assert not plain.fused_noise and plain.z is not None and plain.z2 is not None
    assert rel_l2(plain.sample(start_from=6), out) < 1e-5
    assert plain.steps_left == 0 and int(plain.t) == 0 and int(plain.k) == -1
    monkeypatch.undo()
    # the public route: one sampler, its graph re-used by another seed, re-captured after a weight update
    a = diff.p_sample_loop(x_bcs, C, cidx, seed=3, **kw)
    (cached,) = diff.graph_samplers().values()
    graph = cached.graph
    b = diff.p_sample_loop(x_bcs, C, cidx, seed=4, **kw)
    assert cached.graph is graph and len(diff.graph_samplers()) == 1
    assert rel_l2(diff.p_sample_loop(x_bcs, C, cidx, seed=3, **kw), a) < 1e-5
    assert rel_l2(b, a) > 1e-2  # another x_T at the least
    with torch.no_grad():
        next(diff.model.parameters()).mul_(1.0)
    diff.p_sample_loop(x_bcs, C, cidx, seed=3, **kw)
    assert cached.graph is not graph


# ---------------------------------------------------------------------------------------------------------------------
# 10. the trainer
def test_trainer_samples_with_its_sampling_method(golden):
    """DiffusionTrainer.sample: the keyword override and the `sampling_method` attribute reach the same captured sampler; the
    denormalised output keeps the data values outside the domain."""
    from turbdiff_amd.training import DiffusionTrainer

    g = golden("model_cfg1")
    d = dev()
    torch.manual_seed(3)
    task = DiffusionTrainer(**{**DiffusionTrainer.SHIPPED_CONFIG, "dim": 8, "timesteps": 10, "learned_variances": True},
                            u_net_levels=2, max_train_steps=20).to(d)
    sd = dict(g.sub("sd/"))
    sd.update(golden("options").sub("learned_var/sd/"))
    task.model.model.load_state_dict(sd)
    assert task.sampling_method is None and task.model.learned_variances
    X, Y, Z = g["x"].shape[-3:]
    cell_types = torch.randint(0, 6, (X, Y, Z), generator=torch.Generator().manual_seed(11))
    mean, std = torch.tensor([0.3, -0.1, 0.2, 1.0]), torch.tensor([2.0, 1.5, 0.7, 3.0])
    raw = g["x"] * std.view(4, 1, 1, 1) + mean.view(4, 1, 1, 1)
    batch = SimpleNamespace(x=raw.to(d), cell_idx=g["cell_idx"].to(d), cell_types=cell_types.to(d), mean=mean.to(d), std=std.to(d))
    with pytest.raises(ValueError, match="learned_variances"):
        task.sample(batch, sampling_timesteps=4)
    with pytest.raises(ValueError, match="sampling_timesteps"):
        task.sample(batch, sampling_method="respaced")
    assert not task.model.graph_samplers()
    torch.manual_seed(5)
    a = task.sample(batch, sampling_timesteps=4, sampling_method="respaced")
    (gs,) = task.model.graph_samplers().values()
    assert gs.sampling_timesteps == 4 and gs.sampling_method == "respaced" and gs.steps_left == 0
    task.sampling_timesteps, task.sampling_method = 4, "respaced"
    torch.manual_seed(5)
    b = task.sample(batch)
    assert len(task.model.graph_samplers()) == 1 and rel_l2(b, a) < 1e-5
    inside = torch.zeros(X * Y * Z, dtype=torch.bool)
    inside[g["cell_idx"]] = True
    assert rel_l2(a.cpu().flatten(-3)[..., ~inside], raw.flatten(-3)[..., ~inside]) < 1e-5
    torch.manual_seed(5)
    c = task.sample(batch, sampling_method="ddim")
    assert len(task.model.graph_samplers()) == 2 and torch.isfinite(c).all() and rel_l2(c, a) > 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# 11. the defaults on the same model
def test_default_calls_are_what_they_were(golden):
    """`p_sample_loop(x, C, cidx, seed=s)` gives the same sample before any of the new samplers exists and after two of them
    were built and cached next to it; `sampling_timesteps=4` alone still raises."""
    diff = build_golden(golden, "learned_var_noelbo")
    x, C, cidx, _ = golden_inputs(golden)
    before = diff.p_sample_loop(x, C, cidx, seed=3)
    (gs,) = diff.graph_samplers().values()
    assert gs.signature()[-2:] == ("learned-variances", 0.0) and gs.sampling_method is None and gs.k is None
    with pytest.raises(ValueError, match="learned_variances"):
        diff.p_sample_loop(x, C, cidx, sampling_timesteps=4)
    for method in ("respaced", "ddim"):
        assert torch.isfinite(diff.p_sample_loop(x, C, cidx, seed=3, sampling_timesteps=4, sampling_method=method)).all()
    assert len(diff.graph_samplers()) == 3 and gs in diff.graph_samplers().values()
    after = diff.p_sample_loop(x, C, cidx, seed=3)
    assert torch.equal(after, before)
    with pytest.raises(ValueError, match="learned_variances"):
        diff.p_sample_loop(x, C, cidx, sampling_timesteps=4)
    with pytest.raises(ValueError, match="eta"):
        diff.p_sample_loop(x, C, cidx, sampling_timesteps=4, sampling_method="respaced", eta=0.5)
    assert len(diff.graph_samplers()) == 3
