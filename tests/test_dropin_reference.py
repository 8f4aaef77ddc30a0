"""The drop-in claim, checked against what the reference itself recorded (tests/golden/dropin.npz, written by
tests/golden/make_golden_dropin.py, and tests/golden/grid_io.npz, both from the unmodified reference): with turbdiff_amd.dropin installed, the reference's own
DiffusionTraining (diffusion.py:41-143) constructs OUR DenoisingModel / GaussianDiffusion with the recorded arguments, and
its state_dict has the reference schema; our modules carry every name the reference's define and agree with its numbers."""

import ast
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"


def _dropin():
    return np.load(GOLDEN / "dropin.npz")


def _sub(z, prefix):
    return {k[len(prefix):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix)}


def _pattern(shape, scale):
    """make_golden_dropin.pattern(): exact multiples of `scale` from integer arithmetic, rebuilt rather than stored."""
    i = torch.arange(int(np.prod(shape)), dtype=torch.int64).reshape(shape)
    return ((i * 7919) % 251 - 125).float() * scale


def test_reference_task_builds_our_model():
    import turbdiff_amd.dropin as dropin

    z = _dropin()
    calls = json.loads(str(z["task/calls"]))
    installed = dropin.install()
    try:
        D = sys.modules["turbdiff.models.ddpm"]  # what the reference's `from turbdiff.models.ddpm import ...` now finds
        assert D.__name__ == "turbdiff_amd.models.ddpm", D.__name__
        assert all(sys.modules[k] is m for k, m in installed.items())
        mk = dict(calls["DenoisingModel"]["kwargs"], actfn=getattr(torch.nn, calls["DenoisingModel"]["kwargs"]["actfn"]))
        assert calls["DenoisingModel"]["n_positional"] == 0 and calls["GaussianDiffusion"]["n_positional"] == 1
        model = D.DenoisingModel(**mk)
        diff = D.GaussianDiffusion(model, **calls["GaussianDiffusion"]["kwargs"])
    finally:
        dropin.uninstall()
    assert "turbdiff.models.ddpm" not in sys.modules
    # the reference's task held these classes as task.model / task.model.model
    assert [f"{type(m).__module__}.{type(m).__name__}" for m in (diff, model)] == [str(s) for s in z["task/classes"]]
    manifest = [l.rstrip("\n").split("\t") for l in open(GOLDEN / "state_dict_manifest.txt") if not l.startswith("#")]
    want = [k for k, _ in manifest]
    assert [str(k) for k in z["task/state_dict_keys"]] == want and len(want) == 149
    # the task's own part of that schema (task.model = GaussianDiffusion), key for key and shape for shape
    have = {"model." + k: tuple(v.shape) for k, v in diff.state_dict().items()}
    ours = [(k, ast.literal_eval(s)) for k, s in manifest if k.startswith("model.")]
    assert list(have) == [k for k, _ in ours], (len(have), len(ours), set(have) ^ {k for k, _ in ours})
    assert all(have[k] == tuple(s) for k, s in ours)


def test_module_surface_matches_reference():
    """Every class / function the reference's ddpm.py defines exists here, and the torch-only ones
    (LinearAttention, pad_to_multiple_of, unpad, expand_as) agree with it numerically."""
    import turbdiff_amd.models.ddpm as M

    z = _dropin()
    missing = [str(n) for n in z["names/ddpm"] if not hasattr(M, str(n))]
    assert not missing, missing
    t = lambda k: torch.from_numpy(z[f"surface/{k}"])
    b = M.LinearAttention(8, heads=2, dim_head=4)
    b.load_state_dict(_sub(z, "surface/linear_attention/sd/"), strict=True)
    assert torch.allclose(b(t("linear_attention/x")), t("linear_attention/y"), atol=1e-6)
    for i in range(2):
        pb, qb = M.pad_to_multiple_of(t(f"pad/{i}/x"), 2, mode="constant")
        assert tuple(qb) == tuple(int(v) for v in z[f"surface/pad/{i}/padding"])
        assert torch.equal(pb, t(f"pad/{i}/padded")) and torch.equal(M.unpad(pb, qb), t(f"pad/{i}/unpadded"))
    assert torch.equal(M.expand_as(t("expand_as/x"), t("expand_as/y"), 1), t("expand_as/out"))
    # GeometryEmbedding (ddpm.py:375-395; off in the shipped config, kept on stock torch ops)
    gb = M.GeometryEmbedding(4, 8, torch.nn.SiLU)
    sd = gb.state_dict()
    gb.load_state_dict({k: _pattern(sd[k].shape, 2.0**-12) for k in sorted(sd)}, strict=True)
    with torch.no_grad():
        assert torch.allclose(gb(_pattern((4, 55, 46, 47), 2.0**-6)), t("geometry_embedding/out"), atol=1e-6)
    # SinusoidalPosEmb, normal_kl, normal_log_lk
    assert torch.allclose(M.SinusoidalPosEmb(16)(torch.arange(5.0)), t("sinusoidal_pos_emb/out"), atol=1e-6)
    a, b, c, d = (t(f"normal/{k}") for k in "abcd")
    assert torch.allclose(M.normal_kl(a, b, c, d), t("normal/kl"), atol=1e-6)
    assert torch.allclose(M.normal_log_lk(a, b, c), t("normal/log_lk"), atol=1e-6)


def test_reference_batch_objects_flow_through_gridio():
    import turbdiff_amd.data.ofles as MO
    import turbdiff_amd.models.cell_type_embeddings as MC
    import turbdiff_amd.models.conditioning as MCo
    import turbdiff_amd.models.normalization as MN
    from grid_cases import load_case
    from test_gridio import emulate_embed
    from turbdiff_amd import gridio

    z = _dropin()
    # 1. public names of the reference modules exist here (classes / functions defined in those modules)
    for key, M in (("normalization", MN), ("cell_type_embeddings", MC), ("conditioning", MCo)):
        missing = [str(n) for n in z[f"names/{key}"] if not hasattr(M, str(n))]
        assert not missing, (key, missing)
    for n in ("Variable", "BoundaryCondition", "split_channels", "OpenFOAMMetadata", "OpenFOAMData", "OpenFOAMStats", "OpenFOAMBatch"):
        assert hasattr(MO, n), n
    assert [v.name for v in MO.Variable] == [str(n) for n in z["names/variable/name"]]
    assert [v.dims for v in MO.Variable] == [int(n) for n in z["names/variable/dims"]]
    assert [v.value for v in MO.Variable] == [v.item() for v in z["names/variable/value"]]

    # 2. batch objects built as the reference's were go through the plan (attribute names only) to the reference's numbers
    BC = MO.BoundaryCondition
    for tag in "AB":
        c = load_case(tag)
        vs = tuple(MO.Variable.from_str(n) for n, _ in c.variables)
        bcs = {v: {b: BC(BC.Type.FIXED_VALUE, torch.tensor(val)) for b, val in c.fixed.get(n, {}).items()}
               for (n, _), v in zip(c.variables, vs)}
        meta = MO.OpenFOAMMetadata(file=Path("x") / "data.h5", nu=0.0, h=np.ones(3), cell_counts=np.array(c.cell_counts),
                                   cell_idx=torch.tensor(c.cell_idx), boundaries={k: {"type": "patch", "idx": torch.tensor(i)}
                                                                                  for k, i in c.boundaries.items()},
                                   boundary_conditions=bcs, holes=[])
        data = MO.OpenFOAMData(meta, torch.zeros(1), {v: torch.tensor(c.samples[n]) for (n, _), v in zip(c.variables, vs)})
        ref = c.grid_embedding  # the reference's OpenFOAMData.grid_embedding of this case (make_golden_grid.py)
        plan = gridio.plan_for(data.metadata)
        ours = emulate_embed(plan, plan.features(vs), [c.samples[n] for n, _ in c.variables])
        assert np.array_equal(ours, ref)
        assert np.array_equal(c.cell_types, plan.types.numpy().reshape(plan.counts))
        # the reference's normalisation of that grid, against OUR Normalization and stats object
        mine = MO.OpenFOAMStats({k: {n: torch.tensor(a) for n, a in st.items()} for k, st in c.stats.items()})
        assert c.modes
        for mode, r in c.modes.items():
            b = MN.Normalization(vs, mode).normalize_grid(torch.tensor(ref), mine)
            m2, s2 = mine.normalizers(vs, mode)
            assert torch.equal(torch.from_numpy(r.normalized), b), mode
            assert torch.equal(torch.from_numpy(r.mean), m2) and torch.equal(torch.from_numpy(r.std), s2), mode
