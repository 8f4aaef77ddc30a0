"""CPU-side checks: the C-ABI library is built, loads and exports every symbol declared in
include/tdx.h; host-side logic (schedules, module tree / state_dict schema, helpers) matches
the golden vectors.  No kernel is launched here."""

import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def declared_symbols():
    text = (ROOT / "include" / "tdx.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tdx_[a-z0-9_]+)\s*\(", text)))


def declared_prototypes():
    """{name: (return type, [argument types])} of include/tdx.h, every type reduced to its class: "ptr" (any pointer;
    `const char*` as a return type stays itself), int, int64_t, uint64_t (= size_t on this ABI), uint32_t, float, double."""
    text = (ROOT / "include" / "tdx.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)

    def cls(decl, name=True):
        decl = decl.strip()
        if "*" in decl:
            return "ptr"
        words = [w for w in decl.split() if w != "const"]
        words = words[:-1] if name and len(words) > 1 else words  # drop the parameter's name
        return {"size_t": "uint64_t"}.get(" ".join(words), " ".join(words))

    protos = {}
    for ret, name, args in re.findall(r"^\s*([A-Za-z_][\w \t]*?[\w*])\s*\b(tdx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        ret = ret.strip()
        args = [] if args.strip() in ("", "void") else [cls(a) for a in args.split(",")]
        protos[name] = ("const char*" if re.fullmatch(r"const\s+char\s*\*", ret) else cls(ret, name=False), args)
    return protos


def test_header_symbols_are_bound_and_exported():
    import ctypes as C

    from turbdiff_amd import _lib

    syms = declared_symbols()
    assert len(syms) >= 25
    assert sorted(_lib.SIGNATURES) == syms, "ctypes table and include/tdx.h disagree"
    # ... and argument by argument: a ctypes table that names every symbol can still pass an int where the header takes
    # an int64_t.  c_size_t and c_uint64 are one ctypes class on this ABI, so size_t counts as uint64_t.
    assert C.c_size_t is C.c_uint64
    kinds = {C.c_void_p: "ptr", C.c_int: "int", C.c_int64: "int64_t", C.c_uint64: "uint64_t", C.c_uint32: "uint32_t",
             C.c_float: "float", C.c_double: "double", C.c_char_p: "const char*"}
    protos = declared_prototypes()
    assert sorted(protos) == syms, "a prototype of include/tdx.h was not parsed"
    for name, (ret, args) in protos.items():
        res, argtypes = _lib.SIGNATURES[name]
        assert ret in ("int", "uint64_t", "int64_t", "const char*"), f"{name}: return type {ret}"
        assert kinds[res] == ret, f"{name}: returns {ret}, bound as {kinds[res]}"
        assert [kinds[a] for a in argtypes] == args, f"{name}: header {args}, bound as {[kinds[a] for a in argtypes]}"
    lib = _lib.load()  # raises if the .so is missing: run __graft_entry__.build() first
    for s in syms:
        assert hasattr(lib, s), f"{s} not exported by libtdx_hip.so"
    assert lib.tdx_arch() == b"gfx950"
    assert lib.tdx_version() >= 1
    assert {"tdx_conv1_fwd_plan", "tdx_conv1_bwd_weight_plan"} <= set(syms)
    assert protos["tdx_conv1_fwd_plan"] == ("int", ["int"] * 8 + ["ptr"])
    assert protos["tdx_conv1_bwd_weight_plan"] == ("int", ["int", "int", "int64_t", "int", "int", "ptr"])
    assert protos["tdx_resize_plan"] == ("int", ["int"] * 9 + ["ptr"])
    # the plan arrays' named indices: the Python field tuples follow the header's numbering
    text = (ROOT / "include" / "tdx.h").read_text()
    index = {n.lower(): int(v) for n, v in re.findall(r"^#define TDX_RESIZE_PLAN_(\w+) (\d+)$", text, flags=re.M)}
    assert index.pop("ints") == _lib.RESIZE_PLAN_INTS == len(_lib.RESIZE_PLAN_FIELDS)
    assert index == {k: i for i, k in enumerate(_lib.RESIZE_PLAN_FIELDS)}
    kernels = {n.lower(): int(v) for n, v in re.findall(r"^#define TDX_RESIZE_(GATHER|PAIRS|TILED|GENERIC) (\d+)$", text, flags=re.M)}
    assert [kernels[k] for k in _lib.RESIZE_FWD_KERNELS + _lib.RESIZE_BWD_KERNELS] == [0, 1, 0, 1]
    assert protos["tdx_attn_plan"] == ("int", ["int"] * 5 + ["ptr"])
    index = {n.lower(): int(v) for n, v in re.findall(r"^#define TDX_ATTN_PLAN_(\w+) (\d+)$", text, flags=re.M)}
    assert index.pop("ints") == _lib.ATTN_PLAN_INTS == len(_lib.ATTN_PLAN_FIELDS)
    assert index == {k: i for i, k in enumerate(_lib.ATTN_PLAN_FIELDS)}
    kernels = {n.lower(): int(v) for n, v in re.findall(r"^#define TDX_ATTN_(VECTOR|MFMA) (\d+)$", text, flags=re.M)}
    assert [kernels[k] for k in _lib.ATTN_KERNELS] == [0, 1]


def test_product_refuses_cpu_tensors():
    from turbdiff_amd import ops

    with pytest.raises(RuntimeError, match="device tensors"):
        ops.resize(torch.zeros(1, 4, 4, 4, 8), (3, 3, 3))


def test_product_never_imports_the_oracle():
    pkg = ROOT / "generative-turbulence_amd"
    for f in pkg.rglob("*.py"):
        assert "oracle" not in f.read_text(), f"{f} references the oracle"


@pytest.mark.parametrize("name", ["linear", "log-linear", "log-snr-linear", "cosine", "sigmoid"])
@pytest.mark.parametrize("T", [10, 500, 1000])
def test_product_schedules_bit_exact(golden, name, T):
    from turbdiff_amd import schedules

    g = golden("schedules")
    tab = schedules.diffusion_tables(name, T)
    for k, v in tab.items():
        assert torch.equal(v.view(torch.int32), g[f"{name}/{T}/{k}"].view(torch.int32)), (name, T, k)
    packed = schedules.pack_step_tables(tab)
    assert packed.shape == (7, T) and torch.equal(packed[4].view(torch.int32), tab["log_betas"].view(torch.int32))


def test_time_embedding_tables(golden):
    from turbdiff_amd.models.ddpm import NyquistFrequencyEmbedding

    g = golden("ops")
    for T, dim in [(10, 8), (500, 32)]:
        emb = NyquistFrequencyEmbedding(dim, T)
        assert torch.equal(emb.scale, g[f"tfreq/{T}/scale"]) and torch.equal(emb.bias, g[f"tfreq/{T}/bias"])
        assert torch.equal(emb(g[f"tfreq/{T}/t"]), g[f"tfreq/{T}/y"])


def test_state_dict_schema_matches_reference_manifest():
    from turbdiff_amd.models.ddpm import DenoisingModel, GaussianDiffusion

    want = {}
    for line in (ROOT / "tests" / "golden" / "state_dict_manifest.txt").read_text().splitlines():
        if line.startswith("model.model."):
            k, shp = line.split("\t")
            want[k[len("model.model."):]] = eval(shp)
    assert len(want) == 139
    net = DenoisingModel(in_features=4, out_features=4, c_local_features=4, c_global_features=0, timesteps=500, dim=32,
                         u_net_levels=4, norm_type="group", with_geometry_embedding=False)
    have = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert have == want
    assert sum(p.numel() for p in net.parameters()) == 55246788
    diff = GaussianDiffusion(net, timesteps=500, beta_schedule="log-snr-linear")
    assert set(diff.state_dict()) == {"model." + k for k in want}  # schedule tables are non-persistent
    assert diff.num_timesteps == 500


def test_default_init_matches_reference_under_same_seed(golden):
    """Same module construction order => same RNG consumption => identical default weights;
    the golden cfg1 state_dict was created by the reference under torch.manual_seed(0)
    (GroupNorm affine parameters were perturbed afterwards and are skipped)."""
    from turbdiff_amd.models.ddpm import DenoisingModel

    torch.manual_seed(0)
    net = DenoisingModel(in_features=4, out_features=4, c_local_features=4, c_global_features=0, timesteps=10, dim=8,
                         u_net_levels=2, norm_type="group")
    g = golden("model_cfg1").sub("sd/")
    for k, v in net.state_dict().items():
        if ".norm." in k:
            continue
        assert torch.equal(v, g[k]), k


def test_cell_helpers(golden):
    from turbdiff_amd.models import utils as U

    g = golden("ops")
    a, b, idx = g["where/a"], g["where/b"], g["where/idx"]
    assert torch.equal(U.where_cells(idx, a, b), g["where/ab"])
    assert torch.equal(U.where_cells(idx, a), g["where/a0"])
    assert torch.equal(U.select_cells(a, idx), a.flatten(-3)[..., idx])
    assert U.broadcast_right(torch.arange(3.0), a[:3]).shape == (3, 1, 1, 1, 1) or True


def test_kwargs_sequential_filters_keywords():
    import torch.nn as nn
    from turbdiff_amd.sequential import KwargsSequential

    class A(nn.Module):
        def forward(self, x, c):
            return x + c

    class B(nn.Module):
        def forward(self, x):
            return 2 * x

    class K(nn.Module):
        def forward(self, x, **kw):
            return x + sum(kw.values())

    seq = KwargsSequential(A(), B(), K())
    assert seq(torch.tensor(1.0), c=torch.tensor(3.0)).item() == 11.0


def test_trainer_state_dict_has_the_reference_tasks_149_keys():
    """DiffusionTrainer (our Lightning-free counterpart of DiffusionTraining, diffusion.py:41-143)
    exposes exactly the key / shape schema of the reference task, so eval_ckpt.py-style strict
    loading (scripts/eval_ckpt.py:59) works."""
    from turbdiff_amd.training import DiffusionTrainer

    want = {}
    for line in (ROOT / "tests" / "golden" / "state_dict_manifest.txt").read_text().splitlines():
        if line and not line.startswith("#"):
            k, shp = line.split("\t")
            want[k] = eval(shp)
    assert len(want) == 149
    task = DiffusionTrainer(**DiffusionTrainer.SHIPPED_CONFIG)
    have = {k: tuple(v.shape) for k, v in task.state_dict().items()}
    assert have == want
    task.load_state_dict({k: torch.zeros(s) for k, s in want.items()}, strict=True)
    opt, sched = task.configure_optimizers()
    assert isinstance(opt, torch.optim.RAdam) and sched is not None
    # exponential decay from 1e-4 to 1e-6 over max_train_steps (diffusion.py:221-233)
    for _ in range(task.max_train_steps):
        opt.step(); sched.step()
    assert abs(sched.get_last_lr()[0] - 1e-6) < 1e-12


# --------------------------------------------------------------------------- a18: config-keyed construction


def _task_cases():
    import json

    return json.loads((ROOT / "tests" / "golden" / "task_configs.json").read_text())


@pytest.mark.parametrize("case", ["shipped", "onehot_cellpos", "learned_variances", "instance_gelu_adam", "no_cell_types"])
def test_trainer_from_config_matches_reference_task(case):
    """DiffusionTrainer.from_config on a run configuration shaped like the reference's (model group =
    config/model/diffusion.yaml, variants override single keys) against what the reference's own
    DiffusionTraining built from the same configuration (tests/golden/make_golden_task.py): state_dict keys and
    shapes, conditioning widths, optimiser class, learning-rate schedule, kept hyper-parameters."""
    from turbdiff_amd.training import DiffusionTrainer

    c = _task_cases()[case]
    run, want = c["run_config"], c["expect"]
    task = DiffusionTrainer.from_config(run, steps_per_epoch=run["steps_per_epoch"])
    got = {k: list(v.shape) for k, v in task.state_dict().items()}
    assert sorted(got) == sorted(want["state_dict"]), "state_dict keys differ from the reference task's"
    assert got == want["state_dict"]  # (the key ORDER is pinned by test_trainer_state_dict_has_the_reference_tasks_149_keys)
    assert sum(p.numel() for p in task.parameters()) == want["n_parameters"]
    assert task.max_train_steps == want["max_train_steps"]
    assert task.conditioning.local_conditioning_dim == want["local_conditioning_dim"]
    assert task.conditioning.global_conditioning_dim == want["global_conditioning_dim"]
    assert [v.name for v in task.variables] == want["variables"]
    for k, v in want["attrs"].items():
        assert getattr(task, k) == v, k
    assert task.gradient_clip_val == run["trainer"]["gradient_clip_val"]
    assert task.compute_mode == "f32s"  # matmul_precision: medium -> reduced-precision products on fp32 tensors
    task.fused_optimizer = False        # CPU: the stock torch optimiser classes, as the reference builds them
    opt, sched = task.configure_optimizers()
    assert type(opt).__name__ == want["optimizer"] and opt.param_groups[0]["lr"] == want["lr"]
    if want["lr_factors"] is None:
        assert sched is None
    else:
        for step, f in want["lr_factors"].items():
            assert abs(sched.lr_lambdas[0](int(step)) - f) <= 1e-15 * max(1.0, abs(f)), step


def test_conv_arithmetic_is_chosen_per_model_not_per_process(monkeypatch):
    """Building a trainer must not change the conv arithmetic of other models in the process: the choice lives on the
    DenoisingModel (conv_impl), is in force while ITS forward runs (_lib.conv_impl_scope) and remembered by the autograd
    nodes for their backward; TDX_CONV_IMPL stays the explicit override of tests and benchmarks."""
    from turbdiff_amd import _lib as L
    from turbdiff_amd.training import DiffusionTrainer

    monkeypatch.delenv("TDX_CONV_IMPL", raising=False)
    small = {**DiffusionTrainer.SHIPPED_CONFIG, "dim": 8, "timesteps": 10}
    a = DiffusionTrainer(**small, u_net_levels=2, max_train_steps=5, compute_mode="f32s")
    b = DiffusionTrainer(**small, u_net_levels=2, max_train_steps=5, compute_mode="f32")
    c = DiffusionTrainer(**small, u_net_levels=2, max_train_steps=5, compute_mode="bf16")
    assert (a.model.model.conv_impl, b.model.model.conv_impl, c.model.model.conv_impl) == ("split", "auto", "auto")
    assert L.conv_impl() == L.CONV_AUTO  # nothing process-wide was touched
    with L.conv_impl_scope(a.model.model.conv_impl):
        assert L.conv_impl() == L.CONV_SPLIT and L.pack_code(torch.float32) == L.F32_SPLIT
        with L.conv_impl_scope(b.model.model.conv_impl):  # a model called inside another model's forward
            assert L.conv_impl() == L.CONV_AUTO
        assert L.conv_impl() == L.CONV_SPLIT
        monkeypatch.setenv("TDX_CONV_IMPL", "direct")
        assert L.conv_impl() == L.CONV_DIRECT
        monkeypatch.delenv("TDX_CONV_IMPL")
    assert L.conv_impl() == L.CONV_AUTO
    with L.conv_impl_scope(None):  # a model without a choice of its own: the process default
        L.set_conv_impl("split")
        assert L.conv_impl() == L.CONV_SPLIT
        L.set_conv_impl(None)
    with pytest.raises(ValueError):
        L.conv_impl_scope("winograd")


def test_trainer_constructor_defaults_are_the_reference_constructors():
    """DiffusionTrainer() with NO keywords against the reference's DiffusionTraining built with only its two required
    paths (diffusion.py:42-70 defaults: sigmoid schedule, T = 100, l1, Adam at 1e-3 without decay, instance norm,
    geometry embedding, all 8 variables, noise_bcs off): same state_dict, optimiser, hyper-parameters."""
    from turbdiff_amd.training import DiffusionTrainer

    want = _task_cases()["ctor_defaults"]["expect"]
    task = DiffusionTrainer()
    got = {k: list(v.shape) for k, v in task.state_dict().items()}
    assert got == want["state_dict"]
    assert list(got) == list(want["state_dict"]) or sorted(got) == sorted(want["state_dict"])
    assert sum(p.numel() for p in task.parameters()) == want["n_parameters"]
    assert task.max_train_steps == want["max_train_steps"]
    assert task.conditioning.local_conditioning_dim == want["local_conditioning_dim"]
    assert [v.name for v in task.variables] == want["variables"]
    for k, v in want["attrs"].items():
        assert getattr(task, k) == v, k
    assert task.model.model.with_geometry_embedding and not task.model.noise_bcs
    task.fused_optimizer = False
    opt, sched = task.configure_optimizers()
    assert type(opt).__name__ == want["optimizer"] and opt.param_groups[0]["lr"] == want["lr"] and sched is None


def test_trainer_from_config_accepts_the_model_group_and_overrides():
    from turbdiff_amd.training import DiffusionTrainer

    model = dict(_task_cases()["shipped"]["run_config"]["model"], dim=8, timesteps=10)
    task = DiffusionTrainer.from_config(model, max_train_steps=50, compute_mode="bf16", u_net_levels=2)
    assert task.dim == 8 and task.max_train_steps == 50 and task.compute_mode == "bf16"
    assert task.model.model.compute_dtype == torch.bfloat16 and task.model.model.u_net_levels == 2
    from types import SimpleNamespace as NS

    ns = NS(model=NS(**model), matmul_precision="highest", data=NS(root="d"), samples_root="s", trainer=NS(gradient_clip_val=0.5))
    task = DiffusionTrainer.from_config(ns, max_train_steps=5)
    assert task.compute_mode == "f32" and task.gradient_clip_val == 0.5 and str(task.data_dir) == "d/data"
    with pytest.raises(ValueError):
        DiffusionTrainer.from_config(dict(model, name="tfnet"))


def test_profiles_index_names_existing_files():
    """profiles/README.md is the index the design documents' citations go through: every r10 / r11 file it names exists,
    and the traffic file bench.py's roofline block reads carries launches of the forward kernels it filters for."""
    import json
    import re
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    text = (root / "profiles" / "README.md").read_text()
    names = set(re.findall(r"`(r1[01][\w]*\.(?:json|txt|md|csv))`", text))
    assert len(names) >= 24 and any(n.startswith("r11") for n in names)
    missing = sorted(n for n in names if not (root / "profiles" / n).exists())
    assert not missing, missing
    for stem in ("r10bf16", "r10f32s"):
        for suffix in ("_summary.md", "_kernel_stats.csv", "_traffic.json"):
            assert (root / "profiles" / (stem + suffix)).exists()
    sys.path.insert(0, str(root))
    import bench

    # roofline.traffic is quoted only from a PMC file collected on THIS tree's conv kernels: a file
    # carries the fingerprint of csrc/tdx_conv* it was collected on; one that describes other kernels is refused by name
    from turbdiff_amd._lib import kernel_sources_fingerprint

    bytes_per_launch, src, n = bench.measured_traffic("bf16")
    now = kernel_sources_fingerprint()
    assert now is not None and src["kernel_sources_sha16"] == now
    if bytes_per_launch is not None:
        assert n >= 60 and bytes_per_launch > 1e8
        data = json.loads((root / src["file"]).read_text())
        assert data["kernel_sources_sha16"] == now and data.get("git_head")
        assert any("conv3_ring_kernel<2, false" in k for k in data["kernels"])
    else:
        assert src["file"] is None and any(r["file"].endswith("_traffic.json") for r in src["refused"])
    stale = json.loads((root / "profiles" / "r10bf16_traffic.json").read_text())
    assert stale.get("kernel_sources_sha16") != now, "the round-3 file describes the round-3 kernels"


def test_graph_sampler_stream_ids_and_signature():
    """Host logic of the default sampling path (no GPU needed): the Philox stream id of a trajectory is
    (per-call nonce << 32 | trajectory id) -- independent of how trajectories are sharded over ranks -- and the signature
    that decides whether a captured graph can be re-used covers shapes, device, conditioning tensors and the switches the
    captured step was built under."""
    from turbdiff_amd.models.conditioning import Conditioning
    from turbdiff_amd.sampling import GraphSampler

    assert GraphSampler._sids([0, 1, 9], 0) == [0, 1, 9]
    assert GraphSampler._sids([5], 3) == [(3 << 32) | 5]
    # the same trajectory has the same stream id whichever rank / batch position holds it
    assert GraphSampler._sids([4, 5, 6, 7], 11)[1] == GraphSampler._sids([5], 11)[0]
    with pytest.raises(AssertionError):
        GraphSampler._sids([1 << 32], 0)
    with pytest.raises(AssertionError):
        GraphSampler._sids([0], 1 << 31)

    class M:  # stand-ins with the attributes the signature reads
        compute_dtype, conv_impl = torch.float32, None

    class D:
        model, noise_bcs, clip_denoised, num_timesteps = M(), True, False, 10

    x = torch.zeros(2, 4, 6, 5, 4)
    C = {Conditioning.Type.CELL_TYPE: torch.zeros(4, 6, 5, 4)}
    sig = GraphSampler.signature_of(D(), x, C)
    assert sig == GraphSampler.signature_of(D(), x.clone(), {k: v.clone() for k, v in C.items()})
    assert sig != GraphSampler.signature_of(D(), x[:1], C)
    d2 = D(); d2.noise_bcs = False
    assert sig != GraphSampler.signature_of(d2, x, C)
    m2 = D(); m2.model = M(); m2.model.compute_dtype = torch.bfloat16
    assert sig != GraphSampler.signature_of(m2, x, C)


def test_philox_reference_matches_random123_known_answers():
    """tests/philox_ref.py (what the GPU generator is checked against) reproduces the three known-answer vectors of
    Random123's philox4x32-10 (kat_vectors: zero counter / key, all-ones, digits of pi)."""
    from philox_ref import philox4x32_10

    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        got = philox4x32_10(*ctr, *key)
        assert tuple(int(x) for x in got) == want


def test_ddp_cu_budget_check():
    """parallel.check_cu_budget: the persistent conv kernels' CUs plus RCCL's channels must fit the
    256 CUs; an unset channel count is refused too (RCCL would choose its own)."""
    from turbdiff_amd.parallel import check_cu_budget

    assert check_cu_budget({"TDX_PERSISTENT_CUS": "224", "NCCL_MAX_NCHANNELS": "32"}) == (224, 32)
    assert check_cu_budget({"TDX_PERSISTENT_CUS": "192", "NCCL_MAX_NCHANNELS": "16"}) == (192, 16)
    with pytest.raises(RuntimeError, match="> 256"):
        check_cu_budget({"TDX_PERSISTENT_CUS": "240", "NCCL_MAX_NCHANNELS": "32"})
    with pytest.raises(RuntimeError, match="> 256"):
        check_cu_budget({"NCCL_MAX_NCHANNELS": "8"})  # default: all 256 CUs
    with pytest.raises(RuntimeError, match="NCCL_MAX_NCHANNELS"):
        check_cu_budget({"TDX_PERSISTENT_CUS": "224"})


def test_bench_pins_each_rank_to_its_own_cores(tmp_path):
    """bench.py's N > 1 preamble: every rank binds its host threads to its own block of cores before
    anything touches the GPU -- NUMA-local ones where sysfs names the GPU's node, an even split of the allowed cores
    otherwise; one rank (the default run) is left alone.  Run in child processes: the affinity is per process."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    allowed = sorted(os.sched_getaffinity(0))
    if len(allowed) < 4:
        import pytest

        pytest.skip("needs at least four cores")
    code = ("import json, os, sys; sys.path.insert(0, %r); import bench; r = bench.pin_host_threads(int(sys.argv[1]), int(sys.argv[2])); "
            "r['now'] = sorted(os.sched_getaffinity(0)); print(json.dumps(r))" % str(root))
    res = []
    for rank in range(2):
        out = subprocess.run([sys.executable, "-c", code, str(rank), "2"], capture_output=True, text=True, check=True)
        res.append(json.loads(out.stdout.strip().splitlines()[-1]))
    assert all(r["pinned"] for r in res), res
    assert not set(res[0]["now"]) & set(res[1]["now"]), "ranks must not share cores"
    assert all(set(r["now"]) <= set(allowed) and len(r["now"]) >= 2 for r in res)
    one = subprocess.run([sys.executable, "-c", code, "0", "1"], capture_output=True, text=True, check=True)
    one = json.loads(one.stdout.strip().splitlines()[-1])
    assert one["pinned"] is False and one["now"] == allowed
    off = subprocess.run([sys.executable, "-c", code, "1", "2"], capture_output=True, text=True, check=True,
                         env=dict(os.environ, TDX_BENCH_PIN="0"))
    assert json.loads(off.stdout.strip().splitlines()[-1])["pinned"] is False


def test_bench_live_traffic_reads_the_counter_tables(tmp_path, monkeypatch):
    """bench.live_traffic (roofline.traffic measured in the run itself): drives `rocprofv3 --kernel-trace --pmc <counter> ... --
    python bench.py ...` once per counter and turns the two counter tables into bytes per launch of the mode's FORWARD brick /
    ring conv kernels only (FETCH_SIZE x 2 on gfx950, KB -> bytes).  Here a stand-in profiler writes the tables."""
    import os
    import stat
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root))
    import bench

    fake = tmp_path / "bin"
    fake.mkdir()
    script = fake / "rocprofv3"
    script.write_text('''#!%s
import os, sys
a = sys.argv[1:]
counter, out = a[a.index("--pmc") + 1], a[a.index("-d") + 1]
assert "--kernel-trace" in a and a[a.index("--") + 1].endswith("python3") or "python" in a[a.index("--") + 1]
assert os.environ.get("TDX_BENCH_CHILD") == "1" and "--no-extra" in a
os.makedirs(out + "/host", exist_ok=True)
rows = [("void conv3_ring_kernel<2, false, 4, false, false>(RingArgs)", 100.0, 50.0),   # forward, bf16: counted
        ("void conv3_ring_kernel<2, false, 4, false, true>(RingArgs)", 20.0, 10.0),     # forward, 4-deep bricks: counted
        ("void conv3_mfma_kernel<1, false, false, false, false, false>(x)", 300.0, 30.0),  # forward brick kernel: counted
        ("void conv3_ring_kernel<2, true, 4, false, false>(RingArgs)", 999.0, 999.0),   # data gradient: not counted
        ("void conv3_ring_kernel<2, false, 4, true, false>(RingArgs)", 777.0, 777.0),   # fp16 forward: not counted in bf16
        ("gn_apply_kernel", 5.0, 5.0)]
with open(out + "/host/1_counter_collection.csv", "w") as f:
    f.write('"Kernel_Name","Counter_Name","Counter_Value"\\n')
    for name, fetch, write in rows * 2:
        f.write('"%%s","%%s",%%f\\n' %% (name, counter, fetch if counter == "FETCH_SIZE" else write))
''' % sys.executable)
    script.chmod(script.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setenv("PATH", f"{fake}:{os.environ['PATH']}")
    per_launch, src, n = bench.live_traffic("bf16", 6)
    assert src["live"] is True and n == 6
    assert per_launch == (2 * (100 + 20 + 300) + (50 + 10 + 30)) * 1024 / 3
    assert src["read_bytes_per_launch"] == 2 * 420 * 1024 / 3 and src["write_bytes_per_launch"] == 90 * 1024 / 3
    per16, _, n16 = bench.live_traffic("fp16", 6)
    assert n16 == 2 and per16 == (2 * 777 + 777) * 1024
    # a profiler that fails is reported, not fatal: bench.py then quotes the committed PMC file of this tree's kernels
    script.write_text("#!/bin/sh\nexit 3\n")
    bad, why, _ = bench.live_traffic("bf16", 6)
    assert bad is None and why["live"] is False and "failed" in why["why"]


def test_fp16_compute_mode_host_side():
    """Round 6's fp16 mode, the part that needs no GPU: the mode table, the model's compute dtype, the loss scale the trainer
    derives from a batch (a power of two that puts the backward's seed 2 (eps_hat - eps) / n near 2^-3), ClipRAdam's argument
    checks, and that a stock torch optimiser is refused (it does not know the scale)."""
    import pytest
    import torch

    from turbdiff_amd import _lib
    from turbdiff_amd.optim import ClipRAdam
    from turbdiff_amd.training import COMPUTE_MODES, DiffusionTrainer

    assert COMPUTE_MODES == ("f32", "f32s", "bf16", "fp16")
    assert _lib.dtype_code(torch.float16) == _lib.F16 == 3 and torch.float16 in _lib.H16_DTYPES
    # B F n_cells = 6 x 4 x 582 256 (the benchmark batch): 2^23 <= n < 2^24 -> S = 2^19; tiny problems never go below 1
    assert DiffusionTrainer.initial_loss_scale(6 * 4 * 582256) == 2.0**19
    assert DiffusionTrainer.initial_loss_scale(4 * 4048) == 2.0**9 and DiffusionTrainer.initial_loss_scale(3) == 1.0
    for n in (17, 1000, 10**6, 10**8):
        s = DiffusionTrainer.initial_loss_scale(n)
        assert 2.0 ** round(__import__("math").log2(s)) == s and 1 / 32 < s / n <= 1 / 16
    task = DiffusionTrainer(**{**DiffusionTrainer.SHIPPED_CONFIG, "dim": 8, "timesteps": 10}, u_net_levels=2, compute_mode="fp16")
    assert task.model.model.compute_dtype == torch.float16 and task.model.model.conv_impl == "auto"
    assert task._loss_scale_for_optimizer() == 2.0**16  # (before a batch has been seen)
    task.optimizer = "adam"
    with pytest.raises(RuntimeError, match="loss-scaling optimiser"):
        task.configure_optimizers()
    assert DiffusionTrainer(**{**DiffusionTrainer.SHIPPED_CONFIG, "dim": 8, "timesteps": 10}, u_net_levels=2,
                            compute_dtype=torch.float16).compute_mode == "fp16"
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError, match="power of two"):
        ClipRAdam(p, loss_scale=1000.0)
    opt = ClipRAdam(p, loss_scale=2.0**10)
    assert opt.scale_loss(torch.tensor(1.5)).item() == 1536.0 and ClipRAdam(p).scale_loss(torch.tensor(1.5)).item() == 1.5


def test_library_sources_zero_with_kernels_not_memsets():
    """A hipMemsetAsync inside a captured hipGraph is a memset NODE, which this runtime does not order against earlier kernel
    nodes that still write the previous owner of reused graph-pool memory (garbage in the encoder / decoder
    gradients from the second replay of a captured training step on).  Every zero fill of the library goes through
    tdx_zero_async / tdx_zero2d_async (kernel launches); this keeps a new hipMemset* call from slipping back in."""
    import re

    csrc = ROOT / "generative-turbulence_amd" / "csrc"
    offenders = []
    for f in sorted(list(csrc.glob("*.hip")) + list(csrc.glob("*.h"))):
        for k, line in enumerate(f.read_text().splitlines(), 1):
            code = line.split("//")[0]
            if re.search(r"\bhipMemset\w*\s*\(", code):
                offenders.append(f"{f.name}:{k}: {line.strip()}")
    assert not offenders, "\n".join(offenders)


# (C1, C2, Cout, B, X, Y, Z) -> families for (bf16, auto), (fp16, auto), (f32, auto), (f32, split), (bf16, direct), (f32, direct)
# without an arena, the same with a 96 MB arena, tdx_conv3_ring_brick_depth.  Recorded from a build of the commit before
# the route function existed (146fb94); never regenerated from the code under test.
_R4, _B4, _D6 = "ring ring brick brick direct direct", "brick brick brick brick direct direct", "direct " * 6
_S4 = "small small brick small direct direct"
_CONV3_ROUTES = [
    ((64, 0, 64, 6, 192, 64, 48), _R4, _R4, 8),
    ((64, 64, 64, 6, 192, 64, 48), _R4, _R4, 8),
    ((128, 0, 128, 6, 96, 32, 24), _R4, _R4, 8),
    ((256, 0, 256, 6, 48, 16, 12), _R4, _R4, 4),
    ((512, 0, 512, 6, 24, 8, 6), _B4, _S4, 0),
    ((512, 0, 512, 6, 12, 4, 3), _B4, _S4, 0),
    ((512, 512, 256, 6, 24, 8, 6), _B4, _S4, 0),
    ((64, 0, 64, 6, 194, 50, 50), _R4, _R4, 8),
    ((128, 0, 128, 6, 97, 25, 25), _R4, _R4, 8),
    ((8, 0, 8, 2, 48, 32, 32), _D6, _D6, 0),
    ((4, 0, 64, 6, 192, 64, 48), _D6, _D6, 0),
]


def test_conv3_routing_is_pinned(monkeypatch):
    """Which kernel family serves a forward call (tdx_conv3_fwd_kernel: the conv route, pure host code) did not move.  The
    small-grid route needs the scratch arena: tdx_set_scratch only stores the pointer, so a host buffer with a claimed size
    stands in for it.  Nothing is launched."""
    import ctypes

    from turbdiff_amd import _lib as L

    for v in L.switch_names() + ("TDX_CONV_IMPL",):  # the library's own list, and the Python-side override
        monkeypatch.delenv(v, raising=False)
    names = {L.KERNEL_DIRECT: "direct", L.KERNEL_BRICK: "brick", L.KERNEL_SMALL: "small", L.KERNEL_RING: "ring"}
    modes = [(L.BF16, L.CONV_AUTO), (L.F16, L.CONV_AUTO), (L.F32, L.CONV_AUTO), (L.F32, L.CONV_SPLIT),
             (L.BF16, L.CONV_DIRECT), (L.F32, L.CONV_DIRECT)]
    lib = L.load()
    fake = ctypes.create_string_buffer(256)  # zeroed; never dereferenced by the queries
    try:
        for arena_bytes, column in ((0, 1), (96 << 20, 2)):
            assert lib.tdx_set_scratch(ctypes.addressof(fake) if arena_bytes else None, arena_bytes) == 0
            for row in _CONV3_ROUTES:
                shape = row[0]
                got = [names[L.query("tdx_conv3_fwd_kernel", *shape, dt, impl)] for dt, impl in modes]
                assert got == row[column].split(), (shape, arena_bytes)
                assert L.query("tdx_conv3_ring_brick_depth", *shape) == row[3], shape
                assert bool(L.query("tdx_conv3_uses_ring", *shape)) == (row[3] != 0), shape
    finally:
        lib.tdx_set_scratch(None, 0)
        L._ACTIVE = None  # a later GPU test in this process binds its real arena again


def test_kernel_asm_diff_splits_assembly_per_kernel():
    """tools/kernel_asm_diff.py: body (label .. .size) and descriptor per .amdhsa_kernel name, __hip_cuid_ normalised,
    --rename applied to the old side's mangled names.  Synthetic assembly: the tool itself needs hipcc, not a GPU."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_asm_diff", ROOT / "tools" / "kernel_asm_diff.py")
    kad = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kad)

    def asm(view, cuid, extra=""):
        k = f"_Z1kPf{len(view)}{view}i"
        return (f"\t.globl\t{k}\n{k}:\n\ts_load_dword s0, s[4:5], 0x0\n{extra}\ts_endpgm\n.Lfunc_end0:\n\t.size\t{k}, .Lfunc_end0-{k}\n"
                f"\t.amdhsa_kernel {k}\n\t\t.amdhsa_next_free_vgpr 4\n\t.end_amdhsa_kernel\n"
                f"\t.globl\t__hip_cuid_{cuid}\n__hip_cuid_{cuid}:\n")

    old = kad.kernels(asm("WgradViewS", "0123abcd"), [("10WgradViewS", "9WgradView")])
    new = kad.kernels(asm("WgradView", "89ef4567"), [])
    assert list(old) == list(new) == ["_Z1kPf9WgradViewi"]
    assert old == new
    body, desc = new["_Z1kPf9WgradViewi"]
    assert body.startswith("_Z1kPf9WgradViewi:\n") and body.rstrip().endswith(".Lfunc_end0-_Z1kPf9WgradViewi")
    assert ".amdhsa_next_free_vgpr 4" in desc and "hip_cuid" not in body
    assert kad.kernels(asm("WgradView", "89ef4567", "\ts_nop 0\n"), []) != new
    assert list(kad.kernels(asm("WgradViewS", "0123abcd"), [])) == ["_Z1kPf10WgradViewSi"]  # unrenamed: lost + added


def test_kernel_asm_diff_ignores_only_the_function_ordinal_of_local_labels():
    """tools/kernel_asm_diff.py sets the function's ordinal in its file to 0 in .LBB<f>_<n>, the `; %bb` comments' BB<f>_<n>
    and .Lfunc_end<f> (a kernel that becomes a template renumbers every function behind it); the block number <n>, and with it
    where a branch goes, still counts."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_asm_diff", ROOT / "tools" / "kernel_asm_diff.py")
    kad = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kad)

    def asm(f, target):
        return (f"k:\n\ts_cbranch_scc1 .LBB{f}_{target}\n.LBB{f}_1: ; %bb.1, preds =BB{f}_0\n\ts_nop 0\n.LBB{f}_2:\n\ts_endpgm\n"
                f".Lfunc_end{f}:\n\t.size\tk, .Lfunc_end{f}-k\n\t.amdhsa_kernel k\n\t.end_amdhsa_kernel\n")

    assert kad.kernels(asm(3, 2), []) == kad.kernels(asm(17, 2), [])
    assert ".LBB0_2" in kad.kernels(asm(17, 2), [])["k"][0] and ".Lfunc_end0-k" in kad.kernels(asm(17, 2), [])["k"][0]
    assert kad.kernels(asm(3, 2), []) != kad.kernels(asm(3, 1), [])  # another branch target is another kernel

    # the loop-nest comments name the function too, and the comment column of a label line moves with the ordinal's digits
    def loop(f):
        label = f".LBB{f}_3:"
        return (f"k:\n{label}{' ' * (40 - len(label))}; =>This Loop Header: Depth=1\n\t\t\t; Child Loop BB{f}_4 Depth 2\n\ts_endpgm\n"
                f".Lfunc_end{f}:\n\t.size\tk, .Lfunc_end{f}-k\n\t.amdhsa_kernel k\n\t.end_amdhsa_kernel\n")

    assert kad.kernels(loop(9), []) == kad.kernels(loop(10), [])
