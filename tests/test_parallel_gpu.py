"""Two ranks sharing the one GPU of the test box (gloo backend on device tensors): the
hook-driven bucketed all-reduce works with the HIP autograd Functions, and the averaged
gradients equal the single-process gradients of the global batch."""

import os
import socket
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _build(dev):
    sys.path.insert(0, str(ROOT / "generative-turbulence_amd"))
    from turbdiff_amd.models.conditioning import Conditioning
    from turbdiff_amd.models.ddpm import DenoisingModel, GaussianDiffusion

    g = np.load(ROOT / "tests" / "golden" / "model_cfg1.npz")
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}
    net = DenoisingModel(in_features=4, out_features=4, c_local_features=4, c_global_features=0, timesteps=10, dim=8,
                         u_net_levels=2, norm_type="group")
    net.load_state_dict(sd)
    diff = GaussianDiffusion(net, timesteps=10, beta_schedule="log-snr-linear", loss_type="l2", noise_bcs=True).to(dev)
    x = torch.from_numpy(g["x"]).to(dev)            # global batch of 2
    C = {Conditioning.Type.CELL_TYPE: torch.from_numpy(g["c_local"]).to(dev)}
    md = SimpleNamespace(cell_idx=torch.from_numpy(g["cell_idx"]).to(dev))
    t = torch.from_numpy(g["t"]).to(dev)
    noise = torch.from_numpy(g["loss_nb1/noise"]).to(dev)
    return diff, x, C, md, t, noise


def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    dev = torch.device("cuda:0")
    diff, x, C, md, t, noise = _build(dev)
    from turbdiff_amd.parallel import BucketedDataParallel, init_from_env

    init_from_env("gloo")
    ddp = BucketedDataParallel(diff, bucket_mb=0.25)
    grads = []
    for step in range(2):  # step 0 discovers the ready order, step 1 overlaps
        diff.zero_grad(set_to_none=True)
        loss, _ = diff.p_losses(x[rank : rank + 1], t[rank : rank + 1], C, md, None, noise=noise[rank : rank + 1])
        loss.backward()
        ddp.finish()
        grads.append({n: p.grad.detach().cpu().clone() for n, p in diff.model.named_parameters()})
    # the fused optimiser on the all-reduced gradients (views into the flat buckets)
    from turbdiff_amd.optim import ClipRAdam

    opt = ClipRAdam(diff.parameters(), lr=1e-3, max_norm=0.1)
    opt.step()
    params = {n: p.detach().cpu().clone() for n, p in diff.model.named_parameters()}
    torch.save((grads, ddp.bucket_layout(), params, float(opt.last_grad_norm)), f"{outdir}/rank{rank}.pt")
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_one_gpu_gradient_average(tmp_path):
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=280)
        assert p.exitcode == 0
    res = [torch.load(tmp_path / f"rank{r}.pt") for r in range(2)]
    diff, x, C, md, t, noise = _build(torch.device("cuda:0"))
    loss, _ = diff.p_losses(x, t, C, md, None, noise=noise)  # mean over the global batch of 2
    loss.backward()
    layout = res[0][1]
    assert layout is not None and len(layout) >= 2
    for name, p in diff.model.named_parameters():
        ref = p.grad.cpu()
        for r in range(2):
            for step in range(2):
                got = res[r][0][step][name]
                if ref.norm() < 1e-6:
                    assert got.norm() < 1e-5, name
                else:
                    assert ((got - ref).norm() / ref.norm()).item() < 2e-3, (name, r, step)
        assert torch.equal(res[0][0][1][name], res[1][0][1][name]), f"{name}: ranks disagree"
    # one clip + RAdam step on the global-batch gradients with the stock torch calls
    ref_norm = torch.nn.utils.clip_grad_norm_(diff.parameters(), 0.1)
    torch.optim.RAdam(diff.parameters(), lr=1e-3).step()
    for r in range(2):
        assert abs(res[r][3] - ref_norm.item()) < 2e-3 * ref_norm.item()
        for name, p in diff.model.named_parameters():
            assert torch.allclose(res[r][2][name], p.detach().cpu(), rtol=1e-4, atol=2e-6), (name, r)


def _rccl_worker(port, outdir):
    """World size 1 over backend "nccl" (= RCCL): communicator creation, the hook-driven bucketed all-reduce of
    device buffers on RCCL's stream, finish() -- everything the 2/4/8-GPU runs execute except a second peer."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = torch.device("cuda:0")
    diff, x, C, md, t, noise = _build(dev)
    from turbdiff_amd.parallel import BucketedDataParallel, init_from_env

    rank, world, local = init_from_env("nccl", force=True)
    assert (rank, world) == (0, 1) and torch.distributed.get_backend() == "nccl"
    ddp = BucketedDataParallel(diff, bucket_mb=0.25, force=True)
    assert ddp.active and ddp.bucket_layout() is not None  # static order from DenoisingModel.grad_ready_order()
    res = {}
    for tag, compress in (("f32", None), ("bf16", "bf16")):
        ddp.compress = compress
        if compress:
            ddp._wire = [torch.zeros_like(f, dtype=torch.bfloat16) for f in ddp._flat]
        diff.zero_grad(set_to_none=True)
        loss, _ = diff.p_losses(x, t, C, md, None, noise=noise)
        loss.backward()
        ddp.finish()
        res[tag] = {n: p.grad.detach().cpu().clone() for n, p in diff.model.named_parameters()}
    ddp.allreduce_only()
    torch.save((res, ddp.bucket_layout(), ddp.stats), f"{outdir}/rccl.pt")
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
def test_rccl_world_size_one_runs_the_communicator_path(tmp_path):
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_rccl_worker, args=(_free_port(), str(tmp_path)))
    p.start()
    p.join(timeout=280)
    assert p.exitcode == 0
    res, layout, stats = torch.load(tmp_path / "rccl.pt")
    assert len(layout) >= 2 and stats["steps"] == 2
    diff, x, C, md, t, noise = _build(torch.device("cuda:0"))
    loss, _ = diff.p_losses(x, t, C, md, None, noise=noise)
    loss.backward()
    for name, p in diff.model.named_parameters():
        ref = p.grad.cpu()
        if ref.norm() < 1e-6:
            continue
        assert ((res["f32"][name] - ref).norm() / ref.norm()).item() < 2e-3, name     # atomics: not bit-identical
        assert ((res["bf16"][name] - ref).norm() / ref.norm()).item() < 1e-2, name    # travelled as bfloat16


class _GraphTask:
    """What training.GraphedTrainingStep asks of a task, around a bare GaussianDiffusion, dense inputs and a
    BucketedDataParallel (the trainer's `ddp` attribute)."""

    def __init__(self, diff, ddp):
        self.model, self.ddp, self._opt = diff, ddp, None

    def _model_input(self, b):
        return b.x, b.C

    def _cell_idx(self, b):
        return b.cell_idx

    def parameters(self):
        return self.model.parameters()


def _graph_ddp_worker(rank, world, port, outdir, backend):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = torch.device("cuda:0")
    diff, x, C, md, t, noise = _build(dev)
    from turbdiff_amd.parallel import BucketedDataParallel, init_from_env
    from turbdiff_amd.training import GraphedTrainingStep

    init_from_env(backend, force=world == 1)
    ddp = BucketedDataParallel(diff, bucket_mb=0.25, force=world == 1)
    lo = rank % x.shape[0]
    xs, ts, ns = x[lo : lo + 1], t[lo : lo + 1], noise[lo : lo + 1]
    # the eager data-parallel step on this rank's sample
    diff.zero_grad(set_to_none=True)
    loss, _ = diff.p_losses(xs, ts, C, md, None, noise=ns)
    loss.backward()
    ddp.finish()
    eager = {n: p.grad.detach().cpu().clone() for n, p in diff.model.named_parameters()}
    eager_loss = loss.item()
    del loss
    # the same step replayed from ONE captured graph: staging kernels captured, all-reduces started by the host when the
    # captured backward passes each bucket's boundary
    gs = GraphedTrainingStep(_GraphTask(diff, ddp), inject=True)
    gs.set_draws(ts, ns)
    batch = SimpleNamespace(x=xs, C=C, cell_idx=md.cell_idx)
    graphed, losses = [], []
    for step in range(3):
        l = gs(batch)
        ddp.finish()
        torch.cuda.synchronize()
        graphed.append({n: p.grad.detach().cpu().clone() for n, p in diff.model.named_parameters()})
        losses.append(l.item())
    (slot,) = gs.slots.values()
    plan = slot.ddp_plan
    info = {"order": plan["order"], "flag": int(plan["flag_np"][0]), "replays": slot.replays, "layout": ddp.bucket_layout(),
            "captured_params": len(plan["params"]), "n_params": len(ddp.params), "steps": ddp.stats["steps"]}
    torch.save((eager, eager_loss, graphed, losses, info), f"{outdir}/rank{rank}.pt")
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("backend,world", [("gloo", 2), ("nccl", 1)])
def test_captured_training_step_under_data_parallelism(tmp_path, backend, world):
    """enable_graph_step with BucketedDataParallel.  Two ranks on the one GPU over gloo, and RCCL at world
    size 1: the gradients a replayed graph + host-launched bucket all-reduces leave in p.grad equal the eager data-parallel
    step's (same kernels; the halo-shell atomics of the data gradient differ in the last bits), replay after replay, on
    every rank; every bucket was marked inside the graph in launch order and the mark word counts the replays."""
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_graph_ddp_worker, args=(r, world, port, str(tmp_path), backend)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=280)
        assert p.exitcode == 0
    res = [torch.load(tmp_path / f"rank{r}.pt") for r in range(world)]
    for r, (eager, eager_loss, graphed, losses, info) in enumerate(res):
        assert len(info["layout"]) >= 2 and info["order"] == list(range(len(info["layout"]))), info  # buckets in ready order
        assert info["captured_params"] == info["n_params"] and info["replays"] == 3
        assert info["flag"] == 3 * 64 + len(info["order"]), info  # the last bucket's mark of the third replay
        assert info["steps"] == 1 + 2 + 3  # the eager step, the two warm-up steps of the capture, three replays
        for step, g in enumerate(graphed):
            assert abs(losses[step] - eager_loss) < 1e-5 * abs(eager_loss)
            for name, ref in eager.items():
                if ref.norm() < 1e-6:
                    assert g[name].norm() < 1e-5, name
                else:
                    assert ((g[name] - ref).norm() / ref.norm()).item() < 1e-4, (name, r, step)
    for name in res[0][0]:  # ranks hold the same averaged gradients
        for step in range(3):
            assert torch.equal(res[0][2][step][name], res[-1][2][step][name]), name


def _capture_beside_rccl_worker(port, outdir):
    """World size 1 over RCCL: graph captures (the sampler's reverse step) taken right behind asynchronous collectives, many
    times -- the communicator's watchdog thread polls those collectives' events while the capture is open."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = torch.device("cuda:0")
    diff, x, C, md, t, noise = _build(dev)
    from turbdiff_amd.parallel import init_from_env
    from turbdiff_amd.sampling import GraphSampler

    init_from_env("nccl", force=True)
    buf = torch.ones(1 << 22, device=dev)
    outs = []
    for rep in range(12):
        works = [torch.distributed.all_reduce(buf, async_op=True) for _ in range(4)]
        torch.distributed.barrier()
        gs = GraphSampler(diff, x[:1], C, md.cell_idx, seed=rep, trajectory_ids=[0])  # captures on construction / first run
        gs.run_steps(2)
        for w in works:
            w.wait()
        torch.cuda.synchronize()
        outs.append(bool(torch.isfinite(gs.x_t).all()))
        del gs
    torch.save(outs, f"{outdir}/capture.pt")
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
def test_graph_capture_beside_an_rccl_communicator(tmp_path):
    """Round 6: hipGraph captures in a process that holds an RCCL communicator (the sampling leg of `bench.py --gpus N`): twelve
    sampler captures right behind asynchronous collectives.  ProcessGroupNCCL's watchdog thread polls the collectives' events
    every ~100 ms; a query that lands inside an open capture raises hipErrorStreamCaptureUnsupported under the default "global"
    capture-error mode and aborts the process -- the long capture of the data-parallel training step hit it in 2 of 6 runs
    (test_captured_training_step_under_data_parallelism[nccl-1]; 0 of 20 since), the short sampler capture rarely does.  Both
    now capture in "thread_local" mode."""
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_capture_beside_rccl_worker, args=(_free_port(), str(tmp_path)))
    p.start()
    p.join(timeout=280)
    assert p.exitcode == 0
    outs = torch.load(tmp_path / "capture.pt")
    assert len(outs) == 12 and all(outs)


@pytest.mark.parametrize("fork", ["0", "1"])
@pytest.mark.parametrize("full_size", [False, True])
def test_captured_step_stays_correct_over_replays_with_and_without_the_side_stream(fork, full_size, monkeypatch):
    """Every parameter gradient of every replay against the eager step's, five replays, with the weight gradients on the
    capture's own stream (the default since round 6) and forked onto the side stream (TDX_GRAPH_WGRAD_STREAM=1).  Regression:
    hipMemsetAsync inside a capture becomes a memset NODE that this runtime does not order against earlier kernel nodes still
    writing the previous owner of the same graph-pool block -- from the SECOND replay on, one element of the encoder / decoder
    gradients was garbage as soon as the capture stopped forking (the fork's record_stream had kept those blocks from being
    reused).  The library zeroes with kernels now (tdx_zero_async)."""
    sys.path.insert(0, str(ROOT / "generative-turbulence_amd"))
    from turbdiff_amd.training import GraphedTrainingStep

    monkeypatch.setenv("TDX_GRAPH_WGRAD_STREAM", fork)
    dev = torch.device("cuda:0")
    if full_size:
        sys.path.insert(0, str(ROOT))
        import bench
        from turbdiff_amd.models.conditioning import Conditioning

        diff = bench.build_model(dev)
        bench.set_mode(diff, "bf16")
        xs, c, idx = bench.synthetic_inputs(2, dev, (96, 32, 24))
        C, md = {Conditioning.Type.CELL_TYPE: c}, SimpleNamespace(cell_idx=idx)
        ts = torch.tensor([3, 250], device=dev)
        ns = torch.randn(xs.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
        tol = 3e-2  # bf16: the halo shell's atomics alone move gradients by up to 6e-3 between two eager runs
    else:
        diff, x, C, md, t, noise = _build(dev)
        xs, ts, ns = x[0:1], t[0:1], noise[0:1]
        tol = 1e-4
    diff.zero_grad(set_to_none=True)
    loss, _ = diff.p_losses(xs, ts, C, md, None, noise=ns)
    loss.backward()
    torch.cuda.synchronize()
    eager_loss = loss.item()
    eager = {n: p.grad.detach().clone() for n, p in diff.model.named_parameters()}
    del loss
    gs = GraphedTrainingStep(_GraphTask(diff, None), inject=True)
    gs.set_draws(ts, ns)
    batch = SimpleNamespace(x=xs, C=C, cell_idx=md.cell_idx)
    for replay in range(5):
        l = gs(batch)
        torch.cuda.synchronize()
        assert abs(l.item() - eager_loss) < 1e-5 * abs(eager_loss) or full_size and abs(l.item() - eager_loss) < 1e-3 * abs(eager_loss)
        for n, p in diff.model.named_parameters():
            g, r = p.grad.detach(), eager[n]
            assert torch.isfinite(g).all(), (n, replay)
            if r.norm() > 1e-6:
                assert ((g - r).norm() / r.norm()).item() < tol, (n, replay)


# --------------------------------------------------------------------------- captured data-parallel step, inputs that change
# per replay, a parameter whose gradient is chained eagerly behind the graph, a parameter that receives none

_K = 4                # steps = replays, each with its own batch, geometry, timesteps and noise
_BUCKET_MB = 0.25     # >= 2 buckets for the dim = 8, two-level U-Net
_COUNTS = (12, 10, 9)
_TIMESTEPS = [(1, 8), (6, 2), (9, 4), (0, 7)]
_E2E_LR = 1e-2
_TABLE = "cell_type_embedding.embedding.weight"
_UNUSED = "never_used"


def _trainer_case(dev, unused=False):
    """A DiffusionTrainer in the small configuration of the neighbouring tests (its conditioning comes from the LEARNED
    cell-type table) and _K dense global batches of two samples, each with its own cell types, in-domain cells,
    timesteps and noise.  Same seeds -> the same task and data in every process."""
    sys.path.insert(0, str(ROOT / "generative-turbulence_amd"))
    from turbdiff_amd.training import DiffusionTrainer

    torch.manual_seed(0)
    tr = DiffusionTrainer(**{**DiffusionTrainer.SHIPPED_CONFIG, "dim": 8, "timesteps": 10}, u_net_levels=2,
                          normalization_mode="mean-std", max_train_steps=10, compute_mode="f32")
    if unused:
        setattr(tr, _UNUSED, torch.nn.Parameter(torch.ones(5)))  # requires_grad, never used
    tr.to(dev)
    gen = torch.Generator().manual_seed(21)
    steps = []
    for k in range(_K):
        inside = torch.zeros(_COUNTS, dtype=torch.bool)
        inside[1:-1, 1:-1, 1:-1] = True
        if k % 2:
            inside[3:6, 2:5, 2:6] = False  # another in-domain cell count through the same graph
        steps.append(SimpleNamespace(
            x=(torch.randn(2, 4, *_COUNTS, generator=gen) * 1.5 + 0.1).to(dev),
            cell_types=torch.randint(0, 6, _COUNTS, generator=gen).to(dev),
            mean=torch.tensor([0.1, -0.2, 0.0, 0.3]).to(dev), std=torch.tensor([1.5, 1.2, 0.9, 0.8]).to(dev),
            cell_idx=inside.flatten().nonzero().flatten().to(dev),
            t=torch.tensor(_TIMESTEPS[k]).to(dev), noise=torch.randn(2, 4, *_COUNTS, generator=gen).to(dev)))
    return tr, steps


def _samples(s, lo, hi):
    """Samples lo .. hi - 1 of a global batch (one geometry per batch: cell types and in-domain cells are shared)."""
    return SimpleNamespace(x=s.x[lo:hi], cell_types=s.cell_types, mean=s.mean, std=s.std, cell_idx=s.cell_idx,
                           t=s.t[lo:hi], noise=s.noise[lo:hi])


def _eager_backward(tr, b):
    x, C = tr._model_input(b)
    loss, _ = tr.model.p_losses(x, b.t, C, SimpleNamespace(cell_idx=b.cell_idx), None, noise=b.noise)
    loss.backward()
    return loss.item()  # (no tensor of the autograd graph survives: a later capture needs it gone)


def _grads_of(tr):
    return {n: None if p.grad is None else p.grad.detach().cpu().clone() for n, p in tr.named_parameters()}


def _captured_ddp_worker(rank, world, port, outdir, backend, unused):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = torch.device("cuda:0")
    tr, steps = _trainer_case(dev, unused)
    from turbdiff_amd.optim import ClipRAdam
    from turbdiff_amd.parallel import BucketedDataParallel, init_from_env
    from turbdiff_amd.training import GraphedTrainingStep

    init_from_env(backend, force=world == 1)
    tr.ddp = ddp = BucketedDataParallel(tr, bucket_mb=_BUCKET_MB, force=world == 1)
    mine = [_samples(s, rank, rank + 1) for s in steps]  # this rank's sample of every global batch
    # (1) the eager data-parallel step on every batch
    eager = []
    for b in mine:
        tr.zero_grad(set_to_none=True)
        loss = _eager_backward(tr, b)
        ddp.finish()
        torch.cuda.synchronize()
        eager.append((_grads_of(tr), loss))
    tr.zero_grad(set_to_none=True)
    # (2) the same steps replayed from ONE captured graph
    info = {}
    end_capture = ddp.end_capture

    def end_capture_and_look():
        plan = end_capture()
        info["staged_after_capture"] = sum(len(s) for s in ddp._staged)
        return plan

    ddp.end_capture = end_capture_and_look
    gs = GraphedTrainingStep(tr, inject=True)
    graphed = []
    for b in mine:
        gs.set_draws(b.t, b.noise)
        loss = gs(b)
        ddp.finish()
        torch.cuda.synchronize()
        graphed.append((_grads_of(tr), loss.item()))
    (slot,) = gs.slots.values()
    plan = slot.ddp_plan
    names = {id(p): n for n, p in tr.named_parameters()}
    index = {id(p): i for i, p in enumerate(ddp.params)}
    partial = [b for b in range(len(ddp._buckets)) if b not in plan["order"]]
    info.update(order=list(plan["order"]), n_buckets=len(ddp._buckets), replays=slot.replays,
                chained=[names[id(p)] for p in slot.chained],
                table_bucket=ddp._bucket_of[index[id(tr.cell_type_embedding.embedding.weight)]],
                partial={b: [names[id(ddp.params[i])] for i in ddp._buckets[b]] for b in partial},
                captured_in_partial={b: sum(i in plan["params"] for i in ddp._buckets[b]) for b in partial})
    # (3) end to end: K optimiser steps on eager data-parallel steps and on captured ones, from the same start
    trained = {}
    if not unused:
        del gs, slot, plan
        for mode in ("eager", "captured"):
            tr2, _ = _trainer_case(dev)
            tr2.ddp = ddp2 = BucketedDataParallel(tr2, bucket_mb=_BUCKET_MB, force=world == 1)
            tr2._opt = opt = ClipRAdam(tr2.parameters(), lr=_E2E_LR, max_norm=0.1)
            gs2 = GraphedTrainingStep(tr2, inject=True) if mode == "captured" else None
            for b in mine:
                if gs2 is not None:
                    gs2.set_draws(b.t, b.noise)
                    gs2(b)
                else:
                    opt.zero_grad(set_to_none=True)
                    _eager_backward(tr2, b)
                ddp2.finish()
                opt.step()
            torch.cuda.synchronize()
            trained[mode] = {n: p.detach().cpu().clone() for n, p in tr2.named_parameters()}
            del gs2
    torch.save((eager, graphed, info, trained), f"{outdir}/rank{rank}.pt")
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


_captured_runs = {}


def _captured_run(tmp_path, backend, world, unused):
    """The worker's results per rank (one run per case, shared by the tests that look at it) and the reference."""
    key = (backend, world, unused)
    if key not in _captured_runs:
        ctx = mp.get_context("spawn")
        port = _free_port()
        procs = [ctx.Process(target=_captured_ddp_worker, args=(r, world, port, str(tmp_path), backend, unused)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=280)
            assert p.exitcode == 0
        _captured_runs[key] = [torch.load(tmp_path / f"rank{r}.pt") for r in range(world)]
    return _captured_runs[key], _global_batch_reference(world, unused)


_references = {}


def _global_batch_reference(world, unused):
    """Not the code under test: one process, no BucketedDataParallel, no graph -- stock autograd through the same model on
    the GLOBAL batch (the samples of all ranks) with the same draws.  Per step {name: gradient, or None}."""
    key = (world, unused)
    if key not in _references:
        tr, steps = _trainer_case(torch.device("cuda:0"), unused)
        ref = []
        for s in steps:
            tr.zero_grad(set_to_none=True)
            _eager_backward(tr, _samples(s, 0, world))
            torch.cuda.synchronize()
            ref.append(_grads_of(tr))
        _references[key] = ref
    return _references[key]


def _rel(got, want):
    return ((got - want).norm() / want.norm()).item()


def _check_captured_gradients(res, ref, world):
    """-> the smallest consecutive-step separation of the reference over the partly captured bucket(s)."""
    info = res[0][2]
    # preconditions: the partly captured case
    assert info["n_buckets"] >= 2 and len(info["order"]) < info["n_buckets"], info
    assert _TABLE in info["chained"], info["chained"]
    tb = info["table_bucket"]
    assert tb in info["partial"] and info["captured_in_partial"][tb] >= 1, info
    assert info["replays"] == _K
    # the inputs must tell a refreshed gradient from a stale one: on the reference alone, any two consecutive steps differ
    # by >= 50 x the 2e-3 tolerance in every tensor of the partly captured bucket(s) that has a gradient at all
    separation, checked = float("inf"), 0
    for names in info["partial"].values():
        for name in names:
            for k in range(1, _K):
                a, b = ref[k - 1][name], ref[k][name]
                if a is None or b is None or max(a.norm(), b.norm()) < 1e-6:
                    continue
                separation = min(separation, ((a - b).norm() / max(a.norm(), b.norm())).item())
                checked += 1
    print(f"separation: smallest consecutive-step difference {separation:.3f} over {checked} (tensor, step) pairs")
    assert checked >= 3 * (_K - 1) and separation >= 0.1, (separation, checked)
    bad = []

    def compare(what, got, want, tol, where):
        if want is None:  # the reference gives this parameter no gradient at all: its slice must hold exact zeros
            if got is None or got.count_nonzero() != 0:
                bad.append((what, *where, "not exactly zero", None if got is None else got.abs().max().item()))
        elif want.norm() < 1e-6:
            if not got.norm() < 1e-5:
                bad.append((what, *where, "norm", got.norm().item()))
        elif not _rel(got, want) < tol:
            bad.append((what, *where, "rel-L2", _rel(got, want)))

    for r, (eager, graphed, info_r, _) in enumerate(res):
        if info_r["staged_after_capture"] != 0:  # end_capture() must leave nothing staged
            bad.append(("pairs still staged after end_capture()", "", r, 0, "count", float(info_r["staged_after_capture"])))
        for k in range(_K):
            (ge, le), (gg, lg) = eager[k], graphed[k]
            if not abs(lg - le) < 1e-5 * abs(le):
                bad.append(("loss captured vs eager", "", r, k, "values", (lg, le)))
            for name, want in ref[k].items():
                compare("eager ddp vs global batch", ge[name], want, 2e-3, (name, r, k))
                compare("captured vs global batch", gg[name], want, 2e-3, (name, r, k))
                compare("captured vs eager ddp", gg[name], ge[name] if want is not None else None, 1e-4, (name, r, k))
                if not torch.equal(gg[name], res[0][1][k][0][name]):
                    bad.append(("ranks disagree", name, r, k, "", None))
    print(f"{len(bad)} failed comparisons")
    worst = sorted((b for b in bad if isinstance(b[-1], float)), key=lambda b: -b[-1])[:6]
    assert not bad, (f"{len(bad)} comparisons failed, replays {sorted({b[3] for b in bad})}, "
                     f"tensors {sorted({b[1] for b in bad})[:8]}, largest {worst}")
    return separation


@pytest.mark.timeout(300)
@pytest.mark.parametrize("backend,world", [("gloo", 2), ("nccl", 1)])
def test_captured_ddp_step_refreshes_every_gradient_when_the_inputs_change(tmp_path, backend, world):
    """The captured training step under BucketedDataParallel with what a real run has and the other tests of this file do
    not: inputs that change from replay to replay (batch, geometry, timesteps, noise) and a parameter -- the learned
    cell-type table -- whose gradient is chained eagerly BEHIND the graph.  The table is in no ready order, so it shares
    the last bucket with the last-ready U-Net parameters; that bucket does not fill up during the capture, and its staging
    kernel has to be part of the graph all the same, or from the second replay on its captured parameters keep an old
    step's gradient (all-reduced again and again at world size > 1).

    Every named parameter after every one of four replays, against (i) stock autograd on the global batch in one process
    (2e-3 relative L2: the batch split and the atomics differ), (ii) the eager data-parallel step on the same inputs
    (1e-4: the same kernels); ranks hold bit-equal gradients.  The reference's own consecutive steps differ by >= 0.1 in
    every tensor of the partly captured bucket (asserted; measured: smallest 0.384 at world size 1, 0.267
    at world size 2 -- an encoder bias -- over 96 (tensor, step) pairs, the same from the CPU oracle and on the GPU), so a gradient that is not refreshed cannot pass."""
    res, ref = _captured_run(tmp_path, backend, world, unused=False)
    _check_captured_gradients(res, ref, world)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("backend,world", [("gloo", 2), ("nccl", 1)])
def test_captured_ddp_step_with_a_parameter_that_never_gets_a_gradient(tmp_path, backend, world):
    """The same with one more parameter that requires a gradient and is never used: it sits behind the table in the last
    bucket, which then fills up neither in the capture nor in the table's hook -- finish() completes it after every replay.
    Its slice holds exact zeros after every replay; the captured parameters of that bucket track the reference."""
    res, ref = _captured_run(tmp_path, backend, world, unused=True)
    info = res[0][2]
    assert _UNUSED in info["chained"] and _UNUSED in info["partial"][info["table_bucket"]], info
    assert all(r[_UNUSED] is None for r in ref)
    for eager, graphed, _, _ in res:
        for k in range(_K):
            assert graphed[k][0][_UNUSED] is not None and graphed[k][0][_UNUSED].count_nonzero() == 0, k
    _check_captured_gradients(res, ref, world)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("backend,world", [("gloo", 2), ("nccl", 1)])
def test_training_on_captured_ddp_steps_equals_training_on_eager_ddp_steps(tmp_path, backend, world):
    """What a user would see: two identically initialised trainers, the same four batches and draws, clip 0.1 + RAdam
    (ClipRAdam) after every step -- one on eager data-parallel steps, one on captured ones.  The parameters agree after the
    fourth step within the bound this file uses for parameters after an optimiser step."""
    res, _ = _captured_run(tmp_path, backend, world, unused=False)
    tr0, _ = _trainer_case(torch.device("cpu"))
    start = {n: p.detach().clone() for n, p in tr0.named_parameters()}
    bad = []
    for r, (_, _, _, trained) in enumerate(res):
        assert set(trained) == {"eager", "captured"}
        moved = sum(not torch.equal(trained["eager"][n], start[n]) for n in start)
        assert moved > 0.9 * len(start), "the eager run must have trained"
        for n, want in trained["eager"].items():
            got = trained["captured"][n]
            if not torch.allclose(got, want, rtol=1e-4, atol=2e-6):
                bad.append((n, r, ((got - want).abs() - 1e-4 * want.abs()).max().item()))
            assert torch.equal(got, res[0][3]["captured"][n]), f"{n}: ranks disagree"
    print(f"{len(bad)} parameters differ")
    assert not bad, f"{len(bad)} parameters differ after {_K} steps; largest |difference| - 1e-4 |eager| (bound 2e-6): {sorted(bad, key=lambda b: -b[2])[:6]}"


def _kept_gradients_worker(rank, world, port, outdir):
    """Eager data-parallel steps with zero_grad(set_to_none=False): p.grad stays the bucket slice, backward accumulates
    straight into it, and the hook stages an in-place item (source == destination)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    dev = torch.device("cuda:0")
    diff, x, C, md, t, noise = _build(dev)
    from turbdiff_amd.parallel import BucketedDataParallel, init_from_env

    init_from_env("gloo")
    ddp = BucketedDataParallel(diff, bucket_mb=0.25)
    out, in_place = {}, []
    for keep in (False, True):
        for j in range(2):  # two different inputs per rank, so that a slice that is not rewritten shows
            lo = (rank + j) % 2
            diff.zero_grad(set_to_none=not keep)
            if keep:
                in_place.append(all(p.grad is not None and p.grad.data_ptr() == ddp._views[i][1].data_ptr() for i, p in enumerate(ddp.params)))
            loss, _ = diff.p_losses(x[lo : lo + 1], t[lo : lo + 1], C, md, None, noise=noise[lo : lo + 1])
            loss.backward()
            if keep:
                in_place.append(all(p.grad.data_ptr() == ddp._views[i][1].data_ptr() for i, p in enumerate(ddp.params)))
            ddp.finish()
            torch.cuda.synchronize()
            out[keep, j] = {n: p.grad.detach().cpu().clone() for n, p in diff.model.named_parameters()}
    torch.save((out, in_place, ddp.bucket_layout()), f"{outdir}/rank{rank}.pt")
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
def test_eager_ddp_step_with_gradients_kept_in_their_bucket_slices(tmp_path):
    """zero_grad(set_to_none=False) between data-parallel steps: the gradient accumulates into its bucket slice, the staging
    item has source == destination and is scaled by 1 / world IN PLACE -- once.  Same averaged gradients as the
    set_to_none=True step on the same inputs (1e-4 relative L2: the same kernels, only the atomics differ), two ranks."""
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_kept_gradients_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=280)
        assert p.exitcode == 0
    res = [torch.load(tmp_path / f"rank{r}.pt") for r in range(2)]
    for r, (out, in_place, layout) in enumerate(res):
        assert len(layout) >= 2 and in_place and all(in_place), "the gradients must have lived in their slices"
        for j in range(2):
            for name, want in out[False, j].items():
                got = out[True, j][name]
                if want.norm() < 1e-6:
                    assert got.norm() < 1e-5, (name, r, j)
                else:
                    assert _rel(got, want) < 1e-4, (name, r, j, _rel(got, want))
                assert torch.equal(got, res[0][0][True, j][name]), f"{name}: ranks disagree"
