#!/usr/bin/env python3
"""Golden vectors of the DilResNet regression baseline, from the reference's own classes.

Build container only: imports the unmodified ``turbdiff.models.dilresnet.DilResNetTraining`` and
``turbdiff.data.ofles_seq.OpenFOAMSequenceDataset`` (stand-ins for uninstalled third-party packages as in make_golden.py,
``h5py`` replaced by tests/h5fake.py as in make_golden_repository.py) and records in tests/golden/dilresnet.npz:

* sequence windows (valid_steps, the steps and samples of several batches) over the seeded h5fake cases;
* the task at hidden 16, N 2, dilations [1, 2, 4, 8] on the 9 x 7 x 6 case (every axis shorter than 2 * 8 + 1, so the
  dilation-8 taps clamp on both sides), weights set by ``golden_weights`` (integer arithmetic, rebuilt by the tests):
  forward output, the training loss, every parameter gradient and the conditioning gradient;
* buffers and parameters after 3 optimiser steps (Adam + LambdaLR, clip-by-norm 0.1), the noise draws injected;
* a 5-step ``unroll_samples`` with block_size 2 (inside mask of the case);
* the LR lambda at several steps; a conditioning width 11 variant (cell positions): forward output and the gradient of
  ``encode_c_local``;
* the task's state-dict manifest.

    python tests/golden/make_golden_dilresnet.py
"""

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import h5fake  # noqa: E402
from make_golden import REF, _stub, install_stubs, to_np  # noqa: E402

SEQ_REQUESTS = [[0], [1, 0, 3], [4, 5]]
LR_STEPS = [0, 1, 7, 100, 999, 1000, 5000]
CFG = dict(context_window=1, unroll_steps=1, eval_unroll_steps=5, sample_steps=[], main_sample_step=-1,
           normalization_mode="u:norm-max;p:abs-max", cell_type_features=True, cell_type_embedding_type="learned",
           cell_type_embedding_dim=8, learning_rate=1e-3, min_learning_rate=1e-6, max_train_steps=1000, N=2,
           hidden_dim=16, training_noise_std=1e-3, compute_expensive_sample_metrics=False, cell_pos_features=False)


def golden_weights(module, salt=0):
    """Deterministic parameters from integer arithmetic (the tests rebuild them): uniform-ish in +-1/sqrt(fan_in)."""
    with torch.no_grad():
        for j, (name, p) in enumerate(sorted(module.named_parameters())):
            n = p.numel()
            k = torch.arange(n, dtype=torch.int64)
            v = ((k * 7919 + (j + 1) * 104729 + salt * 15485863) % 20011).double() / 20011.0 * 2.0 - 1.0
            fan_in = p[0].numel() if p.ndim > 1 else 16
            p.copy_((v / fan_in ** 0.5).reshape(p.shape).float())


def stats_of(repo):
    """OpenFOAMStats for the variables u, p from the first case's data (norm(u) max, p min / max)."""
    from turbdiff.data.ofles import OpenFOAMStats

    data = repo.read(0, list(range(len(repo.times[0]))))
    u, p = data.samples[list(data.samples)[0]], data.samples[list(data.samples)[1]]
    un = u.norm(dim=-1)
    st = {"u": {"mean": u.mean(dim=(0, 1)), "std": u.std(dim=(0, 1)), "min": u.amin(dim=(0, 1)), "max": u.amax(dim=(0, 1))},
          "norm(u)": {"mean": un.mean(), "std": un.std(), "min": un.min(), "max": un.max()},
          "p": {"mean": p.mean(dim=(0, 1)), "std": p.std(dim=(0, 1)), "min": p.amin(dim=(0, 1)), "max": p.amax(dim=(0, 1))}}
    return OpenFOAMStats(st), {f"{k}/{n}": to_np(v) for k, d in st.items() for n, v in d.items()}


def main():
    install_stubs()
    _stub("h5py", File=h5fake.File, Group=h5fake.Group)
    sys.path.insert(0, str(REF))
    torch.set_num_threads(8)
    torch.use_deterministic_algorithms(True)
    from turbdiff.data.ofles import OpenFOAMDataRepository, Variable
    from turbdiff.data.ofles_seq import OpenFOAMSequenceDataset
    from turbdiff.models.conditioning import Conditioning
    from turbdiff.models.dilresnet import DilResNetTraining

    out = {}
    files = h5fake.install_cases()
    variables = (Variable.U, Variable.P)
    repo = OpenFOAMDataRepository(files["train"], variables)
    stats, st_np = stats_of(repo)
    out.update({f"stats/{k}": v for k, v in st_np.items()})

    # ---- sequence windows
    for name, (L, s, d) in {"a": (3, 2, 0.05), "b": (2, 1, -1.0), "c": (1, 1, -1.0)}.items():
        ds = OpenFOAMSequenceDataset(OpenFOAMDataRepository(files["train"], variables), stats, sequence_length=L, stride=s,
                                     discard_first_seconds=d)
        out[f"seq/{name}/cfg"] = np.array([L, s, d])
        out[f"seq/{name}/len"] = np.array(len(ds))
        for i, vs in enumerate(ds.valid_steps):
            out[f"seq/{name}/valid_steps/{i}"] = np.asarray(vs)
        if name == "a":
            for r, req in enumerate(SEQ_REQUESTS):
                b = ds[req]
                out[f"seq/a/get/{r}/t"] = to_np(b.data.t)
                for v, x in b.data.samples.items():
                    out[f"seq/a/get/{r}/{v.name}"] = to_np(x)

    # ---- the task
    ds = OpenFOAMSequenceDataset(OpenFOAMDataRepository(files["train"], variables), stats, sequence_length=2, stride=1)
    batch = ds[[0, 3]]                # two windows of case 0 (9 x 7 x 6)
    out["batch/idx"] = np.array([0, 3])

    def build(**over):
        task = DilResNetTraining(data_dir=Path("/fake/data"), samples_root=Path("/fake/samples"), variables=variables,
                                 **{**CFG, **over})
        task.log = lambda *a, **k: None
        return task

    task = build()
    golden_weights(task)
    out["manifest/keys"] = np.array(list(task.state_dict().keys()))
    out["manifest/shapes"] = np.array([",".join(map(str, v.shape)) for v in task.state_dict().values()])

    # LR lambda
    opt_cfg = task.configure_optimizers()
    lam = opt_cfg["lr_scheduler"]["scheduler"].lr_lambdas[0]
    out["lr/steps"] = np.array(LR_STEPS)
    out["lr/values"] = np.array([lam(s) for s in LR_STEPS])

    # forward + gradients of the training loss, the conditioning gradient included
    x, C = task._model_input(batch)
    x0 = x[:, 0]
    c_leaf = {k: v.detach().clone().requires_grad_() for k, v in C.items()}
    y = task.model(x0, c_leaf)
    out["fwd/x0"], out["fwd/y"] = to_np(x0), to_np(y)

    noises = [torch.randn(x0.shape, generator=torch.Generator().manual_seed(100 + i)) for i in range(4)]
    out.update({f"noise/{i}": to_np(n) for i, n in enumerate(noises)})
    real_randn_like = torch.randn_like
    draws = iter(noises)
    torch.randn_like = lambda t, **k: next(draws)
    try:
        orig_input = task._model_input

        def model_input(b):
            xx, CC = orig_input(b)
            CC = {k: v for k, v in CC.items()}
            for k, v in CC.items():
                v.retain_grad()
                model_input.C = CC
            return xx, CC

        task._model_input = model_input
        loss = task.training_step(batch, 0)["loss"]
        loss.backward()
        out["loss0"] = to_np(loss)
        out["dC"] = to_np(model_input.C[Conditioning.Type.CELL_TYPE].grad)
        for k, p in task.named_parameters():
            out[f"grad/{k}"] = to_np(p.grad)
        out["after0/dx_mean"], out["after0/dx_var"] = to_np(task.dx_mean), to_np(task.dx_var)

        # 3 optimiser steps from the same start (fresh task, same weights), clip 0.1
        task = build()
        golden_weights(task)
        task.log = lambda *a, **k: None
        oc = task.configure_optimizers()
        opt, sched = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
        draws = iter(noises[1:])
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = task.training_step(batch, 0)["loss"]
            loss.backward()
            torch.nn.utils.clip_grad_norm_(task.parameters(), 0.1)
            opt.step()
            sched.step()
            losses.append(loss.item())
        out["train/losses"] = np.array(losses)
        for k, v in task.state_dict().items():
            if k.startswith("model.") or k.startswith("cell_type_embedding") or k in ("dx_mean", "dx_var", "n_train_batches_tracked"):
                out[f"train/sd/{k}"] = to_np(v)
    finally:
        torch.randn_like = real_randn_like

    # 5-step unroll in blocks of 2 with the trained buffers and weights
    task.eval()
    with torch.no_grad():
        xs = task.unroll_samples(batch, [0, 1, 2, 3, 4], block_size=2)
    out["unroll/x"] = to_np(xs)
    out["unroll/inside"] = to_np(batch.data.inside_mask)

    # conditioning width 11 (cell positions)
    task11 = build(cell_pos_features=True)
    golden_weights(task11, salt=1)
    x, C = task11._model_input(batch)
    y = task11.model(x[:, 0], C)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(7))
    y.backward(gy)
    out["c11/y"], out["c11/gy"] = to_np(y), to_np(gy)
    out["c11/grad_encode_c_local"] = to_np(task11.model.encode_c_local.weight.grad)
    out["c11/grad_encode"] = to_np(task11.model.encode.weight.grad)

    np.savez_compressed(HERE / "dilresnet.npz", **out)
    print("wrote", HERE / "dilresnet.npz", f"{(HERE / 'dilresnet.npz').stat().st_size / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
