#!/usr/bin/env python3
"""Golden vectors of TF-Net, from the reference's own classes run in float64.

Build container only: imports the unmodified ``turbdiff.models.tfnet`` (stand-ins for uninstalled third-party packages as
in make_golden.py, ``h5py`` replaced by tests/h5fake.py), runs ``LES`` / ``TFNetTraining`` on the CPU with ``.double()`` and
stores numbers only.  Inputs and the state dict are not stored: tests/tfnet_cases.py draws them (the recipe), here and in
the tests.

Shape: B = 2, T = 6, F = 4, grid 34 x 18 x 17, 8 local conditioning channels -- the smallest grid at which every
``clip_spatial`` clips (34 -> 17 -> 9 -> 5 -> 3, 18 -> 9 -> 5 -> 3 -> 2, 17 -> 9 -> 5 -> 3 -> 2).

Stored (float64; split over tfnet*.npz so that no file reaches 1 MiB, see tfnet_cases.FIXTURE_FILES):
* manifest of ``LES().state_dict()``;
* training mode: ``y``; ``dx`` at every second voxel per axis for the recipe's ``dy``; every parameter gradient of at most
  4096 elements in full, of each larger one the norm and 1024 recipe-drawn entries; the running statistics and counters
  of every BatchNorm after the call;
* eval mode: ``y``;
* ``ref32_err/<name>``: the relative L2 distance of the reference's own float32 run to its float64 run, per stored quantity;
* the trainer case (``TFNetTraining`` at the same grid, ``unroll_steps = 2``, an h5fake batch): the ``training_step`` loss, the
  stored-gradient subset, and a 3-step eval rollout subsampled as above.

    python tests/golden/make_golden_tfnet.py
"""

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import h5fake  # noqa: E402
import tfnet_cases as TC  # noqa: E402
from make_golden import REF, _stub, install_stubs  # noqa: E402


def rel(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def model_run(tfnet, key, dtype):
    """Every stored quantity of the model case in `dtype`, as {name: float64 array}."""
    xx, c_local, dy = (t.to(dtype) for t in TC.recipe_inputs())
    model = tfnet.LES(**TC.MODEL_KW)
    model.load_state_dict(TC.recipe_state_dict(TC.manifest_of(model.state_dict())), strict=True)
    model = model.to(dtype)
    out = {}
    model.train()
    x = xx.clone().requires_grad_()
    y = model(x, {key: c_local})
    y.backward(dy)
    out["train/y"] = y.detach().double().numpy()
    out["train/dx"] = TC.subsample(x.grad).double().numpy()
    out.update({f"train/{k}": v for k, v in TC.stored_gradients([(k, p.grad) for k, p in model.named_parameters()]).items()})
    for k, v in model.state_dict().items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            out[f"train/sd/{k}"] = v.double().numpy().copy() if v.is_floating_point() else v.numpy().copy()
    model.load_state_dict(TC.recipe_state_dict(TC.manifest_of(model.state_dict())), strict=True)
    model.eval()
    with torch.no_grad():
        out["eval/y"] = model(xx, {key: c_local}).double().numpy()
    return out, model


def trainer_run(tfnet, ofles, ofles_seq, dtype):
    task = tfnet.TFNetTraining(data_dir=Path("/fake/data"), samples_root=Path("/fake/samples"),
                               variables=(ofles.Variable.U, ofles.Variable.P), **TC.TRAINER_CFG)
    task.log = lambda *a, **k: None
    sd = task.state_dict()
    sd.update({f"model.{k}": v for k, v in TC.recipe_state_dict(TC.manifest_of(task.model.state_dict())).items()})
    task.load_state_dict(sd, strict=True)
    sd0 = {k: v.clone() for k, v in task.state_dict().items()}
    task = task.to(dtype)
    out = {}

    orig_input = task._model_input  # the float32 normalised grid embedding, widened: the model runs in `dtype`

    def model_input(batch):
        x, C = orig_input(batch)
        return x.to(dtype), C

    task._model_input = model_input

    task.train()
    batch, _ = TC.trainer_batch(TC.TRAINER_CFG["unroll_steps"], ofles=ofles, ofles_seq=ofles_seq)
    loss = task.training_step(batch, 0)["loss"]
    loss.backward()
    out["trainer/loss"] = np.array(loss.item())
    named = [(k, p.grad) for k, p in task.named_parameters() if p.grad is not None]
    out.update({f"trainer/{k}": v for k, v in TC.stored_gradients(named, seed=TC.SEED + 7).items()})
    out["trainer/grad_names"] = np.array([k for k, _ in named])
    task.load_state_dict({k: v.to(dtype) if v.is_floating_point() else v for k, v in sd0.items()}, strict=True)
    task.eval()
    batch, _ = TC.trainer_batch(TC.TRAINER_CFG["eval_unroll_steps"], ofles=ofles, ofles_seq=ofles_seq)
    with torch.no_grad():
        x_hat, _ = task._unroll_predict(batch)
    out["trainer/rollout"] = TC.subsample(x_hat).double().numpy()
    out["trainer/sd_keys"] = np.array(list(sd0.keys()))
    return out, sd0


def main():
    install_stubs()
    _stub("h5py", File=h5fake.File, Group=h5fake.Group)
    sys.path.insert(0, str(REF))
    torch.set_num_threads(8)
    torch.manual_seed(0)
    from turbdiff.data import ofles, ofles_seq
    from turbdiff.models import tfnet
    from turbdiff.models.conditioning import Conditioning

    key = Conditioning.Type.CELL_TYPE
    g64, model = model_run(tfnet, key, torch.float64)
    g32, _ = model_run(tfnet, key, torch.float32)
    out = dict(g64)
    out["manifest/keys"] = np.array(list(model.state_dict().keys()))
    out["manifest/shapes"] = np.array([",".join(map(str, v.shape)) for v in model.state_dict().values()])
    torch.manual_seed(1)  # the cell-type embedding's initial values (stored: they are the trainer's only non-recipe parameters)
    t64, sd0 = trainer_run(tfnet, ofles, ofles_seq, torch.float64)
    torch.manual_seed(1)
    t32, _ = trainer_run(tfnet, ofles, ofles_seq, torch.float32)
    out.update(t64)
    for name, a in {**g64, **t64}.items():
        if a.dtype == np.float64:
            out[f"ref32_err/{name}"] = np.array(rel({**g32, **t32}[name], a))
    for k, v in sd0.items():  # the task's parameters outside the model (the cell-type embedding), float32
        if not k.startswith("model.") and v.is_floating_point():
            out[f"trainer/sd0/{k}"] = v.numpy()

    files = {"tfnet_y.npz": ["train/y"], "tfnet_eval.npz": ["eval/y"], "tfnet_dx.npz": ["train/dx"]}
    placed = set()
    for fname, names in files.items():
        np.savez_compressed(HERE / fname, **{n: out[n] for n in names})
        placed.update(names)
    trainer = {k: v for k, v in out.items() if k.startswith("trainer/")}
    np.savez_compressed(HERE / "tfnet_trainer.npz", **trainer)
    placed.update(trainer)
    np.savez_compressed(HERE / "tfnet.npz", **{k: v for k, v in out.items() if k not in placed})
    for fname in TC.FIXTURE_FILES:
        size = (HERE / fname).stat().st_size
        assert size < 1 << 20, (fname, size)
        print("wrote", HERE / fname, f"{size / 1e3:.0f} kB")
    for k in ("train/y", "train/dx", "train/grad/spatial_filter.weight", "eval/y", "trainer/loss", "trainer/rollout"):
        print(k, "ref32_err", float(out[f"ref32_err/{k}"]))


if __name__ == "__main__":
    main()
