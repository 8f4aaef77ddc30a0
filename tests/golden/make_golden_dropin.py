#!/usr/bin/env python3
"""Golden data for tests/test_dropin_reference.py: what the reference itself says about the names, constructor calls and
numbers the drop-in claim rests on, so that the test needs nothing outside this repository.

Runs where the reference checkout is available (make_golden.REF), like the other generators.  Recorded in
tests/golden/dropin.npz:
  task/*        with turbdiff_amd.dropin installed, the reference's DiffusionTraining (dim 32, (u, p), log-snr-linear,
                T = 500, l2, noise_bcs, radam, GroupNorm, no geometry embedding) is constructed; the keyword arguments it
                passes to DenoisingModel / GaussianDiffusion (activation as its class name) and the modules' classes
  names/*       classes / functions defined in the reference's ddpm.py, normalization.py, cell_type_embeddings.py and
                conditioning.py; the members of its data.ofles.Variable (name, dims, value)
  surface/*     seeded inputs, weights and outputs of the reference's LinearAttention, pad_to_multiple_of / unpad,
                expand_as, SinusoidalPosEmb, normal_kl, normal_log_lk; the output of GeometryEmbedding with weights and
                input from pattern() (1.9 MB of input the test rebuilds instead of reading)
The reference's grid embedding, cell types and normalisation of the same cases are tests/golden/grid_io.npz already
(make_golden_grid.py).  Numbers and names only; nothing of the reference's source.

    python tests/golden/make_golden_dropin.py
"""

import inspect
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(ROOT / "generative-turbulence_amd"))
from make_golden import REF, install_stubs  # noqa: E402


def defined_names(mod):
    return sorted(n for n, v in vars(mod).items() if (inspect.isclass(v) or inspect.isfunction(v))
                  and getattr(v, "__module__", "") == mod.__name__)


def pattern(shape, scale):
    """float32 tensor of exact multiples of `scale` in [-125, 125] * scale from integer arithmetic alone: the same bits on every
    machine (tests/test_dropin_reference.py builds it the same way)."""
    i = torch.arange(int(np.prod(shape)), dtype=torch.int64).reshape(shape)
    return ((i * 7919) % 251 - 125).float() * scale


def main():
    install_stubs()
    sys.path.insert(0, str(REF))
    import turbdiff_amd.dropin as dropin

    dropin.install()
    import turbdiff_amd.models.ddpm as M

    out = {}
    calls, inits = {}, {cls: cls.__init__ for cls in (M.DenoisingModel, M.GaussianDiffusion)}
    for cls, init in inits.items():

        def record(self, *a, _init=init, _name=cls.__name__, **k):
            calls[_name] = {"n_positional": len(a), "kwargs": {key: (v.__name__ if inspect.isclass(v) else v) for key, v in k.items()}}
            _init(self, *a, **k)

        cls.__init__ = record
    from turbdiff.data.ofles import Variable as V
    from turbdiff.models.diffusion import DiffusionTraining

    task = DiffusionTraining(Path("/tmp/none"), Path("/tmp/none"), dim=32, variables=(V.U, V.P), beta_schedule="log-snr-linear",
                             timesteps=500, loss="l2", noise_bcs=True, optimizer="radam", norm_type="group",
                             with_geometry_embedding=False)
    for cls, init in inits.items():
        cls.__init__ = init
    out["task/calls"] = np.array(json.dumps(calls, sort_keys=True))
    out["task/classes"] = np.array([f"{type(task.model).__module__}.{type(task.model).__name__}",
                                    f"{type(task.model.model).__module__}.{type(task.model.model).__name__}"])
    out["task/state_dict_keys"] = np.array(list(task.state_dict().keys()))
    dropin.uninstall()

    # the reference's own modules from here on
    for name in list(sys.modules):
        if name == "turbdiff" or name.startswith("turbdiff."):
            del sys.modules[name]
    import turbdiff.data.ofles as RO
    import turbdiff.models.cell_type_embeddings as RC
    import turbdiff.models.conditioning as RCo
    import turbdiff.models.ddpm as R
    import turbdiff.models.normalization as RN

    assert R.__file__.startswith(str(REF)), R.__file__
    for key, mod in (("ddpm", R), ("normalization", RN), ("cell_type_embeddings", RC), ("conditioning", RCo)):
        out[f"names/{key}"] = np.array(defined_names(mod))
    out["names/variable/name"] = np.array([v.name for v in RO.Variable])
    out["names/variable/dims"] = np.array([v.dims for v in RO.Variable])
    out["names/variable/value"] = np.array([v.value for v in RO.Variable])

    torch.manual_seed(0)
    a = R.LinearAttention(8, heads=2, dim_head=4)
    for k, v in a.state_dict().items():
        out[f"surface/linear_attention/sd/{k}"] = v.numpy()
    x = torch.randn(2, 8, 3, 4, 5)
    out["surface/linear_attention/x"], out["surface/linear_attention/y"] = x.numpy(), a(x).detach().numpy()
    for i, shape in enumerate([(1, 2, 5, 4, 6), (1, 2, 4, 4, 4)]):
        x = torch.randn(*shape)
        p, q = R.pad_to_multiple_of(x, 2, mode="constant")
        out[f"surface/pad/{i}/x"], out[f"surface/pad/{i}/padded"] = x.numpy(), p.numpy()
        out[f"surface/pad/{i}/padding"] = np.array(tuple(q))
        out[f"surface/pad/{i}/unpadded"] = R.unpad(p, q).numpy()
    x, y = torch.randn(2, 3, 4), torch.randn(1, 5, 1)
    out["surface/expand_as/x"], out["surface/expand_as/y"] = x.numpy(), y.numpy()
    out["surface/expand_as/out"] = R.expand_as(x, y, 1).numpy()
    g = R.GeometryEmbedding(4, 8, torch.nn.SiLU)
    with torch.no_grad():
        for _, w in sorted(g.state_dict().items()):
            w.copy_(pattern(w.shape, 2.0**-12))
        out["surface/geometry_embedding/out"] = g(pattern((4, 55, 46, 47), 2.0**-6)).numpy()
    out["surface/sinusoidal_pos_emb/out"] = R.SinusoidalPosEmb(16)(torch.arange(5.0)).numpy()
    a, b, c, d = (torch.randn(3, 7) for _ in range(4))
    for k, v in zip("abcd", (a, b, c, d)):
        out[f"surface/normal/{k}"] = v.numpy()
    out["surface/normal/kl"] = R.normal_kl(a, b, c, d).numpy()
    out["surface/normal/log_lk"] = R.normal_log_lk(a, b, c).numpy()

    np.savez_compressed(HERE / "dropin.npz", **out)
    print(f"wrote {HERE / 'dropin.npz'}: {len(out)} arrays")


if __name__ == "__main__":
    main()
