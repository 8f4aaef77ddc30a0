"""Generate tests/golden/actfn.npz from the UNMODIFIED reference: the denoiser built with the `actfn` choices that
options.npz does not cover (relu, softplus, tanh; GELU is options.npz's `gelu` block), as the reference's `actfn_from_str`
constructs them (turbdiff/models/diffusion.py:30-38: the torch module at its default arguments).

Same architecture, weights (seed 0 + the perturbed norm affines of make_golden.make_variant) and inputs as the `options`
block of make_golden.py -- x, c_local, cell_idx and t are read back from options.npz -- and the same outputs per tag:
eps_hat, the training noise, loss, every parameter's gradient norm and the small gradients in full.

    python tests/golden/make_golden_actfn.py
"""

import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden import OUT, REF, install_stubs, to_np  # noqa: E402

ACTFNS = {"relu": torch.nn.ReLU, "softplus": torch.nn.Softplus, "tanh": torch.nn.Tanh}


def main():
    install_stubs()
    sys.path.insert(0, str(REF))
    torch.set_num_threads(8)
    torch.use_deterministic_algorithms(True)

    from turbdiff.models import ddpm as R
    from turbdiff.models.conditioning import Conditioning

    CT = Conditioning.Type.CELL_TYPE
    opt = np.load(OUT / "options.npz")
    base = np.load(OUT / "model_cfg1.npz")
    xs, tv, cs = torch.from_numpy(opt["x"]), torch.from_numpy(opt["t"]), torch.from_numpy(opt["cell_idx"])
    Cs = {CT: torch.from_numpy(opt["c_local"])}

    def make_variant(actfn):  # make_golden.make_variant
        torch.manual_seed(0)
        dm = R.DenoisingModel(in_features=4, out_features=4, c_local_features=4, c_global_features=0, timesteps=10, dim=8,
                              u_net_levels=2, norm_type="group", actfn=actfn)
        gg = torch.Generator().manual_seed(77)
        with torch.no_grad():
            for n, p in dm.named_parameters():
                if ".norm." in n or n.endswith("fn.norm.weight") or n.endswith("fn.norm.bias"):
                    p.add_(0.1 * torch.randn(p.shape, generator=gg))
        return R.GaussianDiffusion(dm, timesteps=10, beta_schedule="log-snr-linear", loss_type="l2", noise_bcs=True)

    gn_ = torch.Generator().manual_seed(4321)
    orig_randn_like = torch.randn_like
    noises = []

    def rec_randn_like(x, **kw):
        noises.append(torch.randn(x.shape, generator=gn_, dtype=x.dtype))
        return noises[-1]

    ax = {}
    for tag, actfn in ACTFNS.items():
        model = make_variant(actfn)
        # the weights equal model_cfg1.npz's `sd/` (no activation has parameters): store only what differs
        for k, v in model.model.state_dict().items():
            key = f"sd/{k}"
            if key not in base.files or base[key].shape != tuple(v.shape) or not np.array_equal(base[key], to_np(v)):
                ax[f"{tag}/sd/{k}"] = to_np(v).astype(np.float32)
        with torch.no_grad():
            ax[f"{tag}/eps_hat"] = to_np(model.model(xs, tv, Cs))
        noises.clear()
        torch.randn_like = rec_randn_like
        try:
            loss, _ = model.p_losses(xs, tv, Cs, SimpleNamespace(cell_idx=cs), None)
        finally:
            torch.randn_like = orig_randn_like
        loss.backward()
        ax[f"{tag}/noise"] = to_np(noises[0])
        ax[f"{tag}/loss"] = to_np(loss)
        for k, p in model.model.named_parameters():
            ax[f"{tag}/gnorm/{k}"] = to_np(p.grad.norm())
            if p.numel() <= 512:
                ax[f"{tag}/grad/{k}"] = to_np(p.grad)
    np.savez_compressed(OUT / "actfn.npz", **ax)
    print({tag: float(ax[f"{tag}/loss"]) for tag in ACTFNS}, sum(1 for k in ax if "/sd/" in k), "weights differ from model_cfg1")


if __name__ == "__main__":
    main()
