"""TF-Net, host side: the LES module schema against the manifest the reference wrote (tests/golden/tfnet.npz), its
re-initialisation, strict loading of a recipe state dict, TFNetTrainer.from_config, the fixture recipe, the restated grid
rule of the BatchNorm kernels, and the float64 restatement of the BatchNorm tail (tests/tfnet_cases.py) against torch's own
F.batch_norm + F.leaky_relu autograd in float64."""

import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import tfnet_cases as TC  # noqa: E402

G = TC.load_fixture()
TFNET_YAML = dict(name="tfnet", batch_size=8, eval_batch_size=16, context_window=6, unroll_steps=4, eval_unroll_steps=30,
                  sample_steps=[], main_sample_step=-1, monitor="val/loss", normalization_mode="u:norm-max;p:abs-max",
                  variables="u,p", cell_type_features=True, cell_type_embedding_type="learned", cell_type_embedding_dim=8,
                  cell_pos_features=False, temporal_filtering_length=4, learning_rate="1e-3", dropout_rate=0.0, kernel_size=3,
                  compute_expensive_sample_metrics=True, shapes_data="shapes-seq", shapes_batch_size=6,
                  shapes_eval_batch_size=4, shapes_max_epochs=2, shapes_discard_first=-1)


def _les():
    from turbdiff_amd.models.tfnet import LES

    return LES(**TC.MODEL_KW)


def test_state_dict_manifest_matches_reference():
    sd = _les().state_dict()
    assert list(sd.keys()) == [str(k) for k in G["manifest/keys"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in G["manifest/shapes"]]
    assert len(sd) == 117 and sum(p.numel() for p in _les().parameters()) == 25_192_579


def test_reinitialisation_statistics():
    torch.manual_seed(3)
    m = _les()
    for enc in m.encoders:
        w = enc.conv1[0].weight  # 64 x 12 x 27 = 20736 draws of N(0, 0.002 / (3 * 3 * 64))
        sigma = 0.002 / (3 * 3 * 64)
        assert abs(w.std().item() / sigma - 1) < 5 / (2 * w.numel()) ** 0.5  # five standard errors of a sample std
        assert abs(w.mean().item()) < 5 * sigma / w.numel() ** 0.5
        for blk in (enc.conv1, enc.conv1_local, enc.conv2, enc.conv3, enc.conv4):
            assert torch.all(blk[0].bias == 0) and torch.all(blk[1].weight == 1) and torch.all(blk[1].bias == 0)
    # outside the encoders the reference keeps torch's default initialisation
    assert m.deconv3[0].weight.std().item() > 1e-3 and m.spatial_filter.bias is None and m.temporal_filter.bias is None


def test_recipe_state_dict_loads_strictly_and_is_reproducible():
    m = _les()
    man = TC.manifest_of(m.state_dict())
    sd = TC.recipe_state_dict(man)
    m.load_state_dict(sd, strict=True)
    again = TC.recipe_state_dict(man)
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    assert sd["encoder_bar.conv1.1.num_batches_tracked"].dtype == torch.int64
    w = sd["encoder_tilde.conv3.0.weight"]
    assert abs(w.std().item() * (128 * 27) ** 0.5 - 1) < 0.01
    assert 0.5 <= sd["encoder_bar.conv2.1.running_var"].min() and sd["encoder_bar.conv2.1.weight"].max() <= 1.5
    xx, c, dy = TC.recipe_inputs()
    assert xx.shape == (2, 6, 4, 34, 18, 17) and c.shape == (8, 34, 18, 17) and dy.shape == (2, 4, 34, 18, 17)
    idx = TC.grad_sample_index(5, 100000)
    assert len(idx) == len(set(idx.tolist())) == TC.GRAD_SAMPLES and idx.max() < 100000


def test_fixture_files_stay_small_and_hold_the_reference_errors():
    for name in TC.FIXTURE_FILES:
        assert (TC.GOLDEN / name).stat().st_size < 1 << 20, name
    assert G["train/y"].shape == (2, 4, 34, 18, 17) and G["train/dx"].shape == (2, 6, 4, 17, 9, 9)
    assert G["train/y"].dtype == np.float64
    # the reference's own float32 run against its float64 run
    assert 1e-7 < float(G["ref32_err/train/y"]) < 2e-6 and 1e-7 < float(G["ref32_err/eval/y"]) < 2e-6
    assert float(G["ref32_err/train/grad/encoder_bar.conv2.0.bias"]) > 1e3  # rounding noise: never compared relatively
    assert int(G["train/sd/encoder_bar.conv1_local.1.num_batches_tracked"]) == 1


def test_decompose_matches_its_definition_in_float64():
    """tfnet.py:304-337 written out with F.conv3d and unfold in float64 against LES.decompose (float32)."""
    m = _les()
    m.load_state_dict(TC.recipe_state_dict(TC.manifest_of(m.state_dict())), strict=True)
    xx = torch.randn(2, 6, 4, 7, 5, 6, generator=torch.Generator().manual_seed(1))
    bar, tilde, prime = m.decompose(xx)
    x = xx.double()
    star = F.conv3d(x.reshape(-1, 1, 7, 5, 6), m.spatial_filter.weight.double(), padding=1).reshape(x.shape)
    win = star.unfold(1, 4, 1)  # (B, 3, F, X, Y, Z, 4)
    rbar = (win * m.temporal_filter.weight.double().reshape(4)).sum(-1)
    for got, ref in ((bar, rbar), (tilde, star[:, -3:] - rbar), (prime, (x - star)[:, -3:])):
        assert got.shape == (2, 12, 7, 5, 6)
        assert ((got.double() - ref.flatten(1, 2)).norm() / ref.norm()).item() < 1e-6


def test_from_config_and_the_other_trainers_still_refuse_tfnet():
    from turbdiff_amd.models.tfnet import LES
    from turbdiff_amd.regression import DilResNetTrainer, TFNetTrainer
    from turbdiff_amd.training import DiffusionTrainer

    t = TFNetTrainer.from_config(TFNET_YAML)
    assert isinstance(t.model, LES) and t.learning_rate == 1e-3 and t.dropout_rate == 0.0
    assert (t.context_window, t.unroll_steps, t.eval_unroll_steps, t.temporal_filtering_length) == (6, 4, 30, 4)
    assert t.model.encoder_bar.conv1[0].in_channels == 12 and t.model.encoder_bar.conv1_local[0].in_channels == 8
    assert t.compute_mode == "f32" and t.gradient_clip_val is None
    assert set(TFNetTrainer.CONFIG_KEYS) <= set(TFNET_YAML)
    root = dict(model=TFNET_YAML, data=dict(root="/data/shapes"), trainer=dict(gradient_clip_val=0.1), samples_root="/s")
    t = TFNetTrainer.from_config(root, compute_mode="bf16")
    assert t.compute_mode == "bf16" and t.gradient_clip_val == 0.1 and t.data_dir == Path("/data/shapes/data")
    opt = t.configure_optimizers()
    assert isinstance(opt, torch.optim.Adam) and opt.param_groups[0]["lr"] == 1e-3
    with pytest.raises(ValueError):
        TFNetTrainer.from_config({**TFNET_YAML, "name": "dilresnet"})
    with pytest.raises(ValueError):
        TFNetTrainer.from_config(TFNET_YAML, compute_mode="fp16")
    with pytest.raises(ValueError):
        DilResNetTrainer.from_config(TFNET_YAML, max_train_steps=1)
    with pytest.raises(ValueError):
        DiffusionTrainer.from_config(TFNET_YAML)
    # the model's state dict inside the task is the reference's, prefixed
    keys = [k[len("model."):] for k in t.state_dict() if k.startswith("model.")]
    assert keys == [str(k) for k in G["manifest/keys"]]
    assert list(t.state_dict().keys()) == [str(k) for k in G["trainer/sd_keys"]]


def test_global_conditioning_is_an_error():
    class _Global:
        local, global_ = False, True

    with pytest.raises(RuntimeError, match="Global conditioning not implemented for TFNet"):
        _les().encode_conditioning({_Global(): torch.zeros(3, 2, 2, 2)}, torch.float32)


def test_restated_grid_rule():
    """The cases of the GPU tests, by the launcher's rule: which are one block, which span several with a ragged end."""
    assert TC.bn_geometry(2, 8).blocks == 1 and TC.bn_geometry(24, 512).blocks == 2
    g = TC.bn_geometry(459, 64)   # 32 rows per block step, 128 per four-in-flight trip
    assert (g.blocks, g.rows, g.ragged) == (4, 32, True)
    g = TC.bn_geometry(5003, 24)  # C / 8 = 3 does not divide 256: one spare thread
    assert g.spare == 1 and g.blocks == 15 and g.ragged and g.full_trips == 0 and g.tail_rows == 3
    g = TC.bn_geometry(2 * 40000, 64, slabs=2)  # a batch-broadcast add: one slab per sample
    assert g.blocks == 313 and g.ragged


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("add_mode", ["none", "same", "bcast"])
def test_float64_restatement_against_torch_autograd(training, add_mode):
    g = torch.Generator().manual_seed(11)
    B, V, Cc = 2, (3, 2, 4), 16
    x = torch.randn(B, *V, Cc, generator=g, dtype=torch.float64).requires_grad_()
    gamma = (torch.rand(Cc, generator=g, dtype=torch.float64) + 0.5).requires_grad_()
    beta = torch.randn(Cc, generator=g, dtype=torch.float64).requires_grad_()
    add = None
    if add_mode != "none":
        add = torch.randn(B if add_mode == "same" else 1, *V, Cc, generator=g, dtype=torch.float64).requires_grad_()
    rm, rv = torch.randn(Cc, generator=g, dtype=torch.float64) * 0.1, torch.rand(Cc, generator=g, dtype=torch.float64) + 0.5
    dy = torch.randn(B, *V, Cc, generator=g, dtype=torch.float64)
    leaves = [t for t in (x, gamma, beta, add) if t is not None]

    y, mean, var = TC.bn_act_ref(x, gamma, beta, TC.SLOPE, add, training, (rm, rv))
    got = torch.autograd.grad(y, leaves, dy)
    rm_t, rv_t = rm.clone(), rv.clone()
    yt = F.leaky_relu(F.batch_norm(x.reshape(-1, Cc), rm_t, rv_t, gamma, beta, training, 0.1, 1e-5), TC.SLOPE).reshape(x.shape)
    if add is not None:
        yt = yt + add
    ref = torch.autograd.grad(yt, leaves, dy)
    assert torch.allclose(y, yt, rtol=1e-12, atol=1e-12)
    for a, b in zip(got, ref):
        assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-10, atol=1e-11)
    if training:
        rows = x.numel() // Cc
        um, uv = TC.running_update(rm, rv, mean, var, rows)
        assert torch.allclose(um, rm_t, rtol=1e-12) and torch.allclose(uv, rv_t, rtol=1e-12)
