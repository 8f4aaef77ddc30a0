"""Flow decomposition without a GPU: the float64 backward restatement of tests/flow_decompose_cases.py (the derivation
csrc/tdx_flow_decompose.hip is written from) against autograd through the float64 forward restatement, the forward
restatement against LES.decompose on the CPU, and what the restated tile rule says about the multi-tile test grid."""

import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import flow_decompose_cases as FC  # noqa: E402


def _draw(T, L, Fn, grid, B=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = T - L + 1
    xx = torch.randn(B, T, Fn, *grid, generator=g, dtype=torch.float64)
    S = torch.randn(3, 3, 3, generator=g, dtype=torch.float64) / 27 ** 0.5
    w = torch.randn(L, generator=g, dtype=torch.float64) / L ** 0.5
    grads = [torch.randn(B, n, Fn, *grid, generator=g, dtype=torch.float64) for _ in range(3)]
    return xx, S, w, grads


@pytest.mark.parametrize("T,L,Fn", [(6, 4, 4), (6, 1, 3)])
def test_backward_restatement_against_autograd(T, L, Fn):
    xx, S, w, grads = _draw(T, L, Fn, FC.HOST_GRID, seed=T + L)
    leaves = [t.clone().requires_grad_() for t in (xx, S, w)]
    want = torch.autograd.grad(FC.decompose_ref(*leaves), leaves, grads)
    got = FC.decompose_bwd_ref(xx.numpy(), S.numpy(), w.numpy(), *(g.numpy() for g in grads))
    for name, a, b in zip(("gxx", "dS", "dw"), got, want):
        b = b.numpy()
        assert a.shape == b.shape, name
        err = np.abs(a - b).max() / np.abs(b).max()
        print(f"FLD host {(T, L, Fn)} {name}: max error / max |ref| = {err:.3e}")
        assert err <= 1e-11, (name, err)


def test_forward_restatement_is_les_decompose():
    from turbdiff_amd.models.tfnet import LES

    m = LES(n_features=4, c_local_features=8, c_global_features=0, context_window=6, kernel_size=3, dropout_rate=0,
            temporal_filtering_length=4)
    with torch.no_grad():
        m.spatial_filter.weight.normal_(0, 27 ** -0.5)
        m.temporal_filter.weight.normal_(0, 0.5)
    xx, _, _, _ = _draw(6, 4, 4, FC.HOST_GRID, seed=3)
    want = m.decompose(xx.float())  # float32 arithmetic on the CPU
    got = FC.decompose_ref(xx.float(), m.spatial_filter.weight.detach().float().reshape(3, 3, 3), m.temporal_filter.weight.detach().float())
    for a, b in zip(got, want):
        assert a.flatten(1, 2).shape == b.shape
        assert (a.flatten(1, 2) - b.double()).norm() / a.norm() < 1e-5
    packed = FC.to_nvc(got[0])
    assert packed.shape == (2, *FC.HOST_GRID, 16) and torch.all(packed[..., 12:] == 0)
    assert torch.equal(FC.from_nvc(packed, 3, 4), got[0])
    assert torch.equal(packed[1, 2, 3, 4, 2 * 4 + 1], got[0][1, 2, 1, 2, 3, 4])  # channel t' F + f


def test_multi_tile_grid_by_the_restated_rule():
    g = FC.tile_geometry(FC.MULTI_GRID, B=2)
    assert all(n >= 2 for n in g.tiles), g
    assert all(0 < r < t for r, t in zip(g.remainder, FC.TILE)), g  # a ragged last tile along every tiled axis
    assert g.blocks == 2 * g.tiles[0] * g.tiles[1] * g.tiles[2] > 1
    assert FC.tile_geometry((1, 1, 1)).blocks == 1 and FC.tile_geometry(FC.HOST_GRID).tiles == (2, 2, 1)
    assert FC.tile_geometry(FC.FIXTURE_GRID).tiles == (9, 5, 2)
    for T, L, Fn in FC.CONFIGS:
        assert FC.supported(2, T, L, Fn, FC.MULTI_GRID)
    assert not FC.supported(1, 9, 1, 1, (3, 3, 3)) and not FC.supported(1, 2, 1, 9, (3, 3, 3)) and not FC.supported(1, 8, 1, 5, (3, 3, 3))
    # no bound on B (past GRID_Y the samples continue along the launch's z axis); the bounds on the grid: V < 2^31, and
    # tiles x 256 threads < 2^32 along the launch's x axis
    assert FC.supported(FC.GRID_Y + 1, 1, 1, 1, (1, 1, 1)) and FC.supported(2**31 - 1, 1, 1, 1, (1, 1, 1))
    assert FC.supported(1, 1, 1, 1, (1024, 1024, 2047)) and not FC.supported(1, 1, 1, 1, (1024, 1024, 2048))  # V = 2^31
    assert FC.supported(1, 1, 1, 1, (1, 1, 2**28 - 16)) and not FC.supported(1, 1, 1, 1, (1, 1, 2**28))  # 2^24 tiles, V = 2^28
    assert FC.tile_geometry((1024, 1024, 2047)).blocks == 2**23  # a grid of full tiles stays far below the tile bound


def test_cpu_tensors_are_refused_before_any_library_call(monkeypatch):
    """LES.forward never reaches the kernels' entry on CPU tensors: flow_decompose_supported says no before any library
    call (the rest of the network then refuses the CPU tensor, as before)."""
    from turbdiff_amd import ops

    xx = torch.randn(1, 6, 4, 3, 3, 3)
    S, w = torch.randn(1, 1, 3, 3, 3), torch.randn(1, 4, 1, 1, 1)
    monkeypatch.setattr(ops.L, "query", lambda *a: pytest.fail("library queried for a CPU tensor"))
    assert not ops.flow_decompose_supported(xx, S, w, torch.float32)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.flow_decompose(xx, S, w, torch.float32)


class _Captured(Exception):
    pass


@pytest.mark.parametrize("on", [False, True], ids=["off", "on"])
def test_the_switch_chooses_the_route(on, monkeypatch):
    """LES.forward with a call the op would take (flow_decompose_supported patched to say so: no GPU here).  Off: neither
    ops function is touched, and the encoders get decompose() + _to_nvc_padded, equal to the float64 restatement.  On: the
    op is asked, once, and its three results go to the encoders as they are."""
    from turbdiff_amd import ops
    from turbdiff_amd.models import tfnet

    m = tfnet.LES(n_features=4, c_local_features=8, c_global_features=0, context_window=6, kernel_size=3, dropout_rate=0,
                  temporal_filtering_length=4)
    xx, _, _, _ = _draw(6, 4, 4, FC.HOST_GRID, seed=5)
    xx = xx.float()
    asked, marks, seen = [], tuple(torch.full((1,), float(i)) for i in range(3)), []

    def record(self, x, c_enc=None, add4=None):
        seen.append(x)
        if len(seen) == 3:
            raise _Captured
        return x, x, x, x

    monkeypatch.setattr(tfnet, "FUSE_DECOMPOSE", on)
    monkeypatch.setattr(tfnet.Encoder, "forward", record)
    monkeypatch.setattr(ops, "flow_decompose_supported", lambda *a: asked.append("supported") or True)
    monkeypatch.setattr(ops, "flow_decompose", lambda *a: asked.append("op") or marks)
    with pytest.raises(_Captured), torch.no_grad():
        m(xx, {}, dtype=torch.float32)
    if on:
        assert asked == ["supported", "op"] and all(a is b for a, b in zip(seen, marks))
        return
    assert asked == []
    want = FC.decompose_ref(xx, m.spatial_filter.weight.detach().reshape(3, 3, 3), m.temporal_filter.weight.detach())
    for got, ref in zip(seen, want):
        assert got.shape == (2, *FC.HOST_GRID, 16) and got.dtype == torch.float32
        assert (got - FC.to_nvc(ref)).norm() / ref.norm() < 1e-5
