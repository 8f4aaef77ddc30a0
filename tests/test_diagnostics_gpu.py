"""The case-diagnostics kernels (csrc/tdx_diagnostics.hip) and turbdiff_amd.data.diagnostics end to end on the GPU, against
the numpy float64 statements of tests/diagnostics_reference.py and the reference scripts' own output in
tests/golden/diagnostics.npz.

Bounds.  Lagged products and squared deviations are sums of N terms that are exact in fp64, so any summation order is within
N 2^-53 sum |terms| of the true value: that bound, computed here, is the tolerance.  A smoothing filter output carries at
most (2 h + 2) 2^-53 of its summed magnitudes, squaring doubles the relative error, and the conditioning kappa <= 100 that
the golden generator asserts turns this into 2 (2 h + 2) 2^-53 kappa < 3e-12 relative, plus the outer sum's N 2^-53: rtol
1e-10.  Against the reference's float32 numbers the distance is the reference's own rounding, which the generator measured
(``f32_gap``): four times that."""

import numpy as np
import pytest
import torch

import diagnostics_cases as DC
import diagnostics_reference as R
import h5fake
from turbdiff_amd.data import diagnostics as D

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    from conftest import GOLDEN

    return np.load(GOLDEN / "diagnostics.npz")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def chunks_of(total, size):
    return [min(size, total - at) for at in range(0, total, size)]


# ------------------------------------------------------------------------------------------------ lagged products
L_TEST = 12


def lag_inputs(n, m, frames, seed):
    """Raw frames with a mean of 1e3 and a fluctuation of 1e-2 in a third of the cells (there the float32 subtraction loses
    bits that a float64 subtraction would keep) and of order one elsewhere; an ascending, gapped cell subset."""
    rng = np.random.default_rng(seed)
    mean = rng.standard_normal((n, 3)).astype(np.float32)
    scale = np.ones((n, 1), dtype=np.float32)
    far = rng.random(n) < 1 / 3
    mean[far] += np.float32(1e3)
    scale[far] = np.float32(1e-2)
    x = (mean[None] + scale[None] * rng.standard_normal((frames, n, 3)).astype(np.float32)).astype(np.float32)
    cells = np.sort(rng.choice(n, size=m, replace=False))
    assert (np.diff(cells) > 1).any() and far[cells].any()
    return x, mean, cells


def run_lagprod(x, mean, cells, plan, max_lag=L_TEST):
    state = D.LagProducts(cells, mean, max_lag, DEV)
    xd, at = dev(x), 0
    for f in plan:
        state.update(xd[at:at + f])
        at += f
    assert at == len(x) and state.seen == len(x)
    return state.result()


@pytest.fixture(scope="module")
def lag_case():
    x, mean, cells = lag_inputs(1031, 347, 40, 5)
    return x, mean, cells, R.lag_products(x, mean, cells, L_TEST)


@pytest.mark.parametrize("plan", [[1] * 40, chunks_of(40, 5), chunks_of(40, 12), chunks_of(40, 16), [40], [3, 16, 1, 13, 7]],
                         ids=["ones", "5", "12=L", "16>L", "40", "mixed"])
def test_lagprod_chunk_plans(lag_case, plan):
    """347 of 1031 cells (3 m = 1041, odd), L = 12, 40 frames: every way of cutting the frames into chunks gives the float64
    statement within the summation bound."""
    x, mean, cells, (want, bound) = lag_case
    got = run_lagprod(x, mean, cells, plan)
    err = np.abs(got - want)
    print(f"lag products, plan {plan[:4]}...: largest error / bound {(err / bound).max():.3e}")
    assert (err <= bound).all()


def test_lagprod_float32_subtraction_is_the_references(lag_case):
    """With the fluctuation formed in float64 instead, lag 0 of these inputs moves by 76 summation bounds (the float32
    difference is rounded wherever x and the mean are not within a factor of two of each other): the test above would see a
    kernel that subtracts in the wrong precision."""
    x, mean, cells, (want, bound) = lag_case
    f64 = (x[:, cells].astype(np.float64) - mean[cells].astype(np.float64)).reshape(len(x), -1)
    assert abs((f64 * f64).sum() - want[0]) > 10 * bound[0]


def test_lagprod_bit_reproducible(lag_case):
    x, mean, cells, _ = lag_case
    a, b = run_lagprod(x, mean, cells, chunks_of(40, 5)), run_lagprod(x, mean, cells, chunks_of(40, 5))
    assert np.array_equal(a, b)


def test_lagprod_many_tiles():
    """4099 cells, all selected but a few: 12 297 columns are 193 column tiles, the last one partial."""
    x, mean, cells = lag_inputs(4099, 4090, 15, 6)
    want, bound = R.lag_products(x, mean, cells, L_TEST)
    got = run_lagprod(x, mean, cells, [7, 8])
    assert (np.abs(got - want) <= bound).all()


def test_lagprod_fewer_frames_than_lags(lag_case):
    """7 frames in all: lags 7 ... 12 never had a partner and are exactly 0."""
    x, mean, cells, _ = lag_case
    want, bound = R.lag_products(x[:7], mean, cells, L_TEST)
    for plan in ([7], [2, 5], [1] * 7):
        got = run_lagprod(x[:7], mean, cells, plan)
        assert (got[7:] == 0.0).all() and (got[:7] != 0.0).all()
        assert (np.abs(got - want) <= bound).all()


def test_lagprod_long_update_is_split():
    """An update of more frames than one kernel call takes (64) is passed in pieces."""
    x, mean, cells = lag_inputs(67, 40, 70, 7)
    want, bound = R.lag_products(x, mean, cells, L_TEST)
    assert (np.abs(run_lagprod(x, mean, cells, [70]) - want) <= bound).all()


# ------------------------------------------------------------------------------------------------ smoothing residual
def run_smooth(x, taps, plan):
    state = D.SmoothResidual(taps, x.shape[1], DEV)
    xd, at = dev(x), 0
    for f in plan:
        state.update(xd[at:at + f])
        at += f
    assert at == len(x) and state.out_frames == len(x) - taps.shape[1] + 1
    return state.result()


def small_taps(rng, W=3, h=3):
    taps = R.residual_filters(np.linspace(1, 2, W), h)
    return taps + 0.01 * rng.standard_normal(taps.shape)  # not symmetric: a flipped filter would be seen


def test_smooth_one_output_frame():
    rng = np.random.default_rng(8)
    x = rng.standard_normal((7, 333)).astype(np.float32)
    taps = small_taps(rng)
    want = R.smooth_energy(x, taps)
    for plan in ([7], [3, 4], [1] * 7):
        np.testing.assert_allclose(run_smooth(x, taps, plan), want, rtol=1e-10, atol=0)


@pytest.mark.parametrize("size", [1, 4, 23])
def test_smooth_small_filter_chunks(size):
    rng = np.random.default_rng(9)
    x = (3.0 + rng.standard_normal((23, 3 * 233))).astype(np.float32)
    taps = small_taps(rng)
    np.testing.assert_allclose(run_smooth(x, taps, chunks_of(23, size)), R.smooth_energy(x, taps), rtol=1e-10, atol=0)


@pytest.fixture(scope="module")
def smooth_case():
    rng = np.random.default_rng(10)
    x = DC.ar1_field(rng, 137, 233).reshape(137, 3 * 233)
    taps = R.residual_filters()
    assert R.smooth_conditioning(x, taps).max() <= 100
    return x, taps, R.smooth_energy(x, taps)


@pytest.mark.parametrize("size", [10, 16, 137])
def test_smooth_full_filter_bank(smooth_case, size):
    """h = 50, 32 widths, 137 frames of 699 columns (11 column tiles, the last one partial): with chunks of 10 the window
    spans 11 chunks; 137 in one update is passed to the kernel in pieces of 64."""
    x, taps, want = smooth_case
    got = run_smooth(x, taps, chunks_of(137, size))
    print(f"smoothing, chunks of {size}: largest relative error {np.abs(got / want - 1).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=0)


def test_smooth_bit_reproducible(smooth_case):
    x, taps, _ = smooth_case
    assert np.array_equal(run_smooth(x, taps, chunks_of(137, 10)), run_smooth(x, taps, chunks_of(137, 10)))


def test_smooth_identity_filter():
    """taps = delta: the energy of the centre frames themselves; a second filter of zeros gives exactly 0."""
    rng = np.random.default_rng(11)
    x = rng.standard_normal((12, 130)).astype(np.float32)
    taps = np.zeros((2, 7))
    taps[0, 3] = 1.0
    got = run_smooth(x, taps, [5, 7])
    centre = x[3:-3].astype(np.float64)
    want = (centre * centre).sum()
    assert abs(got[0] - want) <= centre.size * R.U53 * want and got[1] == 0.0


# ------------------------------------------------------------------------------------------------ squared deviation
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("n", [1031, 4099])
@pytest.mark.parametrize("T", [1, 11])
def test_sqdev_sum(C, n, T):
    rng = np.random.default_rng(100 * C + T)
    mean = (5.0 * rng.standard_normal((n, C))).astype(np.float32)
    x = (mean[None] + rng.standard_normal((T, n, C)).astype(np.float32)).astype(np.float32)
    x[:, 7] = mean[7]  # a cell that sits on the mean adds exactly nothing
    if C == 1:
        x, mean = x[..., 0], mean[..., 0]
    want, bound = R.sqdev(x, mean)
    got = D.sqdev_sum(dev(x), dev(mean))
    assert abs(got.item() - want) <= bound
    again = D.sqdev_sum(dev(x), dev(mean), got.clone())  # added to a running total
    assert abs(again.item() - 2 * want) <= 2 * bound + R.U53 * 2 * want
    only = np.ascontiguousarray(x[:, 7:8])
    assert D.sqdev_sum(dev(only), dev(mean[7:8])).item() == 0.0


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("chunk", [10, 33])
def test_autocorrelation_end_to_end(gold, tmp_path, chunk):
    case = DC.case_dir(tmp_path, "autocorr")
    tree = DC.autocorr_case(case / "data.h5")
    DC.install_mean_flow(case, gold["autocorr/mean_flow_u"])
    res = D.autocorrelation(case, chunk_frames=chunk, opener=h5fake.File, device=DEV)
    assert res.decorrelation_steps == int(gold["autocorr/decorrelation_steps"])
    gap = float(gold["autocorr/f32_gap"])
    err = np.abs(res.corrcoeff - gold["autocorr/corrcoeff"]).max()
    print(f"autocorrelation, chunks of {chunk}: largest distance to the reference {err:.3e}, float32 gap {gap:.3e}")
    assert err <= 4 * gap
    # and the float64 statement, within the summation bound carried through the division by lag 0
    u = np.array(tree["data/u"])
    back = R.back_positions(np.array(tree["grid/cell_idx"]), np.array(tree["grid/cell_counts"]))
    want, bound = R.lag_products(u[len(u) // 2:], gold["autocorr/mean_flow_u"], back, 200)
    tol = bound / want[0] + np.abs(want) / want[0] * (bound[0] / want[0]) + 4 * R.U53
    assert (np.abs(res.corrcoeff - want / want[0]) <= tol).all()
    assert res.max_decorrelated_coeff == np.abs(res.corrcoeff[-100:]).max()
    with np.load(case / "autocorrelation.npz") as z:
        assert sorted(z.files) == ["corrcoeff", "decorrelation_steps"]
        assert z["corrcoeff"].dtype == np.float64 and np.array_equal(z["corrcoeff"], res.corrcoeff)
        assert z["decorrelation_steps"].shape == () and int(z["decorrelation_steps"]) == res.decorrelation_steps


@pytest.mark.parametrize("chunk", [10, 16])
def test_smoothing_error_end_to_end(gold, tmp_path, chunk):
    case = DC.case_dir(tmp_path, "smooth")
    tree = DC.smooth_case(case / "data.h5")
    got = D.smoothing_error(case, chunk_frames=chunk, opener=h5fake.File, device=DEV)
    assert got.shape == (32,) and got.dtype == np.float64
    np.testing.assert_allclose(got, gold["smooth/mses"], rtol=1e-10, atol=0)
    late = np.array(tree["data/u"])[DC.SMOOTH_EARLY:]
    want = R.smooth_energy(late.reshape(len(late), -1), R.residual_filters()) / (late.shape[1] * (len(late) - 100))
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=0)
    assert np.array_equal(np.loadtxt(case / "gaussian-smoothing-error.txt"), got)


@pytest.mark.parametrize("chunk", [10, 5])
def test_mean_forecast_error_end_to_end(gold, tmp_path, chunk):
    train, test = DC.forecast_cases(tmp_path)
    DC.install_mean_flow(train, gold["forecast/mean_flow_u"], gold["forecast/mean_flow_p"])
    got = D.mean_forecast_error(test, train, chunk_frames=chunk, opener=h5fake.File, device=DEV)
    assert sorted(got) == ["p", "u"] and all(isinstance(v, float) for v in got.values())
    for name in ("u", "p"):
        ref, gap = float(gold[f"forecast/{name}"]), float(gold[f"forecast/f32_gap_{name}"])
        print(f"mean forecast {name}, chunks of {chunk}: {got[name]!r}, reference {ref!r}, float32 gap {gap:.3e}")
        assert abs(got[name] - ref) <= 4 * gap
        x = np.array(h5fake.TREES[str(test / "data.h5")][f"data/{name}"])
        want, bound = R.sqdev(x, gold[f"forecast/mean_flow_{name}"])
        assert abs(got[name] - want / np.prod(x.shape[:-1])) <= (bound + 2 * R.U53 * want) / np.prod(x.shape[:-1])
    # the command's walk over the same tree
    import importlib.util
    import json
    from pathlib import Path

    spec = importlib.util.spec_from_file_location("case_diagnostics", Path(__file__).resolve().parent.parent / "tools" / "case_diagnostics.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    table = tool.forecast_walk(tmp_path, tmp_path / "table.json", chunk_frames=chunk, opener=h5fake.File, device=DEV)
    assert table == {DC.FORECAST_INFLOW: {DC.FORECAST_DIMS[0]: got}} == json.loads((tmp_path / "table.json").read_text())
