"""Host side of the case diagnostics (turbdiff_amd/data/diagnostics.py, tools/case_diagnostics.py) without a GPU: filter taps,
the decorrelation rule, the cell selection, the argument checks that come before any kernel, the command's parser and the
forecast table's layout, and the binding of the new kernels."""

import importlib.util
import json
import re
from pathlib import Path

import numpy as np
import pytest

import diagnostics_cases as DC
import diagnostics_reference as R
import h5fake
from turbdiff_amd import _lib
from turbdiff_amd.data import diagnostics as D

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("case_diagnostics", ROOT / "tools" / "case_diagnostics.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_taps_are_the_reference_expression():
    """All 32 widths, bit for bit, and symmetric (so that np.convolve's flip does not matter)."""
    g = D.gaussian_taps()
    assert g.shape == (32, 101) and g.dtype == np.float64
    for row, kernel_width in zip(g, np.linspace(1, 32, 32)):
        kernel = np.exp(-np.linspace(-50, 50, 101) ** 2 / (2 * kernel_width**2))
        kernel /= kernel.sum()
        assert np.array_equal(row, kernel)
        assert np.array_equal(row, row[::-1])
    r = D.residual_taps()
    assert np.array_equal(r, R.residual_filters())
    centre = np.zeros(101)
    centre[50] = 1.0
    assert np.array_equal(r, centre[None] - g) and np.array_equal(r, r[:, ::-1])
    assert np.abs(r.sum(axis=1)).max() < 1e-15  # a constant signal leaves no residual
    small = D.residual_taps(np.array([1.0, 2.5]), 3)
    assert small.shape == (2, 7) and np.array_equal(small, R.residual_filters(np.array([1.0, 2.5]), 3))


def test_decorrelation_rule():
    c = np.concatenate(([1.0, 0.6, -0.3, 0.1, -0.04], 0.01 * np.array([1, -2, 3, -5, 4, 2])))
    steps, threshold = D.decorrelation(c, tail=6)
    assert threshold == 0.05 and steps == 5  # |c[4]| = 0.04 is the first at or below 0.05
    assert D.decorrelation(-c, tail=6) == (5, 0.05)  # magnitudes decide
    c[4] = -0.05
    assert D.decorrelation(c, tail=6)[0] == 5  # at the threshold counts
    # nothing before the tail qualifies: the first qualifying index lies inside the tail (its own maximum)
    c = np.array([1.0, 0.9, 0.8, 0.2, 0.7, 0.3])
    assert D.decorrelation(c, tail=2) == (4, 0.7)
    c = np.array([1.0, 0.9, 0.8, 0.1, 0.7, 0.3])
    assert D.decorrelation(c, tail=3) == (4, 0.7)  # index 3 is in the tail and below its maximum
    assert D.decorrelation(np.array([1.0, 0.5]), tail=2) == (1, 1.0)
    with pytest.raises(ValueError):
        D.decorrelation(c, tail=7)


def test_decorrelation_rule_on_the_reference_output():
    from conftest import GOLDEN

    gold = np.load(GOLDEN / "diagnostics.npz")
    steps, threshold = D.decorrelation(gold["autocorr/corrcoeff"], 100)
    assert steps == int(gold["autocorr/decorrelation_steps"]) and threshold == np.abs(gold["autocorr/corrcoeff"][-100:]).max()
    assert float(gold["autocorr/margin"]) >= 100 * float(gold["autocorr/f32_gap"])
    assert gold["smooth/kappa"].max() <= 100


@pytest.mark.parametrize("counts", [DC.AUTOCORR_COUNTS, (9, 7, 6)])
def test_back_cells(counts):
    """14 x 6 x 5: x >= 8, 180 of 412 cells, clear of the hole; 7 x 5 x 4: x >= 2, a region the hole cuts into."""
    from turbdiff_amd.data.ofles import OpenFOAMDataRepository

    path = f"/fake-back-{counts[0]}/data.h5"
    h5fake.TREES[path] = tree = h5fake.make_case(3, counts=counts)
    meta = OpenFOAMDataRepository([path], (), opener=h5fake.File).read_metadata(0)
    got = D.back_cells(meta.unpadded_cell_idx.numpy(), meta.unpadded_cell_counts)
    want = R.back_positions(np.array(tree["grid/cell_idx"]), counts)
    assert np.array_equal(got, want) and (np.diff(got) > 0).all()
    assert 0 < len(got) < meta.n_cells
    X, Y, Z = (c - 2 for c in counts)
    x = np.array(tree["grid/cell_idx"])[got] // (counts[1] * counts[2]) - 1
    assert x.min() == X - max(Y, Z) and x.max() == X - 1
    if counts == DC.AUTOCORR_COUNTS:
        assert len(got) == 180 and meta.n_cells == 412


def test_too_few_frames_for_the_lags(tmp_path):
    """11 frames, 6 in the second half: lags up to 200 cannot be formed; the check comes before anything touches the GPU."""
    case = DC.case_dir(tmp_path, "short")
    h5fake.TREES[str(case / "data.h5")] = tree = h5fake.make_case(4)
    DC.install_mean_flow(case, np.zeros(tree["data/u"].shape[1:], dtype=np.float32))
    with pytest.raises(ValueError, match="second half"):
        D.autocorrelation(case, opener=h5fake.File, device="cpu")
    with pytest.raises(ValueError, match="tail"):
        D.autocorrelation(case, max_lag=5, tail=7, opener=h5fake.File, device="cpu")


def test_missing_mean_flow_names_the_function_that_writes_it(tmp_path):
    case = DC.case_dir(tmp_path, "nomean")
    h5fake.TREES[str(case / "data.h5")] = h5fake.make_case(4)
    with pytest.raises(FileNotFoundError, match=r"prepare\.mean_flow"):
        D.autocorrelation(case, opener=h5fake.File, device="cpu")
    with pytest.raises(FileNotFoundError, match=r"prepare\.mean_flow"):
        D.mean_forecast_error(case, opener=h5fake.File, device="cpu")


def test_too_few_frames_for_a_window(tmp_path):
    case = DC.case_dir(tmp_path, "short")
    h5fake.TREES[str(case / "data.h5")] = h5fake.make_case(4)  # 11 frames, 10 of them after 0.025
    with pytest.raises(ValueError, match="window needs 101"):
        D.smoothing_error(case, opener=h5fake.File, device="cpu")
    with pytest.raises(ValueError, match="window needs 11"):
        D.smoothing_error(case, half_width=5, opener=h5fake.File, device="cpu")


def test_mismatched_cell_counts(tmp_path):
    a, b = DC.case_dir(tmp_path, "a"), DC.case_dir(tmp_path, "b")
    h5fake.TREES[str(a / "data.h5")] = h5fake.make_case(4)
    DC.install_mean_flow(b, np.zeros((77, 3), dtype=np.float32), np.zeros(77, dtype=np.float32))
    with pytest.raises(ValueError, match="cells"):
        D.mean_forecast_error(a, b, opener=h5fake.File, device="cpu")


def test_state_argument_checks():
    mean = np.zeros((10, 3), dtype=np.float32)
    for cells in ([3, 2], [1, 1], [0, 10], [-1, 2], []):
        with pytest.raises(ValueError):
            D.LagProducts(np.array(cells, dtype=np.int64), mean, 4, "cpu")
    for lag in (0, 256):
        with pytest.raises(ValueError):
            D.LagProducts(np.array([1, 2]), mean, lag, "cpu")
    with pytest.raises(RuntimeError):
        D.LagProducts(np.array([1, 2]), mean.astype(np.float64), 4, "cpu")
    for shape in ((33, 7), (2, 6), (2, 103), (7,)):
        with pytest.raises(ValueError):
            D.SmoothResidual(np.zeros(shape), 5, "cpu")


def test_tool_parser(tool):
    ap = tool.parser()
    a = ap.parse_args(["/data/case"])
    assert (a.case, a.only, a.mean_case, a.discard_first, a.chunk_size, a.forecast_root) == ("/data/case", None, None, 0.025, 10, None)
    a = ap.parse_args(["/data/case", "--only", "smoothing-error", "--discard-first", "0.1", "--chunk-size", "4", "--mean-case", "/m"])
    assert (a.only, a.discard_first, a.chunk_size, a.mean_case) == ("smoothing-error", 0.1, 4, "/m")
    assert tool.DIAGNOSTICS == ("autocorrelation", "smoothing-error", "mean-forecast-error")
    with pytest.raises(SystemExit):
        ap.parse_args(["/data/case", "--only", "regions"])
    a = ap.parse_args(["--forecast-root", "/data", "out.json"])
    assert a.forecast_root == "/data" and a.case == "out.json"
    with pytest.raises(SystemExit):
        ap.parse_args([])


def test_forecast_walk_json_layout(tool, tmp_path):
    """The walk over inflow-*/<d>D directories and the merge into an existing table, with the kernels' part replaced by a
    recorded stand-in: layout and keys are those of scripts/mean-forecast-errors.py:28-49 (json turns the dims into strings)."""
    for d in ("inflow-const/3D", "inflow-const/2D-wide", "inflow-sine/3D", "other/3D"):
        (tmp_path / d / "train" / "high-step").mkdir(parents=True)
        (tmp_path / d / "test" / "high-step").mkdir(parents=True)
    calls = []

    def fake_error(data_case, mean_case, **kwargs):
        calls.append((Path(data_case).relative_to(tmp_path).as_posix(), Path(mean_case).relative_to(tmp_path).as_posix()))
        return {"u": float(len(calls)), "p": 10.0 * len(calls)}

    out = tmp_path / "table.json"
    out.write_text(json.dumps({"old": {"3": {"u": 1.5, "p": 2.5}}, "const": {"3": {"u": -1.0, "p": -1.0}}}))
    table = tool.forecast_walk(tmp_path, out, error=fake_error)
    assert calls == [("inflow-const/2D-wide/test/high-step", "inflow-const/2D-wide/train/high-step"),
                     ("inflow-const/3D/test/high-step", "inflow-const/3D/train/high-step"),
                     ("inflow-sine/3D/test/high-step", "inflow-sine/3D/train/high-step")]
    stored = json.loads(out.read_text())
    assert stored == json.loads(json.dumps(table))
    assert stored == {"old": {"3": {"u": 1.5, "p": 2.5}},
                      "const": {"3": {"u": 2.0, "p": 20.0}, "2": {"u": 1.0, "p": 10.0}},
                      "sine": {"3": {"u": 3.0, "p": 30.0}}}


def test_every_new_header_symbol_is_bound():
    header = (ROOT / "include" / "tdx.h").read_text()
    section = header.split("case diagnostics ------ */")[1].split("/* Counter-based")[0]
    names = set(re.findall(r"\b(tdx_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", section, flags=re.S)))
    assert names == {"tdx_lagprod_workspace_bytes", "tdx_lagprod_update", "tdx_smooth_residual_workspace_bytes",
                     "tdx_smooth_residual_update", "tdx_sqdev_workspace_bytes", "tdx_sqdev_sum", "tdx_fma64_probe"}
    for name in names:
        assert name in _lib.SIGNATURES
    decl = re.search(r"int tdx_lagprod_update\((.*?)\);", section, flags=re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["tdx_lagprod_update"][1]) == 12
    decl = re.search(r"int tdx_smooth_residual_update\((.*?)\);", section, flags=re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["tdx_smooth_residual_update"][1]) == 11
    decl = re.search(r"int tdx_sqdev_sum\((.*?)\);", section, flags=re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["tdx_sqdev_sum"][1]) == 9
