#!/usr/bin/env python3
"""Generate tests/golden/diagnostics.npz by running the *reference's* per-case diagnostic scripts (build container only).

scripts/autocorrelation.py, gaussian-smoothing-error.py and mean-forecast-errors.py are run unmodified with ``runpy`` on the
seeded case files of tests/diagnostics_cases.py; the mean flow they read is made by the reference's own scripts/mean-flow.py.
``h5py`` is replaced by tests/h5fake.py -- behind the views below, which add the boolean row mask that
gaussian-smoothing-error.py indexes with -- and ``tqdm`` by a pass-through if it is not installed.  Only numbers are stored.

    python tests/golden/make_golden_diagnostics.py

Contents: ``autocorr/{corrcoeff, decorrelation_steps, mean_flow_u, f32_gap, margin}``; ``smooth/{mses, kappa}``;
``forecast/{u, p, mean_flow_u, mean_flow_p, f32_gap_u, f32_gap_p}``.  ``f32_gap`` is the distance of the reference's float32
result to a float64 evaluation of the same float32 inputs: the tests allow four times that against the reference's numbers.
The generator asserts on the reference's own output that the coefficients deciding the decorrelation step count keep at least
100 gaps from the threshold, and that the smoothing residual's conditioning stays below 100 for every width.
"""

import json
import runpy
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import diagnostics_cases as DC  # noqa: E402
import diagnostics_reference as R  # noqa: E402
import h5fake  # noqa: E402
from make_golden import REF, _stub, install_stubs  # noqa: E402

SCRIPTS = REF / "scripts"
MAX_LAG, TAIL = 200, 100  # fixed in scripts/autocorrelation.py


class DatasetView:
    """An h5fake dataset that also takes a boolean mask over its first axis, as h5py does (gaussian-smoothing-error.py:25)."""

    def __init__(self, ds):
        self.ds = ds

    def __getitem__(self, idx):
        if isinstance(idx, np.ndarray) and idx.dtype == bool:
            idx = np.nonzero(idx)[0]
        return self.ds[idx]

    def __array__(self, *a, **k):
        return self.ds.__array__(*a, **k)

    def __getattr__(self, name):
        return getattr(self.ds, name)


class GroupView:
    def __init__(self, group):
        self.group = group

    def __getitem__(self, path):
        node = self.group[path]
        return GroupView(node) if isinstance(node, h5fake.Group) else DatasetView(node)

    def items(self):
        return ((name, self[name]) for name in self.group.keys())

    def require_group(self, path):
        return GroupView(self.group.require_group(path))

    def __contains__(self, name):
        return name in self.group

    def __getattr__(self, name):
        return getattr(self.group, name)


class File(h5fake.File):
    def __enter__(self):
        return GroupView(self.root)


def run_script(name, *argv):
    old = sys.argv
    sys.argv = [name, *[str(a) for a in argv]]
    try:
        return runpy.run_path(str(SCRIPTS / name), run_name="__main__")
    finally:
        sys.argv = old


def mean_flow_of(case):
    run_script("mean-flow.py", case)
    mf = h5fake.TREES[str(Path(case) / "mean-flow.h5")]
    u, p = np.array(mf["data/u"]), np.array(mf["data/p"])
    assert u.dtype == np.float32 and p.dtype == np.float32
    return u, p


def main():
    install_stubs()
    _stub("h5py", File=File, Group=GroupView)
    try:
        import tqdm  # noqa: F401
    except ImportError:
        _stub("tqdm", tqdm=lambda it, *a, **k: it)
    sys.path.insert(0, str(REF))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        # (a) autocorrelation
        case = DC.case_dir(tmp, "autocorr")
        tree = DC.autocorr_case(case / "data.h5")
        u_mean, _ = mean_flow_of(case)
        run_script("autocorrelation.py", case)
        got = dict(np.load(case / "autocorrelation.npz"))
        assert sorted(got) == ["corrcoeff", "decorrelation_steps"] and got["corrcoeff"].dtype == np.float64
        assert got["corrcoeff"].shape == (MAX_LAG + 1,)
        # the same float32 fluctuations, summed in float64
        cells = np.array(tree["grid/cell_idx"])
        back = R.back_positions(cells, np.array(tree["grid/cell_counts"]))
        assert 0 < len(back) < len(cells)
        u = np.array(tree["data/u"])
        acc, _ = R.lag_products(u[len(u) // 2:], u_mean, back, MAX_LAG)
        gap = float(np.abs(got["corrcoeff"] - acc / acc[0]).max())
        margin = R.decorrelation_margin(got["corrcoeff"], TAIL)
        print(f"autocorrelation: {len(back)} of {len(cells)} cells, decorrelation steps {int(got['decorrelation_steps'])}, "
              f"float32 gap {gap:.3e}, margin {margin:.3e} = {margin / gap:.0f} gaps")
        assert margin >= 100 * gap, (margin, gap)
        out["autocorr/corrcoeff"], out["autocorr/decorrelation_steps"] = got["corrcoeff"], got["decorrelation_steps"]
        out["autocorr/mean_flow_u"], out["autocorr/f32_gap"], out["autocorr/margin"] = u_mean, np.float64(gap), np.float64(margin)

        # (b) smoothing error
        case = DC.case_dir(tmp, "smooth")
        tree = DC.smooth_case(case / "data.h5")
        run_script("gaussian-smoothing-error.py", case)
        mses = np.loadtxt(case / "gaussian-smoothing-error.txt")
        assert mses.shape == (32,) and mses.dtype == np.float64
        late = np.array(tree["data/u"])[np.array(tree["data/times"]) > DC.DISCARD]
        assert len(late) == DC.SMOOTH_LATE
        kappa = R.smooth_conditioning(late.reshape(len(late), -1), R.residual_filters())
        print(f"smoothing error: mse {mses[0]:.6e} ... {mses[-1]:.6e}, conditioning {kappa.max():.1f} at width "
              f"{1 + int(kappa.argmax())}, {kappa.min():.1f} at width {1 + int(kappa.argmin())}")
        assert kappa.max() <= 100, kappa
        out["smooth/mses"], out["smooth/kappa"] = mses, kappa

        # (c) mean-forecast errors
        root = tmp / "forecast"
        train, test = DC.forecast_cases(root)
        fu_mean, fp_mean = mean_flow_of(train)
        table_path = tmp / "forecast.json"
        run_script("mean-forecast-errors.py", root, table_path)
        table = json.loads(table_path.read_text())
        assert list(table) == [DC.FORECAST_INFLOW] and list(table[DC.FORECAST_INFLOW]) == [DC.FORECAST_DIMS[0]], table
        ref = table[DC.FORECAST_INFLOW][DC.FORECAST_DIMS[0]]
        data = h5fake.TREES[str(test / "data.h5")]
        for name, mean in (("u", fu_mean), ("p", fp_mean)):
            x = np.array(data[f"data/{name}"])
            total, _ = R.sqdev(x, mean)
            f64 = float(total / np.prod(x.shape[:-1]))  # the script's rule: the last axis summed, the others averaged
            out[f"forecast/{name}"] = np.float64(ref[name])
            out[f"forecast/f32_gap_{name}"] = np.float64(abs(ref[name] - f64))
            print(f"mean forecast {name}: reference {ref[name]!r}, float64 {f64!r}, gap {abs(ref[name] - f64):.3e}")
        out["forecast/mean_flow_u"], out["forecast/mean_flow_p"] = fu_mean, fp_mean

    np.savez_compressed(HERE / "diagnostics.npz", **out)
    size = (HERE / "diagnostics.npz").stat().st_size
    assert size < 1 << 20
    print(f"wrote {HERE / 'diagnostics.npz'} ({len(out)} arrays, {size} bytes)")


if __name__ == "__main__":
    main()
