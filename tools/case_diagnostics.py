#!/usr/bin/env python3
"""Per-case diagnostics of a raw ``data.h5`` case: the reference's scripts/autocorrelation.py, gaussian-smoothing-error.py and
mean-forecast-errors.py in one command, on the GPU.

    python tools/case_diagnostics.py CASE [--only autocorrelation|smoothing-error|mean-forecast-error] [--mean-case DIR]
                                          [--discard-first 0.025] [--chunk-size 10]
    python tools/case_diagnostics.py --forecast-root ROOT OUT.json

The first form writes ``autocorrelation.npz`` and ``gaussian-smoothing-error.txt`` beside ``CASE/data.h5`` and prints the
mean-forecast errors of ``CASE`` against the mean flow of ``--mean-case`` (default: its own).  ``autocorrelation`` and
``mean-forecast-error`` read ``mean-flow.h5``, which tools/prepare_dataset.py --only mean-flow writes.  The second form walks
``ROOT/inflow-*/<d>D*`` as scripts/mean-forecast-errors.py does -- the mean flow of ``train/high-step`` against the frames of
``test/high-step`` -- and merges {inflow: {dims: {"u", "p"}}} into ``OUT.json``.  Reading the case files needs h5py.
"""

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "generative-turbulence_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

DIAGNOSTICS = ("autocorrelation", "smoothing-error", "mean-forecast-error")


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("case", metavar="CASE|OUT.json", help="Case directory (with --forecast-root: the JSON file to merge into)")
    ap.add_argument("--only", choices=DIAGNOSTICS, default=None, help="run one diagnostic only")
    ap.add_argument("--mean-case", default=None, help="mean-forecast-error: the case whose mean-flow.h5 is the forecast")
    ap.add_argument("--discard-first", default=0.025, type=float, help="smoothing-error: use the frames with t > this")
    ap.add_argument("--chunk-size", default=10, type=int, help="frames read at once")
    ap.add_argument("--forecast-root", default=None, metavar="ROOT", help="walk ROOT/inflow-*/* and write the table of errors")
    return ap


def forecast_walk(root, out_path, *, error=None, **kwargs):
    """The table of scripts/mean-forecast-errors.py:24-49: {inflow: {dims: {"u": mse, "p": mse}}} for every directory
    ``root/inflow-<inflow>/<dims>D...``, merged into the JSON file ``out_path`` (rewritten after every case).  The dims are
    keyed by their digit as a string, which is what they are once the file has been through JSON.  ``error(data_case,
    mean_case, **kwargs)`` defaults to ``diagnostics.mean_forecast_error``."""
    if error is None:
        from turbdiff_amd.data.diagnostics import mean_forecast_error as error
    root, out_path = Path(root), Path(out_path)
    table = json.loads(out_path.read_text()) if out_path.exists() else {}
    for inflow_root in sorted(root.glob("inflow-*/*")):
        inflow = inflow_root.parent.name[len("inflow-"):]
        dims = int(inflow_root.name[0])
        mse = error(inflow_root / "test" / "high-step", inflow_root / "train" / "high-step", **kwargs)
        print(inflow, f"{dims}D", f"mse_u={mse['u']}", f"mse_p={mse['p']}")
        table.setdefault(inflow, {})[str(dims)] = {"u": mse["u"], "p": mse["p"]}
        out_path.write_text(json.dumps(table))
    return table


def main():
    args = parser().parse_args()
    from turbdiff_amd.data import diagnostics

    if args.forecast_root is not None:
        forecast_walk(args.forecast_root, args.case, chunk_frames=args.chunk_size)
        print(f"wrote {args.case}")
        return
    case = Path(args.case)
    want = DIAGNOSTICS if args.only is None else (args.only,)
    if "autocorrelation" in want:
        r = diagnostics.autocorrelation(case, chunk_frames=args.chunk_size)
        print(f"{case / 'autocorrelation.npz'}: decorrelation steps {r.decorrelation_steps}, max decorrelated coefficient "
              f"{r.max_decorrelated_coeff}")
    if "smoothing-error" in want:
        mses = diagnostics.smoothing_error(case, discard_first=args.discard_first, chunk_frames=args.chunk_size)
        print(f"{case / 'gaussian-smoothing-error.txt'}: mse {mses[0]:.6e} at width 1 ... {mses[-1]:.6e} at width {len(mses)}")
    if "mean-forecast-error" in want:
        mse = diagnostics.mean_forecast_error(case, args.mean_case, chunk_frames=args.chunk_size)
        print(f"{case}: mean-forecast error against {args.mean_case or 'its own mean flow'}: mse_u={mse['u']} mse_p={mse['p']}")


if __name__ == "__main__":
    main()
