#!/usr/bin/env python3
"""tests/golden/ops_call_trace.json: the calls and queries `turbdiff_amd.ops` sends across the C ABI for the cases of
tests/ops_trace_cases.py, recorded on the CPU (no library, no GPU).

The fixture pins what a change of the Python host layer must NOT change, so it is recorded from the PARENT commit's
package -- a checkout of the commit the change starts from -- and never from the tree under test:

    git worktree add /tmp/parent HEAD~1          # or wherever the unchanged package lives
    python tests/golden/make_golden_ops_trace.py --package /tmp/parent/generative-turbulence_amd

tests/test_ops_call_trace.py then requires the working tree's ops.py to produce exactly these traces.  Re-record only
when a change is MEANT to alter what is sent (a new kernel entry, a new argument), again from the tree before it plus
that one alteration reviewed by hand in the fixture's diff.
"""

import argparse
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--package", required=True, help="directory that holds the parent commit's turbdiff_amd package")
    ap.add_argument("--out", default=str(HERE / "ops_call_trace.json"))
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.package).resolve()))
    import ops_trace_cases as cases
    from turbdiff_amd import ops

    assert Path(ops.__file__).resolve().is_relative_to(Path(args.package).resolve()), ops.__file__
    traces = {name: cases.record(ops, name) for name in cases.CASES}
    Path(args.out).write_text(json.dumps(traces, indent=0, separators=(",", ":")) + "\n")
    print(f"{args.out}: {len(traces)} cases, {sum(len(t) for t in traces.values())} records")


if __name__ == "__main__":
    main()
