#!/usr/bin/env python3
"""tests/golden/reverse_step_bits.json: digests of what the reverse-step, loss and Philox kernels of csrc/tdx_ddpm.hip
compute for the cases of tests/reverse_step_cases.py, recorded on the MI355X.

The fixture pins what a change of those kernels must NOT change, so it is recorded from the PARENT commit's library --
built from a checkout of the commit the change starts from -- and never from the tree under test:

    git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/generative-turbulence_amd/csrc
    python tests/golden/make_golden_reverse_step.py --lib /tmp/parent/generative-turbulence_amd/turbdiff_amd/libtdx_hip.so

tests/test_reverse_step_bits.py then requires the working tree's library to reproduce every digest.  Re-record only when
a change is MEANT to alter the arithmetic, again from the tree before it plus that one alteration.
"""

import argparse
import json
import os
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
for p in (HERE.parent, ROOT, ROOT / "generative-turbulence_amd"):
    sys.path.insert(0, str(p))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--lib", required=True, help="the parent commit's libtdx_hip.so")
    ap.add_argument("--out", default=str(HERE / "reverse_step_bits.json"))
    args = ap.parse_args()
    lib = Path(args.lib).resolve()
    assert lib.is_file(), lib
    os.environ["TDX_LIB"] = str(lib)  # read when turbdiff_amd._lib is imported
    import reverse_step_cases as cases
    from turbdiff_amd import _lib, ops

    assert Path(_lib.LIB_PATH).resolve() == lib, _lib.LIB_PATH
    bits = {group: cases.run(ops, group) for group in cases.GROUPS}
    Path(args.out).write_text(json.dumps(bits, indent=0, separators=(",", ":")) + "\n")
    print(f"{args.out}: {sum(len(g) for g in bits.values())} cases in {len(bits)} groups from {lib}")


if __name__ == "__main__":
    main()
