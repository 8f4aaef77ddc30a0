#!/usr/bin/env python3
"""Record a pinned-bits fixture on the MI355X: tests/golden/<FIXTURE of the case module>, the digests of what the kernels
compute for the module's cases.  Case modules: reverse_step_cases (csrc/tdx_ddpm.hip -> reverse_step_bits.json), gn_cases
(csrc/tdx_groupnorm.hip and the codec element -> gn_bits.json), conv3_cases (the brick kernels of the 3x3x3 forward / data
gradient, csrc/tdx_conv3_mfma*.hip, and the ring kernel's remainder slabs -> conv3_bits.json), convg_cases (the general
convolution family, csrc/tdx_convg*.hip -> convg_bits.json), conv1_bits_cases (the 1x1 convolution family, csrc/tdx_conv1*.hip
-> conv1_bits.json), resize_bits_cases (the trilinear resize, csrc/tdx_resize.hip -> resize_bits.json), attention_bits_cases (the
attention family, csrc/tdx_attention*.hip -> attention_bits.json).

A fixture pins what a change of those kernels must NOT change, so it is recorded from the PARENT commit's library --
built from a checkout of the commit the change starts from -- and never from the tree under test:

    git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/generative-turbulence_amd/csrc
    python tests/golden/make_golden_bits.py gn_cases --lib /tmp/parent/generative-turbulence_amd/turbdiff_amd/libtdx_hip.so

The module's test (tests/test_reverse_step_bits.py, tests/test_gn_bits.py, tests/test_conv3_bits.py, tests/test_convg_bits.py, tests/test_conv1_bits.py, tests/test_resize_bits.py, tests/test_attention_bits.py) then requires the working tree's library to
reproduce every digest.  Re-record only when a change is MEANT to alter the arithmetic, again from the tree before it plus
that one alteration.
"""

import argparse
import importlib
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
    ap.add_argument("cases", help="the case module under tests/: reverse_step_cases, gn_cases, conv3_cases, convg_cases, conv1_bits_cases, resize_bits_cases or attention_bits_cases")
    ap.add_argument("--lib", required=True, help="the parent commit's libtdx_hip.so")
    ap.add_argument("--out", help="default: tests/golden/<the module's FIXTURE>")
    args = ap.parse_args()
    lib = Path(args.lib).resolve()
    assert lib.is_file(), lib
    os.environ["TDX_LIB"] = str(lib)  # read when turbdiff_amd._lib is imported
    cases = importlib.import_module(args.cases)
    from turbdiff_amd import _lib

    assert Path(_lib.LIB_PATH).resolve() == lib, _lib.LIB_PATH
    out = Path(args.out or HERE / cases.FIXTURE)
    bits = {group: cases.run(group) for group in cases.GROUPS}
    out.write_text(json.dumps(bits, indent=0, separators=(",", ":")) + "\n")
    print(f"{out}: {sum(len(g) for g in bits.values())} cases in {len(bits)} groups from {lib}")


if __name__ == "__main__":
    main()
