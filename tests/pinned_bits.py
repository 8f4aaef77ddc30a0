"""Pinned-bits fixtures: what the case modules (reverse_step_cases, gn_cases, conv3_cases, convg_cases, conv1_bits_cases, resize_bits_cases, attention_bits_cases), their tests and the recorder
tests/golden/make_golden_bits.py share.

A case module has GROUPS, FIXTURE (the file name under tests/golden/) and run(group) -> {case name: record}.  A record is

    {"sha256": digest of the outputs' bytes, in order,
     "bits":   [hex of each output's bytes]        smallest shape only, so a mismatch there reads in ulps,
     "itemsize": [bytes per element of each output]   beside "bits", where an output is not float32,
     ...}                                          whatever else the case module pins (offsets, loss values)
"""

import hashlib

import numpy as np
import torch

_INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def tensor_bytes(t):
    t = t.detach().cpu().contiguous()
    return t.view(_INT_VIEW[t.dtype]).numpy().tobytes()


def record(outs, smallest=False, **more):
    h = hashlib.sha256()
    for o in outs:
        h.update(tensor_bytes(o))
    rec = {"sha256": h.hexdigest(), **more}
    if smallest:
        rec["bits"] = [tensor_bytes(o).hex() for o in outs]
        if any(o.element_size() != 4 for o in outs):
            rec["itemsize"] = [o.element_size() for o in outs]
    return rec


def ulps(got_hex, want_hex, itemsize=4):
    """Largest distance between two recorded outputs in units of the last place."""
    def ordered(s):  # sign-magnitude bit patterns on a line: negative values mirrored below zero
        i = np.frombuffer(bytes.fromhex(s), dtype=f"<i{itemsize}").astype(np.int64)
        return np.where(i < 0, -(1 << (8 * itemsize - 1)) - i, i)
    return int(np.abs(ordered(got_hex) - ordered(want_hex)).max())


def assert_pinned(got, want, group):
    """Every case of `want` (a group of the fixture) is reproduced by `got` (the same group, run now)."""
    assert sorted(got) == sorted(want)
    for name, w in want.items():
        g = got[name]
        sizes = w.get("itemsize") or [4] * len(w.get("bits", ()))
        for i, (gb, wb) in enumerate(zip(g.get("bits", ()), w.get("bits", ()))):
            assert gb == wb, f"{group} {name}: output {i} is {ulps(gb, wb, sizes[i])} ulp off"
        assert g == w, f"{group} {name}: {[k for k in w if g.get(k) != w[k]]} differ"
