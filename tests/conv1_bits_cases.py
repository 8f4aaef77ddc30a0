"""The bits of the 1x1 convolution family (csrc/tdx_conv1.hip, tdx_conv1_mfma.hip, tdx_conv1_mfma_f32.hip): the cases shared by
tests/test_conv1_bits.py and tests/golden/make_golden_bits.py.

`run(group)` returns one record per case (tests/pinned_bits.py).  The rows are the Gaussian-input rows of tests/conv1_cases.py,
with the tensors, buffers and calls of tests/test_conv1_reference.py (its `_forward`, `_tail_calls`, `_wgrad_call`): what is
held to a derived bound there is held to its recorded bits here.  Only digests are stored, and for one case per group the raw
bits of the first HEAD elements of every output, so that a mismatch there reads in ulps.

    fwd             FWD_INEXACT in every dtype of the row: y of tdx_conv1_fwd
    tail            TAIL_INEXACT in bf16 and fp16: y of tdx_conv1_fwd_gn, and the y of tdx_conv1_fwd it adds onto
    wgrad           WGRAD_INEXACT and NO_ARENA in every dtype of the row, tdx_conv1_bwd_weight and tdx_conv1_bwd_weight_oc with
                    accumulate 0 and 1: the whole dW and dbias buffers under TDX_DETERMINISTIC=1 (slabs in the arena, summed
                    in order).  The atomic merge of TDX_DETERMINISTIC unset is not reproducible from run to run: not pinned.
    wgrad_no_arena  the NO_ARENA rows again with no arena bound: one split straight into dW
"""

import contextlib
import os

import conv1_cases as cases
import conv1_reference as R
from pinned_bits import record as _digest, tensor_bytes

GROUPS = ["fwd", "tail", "wgrad", "wgrad_no_arena"]
FIXTURE = "conv1_bits.json"
HEAD = 256  # elements of each output whose raw bits one case of a group stores
BITS = {"fwd": "v_seam_r65/bf16", "tail": "t_v27/bf16", "wgrad": "wh_128_64_r257/bf16/tdx_conv1_bwd_weight_oc/acc1",
        "wgrad_no_arena": "wv_40_72_r4097/f32/tdx_conv1_bwd_weight/acc0"}
WGRAD_ROWS = cases.WGRAD_INEXACT + [n for n in cases.NO_ARENA if n not in cases.WGRAD_INEXACT]


def record(outs, smallest=False):
    rec = _digest(outs)
    if smallest:
        rec["bits"] = [tensor_bytes(o.flatten()[:HEAD]).hex() for o in outs]
        rec["itemsize"] = [o.element_size() for o in outs]
    return rec


@contextlib.contextmanager
def _env(**values):
    """Library switches for the calls inside (the library reads them per call); None: unset"""
    old = {k: os.environ.get(k) for k in values}
    try:
        for k, v in values.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@contextlib.contextmanager
def no_arena():
    """The launching stream binds "no arena" (TDX_SCRATCH_MB=0) inside, and gets its own arena back afterwards"""
    from turbdiff_amd import _lib as L

    old = L.SCRATCH_BYTES
    try:
        L.SCRATCH_BYTES, L._ACTIVE = 0, None
        yield
    finally:
        L.SCRATCH_BYTES, L._ACTIVE = old, None
        L.ensure_scratch()


def _fwd():
    import test_conv1_reference as T
    from turbdiff_amd import _lib as L

    res = {}
    for name in cases.FWD_INEXACT:
        c = cases.by_name(cases.FWD, name)
        with _env(TDX_CONV1_IMPL="direct" if c.direct else None):
            for dname in c.dtypes:
                dt = R.DTYPES[dname]
                p = T._to(R.gaussian_inputs(c.rows, c.C1, c.C2, c.Cout, dt), T._dev())
                y = T._forward(L, c, p, dt, p["bias"] if c.bias else None, p["add"] if c.add else None, ask=False)
                res[f"{name}/{dname}"] = record([y], f"{name}/{dname}" == BITS["fwd"])
    return res


def _tail():
    import test_conv1_reference as T
    from turbdiff_amd import _lib as L

    res = {}
    for name in cases.TAIL_INEXACT:
        c = cases.by_name(cases.TAIL, name)
        for dname in cases.H16:
            dt = R.DTYPES[dname]
            p = T._to(R.gaussian_inputs(c.B * c.V, c.C1, c.C2, c.Cout, dt), T._dev())
            t = T._to(R.tail_inputs(c.B, c.V, c.Cout, c.G, exact=False, dt=dt), T._dev())
            with _env(TDX_CONV1_IMPL=None):
                fused, _, plain = T._tail_calls(L, c, p, t, dt)
            res[f"{name}/{dname}"] = record([fused, plain], f"{name}/{dname}" == BITS["tail"])
    return res


def _wgrad(names, group):
    import test_conv1_reference as T
    from turbdiff_amd import _lib as L

    res = {}
    for name in names:
        c = cases.by_name(cases.WGRAD, name)
        with _env(TDX_CONV1_IMPL="direct" if c.direct else None, TDX_DETERMINISTIC="1"):
            for dname in c.dtypes:
                dt = R.DTYPES[dname]
                p = T._to(R.gaussian_inputs(c.rows, c.Cin, 0, c.Cout, dt), T._dev())
                x, dy = T._as(p["x1"], dt), T._as(p["dy"], dt)
                for entry, tr, acc in T.ENTRIES:
                    pre_w, pre_b = T._prefills(c.Cin, c.Cout, tr, exact=False)
                    bw, bb = T._wgrad_call(L, entry, tr, acc, x, dy, c.Cin, c.Cout, c.rows, dt, pre_w, pre_b)
                    key = f"{name}/{dname}/{entry}/acc{acc}"
                    res[key] = record([bw, bb], key == BITS[group])
    return res


def _wgrad_no_arena():
    with no_arena():
        return _wgrad(cases.NO_ARENA, "wgrad_no_arena")


def run(group):
    """The records of one group of GROUPS, from the library `turbdiff_amd._lib` is bound to."""
    return {"fwd": _fwd, "tail": _tail, "wgrad": lambda: _wgrad(WGRAD_ROWS, "wgrad"), "wgrad_no_arena": _wgrad_no_arena}[group]()
