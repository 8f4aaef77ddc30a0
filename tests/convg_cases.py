"""The bits of the general 3-D convolution family (csrc/tdx_convg.hip, tdx_convg_mfma.hip, tdx_convg_chain.hip): the cases
shared by tests/test_convg_bits.py and tests/golden/make_golden_bits.py.

`run(group)` returns one record per case (tests/pinned_bits.py).  Inputs are seeded CPU draws copied to the device; only
digests are stored, and for each group's smallest case (one case where a group has one shape) the raw bits of the first HEAD
elements of every output, so that a mismatch there reads in ulps.  The shapes are the rows the tolerance tests already argue
for (tests/test_baseline_convs.py, tests/test_dilresnet_gpu.py; test_convg_bits.py holds the copies below against them):

    mfma_conv     bf16 ops.conv3d on the matrix-core kernels: y and x.grad (gather; scatter^T by residue class, or on the
                  padded grid + fold for replicate padding)
    mfma_deconv   bf16 ops.conv_transpose3d: y (scatter^T) and x.grad (strided gather)
    vector        the vector-ALU kernels: fp32, bf16 under TDX_CONVG_MFMA=0 (the library reads it per call), one row in fp16
    fused         dilresnet.conv_fused: every epilogue option, and the rollout update of the decode conv
    fold          tdx_convg_fold_clamp in three dtypes and dilresnet.fold_fused with residual / mask / accumulator
    wgrad         weight and bias gradients.  They are merged with fp32 atomics, so their bits depend on the order of the adds
                  unless every sum is exact: x and dy are INTEGERS of {-3, .., 3}, every product is at most 9 and every sum
                  over the few thousand rows far below 2^24 -- fp32 addition is then exact in any order, and bf16 holds
                  these integers exactly.  `wgrad_reference` is F.conv3d's float64 gradient on the CPU, which the outputs
                  must EQUAL.
"""

import contextlib
import functools
import os

import torch
import torch.nn.functional as F

from pinned_bits import record as _digest, tensor_bytes
from step_inputs import rnd

# B, Cin, Cout, grid, k, stride, dilation, pad, mode: test_conv3d_matrix_core_kernels_vs_oracle
MFMA_CONV = [
    (2, 8, 24, (7, 9, 5), 3, 1, 3, 3, "replicate"),
    (1, 48, 48, (12, 8, 10), 3, 1, 2, 2, "replicate"),
    (1, 48, 48, (20, 18, 17), 3, 1, 8, 8, "replicate"),
    (1, 16, 8, (9, 9, 8), 3, 2, 1, 1, "zeros"),
    (2, 64, 128, (12, 10, 8), 3, 2, 1, 1, "zeros"),
    (2, 8, 8, (6, 5, 7), 5, 1, 1, 2, "zeros"),
    (1, 8, 16, (8, 6, 6), 3, 1, 1, 0, "zeros"),
    (1, 136, 72, (6, 5, 4), 3, 1, 1, 1, "zeros"),
    (3, 24, 40, (5, 7, 6), 3, 3, 2, 2, "zeros"),
]
# B, Cin, Cout, grid, k, stride, pad: test_conv_transpose3d_matrix_core_kernels_vs_oracle
MFMA_DECONV = [(2, 16, 8, (5, 6, 4), 4, 2, 1), (1, 128, 64, (6, 4, 5), 4, 2, 1), (2, 8, 24, (4, 5, 3), 3, 1, 1),
               (1, 40, 48, (5, 4, 6), 5, 3, 2)]
# test_conv3d_general_vs_oracle
VECTOR = [
    (2, 8, 24, (7, 9, 5), 3, 1, 3, 3, "replicate"),
    (1, 48, 48, (12, 8, 10), 3, 1, 2, 2, "replicate"),
    (1, 16, 8, (9, 9, 8), 3, 2, 1, 1, "zeros"),
    (2, 8, 8, (6, 5, 7), 5, 1, 1, 2, "zeros"),
    (1, 8, 16, (8, 6, 6), 3, 1, 1, 0, "zeros"),
]
FUSED_SHAPE = (2, 11, 6, 19, 16)  # B, X, Y, Z, Cin: test_kernel_epilogue_options
FUSED_COUT, FUSED_DIL = (8, 48, 64), (1, 8)
FUSED_OPTIONS = [(False, 0, False, False), (True, 0, False, False), (True, 1, True, False), (True, 2, True, False),
                 (False, 1, False, True), (False, 2, False, True)]  # relu, addends, with h, fp32 output
FUSED_BITS = "cout8/dil1/relu0/add0/h0/f320"  # the case whose raw bits are stored
ROLLOUT_SHAPE = (3, 9, 7, 12, 48, 4)  # B, X, Y, Z, Cin, F: test_kernel_rollout_mode
FOLD_SHAPE, FOLD_PAD = (3, 5, 9, 4, 48), (1, 8)  # B, X, Y, Z, C: test_kernel_fold_options
# name -> (dtype, transposed, row).  Matrix-core: the strided 64 -> 128 row, 136 -> 72, stride 3, dilation 8 and the 128 -> 64
# transposed row (the kernel then sees the roles of x and dy swapped, no bias).  Vector-ALU: the first four general rows and
# 8 -> 512 channels, above the 256 threads that reduce the outputs ("A bug this surfaced").
WGRAD = {
    **{f"mfma/{i}": ("bf16", False, MFMA_CONV[i]) for i in (4, 7, 8, 2)},
    "mfma/deconv1": ("bf16", True, MFMA_DECONV[1]),
    **{f"vector/{i}": ("f32", False, VECTOR[i]) for i in range(4)},
    "vector/wide": ("f32", False, (1, 8, 512, (4, 4, 4), 3, 1, 1, 1, "zeros")),
}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
GROUPS = ["mfma_conv", "mfma_deconv", "vector", "fused", "fold", "wgrad"]
FIXTURE = "convg_bits.json"


HEAD = 256  # elements of each output whose raw bits the smallest case of a group stores


def record(outs, smallest=False):
    rec = _digest(outs)
    if smallest:
        rec["bits"] = [tensor_bytes(o.flatten()[:HEAD]).hex() for o in outs]
        rec["itemsize"] = [o.element_size() for o in outs]
    return rec


def _name(row, dtype):
    return "-".join("x".join(map(str, f)) if isinstance(f, tuple) else str(f) for f in row) + f"/{dtype}"


def _size(row):
    """Elements of x and y together, up to the stride: what picks the row whose raw bits are stored."""
    return row[0] * row[3][0] * row[3][1] * row[3][2] * (row[1] + row[2])


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def _dev():
    return torch.device("cuda:0")


def _conv(row, dn, smallest):
    """y and x.grad of ops.conv3d; the weight takes no gradient (that is the wgrad group)."""
    from turbdiff_amd import ops

    B, Ci, Co, grid, k, s, d, p, mode = row
    x = rnd(B, *grid, Ci, seed=1).to(DTYPES[dn]).to(_dev()).requires_grad_()
    w = (rnd(Co, Ci, k, k, k, seed=2) / (Ci * k**3) ** 0.5).to(_dev())
    y = ops.conv3d(x, w, rnd(Co, seed=3).to(_dev()), stride=s, dilation=d, padding=p, padding_mode=mode)
    y.backward(rnd(*y.shape, seed=4).to(y.dtype).to(_dev()))
    return record([y, x.grad], smallest)


def _deconv(row, smallest):
    from turbdiff_amd import ops

    B, Ci, Co, grid, k, s, p = row
    x = rnd(B, *grid, Ci, seed=1).bfloat16().to(_dev()).requires_grad_()
    w = (rnd(Ci, Co, k, k, k, seed=2) / (Ci * k**3 / s**3) ** 0.5).to(_dev())
    y = ops.conv_transpose3d(x, w, rnd(Co, seed=3).to(_dev()), stride=s, padding=p)
    y.backward(rnd(*y.shape, seed=4).bfloat16().to(_dev()))
    return record([y, x.grad], smallest)


def _mfma_conv():
    small = min(MFMA_CONV, key=_size)
    return {_name(r, "bf16"): _conv(r, "bf16", r == small) for r in MFMA_CONV}


def _mfma_deconv():
    small = min(MFMA_DECONV, key=_size)
    return {_name(r, "bf16"): _deconv(r, r == small) for r in MFMA_DECONV}


def _vector():
    small = min(VECTOR, key=_size)
    res = {_name(r, "f32"): _conv(r, "f32", r == small) for r in VECTOR}
    with _env("TDX_CONVG_MFMA", "0"):
        res.update({_name(r, "bf16"): _conv(r, "bf16", r == small) for r in VECTOR})
    res[_name(small, "f16")] = _conv(small, "f16", True)
    return res


def _fused():
    from turbdiff_amd import ops
    from turbdiff_amd.models.dilresnet import conv_fused

    d = _dev()
    res = {}
    B, X, Y, Z, cin = FUSED_SHAPE
    x = rnd(B, X, Y, Z, cin, seed=1).bfloat16().to(d)
    for cout in FUSED_COUT:
        w_t = ops._taps_first(0.1 * rnd(cout, cin, 3, 3, 3, seed=2).to(d), 1, 0)
        b = rnd(cout, seed=3).to(d)
        adds = [rnd(B if i == 0 else 1, X, Y, Z, cout, seed=5 + i).bfloat16().to(d) for i in range(2)]
        for dil in FUSED_DIL:
            for relu, n_add, with_h, f32 in FUSED_OPTIONS:
                h = torch.empty(B, X, Y, Z, cout, device=d, dtype=torch.bfloat16) if with_h else None
                out = conv_fused(x, w_t, b, cout, dil, relu=relu, add0=adds[0] if n_add > 0 else None,
                                 add1=adds[1] if n_add > 1 else None, h=h, out_f32=f32)
                name = f"cout{cout}/dil{dil}/relu{int(relu)}/add{n_add}/h{int(with_h)}/f32{int(f32)}"
                res[name] = record([out] + ([h] if with_h else []), name == FUSED_BITS)
    B, X, Y, Z, cin, Fn = ROLLOUT_SHAPE
    u = rnd(B, X, Y, Z, cin, seed=1).bfloat16().to(d)
    w = 0.05 * rnd(8, cin, 3, 3, 3, seed=2)
    b = rnd(8, seed=3)
    w[Fn:], b[Fn:] = 0, 0
    xs = rnd(B, X, Y, Z, Fn, seed=7).to(d)
    inside = (torch.rand(X, Y, Z, generator=torch.Generator().manual_seed(8)) > 0.3).to(torch.uint8).to(d)
    mean, std = rnd(Fn, seed=9).to(d), (rnd(Fn, seed=10).abs() + 0.5).to(d)
    for dil in FUSED_DIL:
        xn = torch.empty_like(xs)
        xb = torch.full((B, X, Y, Z, 8), 7.0, device=d, dtype=torch.bfloat16)
        conv_fused(u, ops._taps_first(w.to(d), 1, 0), b.to(d), 8, dil, out=xb, rollout=(xs, xn, inside, mean, std))
        res[f"rollout/dil{dil}"] = record([xn, xb])
    return res


def _fold():
    from turbdiff_amd import _lib as L
    from turbdiff_amd.models.dilresnet import fold_fused

    d = _dev()
    res = {}
    B, X, Y, Z, C = FOLD_SHAPE
    r, m = (rnd(B, X, Y, Z, C, seed=s).bfloat16().to(d) for s in (2, 3))
    acc0 = rnd(X, Y, Z, C, seed=4).to(d)
    for pad in FOLD_PAD:
        dpad = rnd(B, X + 2 * pad, Y + 2 * pad, Z + 2 * pad, C, seed=1)
        for dn, dt in DTYPES.items():
            src = dpad.to(dt).to(d)
            dx = torch.empty(B, X, Y, Z, C, device=d, dtype=dt)
            L.call("tdx_convg_fold_clamp", L.ptr(src), L.ptr(dx), B, X, Y, Z, pad, C, L.dtype_code(dt), L.stream())
            res[f"clamp/pad{pad}/{dn}"] = record([dx], (pad, dn) == (1, "bf16"))
        src = dpad.bfloat16().to(d)
        for use_res in (False, True):
            for use_mask in (False, True):
                dx = torch.empty_like(r)
                dm = torch.empty_like(r) if use_mask else None
                acc = acc0.clone()
                fold_fused(src, (X, Y, Z), pad, res=r if use_res else None, mask_src=m if use_mask else None, dx=dx,
                           dx_masked=dm, acc=acc)
                res[f"fused/pad{pad}/res{int(use_res)}/mask{int(use_mask)}"] = record([dx] + ([dm] if use_mask else []) + [acc])
    return res


def _integers(*shape, seed):
    return torch.randint(-3, 4, shape, generator=torch.Generator().manual_seed(seed)).double()


def _wgrad_operands(name):
    """x (NCDHW), dy (NCDHW) as float64 integers, and the conv's arguments."""
    _, transposed, row = WGRAD[name]
    if transposed:
        B, Ci, Co, grid, k, s, p = row
        out = tuple((e - 1) * s - 2 * p + k for e in grid)
        d = 1
    else:
        B, Ci, Co, grid, k, s, d, p, _ = row
        out = tuple((e + 2 * p - d * (k - 1) - 1) // s + 1 for e in grid)
    return _integers(B, Ci, *grid, seed=11), _integers(B, Co, *out, seed=12), (Ci, Co, k, s, d, p)


@functools.lru_cache(maxsize=None)
def wgrad_reference(name):
    """(dw, dbias or None) in float64 from F.conv3d / F.conv_transpose3d on the CPU: integers, exact."""
    _, transposed, row = WGRAD[name]
    x, gy, (Ci, Co, k, s, d, p) = _wgrad_operands(name)
    if transposed:
        w = torch.zeros(Ci, Co, k, k, k, dtype=torch.float64, requires_grad=True)
        F.conv_transpose3d(x, w, None, stride=s, padding=p).backward(gy)
        return w.grad, None
    w = torch.zeros(Co, Ci, k, k, k, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
    xp = F.pad(x, (p,) * 6, mode="replicate") if row[8] == "replicate" else x
    F.conv3d(xp, w, b, stride=s, dilation=d, padding=0 if row[8] == "replicate" else p).backward(gy)
    return w.grad, b.grad


@functools.lru_cache(maxsize=None)
def wgrad_outputs(name):
    """(dw, dbias or None) of the kernels, through ops.conv3d / ops.conv_transpose3d's backward."""
    from turbdiff_amd import ops

    dn, transposed, row = WGRAD[name]
    x, gy, (Ci, Co, k, s, d, p) = _wgrad_operands(name)
    nvc = lambda t: t.movedim(1, -1).contiguous().to(DTYPES[dn]).to(_dev())
    if transposed:
        w = torch.zeros(Ci, Co, k, k, k, device=_dev(), requires_grad=True)
        ops.conv_transpose3d(nvc(x), w, None, stride=s, padding=p).backward(nvc(gy))
        return w.grad, None
    w = torch.zeros(Co, Ci, k, k, k, device=_dev(), requires_grad=True)
    b = torch.zeros(Co, device=_dev(), requires_grad=True)
    ops.conv3d(nvc(x), w, b, stride=s, dilation=d, padding=p, padding_mode=row[8]).backward(nvc(gy))
    return w.grad, b.grad


def _wgrad():
    small = min(WGRAD, key=lambda n: WGRAD[n][2][1] * WGRAD[n][2][2] * WGRAD[n][2][4] ** 3)  # the smallest dw
    return {n: record([t for t in wgrad_outputs(n) if t is not None], n == small) for n in WGRAD}


def run(group):
    """The records of one group of GROUPS, from the library `turbdiff_amd._lib` is bound to."""
    return {"mfma_conv": _mfma_conv, "mfma_deconv": _mfma_deconv, "vector": _vector, "fused": _fused, "fold": _fold,
            "wgrad": _wgrad}[group]()
