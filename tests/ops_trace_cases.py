"""What `turbdiff_amd.ops` sends across the C ABI, recorded on the CPU: the recorder and the cases shared by
tests/test_ops_call_trace.py and tests/golden/make_golden_ops_trace.py.

`recording(ops)` replaces `L.call`, `L.query`, `L.ptr` and `L.stream`, so nothing is launched and no library is needed;
the operators then run forward and backward on small CPU tensors and every call and query is written down:

    {"call": name, "args": [...], "work": w, "meta": {...} or null}      {"query": name, "args": [...], "ret": n}

An argument whose ctypes type (`_lib.SIGNATURES`) is a pointer is written as null, "stream", a list of structs (job
tables), one struct (passed with `ctypes.byref`: the conv epilogue) or `[label, byte offset]`.  The label names the allocation the address lies in: `t<k> <dtype> <shape>`, k = order
of first appearance in the case's calls, dtype / shape those of the tensor first seen at it.  Addresses that ops.py
computes itself (`w2.data_ptr() + 4 * C1`) resolve the same way: `Tensor.data_ptr` is wrapped while recording, so every
tensor whose address was taken is known -- and kept alive, so that no two labels can share an address.
"""

import contextlib
import ctypes as C
import json
import os

import torch

B, GRID, GROUPS = 2, (4, 3, 5), 8
STREAM = 0x57AEA  # what the recorder's L.stream returns


class Recorder:
    def __init__(self, signatures):
        self.sig = signatures
        self.trace = []
        self.spans = {}  # allocation base address -> (bytes, first tensor seen in it)
        self.exact = {}  # address -> (dtype, shape) of the last tensor whose data_ptr() it was
        self.labels = {}  # allocation base address -> label

    def saw(self, t, p):
        st = t.untyped_storage()
        self.spans.setdefault(st.data_ptr(), (st.nbytes(), t))
        self.exact[p] = (t.dtype, tuple(t.shape))

    def pointer(self, p):
        if p is None:
            return None
        if p == STREAM:
            return "stream"
        if isinstance(p, C.Array):
            return [self.struct(s) for s in p]
        if isinstance(getattr(p, "_obj", None), C.Structure):  # ctypes.byref(struct)
            return self.struct(p._obj)
        for base, (nbytes, first) in self.spans.items():
            if base <= p < base + max(nbytes, 1):
                if base not in self.labels:
                    dtype, shape = self.exact.get(p, (first.dtype, tuple(first.shape)))
                    self.labels[base] = f"t{len(self.labels)} {str(dtype)[6:]} {list(shape)}"
                return [self.labels[base], p - base]
        raise AssertionError(f"pointer argument {p:#x} belongs to no tensor whose address was taken")

    def struct(self, s):
        return {f: (self.pointer(getattr(s, f)) if ty is C.c_void_p else getattr(s, f)) for f, ty in s._fields_}

    def args(self, name, args):
        types = self.sig[name][1]
        assert len(args) == len(types), f"{name}: {len(args)} arguments for {len(types)} parameters"
        return [self.pointer(a) if ty is C.c_void_p else a for a, ty in zip(args, types)]

    def query(self, name, *args):
        ret = 1 if not name.endswith("_bytes") else 256 + 16 * sum(a for a in args if isinstance(a, int))
        self.trace.append({"query": name, "args": self.args(name, args), "ret": ret})
        return ret

    def call(self, name, *args, work=0.0, meta=None):
        assert meta is None or callable(meta), "meta= stays lazy: a zero-argument callable"
        meta = meta() if meta is not None else None  # its library query is recorded in front of the call
        self.trace.append({"call": name, "args": self.args(name, args), "work": float(work), "meta": meta})

    @staticmethod
    def ptr(t):
        if t is None:
            return None
        if not t.is_contiguous():
            raise RuntimeError("tdx kernels need contiguous tensors")
        return t.data_ptr()


@contextlib.contextmanager
def recording(ops):
    """The recorder, attached to `ops` and its `_lib`; default switches (side stream off: it needs a device)."""
    L = ops.L
    rec = Recorder(L.SIGNATURES)
    real_data_ptr = torch.Tensor.data_ptr

    def data_ptr(t):
        p = real_data_ptr(t)
        rec.saw(t, p)
        return p

    saved = {(m, k): getattr(m, k) for m, ks in ((L, ("call", "query", "ptr", "stream", "_conv_impl_override")),
                                                 (ops, ("WGRAD_STREAM", "WS_CLEAN", "FUSE_SKIP_TAIL"))) for k in ks}
    had_own = "data_ptr" in torch.Tensor.__dict__
    env = os.environ.pop("TDX_CONV_IMPL", None)
    ops._pack_cache.clear()
    ops._CLEAN.clear()
    try:
        L.call, L.query, L.ptr, L.stream, L._conv_impl_override = rec.call, rec.query, rec.ptr, lambda device_index=None: STREAM, None
        ops.WGRAD_STREAM, ops.WS_CLEAN, ops.FUSE_SKIP_TAIL = False, L.WS_CLEAN, True
        torch.Tensor.data_ptr = data_ptr
        yield rec
    finally:
        if had_own:
            torch.Tensor.data_ptr = real_data_ptr
        else:
            del torch.Tensor.data_ptr
        for (m, k), v in saved.items():
            setattr(m, k, v)
        if env is not None:
            os.environ["TDX_CONV_IMPL"] = env
        ops._pack_cache.clear()
        ops._CLEAN.clear()


# --------------------------------------------------------------------------- tensors


def act(c, dtype, grad=True, b=B, grid=GRID):
    return torch.zeros((b, *grid, c), dtype=dtype).requires_grad_(grad)


def par(*shape, grad=True):
    return torch.zeros(shape, dtype=torch.float32).requires_grad_(grad)


def back(*outs):
    torch.autograd.backward(list(outs), [torch.zeros_like(o) for o in outs])


class _DeviceParameter(torch.Tensor):
    """A CPU tensor that says it is on the device: PackPlan accepts device parameters only."""

    is_cuda = True


def block_args(cin, cout, skip, cconv=None, grad=True):
    conv1 = (par(cout, cconv or cin, 3, 3, 3, grad=grad), par(cout, grad=grad))
    conv2 = (par(cout, cout, 3, 3, 3, grad=grad), par(cout, grad=grad))
    norm1, norm2 = (par(cout, grad=grad), par(cout, grad=grad)), (par(cout, grad=grad), par(cout, grad=grad))
    return conv1, norm1, conv2, norm2, ((par(cout, cin, 1, 1, 1, grad=grad), par(cout, grad=grad)) if skip else None)


def block(ops, dtype, c1, c2, cout, skip, film=True, grad=True, x_grad=True, **kw):
    x1 = kw.pop("x1", None)
    if x1 is None:
        x1 = act(c1, dtype, grad and x_grad)
    x2 = act(c2, dtype, grad and x_grad) if c2 else None
    conv1, norm1, conv2, norm2, skip_wb = block_args(c1 + c2, cout, skip, kw.pop("cconv", None), grad)
    if film:
        y = ops.resnet_block(x1, x2, None, None, conv1, norm1, conv2, norm2, skip_wb, GROUPS, film=par(2, B, cout, grad=grad), **kw)
    else:
        y = ops.resnet_block(x1, x2, par(B, cout, grad=grad), par(B, cout, 1, 1, 1, grad=grad), conv1, norm1, conv2, norm2,
                             skip_wb, GROUPS, eps=1e-6, **kw)
    if grad:
        back(y)


# --------------------------------------------------------------------------- cases

bf16, f32 = torch.bfloat16, torch.float32


def _block_unfused_tail(ops):
    ops.FUSE_SKIP_TAIL = False
    block(ops, bf16, 32, 32, 64, True)


def _block_split_scope(ops):
    # the forward runs inside a model's conv_impl_scope, the backward outside: ctx.impl carries the choice over
    x1, x2 = act(32, f32), act(32, f32)
    conv1, norm1, conv2, norm2, skip_wb = block_args(64, 32, True)
    with ops.L.conv_impl_scope("split"):
        y = ops.resnet_block(x1, x2, None, None, conv1, norm1, conv2, norm2, skip_wb, GROUPS, film=par(2, B, 32))
    back(y)


def _block_encoded(ops):
    X, Y, Z = GRID
    enc = ops.encode_deferred(torch.zeros(B, 4, X, Y, Z), torch.zeros(4, X, Y, Z), par(32, 4, 1, 1, 1), par(32),
                              par(32, 4, 1, 1, 1), par(32), bf16)
    block(ops, bf16, 64, 0, 64, False, x1=enc.standin, cconv=32, conv1_input=act(32, bf16, False), conv1_real_channels=8,
          skip_encoded=enc)


def _block_partial(ops):
    with torch.no_grad():
        x1 = act(64, bf16, False)
        conv1, norm1, conv2, norm2, _ = block_args(64, 64, False, grad=False)
        init = ops.conv3_shared_tail(act(32, bf16, False, b=1), conv1[0], 32)
        ops.resnet_block(x1, None, None, None, conv1, norm1, conv2, norm2, None, GROUPS, partial=(32, init), film=par(2, B, 64, grad=False))


def _block_decode(ops):
    with torch.no_grad():
        block(ops, bf16, 64, 0, 64, False, grad=False, decode_wb=(par(4, 64, 1, 1, 1, grad=False), par(4, grad=False)))


def _conv3(ops, dtype, c2, bias, x_grad=True, w_grad=True):
    x2 = act(32, dtype, x_grad) if c2 else None
    back(ops.conv3(act(32, dtype, x_grad), par(64, 32 + c2, 3, 3, 3, grad=w_grad), par(64, grad=w_grad) if bias else None, x2=x2))


def _conv3_gn_stats(ops):
    y, stats = ops.conv3_gn_stats(act(32, bf16), par(64, 64, 3, 3, 3), par(64), GROUPS, eps=1e-6, x2=act(32, bf16))
    back(ops.gn_film_silu(y, par(64), par(64), GROUPS, stats=stats))


def _conv1(ops, dtype, c2, add, x2_grad=True):
    x2 = act(64, dtype, x2_grad) if c2 else None
    back(ops.conv1(act(32, dtype), par(64, 32 + c2, 1, 1, 1), par(64), x2=x2, add=act(64, dtype) if add else None))


def _gn(ops, dtype, film, res, act_):
    scale, shift = (par(B, 32), par(B, 32)) if film else (None, None)
    back(ops.gn_film_silu(act(32, dtype), par(32), par(32), GROUPS, scale, shift, act(32, dtype) if res else None, act=act_))


def _skip_and_resize(ops, use_resized):
    skip, y = ops.skip_and_resize(act(32, bf16), (2, 2, 3))
    back(skip, y) if use_resized else back(skip)


def _layout(ops):
    X, Y, Z = GRID
    back(ops.to_nvc(torch.zeros(B, 32, X, Y, Z, requires_grad=True), bf16))
    back(ops.to_ncv(act(32, bf16)))


def _prefetch(ops):
    dev = lambda *shape: torch.Tensor._make_subclass(_DeviceParameter, torch.zeros(shape), True)
    w3, w1 = [dev(64, 32, 3, 3, 3), dev(32, 64, 3, 3, 3)], [dev(64, 32, 1, 1, 1)]
    plan = ops.prefetch_weights(w3, w1, bf16)
    assert ops.prefetch_weights(w3, w1, bf16, plan) is plan  # nothing changed: no launch
    with torch.no_grad():
        ops.conv3(ops.conv3(act(32, bf16, False), w3[0]), w3[1])
        ops.conv1(act(32, bf16, False), w1[0])


# the DDPM arithmetic: (B, F, X, Y, Z) float32 states, F = 4; the decoder output of a learned-variance model has 2 F planes
def state(f=4, grad=False):
    return torch.zeros((B, f, *GRID)).requires_grad_(grad)


def i64(*shape):
    return torch.zeros(shape, dtype=torch.int64)


def dev_scalar():
    return torch.Tensor._make_subclass(_DeviceParameter, i64(1), False)


def _step_operands():
    X, Y, Z = GRID
    return state(), state(), state(), torch.zeros(X * Y * Z, dtype=torch.uint8), torch.zeros(7, 10), i64(1)


def _p_sample_step(ops):
    x, eps, xb, mask, sched, t = _step_operands()
    ops.p_sample_step(x, eps, state(), state(), xb, mask, sched, 10, t, True, False)
    ops.p_sample_step(x, eps, state(), None, xb, mask, sched, 10, t, False, True, out=x)


def _p_sample_step_rng(ops):
    x, eps, xb, mask, sched, t = _step_operands()
    ops.p_sample_step_rng(x, eps, xb, mask, sched, 10, t, True, False, 1234, i64(B), i64(1))
    ops.p_sample_step_rng(x, eps, xb, mask, sched, 10, t, False, True, (7 << 32) | 5, i64(B), i64(1), out=x)


def _p_sample_step_lv(ops):
    x, _, xb, mask, sched, t = _step_operands()
    ops.p_sample_step_lv(x, state(8), state(), state(), xb, mask, sched, torch.zeros(10), 10, t, True, False)
    ops.p_sample_step_lv(x, state(8), state(), None, xb, mask, sched, torch.zeros(10), 10, t, False, True, out=x)


def _p_sample_step_lv_rng(ops):
    x, _, xb, mask, sched, t = _step_operands()
    ops.p_sample_step_lv_rng(x, state(8), xb, mask, sched, torch.zeros(10), 10, t, True, False, 1234, i64(B), i64(1))
    ops.p_sample_step_lv_rng(x, state(8), xb, mask, sched, torch.zeros(10), 10, t, False, True, 99, i64(B), i64(1), out=x)


def _ddim_step(ops):
    x, eps, xb, mask, _, t = _step_operands()
    ops.ddim_step(x, eps, state(), state(), xb, mask, torch.zeros(6, 4), i64(1), i64(4), t, True, False)
    ops.ddim_step(x, eps, None, None, xb, mask, torch.zeros(6, 4), i64(1), i64(4), t, False, True, out=x)


def _ddim_step_rng(ops):
    x, eps, xb, mask, _, t = _step_operands()
    ops.ddim_step_rng(x, eps, xb, mask, torch.zeros(6, 4), i64(1), i64(4), t, True, False, 1234, i64(B), i64(1))
    ops.ddim_step_rng(x, eps, xb, mask, torch.zeros(6, 4), i64(1), i64(4), t, False, True, 99, i64(B), i64(1), out=x)


def _q_sample(ops):
    _, _, _, mask, _, _ = _step_operands()
    ops.q_sample(state(), state(), torch.zeros(10), torch.zeros(10), i64(B))
    ops.q_sample(state(), state(), torch.zeros(10), torch.zeros(10), i64(1), mask=mask, keep_bcs=True)


def _masked_loss(ops, n_cells):
    _, _, _, mask, _, _ = _step_operands()
    back(ops.masked_loss(state(grad=True), state(), mask, n_cells, l1=True))
    ops.masked_loss(state(), state(), mask, n_cells)  # no gradient asked for


def _elbo_loss(ops, n_cells):
    _, _, _, mask, sched, _ = _step_operands()
    total, parts = ops.elbo_loss(state(8, grad=True), state(), state(), state(), mask, n_cells, i64(B), sched, torch.zeros(10),
                                 l1=True, clip=True, detach_mean=False, elbo_weight=0.1, parts=True)
    back(total)
    ops.elbo_loss(state(8), state(), state(), state(), mask, n_cells, i64(B), sched, torch.zeros(10))


def _randn(ops):
    ops.randn_philox(torch.zeros(37), 1234, (7 << 32) | 5, i64(1))
    ops.randn_philox_batched(state(), 1234, i64(B), i64(1))


# the general convolution family (csrc/tdx_convg*.hip): forward and backward with bias
def _convg(ops, **kw):
    back(ops.conv3d(act(16, bf16), par(24, 16, 3, 3, 3), par(24), **kw))


def _conv_transpose(ops):
    back(ops.conv_transpose3d(act(16, bf16), par(16, 8, 4, 4, 4), par(8), stride=2, padding=1))


def _dilresnet_chain(ops):
    from turbdiff_amd.models.dilresnet import _Chain

    H, Fp, n_blocks, dil = 16, 8, 2, (1, 2)  # two blocks of two layers between encode and decode
    shapes = [(H, Fp)] + [(H, H)] * (n_blocks * len(dil)) + [(Fp, H)]
    wb = [t for co, ci in shapes for t in (par(co, ci, 3, 3, 3), par(co))]
    back(_Chain.apply(act(Fp, bf16), act(H, bf16, b=1), n_blocks, [1, *dil * n_blocks, 1], *wb))


CASES = {
    "block_two_inputs_bf16_fused_tail": lambda ops: block(ops, bf16, 32, 32, 64, True),
    "block_two_inputs_f32_scale_shift": lambda ops: block(ops, f32, 32, 32, 64, True, film=False),
    "block_two_inputs_bf16_unfused_tail": _block_unfused_tail,
    "block_two_inputs_f32_split_scope": _block_split_scope,
    "block_one_input_projected_skip_f32": lambda ops: block(ops, f32, 32, 0, 64, True),
    "block_identity_skip_bf16": lambda ops: block(ops, bf16, 64, 0, 64, False),
    "block_identity_skip_f32_scale_shift": lambda ops: block(ops, f32, 64, 0, 64, False, film=False),
    "block_conv1_input": lambda ops: block(ops, bf16, 64, 0, 64, False, cconv=32, conv1_input=act(32, bf16, False)),
    "block_conv1_input_with_grad": lambda ops: block(ops, bf16, 64, 0, 64, False, cconv=32, conv1_input=act(32, bf16)),
    "block_conv1_input_real_channels": lambda ops: block(ops, f32, 64, 0, 64, False, cconv=32, conv1_input=act(32, f32),
                                                         conv1_real_channels=8),
    "block_skip_encoded": _block_encoded,
    "block_partial_nograd": _block_partial,
    "block_decode_nograd": _block_decode,
    "conv3_bf16": lambda ops: _conv3(ops, bf16, 0, False),
    "conv3_x2_bias_f32": lambda ops: _conv3(ops, f32, 32, True),
    "conv3_weight_grad_only": lambda ops: _conv3(ops, bf16, 32, True, x_grad=False),
    "conv3_data_grad_only": lambda ops: _conv3(ops, bf16, 0, True, w_grad=False),
    "conv3_gn_stats": _conv3_gn_stats,
    "conv3_shared_tail": lambda ops: ops.conv3_shared_tail(act(32, bf16, False, b=1), par(64, 64, 3, 3, 3, grad=False), 32),
    "conv1_bf16": lambda ops: _conv1(ops, bf16, 0, False),
    "conv1_x2_add_f32": lambda ops: _conv1(ops, f32, 64, True),
    "conv1_x2_without_grad": lambda ops: _conv1(ops, bf16, 64, False, x2_grad=False),
    "gn_film_silu_plain": lambda ops: _gn(ops, bf16, False, False, True),
    "gn_film_silu_film_res_f32": lambda ops: _gn(ops, f32, True, True, True),
    "gn_film_silu_film_noact": lambda ops: _gn(ops, bf16, True, False, False),
    "resize": lambda ops: back(ops.resize(act(32, bf16), (7, 5, 9))),
    "skip_and_resize": lambda ops: _skip_and_resize(ops, True),
    "skip_and_resize_resized_unused": lambda ops: _skip_and_resize(ops, False),
    "to_nvc_to_ncv": _layout,
    "prefetch_then_convs": _prefetch,
    "p_sample_step": _p_sample_step,
    "p_sample_step_rng": _p_sample_step_rng,
    "p_sample_step_lv": _p_sample_step_lv,
    "p_sample_step_lv_rng": _p_sample_step_lv_rng,
    "ddim_step": _ddim_step,
    "ddim_step_rng": _ddim_step_rng,
    "q_sample": _q_sample,
    "masked_loss_int_n_cells": lambda ops: _masked_loss(ops, 40),
    "masked_loss_device_n_cells": lambda ops: _masked_loss(ops, dev_scalar()),
    "elbo_loss_int_n_cells": lambda ops: _elbo_loss(ops, 40),
    "elbo_loss_device_n_cells": lambda ops: _elbo_loss(ops, dev_scalar()),
    "randn_philox": _randn,
    "conv3d_zeros_stride2": lambda ops: _convg(ops, stride=2, padding=1),
    "conv3d_replicate_dilated": lambda ops: _convg(ops, dilation=2, padding=2, padding_mode="replicate"),
    "conv_transpose3d": _conv_transpose,
    "dilresnet_chain": _dilresnet_chain,
}


def record(ops, name):
    """The trace of one case as plain JSON values."""
    with recording(ops) as rec:
        CASES[name](ops)
    return json.loads(json.dumps(rec.trace))
