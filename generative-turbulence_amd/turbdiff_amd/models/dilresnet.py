"""DilResNet, the reference's dilated-CNN regression baseline (turbdiff/models/dilresnet.py:47-94), on the HIP kernels.

Same constructor, attribute paths and ``state_dict`` keys as the reference (``encode``, ``encode_c_local``,
``blocks.<b>.layers.<l>``, ``decode``: ``nn.Conv3d`` parameter containers).  ``forward(x, C)`` takes and returns
(B, F, X, Y, Z) fp32 like the reference; the arithmetic follows the dtype of ``x``:

* fp32: every conv is ``ops.conv3d`` (vector-ALU kernels) composed with torch's ReLU and adds -- the parity path;
* bf16: the whole network is ONE autograd node (``_Chain``): every conv carries its ReLU / residual / conditioning adds in its
  epilogue (``tdx_convg_apply_fused``) and the backward folds carry the residual gradient, the ReLU masks and the sum into
  d c_enc (``tdx_convg_fold_fused``), so no elementwise kernel runs between the convs.  ``forward_unfused`` is the same
  network composed from ``ops.conv3d`` and torch elementwise ops in either dtype (the yardstick of the fused chain).

The convg kernels need channel counts that are multiples of 8: the state (F = 4) and the conditioning (8, or 11 with cell
positions) are zero-padded at the model boundary, with zero weight columns / rows; the parameters keep the reference's shapes.
The conditioning conv ``encode_c_local`` does not depend on the state: ``encode_conditioning`` runs it once and ``unroll``
reuses it for every rollout step.
"""

from __future__ import annotations

import ctypes as _C

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from .. import _lib as L
from .. import ops
from .baseline_convs import DilatedCNNBlock
from .conditioning import global_conditioning, local_conditioning


def _up8(n: int) -> int:
    return (n + 7) // 8 * 8


def _pad_conv(conv: nn.Conv3d, cin: int, cout: int):
    """Weight (cout, cin, 3, 3, 3) and bias (cout,) of `conv`, zero-padded; differentiable w.r.t. the parameters."""
    w, b = conv.weight, conv.bias
    w = F.pad(w, (0, 0, 0, 0, 0, 0, 0, cin - w.shape[1], 0, cout - w.shape[0]))
    return w, F.pad(b, (0, cout - b.shape[0]))


def _to_nvc_padded(x: torch.Tensor, channels: int, dtype) -> torch.Tensor:
    """(B, C, X, Y, Z) -> (B, X, Y, Z, channels) in `dtype`, zero channels appended."""
    x = x.movedim(1, -1)
    return F.pad(x, (0, channels - x.shape[-1])).to(dtype).contiguous()


def conv_fused(x, w_t, bias, Cout, dilation, *, relu=False, add0=None, add1=None, h=None, out=None, out_f32=False,
               rollout=None):
    """One replicate-padded 3x3x3 conv (stride 1, padding = dilation) of a bf16 NDHWC tensor with a fused epilogue
    (tdx_convg_apply_fused).  w_t: [27][Cin][Cout] fp32 (ops._taps_first).  An addend of batch 1 is broadcast over the
    batch.  rollout = (x_state, x_next, inside, dx_mean, dx_std): the decode conv's state update; `out` then receives the
    bf16 copy of x_next."""
    B, X, Y, Z, Cin = x.shape
    if out is None:
        out = torch.empty((B, X, Y, Z, Cout), dtype=torch.float32 if out_f32 else x.dtype, device=x.device)
    ep = L.ConvgEpilogue()
    ep.relu, ep.out_f32 = int(relu), int(out_f32)
    bcast = 0
    for a, t in enumerate((add0, add1)):
        if t is None:
            continue
        assert t.dtype == torch.bfloat16 and t.shape[1:] == (X, Y, Z, Cout) and t.shape[0] in (1, B), t.shape
        bcast |= (t.shape[0] == 1 and B > 1) << a
    ep.add0, ep.add1, ep.add_bcast = L.ptr(add0), L.ptr(add1), bcast
    ep.h = L.ptr(h)
    if rollout is not None:
        xs, xn, inside, mean, std = rollout
        assert xs.dtype == torch.float32 and xs.shape[:4] == (B, X, Y, Z) and inside.shape == (X, Y, Z) and inside.dtype == torch.uint8
        ep.x, ep.x_next, ep.inside, ep.dx_mean, ep.dx_std, ep.F = (L.ptr(xs), L.ptr(xn), L.ptr(inside), L.ptr(mean), L.ptr(std),
                                                                  xs.shape[-1])
    L.call("tdx_convg_apply_fused", L.ptr(x), L.ptr(w_t), L.ptr(bias), L.ptr(out), B, X, Y, Z, Cin, X, Y, Z, Cout, 3, dilation,
           dilation, 1, _C.byref(ep), L.dtype_code(x.dtype), L.stream())
    return out


def fold_fused(dpad, grid, pad, *, res=None, mask_src=None, dx=None, dx_masked=None, acc=None):
    B, C = dpad.shape[0], dpad.shape[-1]
    L.call("tdx_convg_fold_fused", L.ptr(dpad), L.ptr(res), L.ptr(mask_src), L.ptr(dx), L.ptr(dx_masked), L.ptr(acc), B, *grid,
           pad, C, L.dtype_code(dpad.dtype), L.stream())


def _adjoint_padded(gz, w_b, Cin, dilation):
    """The data gradient of a replicate-padded conv before the fold: scatter^T of gz on the (E + 2 d)^3 grid."""
    B, X, Y, Z, _ = gz.shape
    p = dilation
    return ops._convg_apply(gz, w_b, None, (X + 2 * p, Y + 2 * p, Z + 2 * p), Cin, 3, 1, dilation, 0, False, True)


def _wgrad(inp, gz, dilation):
    return ops._convg_bwd_weight(inp, gz, 3, 1, dilation, dilation, True, True)


class _Chain(torch.autograd.Function):
    """encode -> N blocks -> decode of a bf16 NDHWC state, one autograd node.  wb = (w, b) of every conv in order (padded
    shapes), dilations = their dilations; c_enc (1, X, Y, Z, H) bf16 or None.  Returns the decode output (B, X, Y, Z, Fp) fp32."""

    @staticmethod
    def forward(ctx, x, c_enc, n_blocks, dilations, *wb):
        ws, bs = wb[0::2], wb[1::2]
        H = ws[0].shape[0]
        n_layers = (len(ws) - 2) // n_blocks
        w_t = [ops._taps_first(w, 1, 0) for w in ws]
        bf = [b.detach().float().contiguous() for b in bs]
        c = c_enc.detach().contiguous() if c_enc is not None else None
        x = x.contiguous()
        u = conv_fused(x, w_t[0], bf[0], H, 1, add0=c)
        acts, hs = [x], []
        for blk in range(n_blocks):
            y = u
            for li in range(n_layers):
                i = 1 + blk * n_layers + li
                acts.append(y)
                if li < n_layers - 1:
                    y = conv_fused(y, w_t[i], bf[i], H, dilations[i], relu=True)
                else:
                    h = torch.empty_like(u)
                    u = conv_fused(y, w_t[i], bf[i], H, dilations[i], relu=True, add0=u, add1=c if blk < n_blocks - 1 else None,
                                   h=h)
                    hs.append(h)
        acts.append(u)
        out = conv_fused(u, w_t[-1], bf[-1], ws[-1].shape[0], 1, out_f32=True)
        ctx.save_for_backward(*acts, *hs, *ws)
        ctx.cfg = (n_blocks, n_layers, tuple(dilations), len(acts), c is not None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        n_blocks, n_layers, dil, n_acts, has_c = ctx.cfg
        saved = ctx.saved_tensors
        acts, hs, ws = saved[:n_acts], saved[n_acts:n_acts + n_blocks], saved[n_acts + n_blocks:]
        x = acts[0]
        B, X, Y, Z, _ = x.shape
        grid, H = (X, Y, Z), ws[0].shape[0]
        n = len(ws)
        gw, gb = [None] * n, [None] * n
        dc = torch.zeros((X, Y, Z, H), dtype=torch.float32, device=x.device) if has_c else None

        gz = g_out.to(torch.bfloat16).contiguous()  # the decode conv has no ReLU: its dz is the output gradient
        gw[-1], gb[-1] = _wgrad(acts[-1], gz, 1)
        dpad = _adjoint_padded(gz, ops._taps_first(ws[-1], 0, 1), H, 1)
        G, dz = torch.empty_like(acts[-1]), torch.empty_like(acts[-1])
        fold_fused(dpad, grid, 1, dx=G, mask_src=hs[-1], dx_masked=dz)  # d u_N; and dz of the last block's last layer
        for blk in reversed(range(n_blocks)):
            for li in reversed(range(n_layers)):
                i = 1 + blk * n_layers + li
                inp = acts[i]
                gw[i], gb[i] = _wgrad(inp, dz, dil[i])
                dpad = _adjoint_padded(dz, ops._taps_first(ws[i], 0, 1), H, dil[i])
                if li > 0:  # the input is the ReLU output of the layer before: mask by it
                    dz = torch.empty_like(inp)
                    fold_fused(dpad, grid, dil[i], mask_src=inp, dx_masked=dz)
                else:  # the block input u_b: + the residual path; its sum over the blocks is d c_enc
                    G_new = torch.empty_like(inp)
                    if blk > 0:
                        dz = torch.empty_like(inp)
                        fold_fused(dpad, grid, dil[i], res=G, dx=G_new, mask_src=hs[blk - 1], dx_masked=dz, acc=dc)
                    else:
                        fold_fused(dpad, grid, dil[i], res=G, dx=G_new, acc=dc)
                    G = G_new
        gw[0], gb[0] = _wgrad(x, G, 1)
        gx = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            fold_fused(_adjoint_padded(G, ops._taps_first(ws[0], 0, 1), x.shape[-1], 1), grid, 1, dx=gx)
        gc = dc.to(torch.bfloat16).unsqueeze(0) if has_c and ctx.needs_input_grad[1] else None
        grads = [g for pair in zip(gw, gb) for g in pair]
        return (gx, gc, None, None, *grads)


class DilResNet(nn.Module):
    """dilresnet.py:47-94."""

    def __init__(self, n_features: int, c_local_features: int, c_global_features: int, N: int = 4, hidden_dim: int = 48):
        super().__init__()
        self.n_features, self.c_local_features, self.c_global_features = n_features, c_local_features, c_global_features
        self.N, self.hidden_dim = N, hidden_dim
        self.dilations = [1, 2, 4, 8]
        self.encode = nn.Conv3d(n_features, hidden_dim, kernel_size=3, padding=1, padding_mode="replicate")
        self.encode_c_local = nn.Conv3d(c_local_features, hidden_dim, kernel_size=3, padding=1, padding_mode="replicate")
        self.blocks = nn.ModuleList([DilatedCNNBlock(hidden_dim, self.dilations) for _ in range(N)])
        self.decode = nn.Conv3d(hidden_dim, n_features, kernel_size=3, padding=1, padding_mode="replicate")
        assert hidden_dim % 8 == 0, "the convg kernels need hidden_dim % 8 == 0"
        self.encode_c_local_calls = 0  # how often the conditioning conv ran (rollouts run it once per batch)

    # ---- boundary: padding to the kernels' channel multiples
    @property
    def state_channels(self) -> int:
        return _up8(self.n_features)

    def _convs(self):
        """(weight, bias, dilation) of encode, every block layer, decode: padded, differentiable."""
        H, Fp = self.hidden_dim, self.state_channels
        we, be = _pad_conv(self.encode, Fp, H)
        out = [(we, be, 1)]
        for blk in self.blocks:
            out += [(l.weight, l.bias, l.dilation[0]) for l in blk.layers]
        wd, bd = _pad_conv(self.decode, H, Fp)
        return out + [(wd, bd, 1)]

    def encode_conditioning(self, C, dtype) -> torch.Tensor | None:
        """encode_c_local of the local conditioning: (1, X, Y, Z, H) in `dtype`, or None without one."""
        if global_conditioning(C) is not None:
            raise RuntimeError("Global conditioning not implemented in DilResNet")
        c = local_conditioning(C)
        if c is None:
            return None
        self.encode_c_local_calls += 1
        cp = _up8(c.shape[0])
        w, b = _pad_conv(self.encode_c_local, cp, self.hidden_dim)
        c = _to_nvc_padded(c.unsqueeze(0), cp, dtype)
        return ops.conv3d(c, w, b, dilation=1, padding=1, padding_mode="replicate")

    def state_input(self, x: torch.Tensor, dtype) -> torch.Tensor:
        return _to_nvc_padded(x, self.state_channels, dtype)

    # ---- the network on NDHWC tensors: (B, X, Y, Z, Fp) -> (B, X, Y, Z, Fp) fp32
    def forward_nvc(self, x: torch.Tensor, c_enc: torch.Tensor | None) -> torch.Tensor:
        if x.dtype == torch.bfloat16:
            convs = self._convs()
            wb = [t for w, b, _ in convs for t in (w, b)]
            return _Chain.apply(x, c_enc, self.N, [d for _, _, d in convs], *wb)
        return self.forward_unfused(x, c_enc)

    def forward_unfused(self, x: torch.Tensor, c_enc: torch.Tensor | None) -> torch.Tensor:
        """The reference's composition (dilresnet.py:82-94): one ops.conv3d per layer, ReLU and adds in torch."""
        convs = self._convs()
        w, b, _ = convs[0]
        u = ops.conv3d(x, w, b, dilation=1, padding=1, padding_mode="replicate")
        for blk in self.blocks:
            if c_enc is not None:
                u = u + c_enc
            u = u + blk(u)
        w, b, _ = convs[-1]
        return ops.conv3d(u, w, b, dilation=1, padding=1, padding_mode="replicate").float()

    def forward(self, x: torch.Tensor, C) -> torch.Tensor:
        """x (B, F, X, Y, Z) -> (B, F, X, Y, Z) fp32; bf16 arithmetic when x is bf16."""
        dtype = x.dtype
        c_enc = self.encode_conditioning(C, dtype)
        out = self.forward_nvc(self.state_input(x, dtype), c_enc)
        return out[..., :self.n_features].movedim(-1, 1)

    # ---- rollout: x_{i+1} = inside ? x_i + dx_mean + dx_std * net(x_i) : x_i  (dilresnet.py:191-200)
    @torch.no_grad()
    def unroll(self, x: torch.Tensor, C, inside: torch.Tensor, dx_mean: torch.Tensor, dx_std: torch.Tensor, steps: int,
               dtype=torch.float32, c_enc=None):
        """States after 1..steps steps, (B, steps, F, X, Y, Z) fp32, from x (B, F, X, Y, Z) fp32; inside (X, Y, Z) bool.
        The state stays fp32; with dtype bf16 the network runs the fused chain and the decode conv applies the update
        (tdx_convg_apply_fused's rollout mode)."""
        if c_enc is None:
            c_enc = self.encode_conditioning(C, dtype)
        Fn = self.n_features
        xs = x.movedim(1, -1).float().contiguous()  # (B, X, Y, Z, F) fp32 state
        out = []
        if dtype != torch.bfloat16:
            mean, std = dx_mean.float(), dx_std.float()
            ins = inside[..., None]
            for _ in range(steps):
                dx = torch.addcmul(mean, std, self.forward_nvc(self.state_input(xs.movedim(-1, 1), dtype), c_enc)[..., :Fn])
                xs = torch.where(ins, xs + dx, xs)
                out.append(xs)
            return torch.stack(out, dim=1).movedim(-1, 2)
        return self._unroll_fused(xs, c_enc, inside, dx_mean, dx_std, steps)

    def _unroll_fused(self, xs, c_enc, inside, dx_mean, dx_std, steps):
        B, X, Y, Z, Fn = xs.shape
        H, Fp = self.hidden_dim, self.state_channels
        convs = self._convs()
        w_t = [ops._taps_first(w, 1, 0) for w, _, _ in convs]
        bf = [b.detach().float().contiguous() for _, b, _ in convs]
        dil = [d for _, _, d in convs]
        n_layers = len(self.blocks[0].layers)
        c = c_enc.detach().contiguous() if c_enc is not None else None
        ins = inside.to(torch.uint8).contiguous()
        mean, std = dx_mean.float().contiguous(), dx_std.float().contiguous()
        xb = _to_nvc_padded(xs.movedim(-1, 1), Fp, torch.bfloat16)
        bufs = [torch.empty((B, X, Y, Z, H), dtype=torch.bfloat16, device=xs.device) for _ in range(4)]
        states = []
        prev = xs
        for _ in range(steps):
            u, un, p, q = bufs
            conv_fused(xb, w_t[0], bf[0], H, 1, add0=c, out=u)
            for blk in range(self.N):
                y = u
                for li in range(n_layers):
                    i = 1 + blk * n_layers + li
                    if li < n_layers - 1:
                        dst = p if y is not p else q
                        y = conv_fused(y, w_t[i], bf[i], H, dil[i], relu=True, out=dst)
                    else:
                        conv_fused(y, w_t[i], bf[i], H, dil[i], relu=True, add0=u, add1=c if blk < self.N - 1 else None, out=un)
                        u, un = un, u
            xn = torch.empty((B, X, Y, Z, Fn), dtype=torch.float32, device=xs.device)
            conv_fused(u, w_t[-1], bf[-1], Fp, 1, out=xb, rollout=(prev, xn, ins, mean, std))
            states.append(xn)
            prev = xn
        return torch.stack(states, dim=1).movedim(-1, 2)
