"""TF-Net, the reference's turbulent-flow baseline (turbdiff/models/tfnet.py:211-368: ``Encoder``, ``LES``), on the HIP kernels.

Same constructor, attribute paths and ``state_dict`` as the reference (``spatial_filter``, ``temporal_filter``,
``encoder_{bar,tilde,prime}.conv{1,1_local,2,3,4}.{0,1}``, ``deconv{3,2,1,0}.0``, ``output_layer``), so state dicts load
either way with ``strict=True``.  ``forward(xx, C)`` takes (B, T, F, X, Y, Z) and returns (B, F, X, Y, Z) fp32.

* The flow decomposition (tfnet.py:304-337: spatial filter, temporal filter over windows, the two residuals, the ``(t f)``
  stacking) and the crossing of its three stacks to NDHWC in the compute dtype (that of ``xx``, or ``dtype``), zero-padded to
  a channel multiple of 8 like ``models.dilresnet`` pads its state, are one kernel forward and one backward
  (``ops.flow_decompose``, csrc/tdx_flow_decompose.hip; ``FUSE_DECOMPOSE``, on by default).  A call the kernels do not take
  (CPU tensors, a non-fp32 ``xx``, T > 8, F > 8, T F > 32, a grid past the bounds of include/tdx.h) or the
  switch off runs ``decompose`` -- fp32 torch ops on NCDHW tensors -- and ``_to_nvc_padded``, as before.
* Every conv() block is a ``ConvBlock``: ``ops.conv3d`` and the fused BatchNorm + LeakyReLU (+ add) tail
  (``ops.batch_norm_act``; ``baseline_convs.FUSE_BATCHNORM``, on by default).  The conditioning branch
  ``conv1_local(c_local[None])`` enters level 1 as the tail's batch-broadcast addend.  At level 4, whose three outputs are only ever summed, the second and third
  encoder's tail takes the running sum as its addend; at levels 1-3 each encoder's own output feeds its next conv, so the
  three are added with torch.  ``clip_spatial`` is a slice of the NDHWC tensor; the deconvs are ``DeconvBlock``s.
* ``encode_conditioning`` runs the three conditioning branches.  They do not depend on the state: in eval mode a rollout
  computes them once and passes them as ``c_enc``; in training mode every call computes them, because each call updates
  those BatchNorms' running statistics in the reference.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from .. import ops
from .baseline_convs import ConvBlock, conv, deconv
from .conditioning import global_conditioning, local_conditioning
from .dilresnet import _pad_conv, _to_nvc_padded, _up8

# LES.forward takes ops.flow_decompose (csrc/tdx_flow_decompose.hip) for every call it supports; False: decompose() and
# three _to_nvc_padded calls in torch, everywhere
FUSE_DECOMPOSE = True


def _first_block(blk: ConvBlock, x: torch.Tensor, add=None) -> torch.Tensor:
    """A ConvBlock whose input carries zero-padded channels: the conv with zero weight columns, then the block's tail."""
    c = blk[0]
    w, b = _pad_conv(c, x.shape[-1], c.out_channels)
    return blk.tail(ops.conv3d(x, w, b, stride=c.stride[0], padding=c.padding[0]), add)


class Encoder(nn.Module):
    """tfnet.py:211-254."""

    def __init__(self, input_channels, c_local_channels, kernel_size, dropout_rate):
        super().__init__()
        self.conv1 = conv(input_channels, 64, kernel_size=kernel_size, stride=2, dropout_rate=dropout_rate)
        self.conv1_local = conv(c_local_channels, 64, kernel_size=kernel_size, stride=2, dropout_rate=dropout_rate)
        self.conv2 = conv(64, 128, kernel_size=kernel_size, stride=2, dropout_rate=dropout_rate)
        self.conv3 = conv(128, 256, kernel_size=kernel_size, stride=2, dropout_rate=dropout_rate)
        self.conv4 = conv(256, 512, kernel_size=kernel_size, stride=2, dropout_rate=dropout_rate)
        for m in self.modules():  # tfnet.py:237-245
            if isinstance(m, (nn.Conv3d, nn.ConvTranspose3d)):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, 0.002 / n)
                if m.bias is not None:
                    m.bias.data.zero_()
            elif isinstance(m, nn.BatchNorm3d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()

    def encode_conditioning(self, c_local: torch.Tensor) -> torch.Tensor:
        """conv1_local of the padded NDHWC conditioning (1, X, Y, Z, Cp) -> (1, X/2, Y/2, Z/2, 64)."""
        return _first_block(self.conv1_local, c_local)

    def forward(self, x: torch.Tensor, c_enc=None, add4=None):
        """NDHWC x -> (out_conv1, out_conv2, out_conv3, out_conv4 + add4)."""
        out1 = _first_block(self.conv1, x, c_enc)
        out2 = self.conv2(out1)
        out3 = self.conv3(out2)
        return out1, out2, out3, self.conv4(out3, add4)


def clip_spatial(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """tfnet.py:257-258 on NDHWC tensors."""
    return a[:, :b.shape[1], :b.shape[2], :b.shape[3]]


class LES(nn.Module):
    """tfnet.py:261-368."""

    def __init__(self, n_features: int, c_local_features: int, c_global_features: int, context_window: int, kernel_size,
                 dropout_rate, temporal_filtering_length):
        super().__init__()
        self.n_features, self.c_local_features, self.c_global_features = n_features, c_local_features, c_global_features
        self.context_window = context_window
        self.spatial_filter = nn.Conv3d(1, 1, kernel_size=3, padding=1, bias=False)
        self.temporal_filter = nn.Conv3d(temporal_filtering_length, 1, kernel_size=1, padding=0, bias=False)
        self.temporal_filtering_length = temporal_filtering_length
        filtered_dim = n_features * (context_window - temporal_filtering_length + 1)
        self.encoder_bar = Encoder(filtered_dim, c_local_features, kernel_size, dropout_rate)
        self.encoder_tilde = Encoder(filtered_dim, c_local_features, kernel_size, dropout_rate)
        self.encoder_prime = Encoder(filtered_dim, c_local_features, kernel_size, dropout_rate)
        self.deconv3 = deconv(512, 256)
        self.deconv2 = deconv(256, 128)
        self.deconv1 = deconv(128, 64)
        self.deconv0 = deconv(64, 32)
        self.output_layer = nn.Conv3d(32, n_features, kernel_size=kernel_size, padding=(kernel_size - 1) // 2)
        self.encode_conditioning_calls = 0  # how often the conditioning branches ran (an eval rollout runs them once)

    @property
    def encoders(self):
        return self.encoder_bar, self.encoder_tilde, self.encoder_prime

    # ---- tfnet.py:304-337, fp32 torch ops on (B, T, F, X, Y, Z)
    def decompose(self, xx: torch.Tensor):
        """(u_bar, u_tilde, u_prime), each (B, (T - L + 1) F, X, Y, Z) fp32."""
        xx = xx.float()
        L = self.temporal_filtering_length
        u_star = F.conv3d(xx.reshape(-1, 1, *xx.shape[-3:]), self.spatial_filter.weight, padding=1).reshape(xx.shape)
        u_prime = xx - u_star
        n = xx.shape[1] - L + 1
        w = self.temporal_filter.weight.reshape(L)
        u_bar = sum(w[l] * u_star[:, l:l + n] for l in range(L))  # the 1x1 conv over each window of L steps
        u_tilde = u_star[:, -n:] - u_bar
        return tuple(u.flatten(1, 2) for u in (u_bar, u_tilde, u_prime[:, -n:]))

    def encode_conditioning(self, C, dtype):
        """[conv1_local(c_local[None]) of the three encoders], each (1, X/2, Y/2, Z/2, 64) in `dtype`; None without a
        local conditioning."""
        if global_conditioning(C) is not None:
            raise RuntimeError("Global conditioning not implemented for TFNet")
        c = local_conditioning(C)
        if c is None:
            return None
        self.encode_conditioning_calls += 1
        c = _to_nvc_padded(c.unsqueeze(0).float(), _up8(c.shape[0]), dtype)
        return [e.encode_conditioning(c) for e in self.encoders]

    def forward(self, xx: torch.Tensor, C, dtype=None, c_enc=None) -> torch.Tensor:
        """xx (B, T, F, X, Y, Z) -> (B, F, X, Y, Z) fp32; the network runs in `dtype` (default: that of xx).  `c_enc`: what
        `encode_conditioning` returned (eval mode only)."""
        dtype = dtype or xx.dtype
        if c_enc is None or self.training:
            c_enc = self.encode_conditioning(C, dtype)
        c_enc = c_enc or (None, None, None)
        sw, tw = self.spatial_filter.weight, self.temporal_filter.weight
        if FUSE_DECOMPOSE and ops.flow_decompose_supported(xx, sw, tw, dtype):
            stacks = ops.flow_decompose(xx, sw, tw, dtype)
        else:
            stacks = self.decompose(xx)
            cp = _up8(stacks[0].shape[1])
            stacks = (_to_nvc_padded(u, cp, dtype) for u in stacks)  # made one at a time, as each encoder takes its own
        levels, sum4 = [], None
        for enc, u, c in zip(self.encoders, stacks, c_enc):
            o1, o2, o3, sum4 = enc(u, c, sum4)
            levels.append((o1, o2, o3))
        out1, out2, out3 = (a + b + c for a, b, c in zip(*levels))
        d3 = self.deconv3(sum4)
        d2 = self.deconv2(out3 + clip_spatial(d3, out3))
        d1 = self.deconv1(out2 + clip_spatial(d2, out2))
        d0 = self.deconv0(out1 + clip_spatial(d1, out1))
        k = self.output_layer
        w, b = _pad_conv(k, 32, _up8(self.n_features))
        X, Y, Z = xx.shape[-3:]
        out = ops.conv3d(d0[:, :X, :Y, :Z].contiguous(), w, b, stride=1, padding=k.padding[0])
        return out[..., :self.n_features].movedim(-1, 1).float()
