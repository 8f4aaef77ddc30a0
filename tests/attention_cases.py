"""Input builders shared by the attention tests (test_hip_ops.py, test_attention_backward.py)."""

import torch


def growing_scores_qkv(B, N, H, D, seed=5):
    """float32 q, k, v of shape (B, N, H, D) that exercise large logits: scores that keep GROWING along the key index for
    the queries that look along +u, queries of very different norms (0.1 .. 5 times N(0,1)), and one outlier key of norm 40
    that no query aligns with.  |q| |k| / sqrt(D) reaches ~200."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, N, H, D, generator=g) * torch.logspace(-1, 0.7, N).reshape(1, N, 1, 1)[:, torch.randperm(N, generator=g)]
    u = torch.nn.functional.normalize(torch.randn(B, 1, H, D, generator=g), dim=-1)
    ramp = torch.linspace(-6.0, 6.0, N).reshape(1, N, 1, 1)
    k = torch.randn(B, N, H, D, generator=g) * 0.3 + u * ramp          # scores grow with the key index for q along +u
    q = q + 2.0 * u * (torch.rand(B, N, H, 1, generator=g) > 0.5)       # half of the queries look along +u
    k[:, N // 3] = 40.0 * torch.nn.functional.normalize(torch.randn(B, H, D, generator=g), dim=-1)  # the outlier
    v = torch.randn(B, N, H, D, generator=g)
    return q, k, v


# ---- what the library plans for a call (csrc/tdx_attention.hip: attn_plan), restated from the documented rule (include/tdx.h)
ARENA_ZERO = 64                                   # the arena's zero block
ARENA_KMAX = 256 * 4                              # key-norm table: one float per (b, h), at most 256
ARENA_PART = 512 * 2 * 256 * 34 * 4               # stream-K partials: 512 workgroups x 2 slots x 256 queries x (O[32], m, l) f32
ARENA_STREAMK = ARENA_ZERO + ARENA_KMAX + ARENA_PART  # smallest arena under which stream-K runs
H16_CODES = (1, 3)                                # TDX_BF16, TDX_F16
PLAN_ENV = {"TDX_ATTN_IMPL": "0", "TDX_ATTN_STREAMK": "1", "TDX_ATTN_BOUND": "1", "TDX_ATTN_BWD_TW": "22"}  # the defaults


def expected_plan(B, N, H, D, dtype, env=None, arena=0):
    """The dict turbdiff_amd._lib.attn_plan must return: `env` {switch: value} over the defaults, `arena` the bound arena's
    bytes (0: none)."""
    env = {**PLAN_ENV, **(env or {})}
    zero = dict.fromkeys(("nqb", "ntile", "nwg", "chunk", "streamk", "bound", "tw_dq", "tw_dkv", "bwd_gx", "bwd_gy", "workspace"), 0)
    if D != 32 or dtype not in (0, 1, 3):
        return {**zero, "fwd": "vector", "bwd": "vector", "status": -2 if D != 32 else -3}
    cdiv = lambda a, b: -(-a // b)
    ws = min(4 * B * N * H, 2**31 - 1)
    if not (dtype in H16_CODES and env["TDX_ATTN_IMPL"] not in ("1", "vector") and N >= 128):
        return {**zero, "fwd": "vector", "bwd": "vector", "status": 0, "bwd_gx": cdiv(N, 64), "bwd_gy": B * H, "workspace": ws}
    nqb, ntile = cdiv(N, 256), cdiv(N, 64)
    nblk = B * H * nqb
    streamk = env["TDX_ATTN_STREAMK"] == "1" and nblk > 512 and nblk % 512 != 0 and ntile >= 16 and arena >= ARENA_STREAMK
    bound = env["TDX_ATTN_BOUND"] == "1" and arena >= ARENA_ZERO + ARENA_KMAX and B * H <= 256 and ntile >= 8
    tw = int(env["TDX_ATTN_BWD_TW"])
    return {"fwd": "mfma", "bwd": "mfma", "status": 0, "nqb": nqb, "ntile": ntile, "nwg": 512 if streamk else nblk,
            "chunk": cdiv(nblk * ntile, 512) if streamk else ntile, "streamk": int(streamk), "bound": int(bound),
            "tw_dq": tw // 10, "tw_dkv": tw % 10, "bwd_gx": cdiv(N, 256), "bwd_gy": B * H, "workspace": ws}
