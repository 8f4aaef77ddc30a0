"""The bits of the reverse-step, loss and Philox kernels of csrc/tdx_ddpm.hip: the cases shared by
tests/test_reverse_step_bits.py and tests/golden/make_golden_bits.py.

`run(group)` launches every case of one group through `turbdiff_amd.ops` on the GPU and returns, per case,

    {"sha256": digest of the outputs' float32 bytes (the launches of the case, in order),
     "after":  [[offset, t] or [offset, k, t] per launch]      in-kernel-noise entries and the Philox fills,
     "loss":   [hex of the float32 loss values per launch]     loss cases (TDX_DETERMINISTIC=1: order-independent sums),
     "bits":   [hex of the output's bytes per launch]}         smallest shape only, so a mismatch there reads in ulps

Inputs are the CPU generator draws the GPU tests use (`rnd(..., seed=)`, `_mask_idx`, `_loss_inputs`); nothing else is stored.
"""

import contextlib
import os

import torch

from pinned_bits import record as _record, tensor_bytes as _bytes
from step_inputs import _loss_inputs, _mask_idx, _tables, rnd

T, S = 10, 4  # the log-snr-linear schedule of the step tests; the DDIM subsequence of T
SEED, OFF0, UNTOUCHED = 1234, 4096, 77
SIDS = [(5 << 32) | 7, 11, (1 << 32) | 2]  # three distinct trajectory streams, two with a nonce in the high word
SMALLEST = (1, 4, 2, 2, 1)  # one quad per plane
# (3,4,6,5,4): quads that straddle the mask edge; (1,4,3,3,3): V = 27, no multiple of 4; (2,4,40,33,28): V = 36 960 >
# 128 * 256, the scalar grid-stride loop takes a second trip; (1,4,48,48,32): F V / 4 = 73 728 > 256 * 256, the 4-wide loop
# takes a second trip and i % v4 wraps with i past the first stride
SHAPES = {
    "tensor": [SMALLEST, (3, 4, 6, 5, 4), (1, 4, 3, 3, 3), (2, 4, 40, 33, 28)],
    "rng": [SMALLEST, (3, 4, 6, 5, 4), (2, 4, 40, 33, 28), (1, 4, 48, 48, 32)],
}
RULES = ("ancestral", "lv", "ddim")
# step index 0, 1 and one middle value; DDIM: the same at eta = 0 and eta = 1
STEPS = {"ancestral": [(None, t) for t in (0, 1, 5)], "lv": [(None, t) for t in (0, 1, 5)],
         "ddim": [(eta, k) for eta in (0.0, 1.0) for k in (0, 1, 2)]}
LOSS_SHAPES = [(2, 4, 6, 5, 4), (2, 4, 7, 5, 3), (2, 4, 40, 33, 28)]  # vector, scalar (V = 105), multi-block
ELBO_T = ([6, 0], [0, 0], [T - 1, 1])
RANDN_N = (5, 36960)

GROUPS = [f"{rule}/{entry}" for rule in RULES for entry in ("tensor", "rng")] + ["masked_loss", "elbo_loss", "randn"]
FIXTURE = "reverse_step_bits.json"


@contextlib.contextmanager
def _deterministic():
    old = os.environ.get("TDX_DETERMINISTIC")
    os.environ["TDX_DETERMINISTIC"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["TDX_DETERMINISTIC"]
        else:
            os.environ["TDX_DETERMINISTIC"] = old


def _name(shape, **flags):
    return "x".join(map(str, shape)) + "".join(f"/{k}{int(v)}" for k, v in flags.items())


def _steps(ops, rule, entry, d):
    from turbdiff_amd import schedules

    tab, packed = _tables("log-snr-linear", T)
    packed, plv = packed.to(d), tab["posterior_log_var"].to(d)
    taus = schedules.ddim_timesteps(T, S)
    tau_d = torch.tensor(taus, device=d)
    ddim_tab = {eta: schedules.ddim_tables("log-snr-linear", T, taus, eta).to(d) for eta in (0.0, 1.0)}
    i64 = lambda v: torch.tensor([v], dtype=torch.int64, device=d)
    res = {}
    for shape in SHAPES[entry]:
        B, F = shape[:2]
        V = shape[2] * shape[3] * shape[4]
        x_t, eps, xb, z, z2 = (rnd(*shape, seed=s).to(d) for s in range(5))
        mo = rnd(B, 2 * F, *shape[2:], seed=5).to(d)
        mask = ops.cell_mask(_mask_idx(V).to(d), V)
        sids = torch.tensor(SIDS[:B], dtype=torch.int64, device=d)
        for nb in (True, False):
            for clip in (False, True):
                outs, after = [], []
                for eta, step in STEPS[rule]:
                    idx, off, t_d = i64(step), i64(OFF0), i64(UNTOUCHED)
                    noise = (z, z2) if entry == "tensor" else ()
                    rng = () if entry == "tensor" else (SEED, sids, off)
                    if rule == "ancestral":
                        fn = ops.p_sample_step if entry == "tensor" else ops.p_sample_step_rng
                        outs.append(fn(x_t, eps, *noise, xb, mask, packed, T, idx, nb, clip, *rng))
                        after.append([int(off), int(idx)])
                    elif rule == "lv":
                        fn = ops.p_sample_step_lv if entry == "tensor" else ops.p_sample_step_lv_rng
                        outs.append(fn(x_t, mo, *noise, xb, mask, packed, plv, T, idx, nb, clip, *rng))
                        after.append([int(off), int(idx)])
                    else:
                        fn = ops.ddim_step if entry == "tensor" else ops.ddim_step_rng
                        outs.append(fn(x_t, eps, *noise, xb, mask, ddim_tab[eta], idx, tau_d, t_d, nb, clip, *rng))
                        after.append([int(off), int(idx), int(t_d)])
                more = {"after": after} if entry == "rng" else {}
                res[_name(shape, nb=nb, clip=clip)] = _record(outs, shape == SMALLEST, **more)
    return res


def _masked_loss(ops, d):
    res = {}
    for shape in LOSS_SHAPES:
        V = shape[2] * shape[3] * shape[4]
        idx = _mask_idx(V)
        mask = ops.cell_mask(idx.to(d), V)
        n = rnd(*shape, seed=2).to(d)
        for l1 in (False, True):
            e = rnd(*shape, seed=1).to(d).requires_grad_()
            loss = ops.masked_loss(e, n, mask, idx.numel(), l1=l1)
            loss.backward()
            res[_name(shape, l1=l1)] = _record([e.grad], loss=[_bytes(loss.reshape(1)).hex()])
    return res


def _elbo_loss(ops, d):
    tab, packed = _tables("log-snr-linear", T)
    packed, plv = packed.to(d), tab["posterior_log_var"].to(d)
    res = {}
    for shape in LOSS_SHAPES:
        V = shape[2] * shape[3] * shape[4]
        idx = _mask_idx(V)
        mask = ops.cell_mask(idx.to(d), V)
        for l1 in (False, True):
            for clip in (False, True):
                for detach in (True, False):
                    grads, losses = [], []
                    for tt in ELBO_T:
                        t = torch.tensor(tt)
                        out, noise, x_start, x_t = (v.to(d) for v in _loss_inputs(shape, t, clip, tab))
                        out.requires_grad_()
                        total, parts = ops.elbo_loss(out, noise, x_start, x_t, mask, idx.numel(), t.to(d), packed, plv, l1=l1,
                                                     clip=clip, detach_mean=detach, elbo_weight=0.1, parts=True)
                        total.backward()
                        grads.append(out.grad)
                        losses.append(_bytes(torch.cat([total.detach().view(1), parts])).hex())
                    res[_name(shape, l1=l1, clip=clip, detach=detach)] = _record(grads, loss=losses)
    return res


def _randn(ops, d):
    res = {}
    sids = torch.tensor(SIDS, dtype=torch.int64, device=d)
    for n in RANDN_N:
        off = torch.full((1,), OFF0, dtype=torch.int64, device=d)
        a = ops.randn_philox(torch.empty(n, device=d), SEED, SIDS[0], off)
        res[f"randn_philox/{n}"] = _record([a], n == RANDN_N[0], after=[[int(off)]])
        off.fill_(OFF0)
        b = ops.randn_philox_batched(torch.empty(len(SIDS), n, device=d), SEED, sids, off)
        res[f"randn_philox_batched/{n}"] = _record([b], n == RANDN_N[0], after=[[int(off)]])
    return res


def run(group):
    """The records of one group of GROUPS, from the library `turbdiff_amd.ops` is bound to."""
    from turbdiff_amd import ops

    d = torch.device("cuda:0")
    if "/" in group:
        return _steps(ops, *group.split("/"), d)
    if group == "randn":
        return _randn(ops, d)
    with _deterministic():
        return _masked_loss(ops, d) if group == "masked_loss" else _elbo_loss(ops, d)
