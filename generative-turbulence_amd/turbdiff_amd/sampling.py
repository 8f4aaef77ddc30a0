"""hipGraph-captured DDPM ancestral sampler (BASELINE.json configs[3]).

The reference's loop (ddpm.py:767-816) pays per step: a host->device scalar for t, ~12 small
elementwise kernels, two index scatters and the Python/launch overhead of ~400 kernels of the
U-Net.  Here ONE reverse step -- U-Net forward, then one kernel that draws the two Philox
noises where they are consumed and applies the update, then the on-device advance of the RNG
offset and decrement of t -- is captured once into a hipGraph and replayed T times;
nothing in the step touches the host.  The timestep and the RNG offset live in device memory,
so a replay needs no new arguments.

Noise comes from a counter-based generator keyed by (seed, trajectory id, offset): results do
not depend on how trajectories are sharded over GPUs.

With `sampling_timesteps = S` the same captured step walks an increasing subsequence tau of S training timesteps with
the generalized DDIM update of Song et al. 2021 (`tdx_ddim_step_rng`; eta = 0 deterministic, eta = 1 the posterior
variance of the sub-sampled chain) instead of the T ancestral ones: the step index k, tau and the [6, S] coefficient
table live in device memory next to t, so a replay still needs no new arguments.

A model with learned variances (`diffusion.learned_variances`, Nichol & Dhariwal 2021) runs the same captured ancestral
step with `tdx_p_sample_step_lv_rng` as its update: the decoder emits [eps_hat | w] and the noise is scaled per voxel.
Over S of T steps such a model is sampled on request, `sampling_method=`: "respaced" is the ancestral step of the shorter
chain over tau with the learned variance interpolating between its own beta' and beta~' (`tdx_p_sample_step_lv_respaced_rng`,
an [8, S] table), "ddim" the DDIM step on the eps_hat half of the output (`tdx_ddim_step_lv_rng`, w never read).
`check_sampling_arguments` is the one place that decides which update a call gets.
"""

from __future__ import annotations

import gc

import torch

from . import _lib as L
from . import ops, schedules

# module constants (tests flip them; they were environment A/B switches while the two routes were being compared):
# FUSED_STEP_NOISE = False: draw z / z2 into tensors with tdx_randn_batched and run tdx_p_sample_step on them (same values);
# COND_TABLE = False: the time MLP runs every reverse step instead of one look-up in a per-timestep table
FUSED_STEP_NOISE = True
COND_TABLE = True


def check_ddim_arguments(diffusion, sampling_timesteps, eta, start_from=None):
    """ValueError for what the DDIM sampler does not cover: learned variances (the per-voxel variance has no DDIM
    counterpart here), a step count outside [1, L], eta outside [0, 1]."""
    if getattr(diffusion, "learned_variances", False):
        raise ValueError("sampling_timesteps needs fixed variances: learned_variances=True has no DDIM counterpart here")
    if not 0.0 <= float(eta) <= 1.0:
        raise ValueError(f"eta = {eta} outside [0, 1]")
    schedules.ddim_timesteps(diffusion.num_timesteps, sampling_timesteps, start_from)


SAMPLING_METHODS = ("ddim", "respaced")


def check_sampling_arguments(diffusion, sampling_timesteps, eta, start_from=None, sampling_method=None):
    """Which update a sampling call gets: None = the ancestral loop over all T steps (fixed or learned variances), "ddim" =
    the DDIM step of a fixed-variance model, "lv-respaced" / "lv-ddim" = the two samplers of a learned-variance model over
    `sampling_timesteps` steps.  ValueError for every combination outside that: a method without a step count; a
    learned-variance model with a step count and no method (a call that raised before the two samplers existed keeps
    raising: they are opt-in); "respaced" for fixed variances (DDIM with eta covers the stochastic case there) or with
    eta != 0 (it has no meaning there); an unknown method; S, start_from or eta out of range."""
    if sampling_method is not None and sampling_method not in SAMPLING_METHODS:
        raise ValueError(f"sampling_method = {sampling_method!r} is none of {SAMPLING_METHODS}")
    if sampling_timesteps is None:
        if sampling_method is not None:
            raise ValueError(f"sampling_method = {sampling_method!r} needs sampling_timesteps")
        return None
    learned = bool(getattr(diffusion, "learned_variances", False))
    if not learned:
        if sampling_method == "respaced":
            raise ValueError('sampling_method="respaced" is the sampler of a model with learned variances; a fixed-variance '
                             'model is sampled over fewer steps by "ddim" (eta > 0 for a stochastic chain)')
        check_ddim_arguments(diffusion, sampling_timesteps, eta, start_from)
        return "ddim"
    if sampling_method is None:
        raise ValueError("sampling_timesteps with learned_variances=True needs a choice of sampler: "
                         'sampling_method="respaced" (the ancestral step of the shorter chain, learned variance kept) or '
                         'sampling_method="ddim" (DDIM on the eps_hat half of the output)')
    if sampling_method == "respaced" and float(eta) != 0.0:
        raise ValueError(f'eta = {eta} has no meaning for sampling_method="respaced": its variance is the learned one')
    if not 0.0 <= float(eta) <= 1.0:
        raise ValueError(f"eta = {eta} outside [0, 1]")
    schedules.ddim_timesteps(diffusion.num_timesteps, sampling_timesteps, start_from)
    return "lv-" + sampling_method


# ---- the update rules of a GraphSampler `s`: (ops entry that draws its noise, ops entry on noise tensors, the operands
# between the mask and noise_bcs, the scalar advance the second entry leaves to its caller).  Plain functions of the sampler:
# stored on it they close over nothing, so they add no reference cycle that would keep its captured graph and pool alive.
def _advance_t(s):
    s.t.sub_(1)


def _advance_ddim(s):
    s.k.sub_(1)
    s.t.copy_(s.tau.index_select(0, s.k.clamp(min=0)))  # after the last step: stays tau[0]


# x_t -> x_{t-1}, then t -= 1; with learned variances the same on the model's output [eps_hat | w], the noise scaled per voxel
_ANCESTRAL = (ops.p_sample_step_rng, ops.p_sample_step, lambda s: (s.d.step_tables, s.d.num_timesteps, s.t), _advance_t)
_LEARNED_VARIANCES = (ops.p_sample_step_lv_rng, ops.p_sample_step_lv,
                      lambda s: (s.d.step_tables, s.d.posterior_log_var, s.d.num_timesteps, s.t), _advance_t)
# x_{tau_k} -> x_{tau_{k-1}}, then k -= 1 and t = tau[k] on the device
_DDIM = (ops.ddim_step_rng, ops.ddim_step, lambda s: (s.ddim_table, s.k, s.tau, s.t), _advance_ddim)
# the same walk for a model with learned variances (the table is [8, S] for the first, [6, S] for the second)
_LV_RESPACED = (ops.p_sample_step_lv_respaced_rng, ops.p_sample_step_lv_respaced, _DDIM[2], _advance_ddim)
_LV_DDIM = (ops.ddim_step_lv_rng, ops.ddim_step_lv, _DDIM[2], _advance_ddim)
_RULES = {"ddim": _DDIM, "lv-respaced": _LV_RESPACED, "lv-ddim": _LV_DDIM}


class GraphSampler:
    """One captured reverse step, replayed T times.  Everything the captured step reads lives in buffers the sampler
    OWNS (boundary values, conditioning tensors, in-domain mask, cached conditioning conv), so `rebind` can point an
    existing graph at another batch / geometry of the same shape by copying into them -- `GaussianDiffusion.
    p_sample_loop` keeps one sampler per input shape and re-uses its graph from call to call."""

    def __init__(self, diffusion, x_bcs, C, cell_idx, seed: int = 0, trajectory_ids=None, use_graph: bool = True, nonce: int = 0,
                 capture_stream=None, sampling_timesteps: int | None = None, eta: float = 0.0,
                 sampling_method: str | None = None):
        self.d = diffusion
        self.sampling_timesteps = None if sampling_timesteps is None else int(sampling_timesteps)
        self.eta = float(eta)
        self.sampling_method = sampling_method
        update = check_sampling_arguments(diffusion, self.sampling_timesteps, self.eta, None, sampling_method)
        self.x_bcs = x_bcs.detach().float().contiguous().clone()
        self.C = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in C.items()} if isinstance(C, dict) else C
        B = self.x_bcs.shape[0]
        dev = self.x_bcs.device
        self.B, self.dev, self.seed = B, dev, int(seed)
        V = self.x_bcs[0, 0].numel()
        self.mask = diffusion.domain_mask(cell_idx, V)[0].clone()
        ids = list(range(B)) if trajectory_ids is None else list(trajectory_ids)
        assert len(ids) == B
        # Philox key = `seed` (a launch argument: fixed once captured); counter words = (offset + element, stream id);
        # stream id = trajectory id in the low 32 bits, `nonce` in the high 31: the nonce lives in device memory, so a
        # captured graph draws fresh noise per call without a re-capture (p_sample_loop passes one per call)
        self.stream_ids = torch.tensor(self._sids(ids, nonce), dtype=torch.int64, device=dev)
        self.offset = torch.zeros(1, dtype=torch.int64, device=dev)
        self.t = torch.zeros(1, dtype=torch.int64, device=dev)
        # S of T steps: step index k into the subsequence tau and the coefficient table ([6, S] DDIM rows, or the [8, S]
        # rows of the respaced chain), all on the device (the shapes are fixed by S, so `reset(start_from)` refills them
        # under a captured graph)
        S = self.sampling_timesteps
        self._update = update
        rows = len(schedules.RESPACED_PACKED_ORDER if update == "lv-respaced" else schedules.DDIM_PACKED_ORDER)
        self.k = None if S is None else torch.zeros(1, dtype=torch.int64, device=dev)
        self.tau = None if S is None else torch.zeros(S, dtype=torch.int64, device=dev)
        self.ddim_table = None if S is None else torch.zeros(rows, S, dtype=torch.float32, device=dev)
        self._taus = None  # host copy of what self.tau / self.ddim_table hold
        self.x_t = torch.empty_like(self.x_bcs)
        # noise drawn inside the update kernel (tdx_p_sample_step_rng) unless the layout rules that out; only then do the
        # two noise tensors exist at all
        self.fused_noise = FUSED_STEP_NOISE and ops.p_sample_step_rng_supported(self.x_t)
        self.z = None if self.fused_noise else torch.empty_like(self.x_bcs)
        self.z2 = None if self.fused_noise or not diffusion.noise_bcs else torch.empty_like(self.x_bcs)
        self.use_graph = use_graph
        self.graph = None
        # ONE stream for every capture of this sampler (its scratch arena is per stream); samplers of one diffusion share it
        self._capture_stream = capture_stream
        with torch.no_grad():
            self.enc = diffusion.model.encode_local(self.C)
        self.c_table = None  # (T, c_dim) conditioning vectors per timestep (DenoisingModel.conditioning_table) or None
        self._table_versions = None
        rule = _RULES[update] if update is not None else (
            _LEARNED_VARIANCES if getattr(diffusion, "learned_variances", False) else _ANCESTRAL)
        self._fused, self._plain, self._operands, self._advance = rule  # the update, chosen once
        self._refresh_tables()
        self.reset()

    @staticmethod
    def _sids(ids, nonce):
        assert 0 <= int(nonce) < 2**31 and all(0 <= int(i) < 2**32 for i in ids)
        return [(int(nonce) << 32) | int(i) for i in ids]

    @staticmethod
    def signature_of(diffusion, x_bcs, C, sampling_timesteps=None, eta=0.0, sampling_method=None):
        """What must match for `rebind`: shapes / dtypes of everything the captured step reads, and the switches the
        captured step was built under.  The last two entries name the update the step applies: None = the ancestral step
        with fixed variances, "learned-variances" = the ancestral step with the per-voxel variance (read with getattr:
        stand-ins for a diffusion need not carry the attribute), an int = the DDIM subsequence length of a fixed-variance
        model, ("learned-variances", method, S) = one of the two samplers of a learned-variance model over S steps; and
        eta.  `sampling_method` changes the signature of no call that leaves it out."""
        c = tuple(sorted((str(k), tuple(v.shape), str(v.dtype)) for k, v in C.items() if torch.is_tensor(v))) \
            if isinstance(C, dict) else None
        m = diffusion.model
        learned = getattr(diffusion, "learned_variances", False)
        if sampling_timesteps is None:
            update = "learned-variances" if learned else None
        elif learned and sampling_method is not None:
            update = ("learned-variances", str(sampling_method), int(sampling_timesteps))
        else:
            update = int(sampling_timesteps)
        return (tuple(x_bcs.shape), str(x_bcs.device), c, getattr(m, "compute_dtype", None), getattr(m, "conv_impl", None),
                L.conv_impl(), diffusion.noise_bcs, diffusion.clip_denoised, diffusion.num_timesteps, update, float(eta))

    def signature(self):
        return self.signature_of(self.d, self.x_bcs, self.C, self.sampling_timesteps, self.eta, self.sampling_method)

    @torch.no_grad()
    def rebind(self, x_bcs, C, cell_idx, nonce=None, trajectory_ids=None):
        """Another batch (and possibly another geometry) of the SAME shapes: copy it into the buffers the captured graph
        reads.  The cached conditioning conv is recomputed into its existing tensors."""
        self.x_bcs.copy_(x_bcs)
        if isinstance(self.C, dict):
            for k, v in C.items():
                if torch.is_tensor(v):
                    self.C[k].copy_(v)
        self.mask.copy_(self.d.domain_mask(cell_idx, self.x_bcs[0, 0].numel())[0])
        self._refresh_enc()
        if nonce is not None or trajectory_ids is not None:
            ids = [int(i) & 0xFFFFFFFF for i in self.stream_ids.tolist()] if trajectory_ids is None else list(trajectory_ids)
            nn = int(self.stream_ids[0].item()) >> 32 if nonce is None else nonce
            self.stream_ids.copy_(torch.tensor(self._sids(ids, nn), dtype=torch.int64))
        return self

    @torch.no_grad()
    def _refresh_enc(self):
        """encode_local(C) (and the cached conditioning conv hanging off it) again, into the tensors the captured graph
        reads: after another geometry was bound or the weights changed."""
        if self.enc is None:
            return
        enc = self.d.model.encode_local(self.C)
        old, new = getattr(self.enc, "first_conv_partial", None), getattr(enc, "first_conv_partial", None)
        if (old is None) != (new is None) or enc.shape != self.enc.shape or enc.dtype != self.enc.dtype:
            self.enc, self.graph = enc, None  # another structure than the captured one: capture again on these tensors
        else:
            self.enc.copy_(enc)
            if old is not None:
                old[1].copy_(new[1])

    @torch.no_grad()
    def _refresh_tables(self):
        """What the step reads that is a function of the WEIGHTS (and the bound geometry) alone: recomputed into the same
        tensors after a weight update (the captured graph keeps their addresses)."""
        if getattr(self, "_table_versions", None) is not None:  # not the constructor's call: enc was just made there
            self._refresh_enc()
        tab = self.d.model.conditioning_table(self.C, self.d.num_timesteps) if COND_TABLE else None
        old = self.c_table
        if tab is not None and old is not None and tab.shape == old.shape and tab.dtype == old.dtype:
            old.copy_(tab)
        else:
            if tab is not None or old is not None:
                self.graph = None  # another structure than the captured one
            self.c_table = tab
        self._table_versions = [(p, p._version) for p in self.d.parameters()]

    def _changed(self, seen) -> bool:
        """Have the diffusion's parameters changed since `seen` = [(tensor, version)] was recorded -- updated in place
        (optimiser step, load_state_dict) or replaced by other tensors (another model assigned, .to(device))?"""
        cur = list(self.d.parameters())
        return len(cur) != len(seen) or any(p is not q or p._version != v for p, (q, v) in zip(cur, seen))

    def _tables_stale(self) -> bool:
        return self._changed(self._table_versions)

    # ---- state
    def _randn(self, out):
        return ops.randn_philox_batched(out, self.seed, self.stream_ids, self.offset)

    @torch.no_grad()
    def reset(self, start_from: int | None = None):
        """x_T ~ N(0, I) (or q_sample(x_bcs, start_from - 1)); t <- T - 1; RNG offset <- 0.  S of T steps: tau and the
        table are refilled when `start_from` changes them; k <- S - 1, t <- tau[S - 1]."""
        d = self.d
        self.offset.zero_()
        T = d.num_timesteps if start_from is None else start_from
        if self.sampling_timesteps is None:
            self.t.fill_(T - 1)
            steps = T
        else:
            steps = self.sampling_timesteps
            taus = schedules.ddim_timesteps(d.num_timesteps, steps, start_from)
            if taus != self._taus:
                self.tau.copy_(torch.tensor(taus, dtype=torch.int64))
                self.ddim_table.copy_(
                    schedules.respaced_tables(d.beta_schedule, d.num_timesteps, taus) if self._update == "lv-respaced"
                    else schedules.ddim_tables(d.beta_schedule, d.num_timesteps, taus, self.eta))
                self._taus = taus
            self.k.fill_(steps - 1)
            self.t.fill_(taus[-1])
        self._randn(self.x_t)
        if start_from is not None:
            tt = torch.full((1,), start_from - 1, dtype=torch.int64, device=self.dev)
            self.x_t.copy_(ops.q_sample(self.x_bcs, self.x_t, d.sqrt_alphas_cumprod, d.sqrt_one_minus_alphas_cumprod, tt))
        if not d.noise_bcs:
            self.x_t.copy_(torch.where(self.mask.view(self.x_t.shape[-3:]).bool(), self.x_t, self.x_bcs))
        self.steps_left = steps

    # ---- one reverse step (graph body)
    def _step(self):
        d = self.d
        kw = {"encoded_local": self.enc} if self.enc is not None else {}
        if self.c_table is not None:
            # all trajectories are at the same t: one row of the table instead of the time MLP (~12 launches per step)
            kw["cond"] = self.c_table.index_select(0, self.t).expand(self.B, -1)
        out = d.model(self.x_t, self.t.expand(self.B), self.C, **kw)
        if self.fused_noise:
            # same draws, same counters, bit-identical x_{t-1}; also advances the offset and the step scalars
            self._fused(self.x_t, out, self.x_bcs, self.mask, *self._operands(self), d.noise_bcs, d.clip_denoised, self.seed,
                        self.stream_ids, self.offset, out=self.x_t)
            return
        self._randn(self.z)
        if d.noise_bcs:
            self._randn(self.z2)
        self._plain(self.x_t, out, self.z, self.z2 if d.noise_bcs else None, self.x_bcs, self.mask, *self._operands(self),
                    d.noise_bcs, d.clip_denoised, out=self.x_t)
        self._advance(self)

    @torch.no_grad()
    def _capture(self):
        # warm up on the sampler's own side stream (packs weights, sizes the allocator, creates that stream's scratch
        # arena), then capture on the same stream: the conv kernels' arena is bound per stream (_lib.ensure_scratch), so
        # nothing is allocated inside the capture and the replayed graph never shares an arena with eager work on another
        # stream.  Re-captures (after a weight update) re-use the stream -- and with it the arena.
        state = (self.x_t.clone(), self.t.clone(), self.offset.clone(), None if self.k is None else self.k.clone())
        if self._capture_stream is None:
            self._capture_stream = torch.cuda.Stream(device=self.dev)
        s = self._capture_stream
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._step()
            self._arena = L.scratch_arena(self.dev)  # held for as long as the graph lives (the arena map is bounded)
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        # capture_error_mode "thread_local": only THIS thread's calls are checked against the capture.  In a process with an RCCL
        # communicator the watchdog thread of ProcessGroupNCCL polls the events of recent collectives (a barrier just before the
        # sampling leg is enough); under the default "global" mode its hipEventQuery during our capture raises
        # hipErrorStreamCaptureUnsupported and aborts the process (seen in 2 of 6 runs of the captured data-parallel step)
        with torch.cuda.graph(self.graph, stream=s, capture_error_mode="thread_local"):
            self._step()
        self.x_t.copy_(state[0]); self.t.copy_(state[1]); self.offset.copy_(state[2])
        if self.k is not None:
            self.k.copy_(state[3])
        # The graph has the addresses of the packed weight operands (ops._pack_cache) baked in.  Keep those
        # buffers alive for as long as the graph lives, and remember the parameter versions they were packed
        # from: a weight update (optimiser step, load_state_dict) makes replay() re-capture instead of running on
        # stale operands.
        self._held = list(ops._pack_cache.values())
        self._versions = [(p, p._version) for p in self.d.parameters()]

    def _stale(self) -> bool:
        return self._changed(self._versions)

    @torch.no_grad()
    def run_steps(self, n: int, pbar: bool = False):
        n = min(n, self.steps_left)
        if n <= 0:
            return self.x_t  # finished trajectory: t is -1, a warm-up / capture step would index the tables out of range
        if self._tables_stale():
            self._refresh_tables()
        if self.use_graph and (self.graph is None or self._stale()):
            # a dead sampler (a dropped diffusion and the samplers in its cache form a cycle) frees its captured graph when the
            # collector finds it; inside a capture that aborts the process.  Collect before the capture, never during it.
            gc.collect()
            was_enabled = gc.isenabled()
            gc.disable()
            try:
                self._capture()
            finally:
                if was_enabled:
                    gc.enable()
        steps = range(n)
        if pbar:
            from tqdm.auto import tqdm

            steps = tqdm(steps, desc="sampling loop time step", total=n, position=1)
        for _ in steps:
            if self.use_graph:
                self.graph.replay()
            else:
                self._step()
        self.steps_left -= n
        return self.x_t

    @torch.no_grad()
    def sample(self, start_from: int | None = None, pbar: bool = False):
        """Full trajectory; returns the (B, F, X, Y, Z) sample with BC cells set to x_bcs."""
        self.reset(start_from)
        self.run_steps(self.steps_left, pbar=pbar)
        return self.x_t.clone()

    # ---- the same noise, as tensors, for cross-checks against the eager loop
    @torch.no_grad()
    def noise_stream(self):
        """Generator yielding exactly the noise tensors sample() consumes, in order."""
        off = torch.zeros(1, dtype=torch.int64, device=self.dev)
        while True:
            out = torch.empty_like(self.x_bcs)
            ops.randn_philox_batched(out, self.seed, self.stream_ids, off)
            yield out
