"""The DilResNet regression baseline's task without Lightning / hydra: ``DilResNetTrainer`` = the reference's
``RegressionTraining`` (turbdiff/models/regression.py) + ``DilResNetTraining`` (turbdiff/models/dilresnet.py:97-226).

* constructor keywords = ``DilResNetTraining.__init__``'s, plus ``gradient_clip_val`` (the trainer's clip-by-norm:
  0.1 in shapes_regression_experiment.yaml, none in regression_experiment.yaml) and ``compute_mode``: "f32" (fp32
  tensors, the unfused parity path) or "bf16" (the fused HIP chain of ``models.dilresnet``);
* the ``dx_mean`` / ``dx_var`` / ``n_train_batches_tracked`` buffers and the reference's ``state_dict`` keys;
* ``training_step``: one-step prediction of the normalised increment x1 - x0 (noise-injected x0), MSE against
  ``F.batch_norm`` of the increment over the in-domain cells (batch statistics for the first 1000 training batches);
* ``configure_optimizers``: Adam + LambdaLR exponential decay to ``min_learning_rate`` over ``max_train_steps`` (on a GPU
  with ``fused_optimizer``: ``optim.ClipAdam``, clip and update in three launches); ``fit_step`` = zero_grad, step, backward,
  clip, optimiser, schedule;
* ``_predict_x`` / ``unroll_samples``: the rollout x <- inside ? x + dx_mean + dx_std model(x) : x.  The conditioning conv
  runs once per batch; in bf16 the decode conv applies the update in its epilogue and the state stays fp32;
* ``validation_step(batch, stores)``: unroll over the batch's target steps, hand the samples at ``sample_steps`` to
  ``SampleStore``s, return the loss and the per-step ``unroll/mse-<var>-<i>`` metrics; ``val_sample_metrics`` are the
  reference's ``SampleMetricsCollection``s (W2-TKE, W2, max-mean-TKE position).

``TFNetTrainer`` = ``RegressionTraining`` + ``TFNetTraining`` (turbdiff/models/tfnet.py:371-430) shares everything above
that is not DilResNet's own through ``_RegressionTrainer``: its ``training_step`` unrolls ``_predict_x`` WITH gradient
(x_i = inside ? model(context, C) : context[:, -1], the context shifted by one step) and takes the MSE over the whole grid;
Adam at a constant rate.

A batch is an ``OpenFOAMBatch`` of sequence windows (``data.ofles_seq``): samples (B, T, n_cells, dims).
"""

from __future__ import annotations

import math
from pathlib import Path

import torch
import torch.nn.functional as F
from torch import nn

from .data.ofles import OpenFOAMData, Variable, split_channels
from .models.cell_type_embeddings import CellTypeEmbedding
from .models.conditioning import Conditioning
from .models.dilresnet import DilResNet
from .models.tfnet import LES
from .models.metrics import (MaxMeanTKEPositionMetric, SampleMetricsCollection, SampleStore, WassersteinMetric,
                             WassersteinTKE)
from .models.normalization import Normalization
from .models.utils import ravel_cells, select_cells
from .training import _get, _has, _raw

COMPUTE_MODES = ("f32", "bf16")
_MODE_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16}


class _RegressionTrainer(nn.Module):
    """What RegressionTraining (regression.py:27-281) gives every regression task: conditioning, normalisation, sample
    stores and metric collections, the model input, the rollout drivers and the validation metrics.  A subclass sets
    ``self.model`` (with ``encode_conditioning``) and defines ``_predict_x``."""

    def __init__(self, data_dir, samples_root, variables, context_window, unroll_steps, eval_unroll_steps, sample_steps,
                 main_sample_step, normalization_mode, cell_type_features, cell_type_embedding_type, cell_type_embedding_dim,
                 cell_pos_features, compute_expensive_sample_metrics):
        super().__init__()
        self.variables = tuple(v if isinstance(v, Variable) else Variable.from_str(v) for v in variables)
        assert Variable.U in self.variables
        self.context_window, self.unroll_steps, self.eval_unroll_steps = context_window, unroll_steps, eval_unroll_steps
        self.cell_type_features = cell_type_features
        self.cell_type_embedding_type, self.cell_type_embedding_dim = cell_type_embedding_type, cell_type_embedding_dim
        self.cell_type_embedding = (CellTypeEmbedding.create(cell_type_embedding_type, cell_type_embedding_dim)
                                    if cell_type_features else None)
        self.cell_pos_features = cell_pos_features
        self.conditioning = Conditioning(self.variables, self.cell_type_embedding, cell_pos_features)
        self.normalization_mode = normalization_mode
        self.normalization = Normalization(self.variables, normalization_mode)
        self.sample_steps, self.main_sample_step = list(sample_steps), main_sample_step
        self.compute_expensive_sample_metrics = compute_expensive_sample_metrics
        self.data_dir = data_dir
        self.val_sample_metrics = nn.ModuleList([self._sample_metrics(f"val/{s}", data_dir) for s in self.sample_steps])
        self.test_sample_metrics = nn.ModuleList([self._sample_metrics(f"test/{s}", data_dir) for s in self.sample_steps])
        root = Path(samples_root) if samples_root is not None else None
        self.val_sample_stores = [SampleStore(root and root / f"val-{s}-samples.h5", self.variables) for s in self.sample_steps]
        self.test_sample_stores = [SampleStore(root and root / f"test-{s}-samples.h5", self.variables) for s in self.sample_steps]
        if len(self.sample_steps) > 0:
            assert self.eval_unroll_steps >= max(self.sample_steps)
        self.loss = nn.MSELoss()
        self.stats = None

    def _set_compute(self, compute_mode, gradient_clip_val):
        if compute_mode not in COMPUTE_MODES:
            raise ValueError(f"compute mode {compute_mode!r} not in {COMPUTE_MODES}")
        self.compute_mode = compute_mode
        self.gradient_clip_val = gradient_clip_val
        self.fused_optimizer = True  # optim.ClipAdam on GPU; False -> clip_grad_norm_ + torch.optim.Adam
        self._opt = self._sched = None

    @staticmethod
    def _sample_metrics(phase: str, data_dir):
        return SampleMetricsCollection(phase, data_dir, [WassersteinTKE(), WassersteinMetric(), MaxMeanTKEPositionMetric()])

    @property
    def compute_dtype(self):
        return _MODE_DTYPE[self.compute_mode]

    @classmethod
    def _config_kwargs(cls, config, name: str, float_keys):
        """(constructor keywords, the model group) from the whole run configuration or its ``model`` group: the class's
        CONFIG_KEYS, variables, cell_pos_features, and from the root data_dir, samples_root, gradient_clip_val."""
        model = _get(config, "model")
        root = config if model is not None else None
        model = model if model is not None else config
        got = _get(model, "name", name)
        if got != name:
            raise ValueError(f"model.name = {got!r}: {cls.__name__} builds the {name} task")
        kw = {k: _raw(model, k) for k in cls.CONFIG_KEYS if _has(model, k)}
        var = _get(model, "variables")
        kw["variables"] = tuple(Variable) if var is None else tuple(
            Variable.from_str(v) for v in (var.split(",") if isinstance(var, str) else var))
        kw["cell_pos_features"] = bool(_get(model, "cell_pos_features", False))
        if "sample_steps" in kw:
            kw["sample_steps"] = list(kw["sample_steps"] or [])
        if root is not None:
            data_root = _get(_get(root, "data"), "root")
            if data_root is not None:
                kw["data_dir"] = Path(data_root) / "data"
            if _get(root, "samples_root") is not None:
                kw["samples_root"] = _get(root, "samples_root")
            clip = _get(_get(root, "trainer"), "gradient_clip_val")
            kw["gradient_clip_val"] = float(clip) if clip is not None else None
        for k in float_keys:  # YAML 1.1 reads "1e-3" as a string
            if isinstance(kw.get(k), str):
                kw[k] = float(kw[k])
        return kw, model

    # ---- model input (regression.py:305-310)
    def _model_input(self, batch):
        """x (B, T, F, X, Y, Z) normalised fp32, and the conditioning dict."""
        data = batch.data
        flat = {v: s.reshape(-1, *s.shape[-2:]) for v, s in data.samples.items()}
        B, T = next(iter(data.samples.values())).shape[:2]
        x = self.normalization.normalized_grid_embedding(OpenFOAMData(data.metadata, data.t, flat), batch.stats)
        return x.reshape(B, T, *x.shape[1:]), self.conditioning(data)

    @torch.no_grad()
    def unroll_samples(self, batch, sample_steps, block_size: int):
        """Denormalised states at the given steps (0 = one step after the context), unrolled in blocks of block_size."""
        assert block_size >= self.context_window
        x_context, C = self._model_input(batch)
        c_enc = self.model.encode_conditioning(C, self.compute_dtype)  # once per batch
        inside = batch.data.metadata.inside_mask
        x_sample = []
        for i in range(0, max(sample_steps) + 1, block_size):
            x_hat = self._predict_x(x_context, C, inside, unroll_steps=block_size, c_enc=c_enc)
            x_context = x_hat[:, -self.context_window:]
            idxs = [j - i for j in sample_steps if i <= j < i + block_size]
            x_sample.append(x_hat[:, idxs])
        return self.normalization.denormalize_grid(torch.cat(x_sample, dim=1), batch.stats)

    def _unroll_predict(self, batch):
        x, C = self._model_input(batch)
        x_context, x_target = x[:, :self.context_window], x[:, self.context_window:]
        x_hat = self._predict_x(x_context, C, batch.data.metadata.inside_mask, unroll_steps=x_target.shape[1])
        return x_hat, x_target

    @torch.no_grad()
    def validation_step(self, batch, stores=None, phase: str = "val"):
        """regression.py:141-158: the loss of the first unroll_steps, the per-step MSE metrics; the samples at
        ``sample_steps`` go to ``stores`` (one SampleStore per sample step; default: this task's own)."""
        if self.stats is None:
            self.stats = batch.stats
        if stores is None:
            stores = self.val_sample_stores if phase == "val" else self.test_sample_stores
        elif isinstance(stores, SampleStore):
            stores = [stores]
        x_hat, x_target = self._unroll_predict(batch)
        x_sample = self.normalization.denormalize_grid(x_hat, batch.stats)
        x_target_denorm = self.normalization.denormalize_grid(x_target, batch.stats)
        for s, store in zip(self.sample_steps, stores):
            store.add_samples(x_sample[:, s - 1], batch.data.metadata)
        metrics = {f"{phase}/loss": self.loss(x_hat[:, :self.unroll_steps], x_target[:, :self.unroll_steps])}
        metrics.update(self.unroll_metrics(x_sample, x_target_denorm, batch, phase=phase))
        return metrics

    def unroll_metrics(self, x_sample, x_target, batch, *, phase: str):
        """regression.py:312-335: per variable and step, the squared error summed over the components, mean over cells."""
        cell_idx = batch.data.metadata.cell_idx.to(x_sample.device)
        xs = split_channels(select_cells(x_sample, cell_idx), self.variables, dim=-2)
        xt = split_channels(select_cells(x_target, cell_idx), self.variables, dim=-2)
        out = {}
        for v in self.variables:
            mse = ((xs[v] - xt[v]) ** 2).sum(dim=-2).mean(dim=-1)
            out.update({f"{phase}/unroll/mse-{v.name.lower()}-{i + 1}": mse[:, i].mean() for i in range(mse.shape[1])})
        return out

    def compute_sample_metrics(self, phase: str = "val", *, expensive_metrics: bool | None = None):
        """The sample metrics over the stores (regression.py:164-189); the main step's also without the step prefix."""
        colls = self.val_sample_metrics if phase == "val" else self.test_sample_metrics
        stores = self.val_sample_stores if phase == "val" else self.test_sample_stores
        if expensive_metrics is None:
            expensive_metrics = self.compute_expensive_sample_metrics
        metrics = {}
        for s, coll, store in zip(self.sample_steps, colls, stores):
            step_metrics = coll.compute(store, self.stats, next(self.parameters()).device, expensive_metrics=expensive_metrics)
            metrics.update(step_metrics)
            if s == self.main_sample_step:
                metrics.update({"/".join([(p := k.split("/"))[0], *p[2:]]): v for k, v in step_metrics.items()})
        return metrics


class DilResNetTrainer(_RegressionTrainer):
    def __init__(self, data_dir=None, samples_root=None, variables=tuple(Variable), context_window: int = 1,
                 unroll_steps: int = 1, eval_unroll_steps: int = 30, sample_steps=(), main_sample_step: int = -1,
                 normalization_mode: str = "mean-std", cell_type_features: bool = True,
                 cell_type_embedding_type: str = "learned", cell_type_embedding_dim: int = 8, cell_pos_features: bool = False,
                 learning_rate: float = 1e-3, min_learning_rate: float = 1e-6, max_train_steps: int = 1000, N: int = 4,
                 hidden_dim: int = 48, training_noise_std: float | None = None, compute_expensive_sample_metrics: bool = True,
                 *, gradient_clip_val: float | None = None, compute_mode: str = "f32"):
        super().__init__(data_dir, samples_root, variables, context_window, unroll_steps, eval_unroll_steps, sample_steps,
                         main_sample_step, normalization_mode, cell_type_features, cell_type_embedding_type,
                         cell_type_embedding_dim, cell_pos_features, compute_expensive_sample_metrics)
        assert unroll_steps == 1, "DilResNet training only uses unroll_steps=1"
        self.learning_rate, self.min_learning_rate, self.max_train_steps = learning_rate, min_learning_rate, max_train_steps
        self.training_noise_std = training_noise_std
        n_features = sum(v.dims for v in self.variables)
        self.model = DilResNet(n_features=n_features, c_local_features=self.conditioning.local_conditioning_dim,
                               c_global_features=self.conditioning.global_conditioning_dim, N=N, hidden_dim=hidden_dim)
        self.register_buffer("dx_mean", torch.zeros(n_features))
        self.register_buffer("dx_var", torch.ones(n_features))
        self.register_buffer("n_train_batches_tracked", torch.tensor(0, dtype=torch.long))

        self._set_compute(compute_mode, gradient_clip_val)

    # ---- construction from a run configuration (config.py:130-156)
    CONFIG_KEYS = ("context_window", "unroll_steps", "eval_unroll_steps", "sample_steps", "main_sample_step",
                   "normalization_mode", "cell_type_features", "cell_type_embedding_type", "cell_type_embedding_dim",
                   "learning_rate", "min_learning_rate", "N", "hidden_dim", "training_noise_std",
                   "compute_expensive_sample_metrics")

    @classmethod
    def from_config(cls, config, *, max_train_steps: int | None = None, steps_per_epoch: int | None = None,
                    compute_mode: str | None = None, **overrides):
        """``config`` is the whole run configuration (``model``, ``data.root``, ``samples_root``,
        ``trainer.gradient_clip_val``, ``matmul_precision``) or its ``model`` group (config/model/dilresnet.yaml).
        ``max_train_steps`` = ``model.max_epochs * len(train_dataloader)`` in the reference: pass it, or
        ``steps_per_epoch``.  Every ``matmul_precision`` maps to "f32" (there is no split-precision convg); bf16 is
        asked for with ``compute_mode``."""
        kw, model = cls._config_kwargs(config, "dilresnet", ("learning_rate", "min_learning_rate", "training_noise_std"))
        if max_train_steps is None and steps_per_epoch is not None:
            max_train_steps = int(_get(model, "max_epochs", 1)) * int(steps_per_epoch)
        if max_train_steps is not None:
            kw["max_train_steps"] = int(max_train_steps)
        kw["compute_mode"] = compute_mode or "f32"
        kw.update(overrides)
        return cls(**kw)

    # ---- training (dilresnet.py:181-211)
    def training_step(self, batch, noise: torch.Tensor | None = None):
        """The loss of one batch.  ``noise``: the standard-normal draw of the input noise (default: ``randn_like``)."""
        x, C = self._model_input(batch)
        x0 = x[:, self.context_window - 1]
        if self.training_noise_std is not None:
            x0 = x0 + self.training_noise_std * (torch.randn_like(x0) if noise is None else noise)
        dx = x[:, self.context_window] - x0
        dx_hat_normed = self.model(x0.to(self.compute_dtype), C)
        cell_idx = batch.data.metadata.cell_idx.to(x.device)
        loss = self.loss(ravel_cells(dx_hat_normed)[..., cell_idx],
                         F.batch_norm(ravel_cells(dx)[..., cell_idx], self.dx_mean, self.dx_var,
                                      training=self.training and self.n_train_batches_tracked.item() < 1000))
        if self.training:
            self.n_train_batches_tracked.add_(1)
        return loss

    def lr_lambda(self, step: int) -> float:
        decay_step = math.log(self.min_learning_rate / self.learning_rate) / self.max_train_steps
        return math.exp(decay_step * min(step, self.max_train_steps))

    def configure_optimizers(self):
        params = list(self.parameters())
        if self.fused_optimizer and params[0].is_cuda:
            from .optim import ClipAdam  # clip + Adam fused; same arithmetic as the two torch calls

            opt = ClipAdam(params, lr=self.learning_rate, max_norm=self.gradient_clip_val or None)
        else:
            opt = torch.optim.Adam(params, lr=self.learning_rate)
        return opt, torch.optim.lr_scheduler.LambdaLR(opt, self.lr_lambda)

    def fit_step(self, batch, noise: torch.Tensor | None = None):
        """zero_grad -> training_step -> backward -> clip -> Adam -> LR schedule (Lightning's order)."""
        if self._opt is None:
            self._opt, self._sched = self.configure_optimizers()
        self.train()
        self._opt.zero_grad(set_to_none=True)
        loss = self.training_step(batch, noise)
        loss.backward()
        if self.gradient_clip_val and not hasattr(self._opt, "max_norm"):
            torch.nn.utils.clip_grad_norm_(self.parameters(), self.gradient_clip_val)
        self._opt.step()
        self._sched.step()
        return loss.detach()

    # ---- rollout (dilresnet.py:213-226, regression.py:99-131)
    @torch.no_grad()
    def _unroll_predict(self, batch):
        return super()._unroll_predict(batch)

    @torch.no_grad()
    def _predict_x(self, x_context, C, inside_mask, *, unroll_steps: int, c_enc=None):
        """(B, unroll_steps, F, X, Y, Z): x <- inside ? x + dx_mean + dx_std model(x) : x from x_context[:, -1]."""
        if c_enc is None:
            c_enc = self.model.encode_conditioning(C, self.compute_dtype)
        return self.model.unroll(x_context[:, -1], C, inside_mask, self.dx_mean, self.dx_var.sqrt(), unroll_steps,
                                 dtype=self.compute_dtype, c_enc=c_enc)


class TFNetTrainer(_RegressionTrainer):
    """RegressionTraining + TFNetTraining (tfnet.py:371-430): the LES model of ``models.tfnet``."""

    def __init__(self, data_dir=None, samples_root=None, normalization_mode: str = "mean-std", variables=tuple(Variable),
                 temporal_filtering_length: int = 4, context_window: int = 6, unroll_steps: int = 4,
                 eval_unroll_steps: int = 30, sample_steps=(), main_sample_step: int = -1, learning_rate: float = 1e-3,
                 dropout_rate: float = 0, kernel_size: int = 3, cell_type_features: bool = True,
                 cell_type_embedding_type: str = "learned", cell_type_embedding_dim: int = 8, cell_pos_features: bool = False,
                 compute_expensive_sample_metrics: bool = True, *, gradient_clip_val: float | None = None,
                 compute_mode: str = "f32"):
        super().__init__(data_dir, samples_root, variables, context_window, unroll_steps, eval_unroll_steps, sample_steps,
                         main_sample_step, normalization_mode, cell_type_features, cell_type_embedding_type,
                         cell_type_embedding_dim, cell_pos_features, compute_expensive_sample_metrics)
        self.temporal_filtering_length = temporal_filtering_length
        self.learning_rate, self.dropout_rate, self.kernel_size = learning_rate, dropout_rate, kernel_size
        self.model = LES(n_features=sum(v.dims for v in self.variables),
                         c_local_features=self.conditioning.local_conditioning_dim,
                         c_global_features=self.conditioning.global_conditioning_dim, context_window=context_window,
                         kernel_size=kernel_size, dropout_rate=dropout_rate,
                         temporal_filtering_length=temporal_filtering_length)
        self._set_compute(compute_mode, gradient_clip_val)

    CONFIG_KEYS = ("context_window", "unroll_steps", "eval_unroll_steps", "sample_steps", "main_sample_step",
                   "normalization_mode", "cell_type_features", "cell_type_embedding_type", "cell_type_embedding_dim",
                   "temporal_filtering_length", "learning_rate", "dropout_rate", "kernel_size",
                   "compute_expensive_sample_metrics")

    @classmethod
    def from_config(cls, config, *, compute_mode: str | None = None, **overrides):
        """``config`` is the whole run configuration or its ``model`` group (config/model/tfnet.yaml); bf16 is asked for
        with ``compute_mode``."""
        kw, _ = cls._config_kwargs(config, "tfnet", ("learning_rate", "dropout_rate"))
        kw["compute_mode"] = compute_mode or "f32"
        kw.update(overrides)
        return cls(**kw)

    # ---- rollout with gradient (regression.py:235-250)
    def _predict_x(self, x_context, C, inside_mask, *, unroll_steps: int, c_enc=None):
        """(B, unroll_steps, F, X, Y, Z): x_i = inside ? model(context, C) : context[:, -1]; the context moves one step
        forward and the prediction stays attached.  The conditioning branch is computed once per rollout in eval mode and
        on every call in training mode (each call updates its BatchNorm's running statistics in the reference)."""
        if self.model.training:
            c_enc = None
        elif c_enc is None:
            c_enc = self.model.encode_conditioning(C, self.compute_dtype)
        x_hat = []
        for _ in range(unroll_steps):
            x_hat_i = torch.where(inside_mask, self.model(x_context, C, dtype=self.compute_dtype, c_enc=c_enc), x_context[:, -1])
            x_hat.append(x_hat_i)
            x_context = x_hat_i if x_context.shape[1] == 1 else torch.cat((x_context[:, 1:], x_hat_i.unsqueeze(1)), dim=1)
        return torch.stack(x_hat, dim=1)

    def training_step(self, batch):
        """regression.py:130-135: MSE of the unrolled prediction over the whole grid."""
        x_hat, x_target = self._unroll_predict(batch)
        return self.loss(x_hat, x_target)

    def configure_optimizers(self):
        params = list(self.parameters())
        if self.fused_optimizer and params[0].is_cuda:
            from .optim import ClipAdam  # clip + Adam fused; same arithmetic as the two torch calls

            return ClipAdam(params, lr=self.learning_rate, max_norm=self.gradient_clip_val or None)
        return torch.optim.Adam(params, lr=self.learning_rate)

    def fit_step(self, batch):
        """zero_grad -> training_step -> backward -> clip -> Adam (Lightning's order)."""
        if self._opt is None:
            self._opt = self.configure_optimizers()
        self.train()
        self._opt.zero_grad(set_to_none=True)
        loss = self.training_step(batch)
        loss.backward()
        if self.gradient_clip_val and not hasattr(self._opt, "max_norm"):
            torch.nn.utils.clip_grad_norm_(self.parameters(), self.gradient_clip_val)
        self._opt.step()
        return loss.detach()
