"""Sequence windows over the case files for the regression baselines (reference turbdiff/data/ofles_seq.py), without
Lightning: ``OpenFOAMSequenceDataset`` and ``OpenFOAMSequenceDataModule`` over the repository, samplers and stats of
``turbdiff_amd.data.ofles``.

A window starts at every step whose time is past ``discard_first_seconds`` and from which ``sequence_length`` steps at the
given ``stride`` fit into the file (the reference's ``valid_steps``).  A batch is a list of flat window indices that all
fall into ONE file (same geometry); its samples come back as (B, T, n_cells, dims) and its times as (B, T).
"""

from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from .ofles import (OpenFOAMBatch, OpenFOAMData, OpenFOAMDataRepository, OpenFOAMEvaluationSampler, OpenFOAMSampler,
                    OpenFOAMStats, Variable, find_data_files, reset_dataset_caches)


class OpenFOAMSequenceDataset(torch.utils.data.Dataset):
    """ofles_seq.py:24-104."""

    def __init__(self, repo, stats, *, sequence_length: int = 8, stride: int = 1, discard_first_seconds: float = -1.0):
        super().__init__()
        self.repo, self.stats = repo, stats
        self.sequence_length, self.stride, self.discard_first_seconds = sequence_length, stride, discard_first_seconds
        assert self.sequence_length >= 1
        assert self.stride >= 1
        self.reset_caches()

    def reset_caches(self):
        self.repo.reset_caches()
        self.valid_steps = []
        span = self.sequence_length * self.stride - 1
        for times in self.repo.times:
            idxs = np.nonzero(np.asarray(times) > self.discard_first_seconds)[0]
            # only the steps from which a whole window fits (idxs[:-0] of the reference is empty: span 0 keeps none)
            idxs = idxs[:-span] if span > 0 else idxs[:0]
            assert np.all(np.diff(idxs) == 1), "All steps should be consecutive"
            self.valid_steps.append(idxs)

    def sample_idxs_by_file(self):
        i, indices = 0, []
        for steps in self.valid_steps:
            indices.append(list(range(i, i + len(steps))))
            i += len(steps)
        return indices

    def __len__(self):
        return sum(len(vs) for vs in self.valid_steps)

    def window_steps(self, index):
        """(file index, the steps a batch of flat window indices reads, window after window)."""
        index = np.atleast_1d(np.asarray(index, dtype=np.int64)).copy()
        file_idx = 0
        while index.min() >= len(self.valid_steps[file_idx]):
            index -= len(self.valid_steps[file_idx])
            file_idx += 1
        assert index.max() < len(self.valid_steps[file_idx]), "All samples have to be from the same geometry"
        start = self.valid_steps[file_idx]
        steps = [s for i in index for s in range(int(start[i]), int(start[i]) + self.sequence_length * self.stride, self.stride)]
        return file_idx, steps

    def __getitem__(self, index):
        file_idx, steps = self.window_steps(index)
        data = self.repo.read(file_idx, steps)
        T = self.sequence_length
        t = data.t.reshape(-1, T, *data.t.shape[1:])
        samples = {v: s.reshape(-1, T, *s.shape[1:]) for v, s in data.samples.items()}
        return OpenFOAMBatch(OpenFOAMData(data.metadata, t, samples), self.stats)


class OpenFOAMSequenceDataModule:
    """ofles_seq.py:107-209 without Lightning: ``setup(stage)`` loads ``<root>/stats.pickle``; training windows have
    ``seq_len`` steps, validation / test windows ``eval_seq_len``."""

    def __init__(self, root: Path, discard_first_seconds: float, num_workers: int = 2, batch_size: int = 1, seq_len: int = 2,
                 eval_batch_size: int = 8, eval_seq_len: int = 100, val_samples: int = 8, test_samples: int = 32,
                 pin_memory: bool = True, variables=tuple(Variable), stride: int = 1, *, opener=None, list_cases=None):
        self.root, self.discard_first_seconds, self.num_workers = Path(root), discard_first_seconds, num_workers
        self.batch_size, self.seq_len, self.eval_batch_size, self.eval_seq_len = batch_size, seq_len, eval_batch_size, eval_seq_len
        self.val_samples, self.test_samples, self.pin_memory = val_samples, test_samples, pin_memory
        self.variables, self.stride = tuple(variables), stride
        self._opener, self._list_cases = opener, list_cases or find_data_files
        self.train_dataset = self.val_dataset = self.test_dataset = None
        self.stats = None

    def setup(self, stage: str, stats=None):
        self.stats = stats if stats is not None else OpenFOAMStats.from_file(self.root / "stats.pickle")
        if stage in ("fit",) and self.train_dataset is None:
            self.train_dataset = self._dataset("train", self.seq_len)
        if stage in ("fit", "validate") and self.val_dataset is None:
            self.val_dataset = self._dataset("val", self.eval_seq_len)
        if stage in ("test",) and self.test_dataset is None:
            self.test_dataset = self._dataset("test", self.eval_seq_len)

    def _dataset(self, phase: str, seq_len: int):
        repo = OpenFOAMDataRepository(self._list_cases(self.root / phase), self.variables, opener=self._opener)
        return OpenFOAMSequenceDataset(repo, self.stats, sequence_length=seq_len, stride=self.stride,
                                       discard_first_seconds=self.discard_first_seconds)

    def _loader(self, dataset, sampler):
        return torch.utils.data.DataLoader(dataset, sampler=sampler, worker_init_fn=reset_dataset_caches, batch_size=None,
                                           num_workers=self.num_workers, pin_memory=self.pin_memory)

    def train_dataloader(self):
        return self._loader(self.train_dataset, OpenFOAMSampler(self.train_dataset, batch_size=self.batch_size, shuffle=True))

    def val_dataloader(self):
        return self._loader(self.val_dataset, OpenFOAMEvaluationSampler(self.val_dataset, batch_size=self.eval_batch_size,
                                                                        samples_per_file=self.val_samples))

    def test_dataloader(self):
        return self._loader(self.test_dataset, OpenFOAMEvaluationSampler(self.test_dataset, batch_size=self.eval_batch_size,
                                                                         samples_per_file=self.test_samples))
