#!/usr/bin/env python3
"""Generate tests/golden/prepare.npz by running the *reference's* case-preparation scripts (build container only).

scripts/dataset-stats.py, mean-flow.py, homogeneous-regions.py and max-mean-tke.py are run unmodified with ``runpy`` on the
seeded case files of tests/prepare_cases.py.  ``h5py`` is replaced by tests/h5fake.py, ``joblib``'s parallel run by a
sequential one (worker processes would see neither), and ``np.random.default_rng`` hands out a generator that records what
``choice`` returns: those are the k-means++ picks, which the script keeps in a local variable.  Only numbers are stored.

    python tests/golden/make_golden_prepare.py

Contents: ``stats/<field>/<min|max|mean|std>`` of the two training cases at --chunk-size 4; ``proto/mean_flow/{u,p}``,
``proto/picks``, ``proto/assignments`` (-k 8) and ``proto/split/{assignments,raw_assignments}`` (--max-cluster-size 200) of
the prototype case; ``tke/value`` of the 5000-frame case; ``w2n/D`` = the script's wasserstein2_normal on
prepare_cases.w2n_inputs().  The generator asserts on the reference's own output that the picks cover all groups, that the
partition is the true one and that the smallest relative gap between a cell's best and second-best distance exceeds 0.5.
"""

import contextlib
import pickle
import runpy
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import h5fake  # noqa: E402
import prepare_cases as PC  # noqa: E402
from make_golden import REF, _stub, install_stubs  # noqa: E402

SCRIPTS = REF / "scripts"


class SequentialParallel:
    def __init__(self, *a, **k):
        pass

    def __call__(self, tasks):
        return (fn(*args, **kwargs) for fn, args, kwargs in tasks)


def delayed(fn):
    return lambda *args, **kwargs: (fn, args, kwargs)


@contextlib.contextmanager
def parallel_backend(*a, **k):
    yield


class RecordingRng:
    def __init__(self, rng):
        self.rng, self.picks = rng, []

    def choice(self, *a, **k):
        value = self.rng.choice(*a, **k)
        self.picks.append(int(value))
        return value


def run_script(name, *argv):
    old = sys.argv
    sys.argv = [name, *[str(a) for a in argv]]
    try:
        return runpy.run_path(str(SCRIPTS / name), run_name="__main__")
    finally:
        sys.argv = old


def placeholder(path):
    """The reference lists cases with Path.is_file: an empty file stands where the in-memory tree is registered."""
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    Path(path).touch()


def main():
    install_stubs()
    _stub("h5py", File=h5fake.File, Group=h5fake.Group)
    _stub("joblib", Parallel=SequentialParallel, delayed=delayed, parallel_backend=parallel_backend)
    sys.path.insert(0, str(REF))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        # (a) dataset statistics
        root = tmp / "dataset"
        for path in PC.install_stats_cases(root)["train"]:
            placeholder(path)
        run_script("dataset-stats.py", "--chunk-size", PC.STATS_CHUNK, "--parallel", 1, root)
        for field, st in pickle.loads((root / "stats.pickle").read_bytes()).items():
            for key, value in st.items():
                assert value.dtype == np.float32, (field, key, value.dtype)
                out[f"stats/{field}/{key}"] = value

        # (b) mean flow and homogeneous regions of the prototype case
        proto = PC.case_dir(tmp, "proto")
        tree, groups = PC.prototype_case(proto / "data.h5")
        run_script("mean-flow.py", proto)
        mf = h5fake.TREES[str(proto / "mean-flow.h5")]
        out["proto/mean_flow/u"], out["proto/mean_flow/p"] = np.array(mf["data/u"]), np.array(mf["data/p"])
        assert out["proto/mean_flow/u"].dtype == np.float32 and out["proto/mean_flow/p"].dtype == np.float32

        real_rng = np.random.default_rng
        recorders = []

        def recording_rng(seed):
            recorders.append(RecordingRng(real_rng(seed)))
            return recorders[-1]

        np.random.default_rng = recording_rng
        try:
            g = run_script("homogeneous-regions.py", "-k", PC.PROTO_K, proto)
            plain = dict(np.load(proto / "regions.npz"))
            run_script("homogeneous-regions.py", "-k", PC.PROTO_K, "--max-cluster-size", PC.PROTO_MAX_CLUSTER, proto)
            split = dict(np.load(proto / "regions.npz"))
        finally:
            np.random.default_rng = real_rng
        assert recorders[0].picks == recorders[1].picks and len(recorders[0].picks) == PC.PROTO_K
        picks = np.array(recorders[0].picks)
        assert sorted(plain) == ["assignments"] and sorted(split) == ["assignments", "raw_assignments"]
        assert np.array_equal(split["raw_assignments"], plain["assignments"])
        assert np.bincount(plain["assignments"]).max() > PC.PROTO_MAX_CLUSTER, "the split run must split something"
        out["proto/picks"], out["proto/assignments"] = picks, plain["assignments"]
        out["proto/split/assignments"], out["proto/split/raw_assignments"] = split["assignments"], split["raw_assignments"]

        # the properties the exact-label test rests on, from the reference's own output
        assert set(groups[picks]) == set(range(PC.PROTO_K)), "the k-means++ picks must cover all groups"
        a = plain["assignments"]
        assert len({(int(x), int(y)) for x, y in zip(groups, a)}) == PC.PROTO_K, "the partition must be the true one"
        t = np.array(tree["data/times"])
        u = np.array(tree["data/u"])[t > PC.PROTO_DISCARD]
        u_mean, u_cov = np.mean(u, axis=0), np.var(u, axis=0)
        cm = np.stack([u_mean[a == c].mean(axis=0) for c in range(PC.PROTO_K)]).astype(np.float64)
        cc = np.stack([u_cov[a == c].mean(axis=0) for c in range(PC.PROTO_K)]).astype(np.float64)
        D = np.sort(g["wasserstein2_normal"](cm, cc, u_mean, u_cov), axis=0)
        gap = ((D[1] - D[0]) / D[1]).min()
        assert gap > 0.5, gap
        print(f"prototype case: {len(a)} cells, picks {picks.tolist()}, smallest relative gap {gap:.3f}, "
              f"cluster sizes {np.bincount(a).tolist()} -> {np.bincount(split['assignments']).tolist()}")

        # the distance formula itself
        mean, var, cmean, cvar = PC.w2n_inputs()
        out["w2n/D"] = g["wasserstein2_normal"](cmean, cvar, mean, var)

        # (c) position of the maximum of the mean TKE profile
        tke = PC.case_dir(tmp, "tke")
        PC.tke_case(tke / "data.h5")
        run_script("max-mean-tke.py", tke)
        out["tke/value"] = np.load(tke / "max-mean-tke.npy")
        print("max-mean-tke:", out["tke/value"])

    np.savez_compressed(HERE / "prepare.npz", **out)
    size = (HERE / "prepare.npz").stat().st_size
    assert size < 1 << 20
    print(f"wrote {HERE / 'prepare.npz'} ({len(out)} arrays, {size} bytes)")


if __name__ == "__main__":
    main()
