#!/usr/bin/env python3
"""Prepare a dataset of raw ``data.h5`` case files for training and evaluation: the reference's scripts/dataset-stats.py,
mean-flow.py, homogeneous-regions.py and max-mean-tke.py in one command, on the GPU.

    python tools/prepare_dataset.py ROOT [--only stats|mean-flow|regions|max-mean-tke] [options]

Writes ``ROOT/stats.pickle`` from the cases under ``ROOT/train`` and, for every case of ``ROOT/{train,val,test}``,
``mean-flow.h5``, ``regions.npz`` and ``max-mean-tke.npy`` beside its ``data.h5`` (``turbdiff_amd.data.prepare``).  The
options carry the names they have in the four scripts.  Reading the case files needs h5py.
"""

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "generative-turbulence_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

PRODUCTS = ("stats", "mean-flow", "regions", "max-mean-tke")  # turbdiff_amd.data.prepare.PRODUCTS


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("dir", help="Dataset directory")
    ap.add_argument("--only", choices=PRODUCTS, default=None, help="make one product only")
    ap.add_argument("--discard-first", default=0.025, type=float, help="mean flow, regions: use the frames with t > this")
    ap.add_argument("--seed", default=713879, type=int, help="regions: seed of the k-means++ draws")
    ap.add_argument("-k", default=32, type=int, help="regions: number of clusters")
    ap.add_argument("--epsilon", default=1e-3, type=float, help="regions: stop when the centroids move less than this on average")
    ap.add_argument("--max-iter", default=100, type=int, help="regions: at most this many Lloyd iterations")
    ap.add_argument("--max-cluster-size", default=None, type=int, help="regions: split clusters with more cells than this")
    ap.add_argument("--chunk-size", default=10, type=int, help="frames read at once from each file")
    return ap


def main():
    args = parser().parse_args()
    from turbdiff_amd.data import prepare

    assert prepare.PRODUCTS == PRODUCTS
    out = prepare.prepare_dataset(args.dir, only=args.only, discard_first=args.discard_first, seed=args.seed, k=args.k,
                                  epsilon=args.epsilon, max_iter=args.max_iter, max_cluster_size=args.max_cluster_size,
                                  chunk_frames=args.chunk_size)
    for name, result in out.items():
        if name == "stats":
            print(f"{Path(args.dir) / 'stats.pickle'}: " + ", ".join(f"{f} mean {st['mean']} std {st['std']}" for f, st in result.items()))
            continue
        line = [name + ":"]
        if "mean-flow" in result:
            line.append("mean-flow.h5")
        if "regions" in result:
            r = result["regions"]
            line.append(f"regions.npz ({r.iterations} iterations, {'converged' if r.converged else 'NOT converged'}, "
                        f"{int(r.assignments.max()) + 1} regions)")
        if "max-mean-tke" in result:
            line.append(f"max-mean-tke.npy = {result['max-mean-tke']}")
        print(" ".join(line))


if __name__ == "__main__":
    main()
