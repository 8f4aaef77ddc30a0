"""Plain numpy statements of the two formulas behind the case-preparation kernels (csrc/tdx_prepare.hip), for the tests.
Neither uses the kernels nor the host module.

``w2n_distance_sq``: squared 2-Wasserstein distance between diagonal normals, cells against centroids,

    d^2 = max(0, |cm - m|^2 + sum cvar + sum var - 2 sum sqrt(cvar var))

in float64, with one exception: the cells arrive as float32, and the sum of a cell's three variances is the float32 sum
(v0 + v1) + v2, promoted afterwards -- numpy reduces a float32 array in float32.  ``w2n_magnitude`` is the sum of the
absolute values of the terms, the scale on which rounding errors of the formula live.

``temporal_moments``: the two-pass float64 mean and population variance over the frames.
"""

import numpy as np


def w2n_terms(mean, var, cmean, cvar):
    """(k, n) arrays: |cm - m|^2, sum cvar, sum var (float32 sum), sum sqrt(cvar var)."""
    mean, var = np.asarray(mean, dtype=np.float32), np.asarray(var, dtype=np.float32)
    cmean, cvar = np.asarray(cmean, dtype=np.float64), np.asarray(cvar, dtype=np.float64)
    diff = cmean[:, None, :] - mean[None, :, :].astype(np.float64)
    nrm = diff[..., 0] ** 2 + diff[..., 1] ** 2 + diff[..., 2] ** 2
    scv = (cvar[:, 0] + cvar[:, 1]) + cvar[:, 2]
    sv = ((var[:, 0] + var[:, 1]) + var[:, 2]).astype(np.float64)  # float32 additions
    assert (var[:, 0] + var[:, 1]).dtype == np.float32
    root = np.sqrt(cvar[:, None, :] * var[None, :, :].astype(np.float64))
    cross = (root[..., 0] + root[..., 1]) + root[..., 2]
    k, n = len(cmean), len(mean)
    return nrm, np.broadcast_to(scv[:, None], (k, n)), np.broadcast_to(sv[None, :], (k, n)), cross


def w2n_distance_sq(mean, var, cmean, cvar):
    nrm, scv, sv, cross = w2n_terms(mean, var, cmean, cvar)
    return np.clip(nrm + scv + sv - 2.0 * cross, 0.0, None)


def w2n_magnitude(mean, var, cmean, cvar):
    """|cm|^2 + |m|^2 + sum cvar + sum var, (k, n): what the tolerances of the distance tests are relative to."""
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    cmean, cvar = np.asarray(cmean, dtype=np.float64), np.asarray(cvar, dtype=np.float64)
    return ((cmean**2).sum(-1) + cvar.sum(-1))[:, None] + ((mean**2).sum(-1) + var.sum(-1))[None, :]


def temporal_moments(x):
    """(mean, population variance) over axis 0 of float32 frames, two passes in float64."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.sum(axis=0) / x.shape[0]
    return mean, ((x - mean) ** 2).sum(axis=0) / x.shape[0]


def adjacent_f32(got, want64):
    """True where the float32 array ``got`` equals the float64 ``want64`` cast to float32 or one of its two float32
    neighbours."""
    want = np.asarray(want64).astype(np.float32)
    got = np.asarray(got, dtype=np.float32)
    return (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))
