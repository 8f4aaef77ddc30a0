"""Plain numpy float64 statements of what the case-diagnostics kernels compute, with the error bounds the tests use.  Nothing
here touches the kernels or turbdiff_amd.data.diagnostics."""

import numpy as np

U53 = 2.0**-53


def back_positions(cell_idx, padded_counts):
    """Positions in the cell list of the cells whose unpadded x index is >= X - max(Y, Z) (unpadded sizes), by way of
    np.unravel_index on the padded grid."""
    X, Y, Z = (int(c) - 2 for c in padded_counts)
    x = np.unravel_index(np.asarray(cell_idx), tuple(int(c) for c in padded_counts))[0] - 1
    return np.nonzero(x >= X - max(Y, Z))[0]


def residual_filters(widths=None, half_width=50):
    """(W, 2 h + 1) float64: delta - g, g the normalised Gaussian of the given width sampled at -h ... h."""
    widths = np.linspace(1, 32, 32) if widths is None else widths
    rows = []
    for width in widths:
        g = np.exp(-np.linspace(-half_width, half_width, 2 * half_width + 1) ** 2 / (2 * width**2))
        g /= g.sum()
        g = -g
        g[half_width] += 1.0
        rows.append(g)
    return np.stack(rows)


def fluctuation(x, mean, cells):
    """x[:, cells] - mean[cells] as the reference forms it: one float32 subtraction."""
    f = x[:, cells] - mean[cells]
    assert f.dtype == np.float32
    return f.reshape(len(x), -1)


def lag_products(x, mean, cells, max_lag):
    """(acc, bound): acc[i] = sum over t >= i and the columns of f[t] f[t - i] in float64 (the products of two float32 values
    are exact there), and the bound N 2^-53 sum |terms| on what any summation order of those N exact terms can be off by.
    Lags beyond the frames are 0 with bound 0."""
    f = fluctuation(x, mean, cells).astype(np.float64)
    T = len(f)
    acc, bound = np.zeros(max_lag + 1), np.zeros(max_lag + 1)
    for i in range(min(max_lag, T - 1) + 1):
        terms = f[i:] * f[:T - i]
        acc[i] = terms.sum()
        bound[i] = terms.size * U53 * np.abs(terms).sum()
    return acc, bound


def filter_outputs(x, taps):
    """(W, T - K + 1, n) float64: o[w, t] = sum_k taps[w, k] x[t + k]."""
    x = np.asarray(x, dtype=np.float64)
    K = taps.shape[1]
    windows = np.lib.stride_tricks.sliding_window_view(x, K, axis=0)  # (T - K + 1, n, K)
    return np.einsum("wk,tnk->wtn", taps, windows)


def smooth_energy(x, taps):
    """(W,) float64: sum over the output frames and columns of the squared filter outputs."""
    o = filter_outputs(x, taps)
    return (o * o).sum(axis=(1, 2))


def smooth_conditioning(x, taps):
    """kappa[w] = sqrt(sum S^2 / sum d^2), S = sum_k |taps[w, k] x[t + k]|, d the filter output: how much larger the summed
    magnitudes are than the residual they leave."""
    d = filter_outputs(x, taps)
    S = filter_outputs(np.abs(np.asarray(x, dtype=np.float64)), np.abs(taps))
    return np.sqrt((S * S).sum(axis=(1, 2)) / (d * d).sum(axis=(1, 2)))


def sqdev(x, mean):
    """(sum, bound): the float64 sum of the float32 values (x - mean) ** 2 and N 2^-53 sum |terms|."""
    sq = (x - mean) ** 2
    assert sq.dtype == np.float32
    total = sq.sum(dtype=np.float64)
    return total, sq.size * U53 * total


def decorrelation_margin(corrcoeff, tail):
    """Smallest distance to the threshold max |corrcoeff[-tail:]| among the coefficients that decide the step count: those
    up to and including the first at or below it."""
    c = np.abs(np.asarray(corrcoeff))
    threshold = c[-tail:].max()
    first = int(np.nonzero(c <= threshold)[0][0])
    if first >= len(c) - tail:  # decided inside the tail, where the largest coefficient is the threshold itself
        return 0.0
    return float(np.abs(c[:first + 1] - threshold).min())
