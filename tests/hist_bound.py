"""Per-cell bounds for a histogram that is an fp32 sum of known addends.

The oracle (OracleScene.render(..., addends=True)) returns, per histogram channel, ref = the exact sum of the addends (in
double), S = sum |a| and N = the number of non-zero addends.  The device adds the same fp32 addends (the per-path records
are bit-equal), in an order of its own: atomics, LDS partials, wave shuffles, shards.  Any fp32 summation of N addends,
whatever the order or tree, satisfies

    |fl(sum) - sum| <= gamma_{N-1} * S,    gamma_k = k u / (1 - k u),  u = 2^-24

(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4 for recursive summation; the same bound holds for
any binary tree of additions, whose depth is at most N - 1).  So every cell is checked at its own scale, instead of at the
scale of the brightest path of the launch.

HIST_BOUND_LOG=<file>: each check appends one line with the largest |h - ref| / bound it saw.
"""
import os

import numpy as np

U = 2.0 ** -24
# Hardware float atomics may flush a subnormal addend or partial sum to zero; each of the N additions then loses at most
# the smallest normal float.  This slack is explicit so that it is never mistaken for rounding.
FTZ_SLACK = 2.0 ** -126


def gamma(k):
    k = np.asarray(k, np.float64)
    ku = k * U
    with np.errstate(divide="ignore"):
        return np.where(ku < 1.0, ku / (1.0 - ku), np.inf)


def fp32_sum_bound(S, N):
    """The bound on |fl(sum) - sum| for one fp32 summation of N non-zero addends of magnitude sum S."""
    N = np.asarray(N, np.int64)
    return gamma(np.maximum(N - 1, 0)) * np.asarray(S, np.float64) + N * FTZ_SLACK


def count_channels(lp, sd=None):
    """Flat indices of the channels whose addends are all 0 or 1 and must therefore be exact: valid (A) and W of every
    pixel of a render, W of every ADC cell.  None of them under a wide reconstruction filter (their addends are weights)."""
    from beifong_amd import capi
    if sd is not None and np.float32(sd.desc.sensor.rfilter.radius) > np.float32(0.5) + np.float32(1500 * 2.0 ** -24):   # rfilter_wide
        return np.zeros(0, np.int64)
    if lp.mode in (capi.BF_MODE_RECEIVE_RAW, capi.BF_MODE_RECEIVE_IQ):
        c = 3 + (lp.phase_bins if lp.mode == capi.BF_MODE_RECEIVE_RAW else 0)
        cells = lp.bins * lp.bins_y
        return np.arange(cells, dtype=np.int64) * c + 2
    c = {capi.BF_MODE_PATH: 5, capi.BF_MODE_RANGE: 5 + lp.bins, capi.BF_MODE_TIME: 5 + 3 * lp.bins}[lp.mode]
    pixels = lp.film_width * lp.film_height if (lp.spp and lp.film_width and lp.film_height) else 1
    base = np.arange(pixels, dtype=np.int64) * c
    return np.concatenate([base + 3, base + 4])


def _report(what, err, bound, N, S, ref, vals, bad):
    idx = np.flatnonzero(bad)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = idx[np.argsort(-np.nan_to_num(ratio[idx], nan=np.inf))][:8]
    lines = [f"{what}: {idx.size} of {err.size} cells outside the fp32 summation bound"]
    for i in worst:
        lines.append(f"  cell {i}: N={int(N[i])} S={S[i]:.9g} ref={ref[i]:.9g} " + " ".join(f"{k}={v[i]!r}" for k, v in vals)
                     + f" |diff|={err[i]:.3g} bound={bound[i]:.3g}")
    return "\n".join(lines)


def _log(what, err, bound):
    pos = bound > 0
    r = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    path = os.environ.get("HIST_BOUND_LOG")
    if path:
        with open(path, "a") as f:
            f.write(f"{what}: cells {err.size} nonzero {int(pos.sum())} max |h-ref|/bound {r:.4g}\n")
    return r


def _flat(a, dtype):
    return np.asarray(a).reshape(-1).astype(dtype, copy=False)


def assert_fp32_sum(h_dev, ref, S, N, what, counts=None):
    """h_dev (one fp32 summation of the oracle's addends) against the oracle's exact sum ref, cell by cell: N = 0 cells
    exactly 0, the rest within gamma_{N-1} S + N 2^-126, the count channels `counts` (flat indices) exactly equal.
    Returns the largest |h - ref| / bound."""
    h = _flat(h_dev, np.float64)
    ref, S, N = _flat(ref, np.float64), _flat(S, np.float64), _flat(N, np.int64)
    assert h.shape == ref.shape == S.shape == N.shape, (what, h.shape, ref.shape)
    err = np.abs(h - ref)
    bound = fp32_sum_bound(S, N)
    bad = ~(err <= bound)
    bad |= (N == 0) & (h != 0.0)
    if counts is not None and len(counts):
        c = np.zeros(h.size, bool)
        c[np.asarray(counts)] = True
        bad |= c & (h != ref)
    assert not bad.any(), _report(what, err, bound, N, S, ref, [("h", h)], bad)
    return _log(what, err, bound)


def assert_two_fp32_sums(h1, h2, S, N, what, counts=None):
    """Two fp32 summations of the same addends (two HIP results), S and N from the oracle: each lies within
    gamma_{N-1} S + N 2^-126 of the exact sum, so they lie within twice that of each other; N = 0 cells are 0 in both,
    count channels equal."""
    a, b = _flat(h1, np.float64), _flat(h2, np.float64)
    S, N = _flat(S, np.float64), _flat(N, np.int64)
    assert a.shape == b.shape == S.shape == N.shape, (what, a.shape, b.shape, S.shape)
    err = np.abs(a - b)
    bound = 2.0 * fp32_sum_bound(S, N)
    bad = ~(err <= bound)
    bad |= (N == 0) & ((a != 0.0) | (b != 0.0))
    if counts is not None and len(counts):
        c = np.zeros(a.size, bool)
        c[np.asarray(counts)] = True
        bad |= c & (a != b)
    assert not bad.any(), _report(what, err, bound, N, S, a, [("h1", a), ("h2", b)], bad)
    return _log(what, err, bound)


def assert_close_hists(hb, hs, n_paths, amax, add, lp, sd, what="two HIP histograms"):
    """Two HIP histograms of one launch (batched / rolling / sharded against stand-alone): the whole-histogram tolerance
    n_paths 2^-24 max(amax, 1) 4, and per cell assert_two_fp32_sums with add = the oracle's Addends of that launch."""
    atol = n_paths * 2.0 ** -24 * max(amax, 1.0) * 4
    assert np.allclose(hb, hs, rtol=2e-5, atol=atol), float(np.abs(hb - hs).max())
    return assert_two_fp32_sums(hb, hs, add.S, add.N, what, counts=count_channels(lp, sd))
