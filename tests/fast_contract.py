"""The tolerance contract of BF_FLAG_FAST renders (include/beifong_hip.h, DESIGN.md "Fast arithmetic"), as plain functions.

A fast render F is compared with the oracle O of the same launch:
  1. per path: F AGREES with O when valid and n_rays are equal, |aux_F - aux_O| <= 1e-5 |aux_O| and
     |L_F - L_O| <= 1e-4 |L_O| + 1e-7 max_p |L_O,p|; the share of paths that do not (diverged) is pinned per scene;
  2. 1 x 1 box-filtered films in the path / range / time modes: the cell of a record follows from its aux and the launch
     (film_addends restates the rule), so F's device histogram must be the fp32 sum of F's own records;
  3. every other mode (receive raw / I/Q / mix_resample, W x H films): the whole-histogram bound of whole_hist_bound;
  4. reported only: the RMSE of h_F - h_O over the bins, divided by max |h_O|.

FAST_CONTRACT_LOG=<file>: every check appends one JSON line with the scene's figures.
"""
import json
import os

import numpy as np

from beifong_amd import capi

U = 2.0 ** -24
AUX_RTOL = 1e-5
L_RTOL, L_ATOL_REL = 1e-4, 1e-7
# the matrix of srgb_to_xyz (include/mitsuba/core/spectrum.h:281-287; bf_device_core.h / the oracle apply it to grey values)
_M = np.array([0.412453, 0.357580, 0.180423, 0.212671, 0.715160, 0.072169, 0.019334, 0.119193, 0.950227], np.float32).reshape(3, 3)


def agreement(rf, ro):
    """(agree mask, largest |dL| / |L_O| among agreeing paths with L_O != 0) of fast records rf against oracle records ro"""
    Lf, Lo = rf["L"].astype(np.float64), ro["L"].astype(np.float64)
    af, ao = rf["aux"].astype(np.float64), ro["aux"].astype(np.float64)
    fin = np.isfinite(Lo)
    lmax = float(np.abs(Lo[fin]).max()) if fin.any() else 0.0
    same_L = (Lf == Lo) | (np.isnan(Lf) & np.isnan(Lo)) | (np.abs(Lf - Lo) <= L_RTOL * np.abs(Lo) + L_ATOL_REL * lmax)
    same_aux = (af == ao) | (np.isnan(af) & np.isnan(ao)) | (np.abs(af - ao) <= AUX_RTOL * np.abs(ao))
    agree = (rf["valid"] == ro["valid"]) & (rf["n_rays"] == ro["n_rays"]) & same_L & same_aux
    sel = agree & fin & (Lo != 0) & np.isfinite(Lf)
    worst = float((np.abs(Lf[sel] - Lo[sel]) / np.abs(Lo[sel])).max()) if sel.any() else 0.0
    return agree, worst


def is_box_1x1(sd, lp):
    """1 x 1 film of a render mode under the box filter (no reconstruction filter wider than a pixel)"""
    if lp.mode not in (capi.BF_MODE_PATH, capi.BF_MODE_RANGE, capi.BF_MODE_TIME):
        return False
    if lp.spp and lp.film_width and lp.film_height and lp.film_width * lp.film_height > 1:
        return False
    return not np.float32(sd.desc.sensor.rfilter.radius) > np.float32(0.5) + np.float32(1500 * 2.0 ** -24)


def _fma32(a, b, c):
    """fp32 fused multiply-add: a * b is exact in long double, the sum rounds there and once more to float32"""
    ld = np.longdouble
    return (ld(a) * ld(b) + ld(c)).astype(np.float32)


def _xyz(l, rgb):
    l = np.asarray(l, np.float32)
    if not rgb:
        return [l, l, l]
    # M (l, l, l) as enoki's matrix * vector: col0 * v0, then fmadd(col_j, v_j, acc)
    return [_fma32(_M[i, 2], l, _fma32(_M[i, 1], l, (_M[i, 0] * l).astype(np.float32))) for i in range(3)]


def film_addends(rec, lp):
    """ref (float64), S, N of the histogram that the records `rec` of a 1 x 1 box-filtered film make in the path / range / time
    modes.  The rule (ImageBlock::put of the integrators' AOVs, range.cpp / time.cpp):
      channels X, Y, Z = srgb_to_xyz(L) (grey L in the mono modes), A = valid, W = 1;
      range: + bin i = L where lo_i <= aux < hi_i, lo_i = i * bin_width and hi_i = lo_i + bin_width in fp32;
      time : + the three channels X, Y, Z of srgb_to_xyz(L) in that bin;
      a path with a non-finite channel is dropped (warn_invalid) and adds nothing, not even W.
    L is the record's radiance: on these films the sensor's ray weight is 1, so the AOV's pre-weight radiance is the same value."""
    L = rec["L"].astype(np.float32)
    aux = rec["aux"].astype(np.float32)
    rgb = lp.color_mode == capi.BF_COLOR_RGB
    xyz = _xyz(L, rgb)
    bins = lp.bins if lp.mode in (capi.BF_MODE_RANGE, capi.BF_MODE_TIME) else 0
    per = 1 if lp.mode == capi.BF_MODE_RANGE else 3
    n_chan = 5 + per * bins
    n = L.size
    cols = [xyz[0], xyz[1], xyz[2], np.where(rec["valid"] != 0, np.float32(1), np.float32(0)), np.ones(n, np.float32)]
    ok = np.ones(n, bool)
    for c in cols:
        ok &= np.isfinite(c)
    ref = np.zeros(n_chan)
    S = np.zeros(n_chan)
    N = np.zeros(n_chan, np.int64)

    def add(ch, v, m):
        v = np.where(m, v, np.float32(0)).astype(np.float64)
        np.add.at(ref, ch, v)
        np.add.at(S, ch, np.abs(v))
        np.add.at(N, ch, (v != 0).astype(np.int64))

    for k, c in enumerate(cols):
        add(np.full(n, k), c, ok)
    if bins:
        bw = np.float32(lp.bin_width)
        lo = (np.arange(bins, dtype=np.float32) * bw).astype(np.float32)
        hi = (lo + bw).astype(np.float32)
        vals = [L] if per == 1 else (xyz if rgb else [L, L, L])
        idx = np.searchsorted(lo, aux, side="right") - 1          # the last bin with lo <= aux (NaN: past the end)
        for k in (idx - 1, idx):                                  # fp32 edges: a value may sit in a neighbour's [lo, hi) too
            kk = np.clip(k, 0, bins - 1)
            inside = ok & (k >= 0) & (k < bins) & (aux >= lo[kk]) & (aux < hi[kk])
            for j, v in enumerate(vals):
                add(5 + per * kk + j, v, inside)
    return ref, S, N


def near_edge(aux_o, sd, lp):
    """agreeing paths whose record may change cells under a relative change of aux below AUX_RTOL: aux_O within 1e-5 |aux_O| of
    a cell edge on the axis the record carries (range / time bins; the ADC's time axis in the raw receive mode)"""
    a = aux_o.astype(np.float64)
    if lp.mode in (capi.BF_MODE_RANGE, capi.BF_MODE_TIME):
        w = float(np.float32(lp.bin_width))
    elif lp.mode == capi.BF_MODE_RECEIVE_RAW:
        s = sd.desc.sensor
        if lp.bins <= 1:
            return np.zeros(a.size, bool)
        w = float(s.t_bandwidth) / float(s.t_bins)
    else:
        return np.zeros(a.size, bool)          # the path mode has no axis; I/Q records carry Q, not a coordinate
    with np.errstate(invalid="ignore"):
        q = a / w
        d = np.abs(q - np.round(q)) * w
        return np.isfinite(a) & (d <= AUX_RTOL * np.abs(a) + 1e-30)


def channels_per_path(lp):
    """k: the channels one path writes in the launch's mode"""
    if lp.mode == capi.BF_MODE_RECEIVE_RAW:
        return 3 + (1 if lp.phase_bins else 0)
    if lp.mode == capi.BF_MODE_RECEIVE_IQ:
        return 3
    return 5 + {capi.BF_MODE_PATH: 0, capi.BF_MODE_RANGE: 1, capi.BF_MODE_TIME: 3}[lp.mode]


def whole_hist_bound(h_f, h_o, add_o, rf, ro, agree, sd, lp):
    """sum_c |h_F - h_O| and its bound 2 gamma sum_c S_O + 1e-4 sum_c S_O + 2 sum_diverged (|L_F| + |L_O|) k + 2 sum_edge |L_O| k
    (in the I/Q mode a record's magnitude is |L| + |aux|: its aux is the Q channel)"""
    hf, ho = np.asarray(h_f, np.float64).reshape(-1), np.asarray(h_o, np.float64).reshape(-1)
    S, N = np.asarray(add_o.S, np.float64).reshape(-1), np.asarray(add_o.N, np.int64).reshape(-1)
    n = int(N.max()) if N.size else 0
    gam = n * U / (1 - n * U)
    k = channels_per_path(lp)

    def mag(r):
        m = np.abs(r["L"].astype(np.float64))
        if lp.mode == capi.BF_MODE_RECEIVE_IQ:
            m = m + np.abs(r["aux"].astype(np.float64))
        return np.nan_to_num(m, nan=0.0, posinf=0.0)

    mf, mo = mag(rf), mag(ro)
    edge = agree & near_edge(ro["aux"], sd, lp)
    bound = (2 * gam + 1e-4) * S.sum() + 2 * k * (mf[~agree] + mo[~agree]).sum() + 2 * k * mo[edge].sum()
    err = float(np.abs(hf - ho).sum())
    return err, float(bound), int(edge.sum())


def rmse(h_f, h_o):
    hf, ho = np.asarray(h_f, np.float64).reshape(-1), np.asarray(h_o, np.float64).reshape(-1)
    m = float(np.abs(ho).max())
    return float(np.sqrt(np.mean((hf - ho) ** 2)) / m) if m > 0 else 0.0


def log(**fig):
    path = os.environ.get("FAST_CONTRACT_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(fig) + "\n")
