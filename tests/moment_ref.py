"""Expected second moments of a BF_FLAG_MOMENT render, derived from what the oracle returns WITHOUT the flag.

For a launch of n paths the addends of path p are the histogram of the oracle rendering that path alone (n_paths = 1,
path_offset = p, same seed): every cell of it is one fp32 addend x_p or 0.  The expected m2_ cell is E = sum_p x_p^2 in
float64 (so S2 = E), N the number of non-zero x_p.  The device cell is an fp32 sum of N terms fl(x_p^2):

    |h - E| <= gamma_{N-1} S2 + u S2 + 2 N 2^-126 <= gamma_N S2 + 2 N 2^-126

(summation, tests/hist_bound.py, + one rounding per square; the last term: a subnormal square or partial sum flushed).
Where x is recomputed here in float64 through srgb_to_xyz_grey (three fp32 roundings on the device, doubled by the square)
the bound is gamma_{N+8}; under a wide filter the addend w x^2 is recovered as (w x)^2 / w from the single-path cells
(w = the cell's W addend): gamma_{N+4}.  Cells with N = 0 are exactly 0.
"""
import numpy as np

from beifong_amd import capi
from tests.hist_bound import FTZ_SLACK, _log, _report, gamma

# srgb_to_xyz_grey (spectrum.h:281-287): rows of the sRGB -> XYZ matrix as the kernels hold them (fp32 constants)
_M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], np.float32)
XYZ_GREY = _M.astype(np.float64).sum(axis=1)


def copy_launch(lp, **kw):
    out = capi.bf_launch.from_buffer_copy(lp)
    for k, v in kw.items():
        setattr(out, k, v)
    return out


def plain(lp):
    """the same launch without BF_FLAG_MOMENT (what the oracle renders)"""
    return copy_launch(lp, flags=lp.flags & ~capi.BF_FLAG_MOMENT)


def with_moment(lp, extra=0):
    return copy_launch(lp, flags=lp.flags | capi.BF_FLAG_MOMENT | extra)


def n_aov(lp):
    return {capi.BF_MODE_PATH: 0, capi.BF_MODE_RANGE: lp.bins, capi.BF_MODE_TIME: 3 * lp.bins}[lp.mode]


def cells_of(lp):
    """(cells, channels per cell without the flag, with the flag)"""
    if lp.mode == capi.BF_MODE_RECEIVE_RAW:
        return lp.bins * lp.bins_y, 3 + lp.phase_bins, 4 + lp.phase_bins
    if lp.mode == capi.BF_MODE_RECEIVE_IQ:
        return lp.bins * lp.bins_y, 3, 5
    a = n_aov(lp)
    pixels = lp.film_width * lp.film_height if (lp.spp and lp.film_width and lp.film_height) else 1
    return pixels, 5 + a, 11 + 2 * a


def first_moment_part(hist_m, lp):
    """the channels a render without the flag has, cut out of a moment histogram: [cells, channels without the flag]"""
    cells, c0, c1 = cells_of(lp)
    return np.asarray(hist_m).reshape(cells, c1)[:, :c0]


def range_bins(aux, w, bins):
    """range.cpp:141-161 / time.cpp:134-153: bin i takes the sample iff (float) i * w <= aux < (float) i * w + w, in fp32, for
    the candidates around floor(aux / w); returns [n, 3] bin indices, -1 = none"""
    aux = np.asarray(aux, np.float32)
    w = np.float32(w)
    fin = np.isfinite(aux)
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.floor(np.where(fin, aux, np.float32(0)) / w)
    k = np.clip(k, -2.0, float(bins) + 2.0).astype(np.int64)
    out = np.full((aux.size, 3), -1, np.int64)
    for j, d in enumerate((-1, 0, 1)):
        i = k + d
        lo = (i.astype(np.float32) * w).astype(np.float32)
        hi = (lo + w).astype(np.float32)
        take = fin & (i >= 0) & (i < bins) & (aux >= lo) & (aux < hi)
        out[take, j] = i[take]
    return out


class M2(object):
    """expected m2_ cells in the order of capi.moment_layout(lp)[1].reshape(-1): E (float64), N, and what the bound's gamma
    index adds to N"""

    def __init__(self, E, N, extra, sel=None):
        self.E, self.N = np.asarray(E, np.float64).reshape(-1), np.asarray(N, np.int64).reshape(-1)
        self.extra = np.broadcast_to(np.asarray(extra, np.int64), self.N.shape)
        self.sel = np.ones(self.N.shape, bool) if sel is None else np.asarray(sel, bool).reshape(-1)      # pairs that are checked

    def bound(self):
        return gamma(self.N + self.extra) * self.E + 2.0 * self.N * FTZ_SLACK


def from_records(rec, lp):
    """1 x 1 film, sensor weight 1 (perspective): x = record.L, its bin from record.aux.  Pairs: [A nested AOVs, nested.X .Y .Z]"""
    a = n_aov(lp)
    L = rec["L"].astype(np.float64)
    ok = np.isfinite(L)
    L = np.where(ok, L, 0.0)
    rgb = lp.color_mode == capi.BF_COLOR_RGB
    xyz = XYZ_GREY if rgb else np.ones(3)
    E, N = np.zeros(a + 3), np.zeros(a + 3, np.int64)
    for c in range(3):
        x = L * xyz[c]
        E[a + c] = np.sum(x * x)
        N[a + c] = np.count_nonzero(x)
    if a:
        per = 3 if lp.mode == capi.BF_MODE_TIME else 1
        b = range_bins(rec["aux"], lp.bin_width, lp.bins)
        for j in range(3):
            sel = ok & (b[:, j] >= 0) & (L != 0.0)
            for c in range(per):
                x = L[sel] * (xyz[c] if per == 3 else 1.0)
                np.add.at(E, b[sel, j] * per + c, x * x)
                np.add.at(N, b[sel, j] * per + c, 1)
    # recomputed through the XYZ matrix in float64: gamma_{N+8} (module docstring); x = L itself otherwise
    extra = np.zeros(a + 3, np.int64)
    if rgb:
        extra[a:] = 8
        if lp.mode == capi.BF_MODE_TIME:
            extra[:a] = 8
    return M2(E, N, extra)


def single_paths(osc, lp, wide=False):
    """The per-path decomposition of the launch `lp` (no flag): every path rendered alone by the oracle.  Returns
    (ref, S, N, E2) per channel of the plain layout: sum x, sum |x|, the non-zero addends, sum x^2 — under a wide filter
    E2 = sum (w x)^2 / w with w the W addend of the cell's pixel (render modes) or ADC cell."""
    lp = plain(lp)
    cells, c0, _ = cells_of(lp)
    w_off = 2 if lp.mode in (capi.BF_MODE_RECEIVE_RAW, capi.BF_MODE_RECEIVE_IQ) else 4
    n = cells * c0
    ref, S, N, E2 = np.zeros(n), np.zeros(n), np.zeros(n, np.int64), np.zeros(n)
    one = copy_launch(lp, n_paths=1)
    for p in range(lp.n_paths):
        one.path_offset = lp.path_offset + p
        h = osc.render(one)[0].astype(np.float64)
        nz = np.flatnonzero(h)
        x = h[nz]
        ref[nz] += x
        S[nz] += np.abs(x)
        N[nz] += 1
        if wide:
            w = h[(nz // c0) * c0 + w_off]
            E2[nz] += x * x / w
        else:
            E2[nz] += x * x
    return ref, S, N, E2


def m2_from_single(E2, N, lp, extra=0, weight_one=False):
    """single_paths' E2 / N gathered into the order of capi.moment_layout(with_moment(lp)).  nested.X .Y .Z have no channel in
    the plain layout: with weight_one (sensor weight 1: perspective) they received the addends of the base X Y Z, bit for
    bit; otherwise those pairs are left unchecked (M2.sel)."""
    cells, c0, c1 = cells_of(lp)
    first, _ = capi.moment_layout(with_moment(lp))
    first = first.reshape(-1)
    ch = first % c1
    nested = ch >= c0
    plain_idx = (first // c1) * c0 + np.where(nested, ch - c0, ch)
    return M2(E2[plain_idx], N[plain_idx], extra, sel=(~nested) | weight_one)


class Expected(object):
    """ref, bound and N of EVERY channel of a moment histogram: the first-moment channels from the plain-layout (ref, S, N) of
    the launch without the flag (the oracle's Addends or single_paths'), nested.X .Y .Z from the base X Y Z where the sensor
    weight is 1, the m2_ channels from an M2.  `sel`: the channels that are checked; `counts`: those that must be exact."""

    def __init__(self, lp, ref, S, N, m2, weight_one, counts=None):
        from tests.hist_bound import count_channels, fp32_sum_bound
        cells, c0, c1 = cells_of(lp)
        lm = with_moment(lp)
        first, second = (a.reshape(-1) for a in capi.moment_layout(lm))
        n = cells * c1
        self.ref, self.bound, self.N, self.sel = np.zeros(n), np.zeros(n), np.zeros(n, np.int64), np.zeros(n, bool)
        ref, S, N = (np.asarray(a).reshape(cells, c0) for a in (ref, S, N))
        b = fp32_sum_bound(S, N)
        idx = (np.arange(cells)[:, None] * c1 + np.arange(c0)[None, :])
        self.ref[idx], self.bound[idx], self.N[idx], self.sel[idx] = ref, b, N, True
        if c1 - c0 >= 6:          # render modes (A + 6 more channels; receive modes: 1 or 2): nested.XYZ sit at channel c0 ..
            nidx = (np.arange(cells)[:, None] * c1 + c0 + np.arange(3)[None, :])
            self.ref[nidx], self.bound[nidx], self.N[nidx], self.sel[nidx] = ref[:, :3], b[:, :3], N[:, :3], weight_one
        self.ref[second], self.bound[second], self.N[second], self.sel[second] = m2.E, m2.bound(), m2.N, m2.sel
        self.counts = np.zeros(n, bool)
        pc = count_channels(plain(lp)) if counts is None else np.asarray(counts)
        if len(pc):
            self.counts[(pc // c0) * c1 + pc % c0] = True

    def check(self, h, what):
        """one moment histogram against the expected values, every cell within its bound"""
        h = np.asarray(h, np.float64).reshape(-1)
        assert h.shape == self.ref.shape, (what, h.shape, self.ref.shape)
        err = np.abs(h - self.ref)
        bad = (~(err <= self.bound) | ((self.N == 0) & (h != 0.0)) | (self.counts & (h != self.ref))) & self.sel
        assert not bad.any(), _report(what, err, self.bound, self.N, self.ref, self.ref, [("h", h)], bad)
        return _log(what, err[self.sel], self.bound[self.sel])

    def check_two(self, h1, h2, what):
        """two moment histograms of the same launch: each within its bound of the exact sum, so within twice of each other"""
        a, b = np.asarray(h1, np.float64).reshape(-1), np.asarray(h2, np.float64).reshape(-1)
        assert a.shape == b.shape == self.ref.shape, (what, a.shape, b.shape)
        err = np.abs(a - b)
        bad = (~(err <= 2.0 * self.bound) | ((self.N == 0) & ((a != 0.0) | (b != 0.0))) | (self.counts & (a != b))) & self.sel
        assert not bad.any(), _report(what, err, 2.0 * self.bound, self.N, self.ref, a, [("h1", a), ("h2", b)], bad)
        return _log(what, err[self.sel], 2.0 * self.bound[self.sel])
