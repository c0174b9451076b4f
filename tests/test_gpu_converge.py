"""Render until a relative standard error is reached (bf_render_converge_device) on the GPU.

The statistic kernels are held to capi.converge_statistic within 4 ulp of fp64 (both sides do the same handful of correctly
rounded operations; measured: 0 ulp in every case); the accumulator to the float64 sum of its renders within gamma_6 sum |h_k| per cell and to the oracle's
sum with the bounds of tests/moment_ref.py; the stop rule to the history it returns; the statistic's value to the interval
the oracle's per-cell bounds allow."""
import functools
import threading

import numpy as np
import pytest

from beifong_amd import capi, scenes
from tests import moment_ref as mr
from tests.hist_bound import assert_two_fp32_sums, count_channels, gamma
from tests.rolling_helpers import _same_records, _Sequence
from tests.test_gpu_moment import BINS, DR, HOST_XML, _bus, _bus_launch, _receive_scene

pytestmark = pytest.mark.gpu
M = capi.BF_FLAG_MOMENT
INF = float("inf")
N_PATHS = 1 << 12
FLOOR = 0.05          # of the bus tests: four significant range bins, none near the threshold (test 4 asserts both)


def _seeds(lp, n):
    """the seeds of the first n renders of a converge call on lp: n_paths apart, so that the renders share no path"""
    return [int(s) for s in capi.converge_seeds(lp, n)]


BUS_SEEDS = tuple(1 + k * N_PATHS for k in range(16))      # of a call on the bus launch of seed 1


def _ulps(a, b):
    """distance of two float64 in units in the last place (both finite and of one sign, or equal)"""
    if a == b:
        return 0
    assert np.isfinite(a) and np.isfinite(b), (a, b)
    ia, ib = (int(np.array(x, np.float64).view(np.int64)) for x in (a, b))
    return abs(ia - ib)


def _assert_statistic(got, want, what):
    (stat, n_sig), (stat_w, n_sig_w) = got, want
    print(f"{what}: device {stat!r} ({n_sig}), specification {stat_w!r} ({n_sig_w})")
    assert n_sig == n_sig_w, what
    assert not np.isnan(stat) and _ulps(stat, stat_w) <= 4, (what, stat, stat_w)


def _on_device(h):
    import torch
    return torch.from_numpy(np.ascontiguousarray(h, dtype=np.float32)).cuda()


def _kernel_against_spec(g, h, lm, what, floors=(0.0, 0.01, 1.0)):
    d = _on_device(h)
    for floor in floors:
        _assert_statistic(g.converge_statistic_device(lm, d.data_ptr(), floor), capi.converge_statistic(h, lm, floor), f"{what}, floor {floor}")
    z = _on_device(np.zeros_like(h))
    assert g.converge_statistic_device(lm, z.data_ptr(), 0.01) == (INF, 0)


def _range_launch(bins, seed=1, n_paths=N_PATHS):
    return capi.make_launch(capi.BF_MODE_RANGE, n_paths, seed=seed, bins=bins, bin_width=BINS * DR / bins, color_mode=capi.BF_COLOR_RGB, flags=M)


# ---- 1. the kernels against their specification ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [1, 13, 64, 257])
def test_statistic_of_range_renders(hiplib, bins):
    _, g, _ = _bus()
    lm = _range_launch(bins)
    h = g.render(lm)[0]
    assert np.count_nonzero(h[capi.converge_layout(lm)[0]]) >= 1
    _kernel_against_spec(g, h, lm, f"range, {bins} bins")
    # two renders added: n = 2 n_paths
    _kernel_against_spec(g, h + g.render(_range_launch(bins, seed=2))[0], lm, f"range, {bins} bins, two renders")


@pytest.mark.parametrize("mode", [capi.BF_MODE_PATH, capi.BF_MODE_TIME], ids=["path", "time"])
def test_statistic_of_path_and_time_renders(hiplib, mode):
    _, g, _ = _bus()
    lm = _bus_launch(mode, n_paths=N_PATHS)
    first = capi.converge_layout(lm)[0]
    assert first.shape == ((1, 1) if mode == capi.BF_MODE_PATH else (1, 3 * BINS))
    _kernel_against_spec(g, g.render(lm)[0], lm, f"mode {mode}")


@pytest.mark.parametrize("form", ["raw_phase4", "iq"])
def test_statistic_of_receive_renders(hiplib, form):
    sd, lp = _receive_scene("plate")
    lp.mode = capi.BF_MODE_RECEIVE_IQ if form == "iq" else capi.BF_MODE_RECEIVE_RAW
    lp.phase_bins = 4 if form == "raw_phase4" else 0
    lm = mr.with_moment(lp)
    g = capi.Scene(sd)
    h = g.render(lm)[0]
    assert np.count_nonzero(h[capi.converge_layout(lm)[0]]) >= 1
    _kernel_against_spec(g, h, lm, f"receive {form}")


@pytest.mark.parametrize("film, bins", [((8, 6), 16), ((5, 3), 7)], ids=["8x6x16", "5x3x7"])
def test_statistic_of_films(hiplib, film, bins):
    sd, lp = scenes.film_half_lit(film=film, spp=64, mode=capi.BF_MODE_RANGE, bins=bins, dr=6.4 / bins)
    lm = mr.with_moment(lp)
    g = capi.Scene(sd)
    h = g.render(lm)[0]
    first, _, w = capi.converge_layout(lm)
    assert first.shape == (film[0] * film[1], bins) and np.count_nonzero(h[first]) >= 4 and h[w].min() >= 2
    _kernel_against_spec(g, h, lm, f"film {film}")


def test_statistic_of_hand_made_buffers(hiplib):
    _, g, _ = _bus()
    rng = np.random.default_rng(5)
    # more pairs than one workgroup covers, a count that is no multiple of the wave, and a single pair
    for bins in (1, 63, 1000, 3001):
        lm = capi.make_launch(capi.BF_MODE_RANGE, N_PATHS, bins=bins, bin_width=1.0, flags=M)
        h = np.zeros(11 + 2 * bins, np.float32)
        x = rng.uniform(0.1, 4.0, bins)
        h[4] = 1000.0
        h[5:5 + bins] = 1000.0 * x
        h[8 + bins:8 + 2 * bins] = 1000.0 * x * x * rng.uniform(1.0, 3.0, bins)
        h[5 + bins:8 + bins] = 1.0e9                    # nested.X .Y .Z: not watched
        _kernel_against_spec(g, h, lm, f"hand-made, {bins} bins", floors=(0.0, 0.3, 1.0))
        for bad, cell in ((np.nan, 5 + bins // 2), (np.inf, 0), (-np.inf, h.size - 1)):
            hb = h.copy()
            hb[cell] = bad
            assert g.converge_statistic_device(lm, _on_device(hb).data_ptr(), 0.3) == (INF, 0) == capi.converge_statistic(hb, lm, 0.3)
        h1 = h.copy()
        h1[4] = 1.0                                     # n < 2
        assert g.converge_statistic_device(lm, _on_device(h1).data_ptr(), 0.3)[0] == INF
    # a film of 96 x 64 pixels x 8 bins: 49152 pairs over 1 622 016 floats, every pixel with its own W
    lm = capi.make_launch(capi.BF_MODE_RANGE, 96 * 64 * 4, bins=8, bin_width=1.0, flags=M, film=(96, 64), spp=4)
    h = np.zeros((96 * 64, 27), np.float32)
    h[:, 4] = rng.integers(2, 50, 96 * 64)
    x = rng.uniform(0.0, 2.0, (96 * 64, 8)) * (rng.uniform(0, 1, (96 * 64, 8)) > 0.3)
    h[:, 5:13] = h[:, 4:5] * x
    h[:, 16:24] = h[:, 4:5] * x * x * rng.uniform(1.0, 2.0, (96 * 64, 8))
    _kernel_against_spec(g, h.reshape(-1), lm, "hand-made film", floors=(0.01, 0.5, 1.0))


# ---- 2. the accumulator is the sum of its renders ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_render(seed):
    """one bus render of N_PATHS paths by the oracle: (Addends of the plain layout, M2 of the pairs)"""
    _, _, osc = _bus()
    lp = _bus_launch(n_paths=N_PATHS, seed=seed, flags=0)
    _, rec, _, add = osc.render(lp, records=True, threads=8, addends=True)
    return add, mr.from_records(rec, lp)


def _oracle_sum(n):
    """mr.Expected of the sum of the first n renders of a converge call on the bus launch of seed 1 (_oracle_sum_of)"""
    assert list(BUS_SEEDS[:n]) == _seeds(_bus_launch(n_paths=N_PATHS, seed=1), n)
    return _oracle_sum_of(BUS_SEEDS[:n])


def _oracle_sum_of(seeds):
    """mr.Expected of the sum of the renders `seeds`: one fp32 summation of all their addends, in whatever tree"""
    parts = [_oracle_render(s) for s in seeds]
    ref, S, N = (sum(getattr(a, k) for a, _ in parts) for k in ("ref", "S", "N"))
    m2 = mr.M2(sum(m.E for _, m in parts), sum(m.N for _, m in parts), parts[0][1].extra)
    return mr.Expected(_bus_launch(n_paths=N_PATHS, flags=0), ref, S, N, m2, weight_one=True)


@functools.lru_cache(maxsize=None)
def _converged_bus():
    """render_converge(target 0, R = 2, three rounds) of the bus from seed 1: every round is performed"""
    _, g, _ = _bus()
    return g.render_converge(_bus_launch(n_paths=N_PATHS, seed=1, flags=0), 0.0, floor=FLOOR, round_renders=2, min_rounds=1, max_rounds=3)


def test_accumulator_is_the_sum_of_its_renders(hiplib):
    sd, _, _ = _bus()
    acc, rounds, history, n_sig, st = _converged_bus()
    assert rounds == 3 and history.shape == (3,) and st.n_paths == 6 * N_PATHS and st.kernel_variant & capi.BF_VARIANT_MOMENT
    g2 = capi.Scene(sd)
    hs = np.array([g2.render(_bus_launch(n_paths=N_PATHS, seed=s))[0] for s in BUS_SEEDS[:6]], np.float64)
    err, bound = np.abs(acc - hs.sum(axis=0)), gamma(6) * np.abs(hs).sum(axis=0)
    print("accumulator against the float64 sum of six renders: worst |diff| / bound", float((err[bound > 0] / bound[bound > 0]).max()))
    assert np.all(err <= bound) and acc[4] == 6 * N_PATHS
    # ... and to the oracle's sum of the same six renders, first and second moments
    r = _oracle_sum(6).check(acc, "accumulator of six renders")
    print("accumulator against the oracle: worst |diff| / bound", r)


# ---- 3. the stop rule ----------------------------------------------------------------------------------------------------------------
def _check_rule(history, rounds, target, min_rounds, max_rounds, what):
    print(f"{what}: rounds {rounds}, history {history.tolist()}")
    assert history.shape == (rounds,) and not np.isnan(history).any()
    hits = [r for r in range(rounds) if r >= min_rounds - 1 and history[r] <= target]
    if hits:
        k = hits[0]
        assert rounds == min(k + 2, max_rounds), what
    else:
        assert rounds == max_rounds, what


def _converge_device(g, lp, target, **kw):
    import torch
    lm = mr.with_moment(lp)
    d = torch.full((g.channels(lm),), 7.0, dtype=torch.float32, device="cuda")      # (the callee zeroes it)
    rounds, history, n_sig, st = g.render_converge_device(lp, d.data_ptr(), target, **kw)
    assert st is None
    return d.cpu().numpy(), rounds, history, n_sig


def test_stop_rule(hiplib):
    _, g, _ = _bus()
    lp = _bus_launch(n_paths=N_PATHS, seed=1, flags=0)
    lm = mr.with_moment(lp)
    acc0, _, hist0, n_sig0, _ = _converged_bus()
    # target 0: every round; the last entry is the statistic of what came back
    _check_rule(hist0, 3, 0.0, 1, 3, "target 0")
    _assert_statistic((hist0[-1], n_sig0), capi.converge_statistic(acc0, lm, FLOOR), "last entry, target 0")
    assert np.all(np.isfinite(hist0)) and np.all(hist0 > 0.0)
    # target +inf: as early as the rule permits
    for min_rounds, max_rounds in ((1, 6), (3, 6), (3, 3), (6, 6)):
        acc, rounds, history, n_sig = _converge_device(g, lp, INF, floor=FLOOR, round_renders=2, min_rounds=min_rounds, max_rounds=max_rounds)
        assert rounds == min(min_rounds + 1, max_rounds)
        _check_rule(history, rounds, INF, min_rounds, max_rounds, f"target inf, min {min_rounds}, max {max_rounds}")
        _assert_statistic((history[-1], n_sig), capi.converge_statistic(acc, lm, FLOOR), "last entry, target inf")
        # (two runs of the same rounds agree to the rounding of the renders' fp32 sums, not to the bit: both lie in the oracle's interval)
        _in_intervals(history[:3], f"target inf, min {min_rounds}")
    # Targets between two entries of a first run of all six rounds: a second run stops exactly where that history says.  (The
    # accumulator is a deterministic function of its blocks; the blocks themselves are fp32 sums in the order the atomics land,
    # so two runs agree to the rounding of those sums, 1e-8 relative in the statistic, not to the bit: every target is the
    # midpoint of two neighbouring entries that are at least 1e-3 apart, relative.)  The history of independent samples need
    # not fall from round to round: a rare strong path can make a bin significant, or raise one's variance estimate.
    acc6, rounds6, hist6, n_sig6 = _converge_device(g, lp, 0.0, floor=FLOOR, round_renders=2, min_rounds=1, max_rounds=6)
    _check_rule(hist6, rounds6, 0.0, 1, 6, "target 0, six rounds")
    assert rounds6 == 6 and np.all(np.isfinite(hist6))
    _in_intervals(hist6[:3], "target 0, six rounds")
    _assert_statistic((hist6[-1], n_sig6), capi.converge_statistic(acc6, lm, FLOOR), "last entry, six rounds")
    order = np.sort(hist6)
    assert np.all(np.diff(order) >= 1e-3 * order[1:])
    cases = [(0.5 * (lo + hi), m, mx) for lo, hi in zip(order[:-1], order[1:]) for m, mx in ((1, 6), (2, 6), (3, 6), (1, 2))]
    seen = set()
    for target, min_rounds, max_rounds in cases:
        hits = [r for r in range(max_rounds) if r >= min_rounds - 1 and hist6[r] <= target]
        want = min(hits[0] + 2, max_rounds) if hits else max_rounds
        what = f"middle target {target!r}, min {min_rounds}, max {max_rounds}"
        acc, rounds, history, n_sig = _converge_device(g, lp, target, floor=FLOOR, round_renders=2, min_rounds=min_rounds, max_rounds=max_rounds)
        assert rounds == want, (what, rounds, want, hist6.tolist())
        _check_rule(history, rounds, target, min_rounds, max_rounds, what)
        assert np.all((history <= target) == (hist6[:rounds] <= target)), what
        _in_intervals(history[:3], what)
        _assert_statistic((history[-1], n_sig), capi.converge_statistic(acc, lm, FLOOR), "last entry, " + what)
        if rounds == 3:
            _oracle_sum(6).check_two(acc, acc0, "two runs of the same three rounds")
        seen.add(bool(hits) and hits[0] > min_rounds - 1)
    # among them a target that a round before k* missed (max_rounds cutting the look-ahead round off: target inf above)
    assert True in seen


# ---- 4. what the statistic means, against the oracle -------------------------------------------------------------------------------
def _rel(m1, m2, n):
    mean = m1 / n
    return np.sqrt(np.maximum(m2 / n - mean * mean, 0.0) / (n - 1.0)) / np.abs(mean)


@functools.lru_cache(maxsize=None)
def _oracle_intervals():
    """[(lo, hi, significant bins)] of the statistic after rounds 0, 1, 2 of the bus rounds (R = 2, BUS_SEEDS), by the oracle alone"""
    floor = float(np.float32(FLOOR))
    lm = _bus_launch(n_paths=N_PATHS, seed=1)
    first, second, _ = (a.reshape(-1) for a in capi.converge_layout(lm))
    intervals = []
    for r in range(3):
        exp = _oracle_sum(2 * (r + 1))
        n = float(N_PATHS * 2 * (r + 1))
        m1, b1, m2, b2, N = np.abs(exp.ref[first]), exp.bound[first], exp.ref[second], exp.bound[second], exp.N[first]
        top = int(np.argmax(m1))
        sig = m1 - b1 >= floor * (m1[top] + b1[top])
        out = m1 + b1 < floor * (m1[top] - b1[top])
        assert np.all(sig | out), "a watched bin lies within its bound of the significance threshold"
        assert sig.sum() >= 3 and N[sig].min() >= 64 and np.all(m1[sig] > b1[sig])
        lo = _rel(m1 + b1, np.maximum(m2 - b2, 0.0), n)[sig].max()
        hi = _rel(m1 - b1, m2 + b2, n)[sig].max()
        intervals.append((lo, hi, int(sig.sum())))
    return intervals


def _in_intervals(history, what):
    for r, (lo, hi, k) in enumerate(_oracle_intervals()[:len(history)]):
        print(f"{what}, round {r}: {lo!r} <= {history[r]!r} <= {hi!r}, {k} significant bins")
        assert lo <= history[r] <= hi, (what, r)


def test_statistic_history_lies_in_the_oracles_interval(hiplib):
    """The watched bins of the bus (range mode, floor 0.05: the bins that carry at least a twentieth of the strongest, three or
    more of them with 64 addends or more each in every round: asserted in _oracle_intervals).  Per round the oracle gives E and N of every m1 and m2 cell of the accumulator
    (tests/moment_ref.py) and so the cell's interval E +- bound; the statistic is increasing in every m2 and decreasing in
    every |m1|, so it lies between its values at the interval ends.  The floor is such that no watched bin is within its
    bound of the significance threshold (asserted, by the oracle alone, in _oracle_intervals), so the share of bins excluded
    for that reason is 0."""
    intervals = _oracle_intervals()      # the oracle alone first, then the device
    _, _, history, n_sig, _ = _converged_bus()
    _in_intervals(history, "three rounds")
    assert n_sig == intervals[-1][2]


def test_accumulated_error_bar_brackets_the_spread_over_disjoint_calls(hiplib):
    """What the statistic the stop rule acts on means: the relative standard error of the accumulated mean.  STATISTICAL, with
    its condition: the bus in range mode, one call of four rounds of four renders (2^16 paths, BUS_SEEDS) and its significant
    bins at FLOOR (the bins the statistic watches; by the oracle each has 64 addends or more after two renders already, asserted
    in _oracle_intervals, so eight times that here, and its variance estimate is better than the spread's own error).  rel of each such bin, from the accumulator of that ONE call,
    against the relative spread (sample standard deviation) of the bin's accumulated mean over 16 further calls whose seeds
    are 1000003 apart, more than the 2^16 streams a call covers, so that no two of the 17 calls share a path.  The two must
    agree within a factor 2 either way, as tests/test_gpu_moment.py asks of one render: the spread of 16 means has a
    relative error of 1 / sqrt(30) = 18 %, so a factor 2 is ln 2 / 0.18 = 3.8 standard deviations, and the seeds are fixed.
    Renders that shared their paths (consecutive seeds) would show a spread sqrt(16) = 4 times the error bar."""
    _, g, _ = _bus()
    lp = _bus_launch(n_paths=N_PATHS, seed=1, flags=0)
    lm = mr.with_moment(lp)
    kw = dict(floor=FLOOR, round_renders=4, min_rounds=1, max_rounds=4, want_stats=False)
    first, second, _ = (a.reshape(-1) for a in capi.converge_layout(lm))
    n = 16.0 * N_PATHS
    acc, rounds, history, n_sig, _ = g.render_converge(lp, 0.0, **kw)
    assert rounds == 4 and acc[4] == n and list(BUS_SEEDS) == _seeds(lp, 16)
    m1 = acc[first].astype(np.float64)
    sig = np.abs(m1) >= float(np.float32(FLOOR)) * np.abs(m1).max()
    rel = _rel(m1, acc[second].astype(np.float64), n)[sig]
    assert sig.sum() == n_sig >= 3 and _ulps(rel.max(), history[-1]) <= 4
    # (the error bar of 16 renders is that of one round over sqrt(4): n, m1 and m2 grew with new samples)
    means = []
    for k in range(16):
        h, r, _, _, _ = g.render_converge(mr.copy_launch(lp, seed=(65 + k) * 1000003), 0.0, **kw)
        assert r == 4 and h[4] == n
        means.append(h[first].astype(np.float64)[sig] / n)
    means = np.array(means)
    spread = means.std(axis=0, ddof=1) / np.abs(means.mean(axis=0))
    ratio = spread / rel
    print("spread of the accumulated mean over 16 disjoint calls / rel of one call, per significant bin:", ratio.tolist(),
          "statistic", float(history[-1]))
    assert 0.5 <= ratio.min() and ratio.max() <= 2.0, ratio


# ---- 5. launch forms --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["raw", "iq"])
def test_receive_rounds_of_four(hiplib, form):
    sd, lp = _receive_scene("plate")
    lp.mode = capi.BF_MODE_RECEIVE_IQ if form == "iq" else capi.BF_MODE_RECEIVE_RAW
    lm = mr.with_moment(lp)
    g, g2 = capi.Scene(sd), capi.Scene(sd)
    acc, rounds, history, n_sig, st = g.render_converge(lp, 0.0, floor=0.1, round_renders=4, max_rounds=2)
    assert rounds == 2 and st.n_paths == 8 * lp.n_paths
    hs = np.array([g2.render(mr.copy_launch(lm, seed=s))[0] for s in _seeds(lp, 8)], np.float64)
    assert np.all(np.abs(acc - hs.sum(axis=0)) <= gamma(8) * np.abs(hs).sum(axis=0))
    w = capi.converge_layout(lm)[2]
    assert acc[w].sum() + st.n_invalid == 8 * lp.n_paths
    _assert_statistic((history[-1], n_sig), capi.converge_statistic(acc, lm, 0.1), f"receive {form}, two rounds of four")


def test_film_rounds_are_single_renders(hiplib):
    sd, lp = scenes.film_half_lit(film=(8, 6), spp=64, mode=capi.BF_MODE_RANGE, bins=16, dr=0.4)
    lm = mr.with_moment(lp)
    g, g2 = capi.Scene(sd), capi.Scene(sd)
    with pytest.raises(capi.BeifongError, match=r"status 1\).*multi-pixel"):
        g.render_converge(lp, 0.0, round_renders=2, max_rounds=2)
    # (floor 0.01: with a high one only the evenly lit pixels are significant, whose samples are all equal: stat 0 <= target 0)
    acc, rounds, history, n_sig, st = g.render_converge(lp, 0.0, floor=0.01, round_renders=1, max_rounds=3)
    assert rounds == 3 and acc.size == 48 * (11 + 32) and np.all(history > 0.0) and st.n_paths == 3 * lp.n_paths
    hs = np.array([g2.render(mr.copy_launch(lm, seed=s))[0] for s in _seeds(lp, 3)], np.float64)
    assert np.all(np.abs(acc - hs.sum(axis=0)) <= gamma(3) * np.abs(hs).sum(axis=0))
    _assert_statistic((history[-1], n_sig), capi.converge_statistic(acc, lm, 0.01), "film, three rounds")
    # with floor 1 only the brightest bins are watched, and their samples are all equal: stat 0 meets target 0 in round 0
    acc, rounds, history, n_sig, st = g.render_converge(lp, 0.0, floor=1.0, round_renders=1, max_rounds=3)
    assert rounds == 2 and history.tolist() == [0.0, 0.0] and n_sig >= 1


def test_call_while_a_rolling_sequence_is_open(hiplib):
    _, g, _ = _bus()
    from tests.test_gpu_moment import _bus_expected
    lp = _bus_launch(n_paths=N_PATHS)
    seq = _Sequence(g, lp, [5, 6])
    seq.issue()
    acc, rounds, history, n_sig = _converge_device(g, _bus_launch(n_paths=N_PATHS, seed=1, flags=0), 0.0, floor=FLOOR, round_renders=2, max_rounds=3)
    assert rounds == 3
    _in_intervals(history, "behind an open rolling sequence")
    _oracle_sum(6).check(acc, "accumulator behind an open rolling sequence")
    g.flush()
    h, recs = seq.results()
    for k, seed in enumerate([5, 6]):
        rec_o, exp = _bus_expected(capi.BF_MODE_RANGE, capi.BF_COLOR_RGB, N_PATHS, seed)
        _same_records(recs[k], rec_o)
        exp.check(h[k], f"rolling render {k} around a converge call")
        assert h[k][4] == N_PATHS


def test_clone_converges_concurrently_on_another_stream(hiplib):
    import torch
    _, g, _ = _bus()
    exp = _oracle_sum(6)
    handles = [g, g.clone()]
    streams = [torch.cuda.Stream() for _ in handles]
    lm = _bus_launch(n_paths=N_PATHS, seed=1)
    bufs = [torch.zeros(g.channels(lm), dtype=torch.float32, device="cuda") for _ in handles]
    torch.cuda.synchronize()
    out = [None, None]

    def run(k):
        out[k] = handles[k].render_converge_device(lm, bufs[k].data_ptr(), 0.0, floor=FLOOR, round_renders=2, max_rounds=3,
                                                   stream=streams[k].cuda_stream)

    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    for k in range(2):
        assert out[k] is not None and out[k][0] == 3
        _in_intervals(out[k][1], f"handle {k} of two converging side by side")
        exp.check(bufs[k].cpu().numpy(), f"accumulator of handle {k}")


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was(hiplib):
    """After every refusal a plain render on the handle is what it was before: its path records bit-equal, its count channels
    equal, and its histogram the same fp32 sum of the same addends.  The histogram itself is not reproducible to the bit from
    one render to the next (float atomics land in an order of their own), so it is held to the bound two summations of the
    oracle's addends obey (tests/hist_bound.py), cell by cell."""
    import torch
    sd, g, osc = _bus()
    lp = _bus_launch(n_paths=N_PATHS, seed=9, flags=0)
    add = osc.render(lp, threads=8, addends=True)[3]
    h0, rec0, _ = g.render(lp, records=True)

    def still_the_same(handle, what):
        h1, rec1, _ = handle.render(lp, records=True)
        _same_records(rec1, rec0)
        assert_two_fp32_sums(h1, h0, add.S, add.N, f"plain render after the refusal of {what}", counts=count_channels(lp, sd))
    d = torch.zeros(g.channels(mr.with_moment(lp)), dtype=torch.float32, device="cuda")
    ok = dict(target=0.1, floor=0.01, round_renders=2, min_rounds=1, max_rounds=3)
    cases = [
        (dict(flags=capi.BF_FLAG_FAST), {}, "BF_FLAG_FAST"),
        (dict(flags=capi.BF_FLAG_ROLLING), {}, "BF_FLAG_ROLLING"),
        ({}, dict(target=-0.1), "target"),
        ({}, dict(target=float("nan")), "target"),
        ({}, dict(floor=-0.5), "floor"),
        ({}, dict(floor=1.5), "floor"),
        ({}, dict(round_renders=0), "round_renders"),
        ({}, dict(max_rounds=0, min_rounds=0), "max_rounds"),
        ({}, dict(min_rounds=4), "min_rounds"),
        (dict(n_paths=0), {}, "n_paths"),
    ]
    for launch_kw, call_kw, match in cases:
        bad = mr.copy_launch(lp, **launch_kw)
        kw = dict(ok, **call_kw)
        with pytest.raises(capi.BeifongError, match=rf"status 1\).*{match}"):
            g.render_converge_device(bad, d.data_ptr(), kw.pop("target"), **kw)
        still_the_same(g, match)
    assert float(d.abs().sum()) == 0.0
    # a multi-pixel film with two renders per round, on the same handle (the bus scene under a 4 x 2 film)
    film = mr.copy_launch(lp, film_width=4, film_height=2, spp=N_PATHS // 8)
    df = torch.zeros(g.channels(mr.with_moment(film)), dtype=torch.float32, device="cuda")
    with pytest.raises(capi.BeifongError, match=r"status 1\).*multi-pixel"):
        g.render_converge_device(film, df.data_ptr(), 0.1, floor=0.01, round_renders=2, min_rounds=1, max_rounds=3)
    still_the_same(g, "a film with round_renders 2")
    assert float(df.abs().sum()) == 0.0


# ---- 7. the host layer ------------------------------------------------------------------------------------------------------------------
def test_moment_integrator_renders_until_converged(hiplib):
    from beifong_amd import mitsuba as m
    from beifong_amd.mitsuba.core.xml import load_string
    from tests.oracle_lib import OracleScene
    m.set_variant("scalar_rgb")
    props = '<float name="rel_stderr" value="$err"/><float name="significance" value="0.25"/><integer name="max_passes" value="6"/>' \
            '<integer name="passes_per_round" value="2"/>'
    xml = HOST_XML.replace('<integrator type="moment">', '<integrator type="moment">' + props, 1)
    scene = load_string(xml, spp=2048, err=1.0e-6)
    sensor, integ = scene.sensors()[0], scene.integrator()
    integ.render(scene, sensor)
    rounds, stat, n_sig = integ.converge_stats()
    img = np.array(sensor.film().bitmap(raw=True)).reshape(-1)
    lp = integ.launch_for(sensor)
    assert rounds == 3 and lp.n_paths == 2048 and img[4] == 6 * 2048 and integ.stats()[0].n_paths == 6 * 2048
    _assert_statistic((stat, n_sig), capi.converge_statistic(img, lp, 0.25), "the film of the converging integrator")
    # the same six renders through the C ABI
    g = capi.Scene(scene.flat_desc(sensor))
    hs = np.array([g.render(mr.copy_launch(lp, seed=s))[0] for s in _seeds(lp, 6)], np.float64)
    assert np.all(np.abs(img - hs.sum(axis=0)) <= gamma(6) * np.abs(hs).sum(axis=0))
    # an easy target stops after the look-ahead round
    scene = load_string(xml, spp=2048, err=1.0e3)
    scene.integrator().render(scene, scene.sensors()[0])
    assert scene.integrator().converge_stats()[0] == 2
    # rel_stderr = 0 is the moment integrator as it was.  A render is not reproducible to the bit (float atomics land in an order
    # of their own; tests/test_gpu_moment.py holds the integrator's bitmap to the oracle for that reason), so "equal to today's
    # render" is: the same launch bytes, the bitmap within the oracle's bound, and within the two-run bound of the bitmap of a
    # moment integrator that has no rel_stderr property at all
    scene = load_string(HOST_XML.replace('<integrator type="moment">', '<integrator type="moment"><float name="rel_stderr" value="0"/>', 1), spp=2048)
    sensor, integ = scene.sensors()[0], scene.integrator()
    integ.render(scene, sensor)
    assert integ.converge_stats() == (0, 0.0, 0)
    img0 = np.array(sensor.film().bitmap(raw=True)).reshape(-1)
    l0 = mr.plain(integ.launch_for(sensor))
    assert bytes(integ.launch_for(sensor)) == bytes(lp)
    _, rec_o, _, add = OracleScene(scene.flat_desc(sensor)).render(l0, records=True, threads=8, addends=True)
    exp = mr.Expected(l0, add.ref, add.S, add.N, mr.from_records(rec_o, l0), weight_one=True)
    exp.check(img0, "rel_stderr = 0")
    assert img0[4] == 2048
    scene = load_string(HOST_XML, spp=2048)
    sensor, integ = scene.sensors()[0], scene.integrator()
    integ.render(scene, sensor)
    assert integ.converge_stats() == (0, 0.0, 0) and bytes(integ.launch_for(sensor)) == bytes(lp)
    exp.check_two(img0, np.array(sensor.film().bitmap(raw=True)).reshape(-1), "rel_stderr = 0 against no rel_stderr")
