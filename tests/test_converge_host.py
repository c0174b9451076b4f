"""Render until converged, without a GPU: the numpy statement of the statistic (capi.converge_statistic: the specification
the kernels of bf_converge.hip are held to), the new symbols, the unchanged ABI handshake and the `moment` plugin's
properties."""
import ctypes as C
import re

import numpy as np
import pytest

from beifong_amd import capi
from tests.test_moment_host import MOMENT_XML, mitsuba  # noqa: F401  (the fixture)

M = capi.BF_FLAG_MOMENT
INF = float("inf")


def _path(n=1000):
    """path mode: the one watched pair is nested.Y (channels 6 and 9), n is W (channel 4)"""
    return capi.make_launch(capi.BF_MODE_PATH, n, flags=M), np.zeros(11, np.float32)


def _range(bins, n=1000):
    lp = capi.make_launch(capi.BF_MODE_RANGE, n, bins=bins, bin_width=1.0, flags=M)
    h = np.zeros(11 + 2 * bins, np.float32)
    h[4] = n
    return lp, h


def test_equal_samples_have_no_error():
    lp, h = _path()
    h[4], h[6], h[9] = 1000, 3.0 * 1000, 9.0 * 1000
    assert capi.converge_statistic(h, lp, 0.01) == (0.0, 1)
    # nested.X and nested.Z are not watched in path mode: whatever they hold changes nothing
    h[5], h[8], h[7] = 7.0, 1.0e6, 5000.0
    assert capi.converge_statistic(h, lp, 0.01) == (0.0, 1)


def test_two_bins_by_hand():
    n = 1000
    lp, h = _range(2, n)
    # bin 0: samples {0, 2} in equal numbers: mean 1, E x^2 = 2, var_of_mean = 1 / (n - 1)
    h[5], h[5 + 5] = n, 2 * n
    # bin 1: a quarter of the samples is 4: mean 1, E x^2 = 4, var_of_mean = 3 / (n - 1)
    h[6], h[6 + 5] = n, 4 * n
    stat, n_sig = capi.converge_statistic(h, lp, 0.5)
    assert n_sig == 2 and stat == np.sqrt(3.0 / (n - 1))
    # the watched pairs are the A nested AOVs: a noisy nested.X (channel 5 + bins) is not among them
    h[7], h[7 + 5] = 1.0, 1.0e6
    assert capi.converge_statistic(h, lp, 0.5) == (stat, 2)
    first, second, w = capi.converge_layout(lp)
    assert first.tolist() == [[5, 6]] and second.tolist() == [[10, 11]] and w.tolist() == [[4]]


def test_the_floor_counts_a_bin_at_it_and_ignores_one_below():
    n = 1024
    lp, h = _range(3, n)
    h[5], h[5 + 6] = 1024.0, 1024.0            # samples all 1: rel 0
    h[6], h[6 + 6] = 512.0, 512.0 * 8          # at half the largest: mean 0.5, E x^2 = 4
    h[7], h[7 + 6] = 256.0, 256.0 * 64         # a quarter of the largest, noisier still
    rel1 = np.sqrt((4.0 - 0.25) / (n - 1)) / 0.5
    rel2 = np.sqrt((16.0 - 0.0625) / (n - 1)) / 0.25
    assert capi.converge_statistic(h, lp, 0.5) == (rel1, 2)              # |m1| == floor * max counts
    assert capi.converge_statistic(h, lp, 0.5000001) == (0.0, 1)
    assert capi.converge_statistic(h, lp, 0.25) == (rel2, 3)
    assert capi.converge_statistic(h, lp, 1.0) == (0.0, 1)
    # floor 0 admits the empty bins too, whose mean is 0
    lp4, h4 = _range(4, n)
    h4[5], h4[5 + 7] = 1024.0, 1024.0
    assert capi.converge_statistic(h4, lp4, 0.0) == (INF, 4)
    with pytest.raises(ValueError):
        capi.converge_statistic(h, lp, 1.5)


def test_the_three_infinite_cases_are_never_nan():
    lp, h = _range(2)
    assert capi.converge_statistic(h, lp, 0.01) == (INF, 0)             # all zero: nothing is significant
    assert capi.converge_statistic(np.zeros_like(h), lp, 0.0) == (INF, 0)
    h[4], h[5], h[10] = 1.0, 2.0, 4.0                                    # n == 1
    assert capi.converge_statistic(h, lp, 0.01) == (INF, 1)
    h[4] = 1000.0
    assert capi.converge_statistic(h, lp, 0.01)[0] < INF
    for bad in (np.nan, np.inf, -np.inf):
        for cell in (0, 6, 11):                                          # any cell, watched or not
            g = h.copy()
            g[cell] = bad
            assert capi.converge_statistic(g, lp, 0.01) == (INF, 0)
    with pytest.raises(ValueError):
        capi.converge_statistic(h[:-1], lp, 0.01)


def test_layouts_pick_the_watched_pairs():
    # receive RAW with phase bins: Y of every cell (channel 0, m2_Y last), n = the cell's W
    lp = capi.make_launch(capi.BF_MODE_RECEIVE_RAW, 64, bins=2, bins_y=1, phase_bins=3, flags=M)
    first, second, w = capi.converge_layout(lp)
    assert (first.tolist(), second.tolist(), w.tolist()) == ([[0], [7]], [[6], [13]], [[2], [9]])
    h = np.zeros(14, np.float32)
    h[0:7] = [10.0, 1.0, 10.0, 99.0, 99.0, 99.0, 10.0]                  # ten samples 1
    h[7:14] = [10.0, 1.0, 20.0, 0.0, 0.0, 0.0, 10.0]                    # ten samples 1 and ten 0: mean .5, E x^2 = .5
    assert capi.converge_statistic(h, lp, 0.5) == (np.sqrt((0.5 - 0.25) / 19) / 0.5, 2)
    # receive IQ: I and Q of every cell
    lp = capi.make_launch(capi.BF_MODE_RECEIVE_IQ, 64, bins=2, bins_y=1, flags=M)
    first, second, w = capi.converge_layout(lp)
    assert (first.tolist(), second.tolist(), w.tolist()) == ([[0, 1], [5, 6]], [[3, 4], [8, 9]], [[2], [7]])
    h = np.array([10.0, -10.0, 10.0, 10.0, 10.0, 0.0, 20.0, 40.0, 0.0, 20.0], np.float32)
    stat, n_sig = capi.converge_statistic(h, lp, 0.5)
    assert n_sig == 3 and stat == np.sqrt((20.0 / 40 - 0.25) / 39) / 0.5
    # a film: the A AOVs of every pixel with the pixel's own W; time mode has 3 bins of them
    lp = capi.make_launch(capi.BF_MODE_TIME, 8, bins=2, bin_width=1.0, flags=M, film=(2, 1), spp=4)
    first, second, w = capi.converge_layout(lp)
    assert first.shape == (2, 6) and first[1].tolist() == list(range(23 + 5, 23 + 11)) and second[0, 0] == 5 + 9 and w.tolist() == [[4], [27]]
    h = np.zeros(46, np.float32)
    h[4], h[5], h[14] = 4.0, 4.0, 4.0                                    # pixel 0: four samples 1
    h[27], h[28 + 5], h[28 + 5 + 9] = 2.0, 2.0, 4.0                      # pixel 1, last AOV: samples {0, 2}: mean 1, E x^2 = 2, n = 2
    assert capi.converge_statistic(h, lp, 0.5) == (np.sqrt(1.0 / 1.0), 2)
    # the launch need not carry the flag: the converge entries force it on
    assert capi.converge_statistic(h, capi.make_launch(capi.BF_MODE_TIME, 8, bins=2, bin_width=1.0, film=(2, 1), spp=4), 0.5)[1] == 2


def test_symbols_and_the_unchanged_handshake(hiplib):
    new = ["bf_render_converge_device", "bf_render_converge", "bf_converge_statistic_device"]
    for name in new:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(hiplib, name)
    assert hiplib.bf_version() == 5 and capi.BF_ABI_VERSION == 5
    assert [t.__name__ for t in capi.ABI_STRUCTS] == ["bf_material", "bf_shape", "bf_emitter", "bf_sensor", "bf_scene_desc", "bf_launch",
                                                      "bf_path_record", "bf_stats", "bf_scene_info", "bf_batch"]
    assert hiplib.bf_abi_sizeof(len(capi.ABI_STRUCTS)) == 0
    for m in ("render_converge", "render_converge_device", "converge_statistic_device"):
        assert callable(getattr(capi.Scene, m))


def test_the_statistic_entry_refuses_before_it_touches_the_device(hiplib):
    """null pointers, a floor outside [0, 1] and a launch without cells are refused on the host"""
    lp = capi.make_launch(capi.BF_MODE_RANGE, 8, bins=4, bin_width=1.0, flags=M)
    stat, n_sig = C.c_double(), C.c_uint64()
    fn = hiplib.bf_converge_statistic_device
    assert fn(C.byref(lp), None, 0.01, C.byref(stat), C.byref(n_sig), None) == capi.BF_ERR_INVALID
    for floor in (-0.1, 1.5, float("nan")):
        assert fn(C.byref(lp), C.c_void_p(256), floor, C.byref(stat), C.byref(n_sig), None) == capi.BF_ERR_INVALID
        assert b"floor" in hiplib.bf_last_error()
    lp0 = capi.make_launch(capi.BF_MODE_RECEIVE_RAW, 8, bins=0, bins_y=0, flags=M)
    assert fn(C.byref(lp0), C.c_void_p(256), 0.01, C.byref(stat), C.byref(n_sig), None) == capi.BF_ERR_INVALID
    rounds = C.c_uint32()
    assert hiplib.bf_render_converge_device(None, C.byref(lp), 0.1, 0.01, 4, 1, 8, C.c_void_p(256), None, C.byref(rounds), None, None,
                                            None) == capi.BF_ERR_INVALID


def _with(props, xml=MOMENT_XML):
    out = xml.replace('<integrator type="moment">', '<integrator type="moment">' + props, 1)
    assert out != xml
    return out


def test_moment_plugin_parses_the_converge_properties(mitsuba):  # noqa: F811
    from beifong_amd.mitsuba.core.xml import load_dict, load_string
    scene = load_string(_with('<float name="rel_stderr" value="0.05"/><float name="significance" value="0.1"/>'
                              '<integer name="max_passes" value="12"/><integer name="passes_per_round" value="3"/>'))
    integ = scene.integrator()
    # the launch is the per-render one, and nothing has rendered yet
    lp = integ.launch_for(scene.sensors()[0])
    assert lp.n_paths == 64 and lp.flags & M
    assert integ.converge_stats() == (0, 0.0, 0)
    # rel_stderr = 0 is the integrator as it was
    load_string(_with('<float name="rel_stderr" value="0"/>'))
    # -D substitution and load_dict reach the same properties
    load_string(_with('<float name="rel_stderr" value="$err"/>'), err=0.1)
    from beifong_amd.mitsuba.core import Transform4f
    look = Transform4f.look_at([0, 0, 0], [0, -1, 0], [0, 0, 1])
    load_dict({"type": "scene",
               "integrator": {"type": "moment", "rel_stderr": 0.05, "max_passes": 8, "passes_per_round": 2,
                              "nested": {"type": "range", "integrator": {"type": "pathlength"}, "dr": 0.5, "bins": 4}},
               "sensor": {"type": "perspective", "to_world": look, "sampler": {"type": "independent", "sample_count": 64},
                          "film": {"type": "hdrfilm", "rfilter": {"type": "box"}, "width": 1, "height": 1}},
               "emitter": {"type": "spot", "intensity": {"type": "spectrum", "value": 10}, "to_world": look},
               "shape": {"type": "rectangle", "to_world": Transform4f.look_at([0, -1, 0], [0, 0, 0], [0, 0, 1]),
                         "bsdf": {"type": "twosided", "bsdf": {"type": "diffuse"}}}})


@pytest.mark.parametrize("props, match", [
    ('<float name="rel_stderr" value="-0.1"/>', "rel_stderr"),
    ('<float name="significance" value="0.1"/>', "significance.*without.*rel_stderr"),
    ('<integer name="max_passes" value="8"/>', "max_passes.*without.*rel_stderr"),
    ('<float name="rel_stderr" value="0"/><integer name="passes_per_round" value="2"/>', "passes_per_round.*without.*rel_stderr"),
    ('<float name="rel_stderr" value="0.1"/><float name="significance" value="1.5"/>', "significance"),
    ('<float name="rel_stderr" value="0.1"/><integer name="max_passes" value="0"/>', "max_passes"),
    ('<float name="rel_stderr" value="0.1"/><integer name="max_passes" value="10"/><integer name="passes_per_round" value="4"/>',
     "max_passes.*multiple.*passes_per_round"),
    ('<float name="rel_stderr" value="0.1"/><integer name="passes_per_round" value="-1"/>', "passes_per_round"),
    ('<float name="rel_stderr" value="0.1"/><boolean name="fast_math" value="true"/>', "fast_math"),
])
def test_moment_plugin_refuses_by_name(mitsuba, props, match):  # noqa: F811
    from beifong_amd.mitsuba import _host
    from beifong_amd.mitsuba.core.xml import load_string
    with pytest.raises(_host.HostError, match=re.compile(match, re.S)):
        load_string(_with(props))
    below = MOMENT_XML.replace('<integrator type="pathlength">', '<integrator type="pathlength"><boolean name="fast_math" value="true"/>')
    with pytest.raises(_host.HostError, match="fast_math"):
        load_string(_with('<float name="rel_stderr" value="0.1"/>', below))


def test_converge_seeds_are_n_paths_apart():
    """render k of a call draws from the streams seed + k n_paths + path_offset + p, p < n_paths: disjoint from every other render's"""
    lp = capi.make_launch(capi.BF_MODE_RANGE, 4096, seed=7, bins=4, bin_width=1.0)
    assert capi.converge_seeds(lp, 4).tolist() == [7, 7 + 4096, 7 + 8192, 7 + 12288]
    lp.seed = (1 << 64) - 1
    s = capi.converge_seeds(lp, 2)
    assert s.dtype == np.uint64 and s.tolist() == [(1 << 64) - 1, 4095]
