"""Returns by target class (BF_FLAG_CLASSES), the part that needs no GPU: the reference helper's own checks on the four scene
families the GPU tests use (tests/class_ref.py: the composed first hit equals record.valid for every path, and stays below
the far clip), the shapes of capi.split_classes, and the two new exports of the built library."""
import ctypes as C

import numpy as np
import pytest

from beifong_amd import capi, scenes
from tests import class_ref
from tests.oracle_lib import OracleScene

N = 4096


def _counts(shape, n_shapes):
    return [int((shape == s).sum()) for s in range(n_shapes)], int((shape < 0).sum())


def test_first_hits_c4():
    sd, lp = scenes.multi_mesh_radar(n_paths=N, bins=64, dr=0.4, seed=3, scale=0.01)
    shape, hit = class_ref.first_hits(sd, lp)
    per_shape, miss = _counts(shape, len(sd.shapes))
    # TX aperture, ground, bus, car, motorbike
    assert per_shape[0] == 0 and min(per_shape[1:]) >= 100 and miss >= 100, (per_shape, miss)
    assert sum(per_shape) + miss == N and int(hit.sum()) == sum(per_shape)


def test_first_hits_fluxmeter_time_mode():
    sd, lp = scenes.trans_rad(spp=N)
    shape, _ = class_ref.first_hits(sd, lp)
    per_shape, miss = _counts(shape, len(sd.shapes))
    # the flux meter's aperture, the target, the ground
    assert per_shape[0] == 0 and per_shape[1] >= 100 and per_shape[2] >= 100 and miss >= 100, (per_shape, miss)


def test_first_hits_film():
    sd, lp = class_ref.film_scene()
    shape, _ = class_ref.first_hits(sd, lp)
    per_shape, miss = _counts(shape, len(sd.shapes))
    assert per_shape[0] == 0 and per_shape[1] >= 100 and per_shape[2] >= 100 and miss >= 100, (per_shape, miss)


@pytest.mark.parametrize("mode", [capi.BF_MODE_RECEIVE_RAW, capi.BF_MODE_RECEIVE_IQ], ids=["raw", "iq"])
def test_first_hits_receive_through_the_twin(mode):
    sd, lp = class_ref.receive_scene()
    lp.mode = mode
    twin = class_ref.fluxmeter_twin(class_ref.receive_scene)
    shape, _ = class_ref.first_hits(sd, lp, twin=twin)
    per_shape, miss = _counts(shape, len(sd.shapes))
    # TX aperture, RX aperture, ground, bus
    assert per_shape[0] == 0 and per_shape[1] == 0 and per_shape[2] >= 100 and per_shape[3] >= 100 and miss >= 100, (per_shape, miss)
    # traced on the twin instead: the same first hits
    shape_t, _ = class_ref.first_hits(sd, lp, twin=twin, trace_sd=twin, records=OracleScene(sd).render(lp, records=True, threads=8)[1])
    assert np.array_equal(shape, shape_t)


def test_per_class_bookkeeping():
    """per_class asserts that its blocks add up to the oracle's Addends; here also: an unpopulated class is all zeros"""
    sd, lp = scenes.multi_mesh_radar(n_paths=512, bins=16, dr=1.6, seed=3, scale=0.01)
    exp, rec, add = class_ref.expected(sd, lp, [0, 1, 2, 3, 4], 7, 5)
    assert exp.ref.shape == (7, 21) and not exp.N[0].any() and not exp.N[6].any()
    assert int(exp.N[:, 4].sum()) == 512 and np.array_equal(exp.population(), exp.N[:, 4])
    merged = exp.merged([0, 1, 2, 2, 2, 3, 0])
    assert merged.ref.shape == (4, 21) and np.array_equal(merged.N[2], exp.N[2] + exp.N[3] + exp.N[4])


def test_split_classes_shapes():
    lp = capi.make_launch(capi.BF_MODE_RANGE, 16, bins=7, bin_width=1.0)
    flat = np.arange(5 * 12, dtype=np.float32)
    v = capi.split_classes(flat, lp, 5)
    assert v.shape == (5, 12) and v[3, 2] == flat[3 * 12 + 2] and np.shares_memory(v, flat)
    assert capi.split_classes(np.zeros((3, 5 * 12), np.float32), lp, 5).shape == (3, 5, 12)
    assert capi.split_classes(np.zeros((2, 3, 12), np.float32), lp, 1).shape == (2, 3, 1, 12)
    iq = capi.make_launch(capi.BF_MODE_RECEIVE_IQ, 16, bins=4, bins_y=2)
    assert capi.split_classes(np.zeros(2 * 24, np.float32), iq, 2).shape == (2, 24)
    for bad, n in ((flat, 4), (flat[:-1], 5), (flat, 0)):
        with pytest.raises(ValueError):
            capi.split_classes(bad, lp, n)


def test_library_exports_the_class_entries():
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("bf_scene_set_classes", "bf_scene_launch_channels"):
        assert name in capi.EXPORTED_SYMBOLS
        getattr(lib, name)          # AttributeError: not exported
    assert capi.BF_FLAG_CLASSES == 1024 and capi.BF_VARIANT_CLASS == 16 and capi.BF_MAX_CLASSES == 256
    # without a scene the count is the plain one
    lp = capi.make_launch(capi.BF_MODE_RANGE, 16, bins=7, bin_width=1.0, flags=capi.BF_FLAG_CLASSES)
    lib = capi.load_library()
    assert lib.bf_scene_launch_channels(None, C.byref(lp)) == lib.bf_launch_channels(C.byref(lp)) == 12
