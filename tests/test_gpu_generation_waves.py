"""The launches of wf_shade that START paths — the first launch of a pool (wf_shade<1>) and the wake launch of a rolling call
(wf_shade<2>) — run at four waves per SIMD where their four-wave build is scratch-free (bf_variant.h: shade_variant:
the lean variants, except the wake launch of a receive-mode sequence), on a grid sized for four workgroups per CU (bf_render.cpp:
wf_setup); the walk launches, and the generation launches of every other variant, stay at three.  A path must be the same path
whatever launch generated it: every per-path record here is held bit for bit to the oracle's (and, for rolling sequences, to a
stand-alone render's), also with a pool far smaller than the grid, with two clones sharing the grids, under an explicit
BF_SHADE_WAVES=3 (a fresh process: every launch at the old budget) and where four workgroups' LDS do not fit a CU and the launch
falls back to three.  bfdbg_scene_generation_waves (a test hook, not the ABI) says which build the last generation launch ran.

Histograms are sums of fp32 atomics, whose order follows the grid: two launches of the same paths on different grids differ in the
last bits (as two runs of one build do).  They are held per cell to the fp32 summation bound around the oracle's exact sum
(tests/hist_bound.py), the count channels exactly; only the records can be, and are, bit-equal."""
import contextlib
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from beifong_amd import capi, scenes
from tests.hist_bound import assert_fp32_sum, count_channels
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _launch_like, _same_records, _Sequence

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TRIS = 2000
SEEDS = [31, 7, 2 ** 40 + 5, 31]


@contextlib.contextmanager
def _env(**kv):
    """BF_* knobs are read when a scene is created: set for the block, restored after it"""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _scene(kind, n_paths, bins=64):
    """(scene description, launch, oracle) — built once per shape and shared, never changed"""
    if kind == "range":
        sd, lp = scenes.bus_radar(n_tris=N_TRIS, n_paths=n_paths, bins=bins, dr=25.6 / bins)
    elif kind == "spot":                        # a spot emitter and a fluxmeter: outside the lean profile, the general kernels
        sd, lp = scenes.trans_rad(spp=n_paths)
    else:
        sd, lp = scenes.bus_receive(n_tris=N_TRIS, n_paths=n_paths, t_bins=bins, dr=25.6 / bins)
        if kind == "receive_iq":
            lp.mode = capi.BF_MODE_RECEIVE_IQ
    return sd, lp, OracleScene(sd)


@functools.lru_cache(maxsize=None)
def _oracle_render(kind, n_paths, seed, bins=64):
    sd, lp, o = _scene(kind, n_paths, bins)
    l1 = _launch_like(lp, seed)
    _, rec, _, add = o.render(l1, records=True, threads=8, addends=True)
    return l1, rec, add


def _hold_to_oracle(kind, n_paths, seed, hist, rec, what, bins=64):
    sd = _scene(kind, n_paths, bins)[0]
    l1, ro, add = _oracle_render(kind, n_paths, seed, bins)
    _same_records(rec, ro)
    assert_fp32_sum(hist, add.ref, add.S, add.N, what, counts=count_channels(l1, sd))


def _fresh(kind, n_paths, seed=SEEDS[0], bins=64):
    """one stand-alone render of a new handle: (histogram, records, waves of its first launch)"""
    sd, lp, _ = _scene(kind, n_paths, bins)
    g = capi.Scene(sd)
    h, r, _ = g.render(_launch_like(lp, seed), records=True)
    waves = g.debug_generation_waves()
    g.close()
    return h, r, waves


def _gen_waves(kind, wake=False):
    """bf_variant.h: shade_variant's rule for four waves — a LEAN launch that starts paths, asked for four: the first launch (first = 1)
    of either mode class, the wake launch (first = 2) outside the receive modes; every other launch three.  The spot scene is outside the
    lean profile, and so is every scene under the knobs that take the lean kernels away (bf_render.cpp: lean_profile: BF_LEAN=0, a walk
    or tail budget other than three); an explicit BF_SHADE_WAVES is every shading launch's budget, so nothing asks for four."""
    e = os.environ
    lean = kind != "spot" and e.get("BF_LEAN", "1") != "0" and e.get("BF_TAIL_WAVES", "3") != "2"
    asked_four = "BF_SHADE_WAVES" not in e
    receive = kind in ("receive", "receive_iq")
    return 4 if asked_four and lean and (not wake or not receive) else 3


def _rolling(kind, n_paths, n_handles=1):
    """rolling sequences of len(SEEDS) renders, flushed, on n_handles clones with a stream each, issued round-robin:
    per handle (histograms, records, waves of its last wake launch)"""
    import torch
    sd, lp, _ = _scene(kind, n_paths)
    hs = [capi.Scene(sd)]
    hs += [hs[0].clone() for _ in range(n_handles - 1)]
    streams = [torch.cuda.Stream() for _ in hs]
    seqs = [_Sequence(h, lp, SEEDS) for h in hs]
    for k in range(len(SEEDS)):
        for j, q in enumerate(seqs):
            q.issue(ks=[k], stream=streams[j].cuda_stream)
    waves = [h.debug_generation_waves() for h in hs]
    for j, h in enumerate(hs):
        h.flush(stream=streams[j].cuda_stream)
    out = [q.results() + (waves[j],) for j, q in enumerate(seqs)]
    for h in hs[1:] + hs[:1]:
        h.close()
    return out


# ---- the three cases that also run under BF_SHADE_WAVES=3 in a fresh process (same code both times) ----------------------------
def _case_fresh():
    return _fresh("range", 1000)


def _case_rolling():
    return _rolling("range", 1 << 12)[0]


def _case_small_pool():
    with _env(BF_WF_POOL="4096"):
        return _fresh("range", 1 << 14)


CASES = {"fresh": _case_fresh, "rolling": _case_rolling, "small_pool": _case_small_pool}


def _records_of(out):
    recs = out[1]
    return list(recs) if isinstance(recs, list) else [recs]


def _dump_cases(path):
    """child-process entry: every case's records and generation waves into one .npz"""
    d = {}
    for name, fn in CASES.items():
        out = fn()
        d[f"{name}_waves"] = np.int64(out[2])
        for k, r in enumerate(_records_of(out)):
            d[f"{name}_{k}"] = r
    np.savez(path, **d)


@pytest.fixture(scope="module")
def old_budget(tmp_path_factory):
    """the three cases in a fresh process under an explicit BF_SHADE_WAVES=3, run once"""
    out = tmp_path_factory.mktemp("old_budget") / "cases.npz"
    code = (f"import sys; sys.path.insert(0, {ROOT!r})\n"
            "import torch\n"                                          # (torch's HIP runtime first, as tests/conftest.py does)
            "from tests import test_gpu_generation_waves as t\n"
            f"t._dump_cases({str(out)!r})\n")
    p = subprocess.run([sys.executable, "-c", code], env={**os.environ, "BF_SHADE_WAVES": "3"}, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    return np.load(out)


# ---- fresh pool: the first launch at four waves, against the oracle -------------------------------------------------------------
@pytest.mark.parametrize("n_paths", [64, 1000, 1 << 14])
@pytest.mark.parametrize("kind", ["range", "receive", "receive_iq", "spot"])
def test_first_launch_at_four_waves_against_the_oracle(hiplib, kind, n_paths):
    """one batch, a ragged pool, 256 batches; the lean kernels of both mode classes at four waves, the general kernels (spot
    emitter), whose four-wave build would spill, at three"""
    h, r, waves = _fresh(kind, n_paths)
    assert waves == _gen_waves(kind)
    _hold_to_oracle(kind, n_paths, SEEDS[0], h, r, f"fresh {kind} {n_paths}")


# ---- rolling: the wake launch at four waves ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n_handles", [("range", 1), ("range", 2), ("receive_iq", 1), ("receive", 1)])
def test_wake_launch_at_four_waves_rolling_sequence(hiplib, kind, n_handles):
    """four renders of 2^12 paths and a flush — alone, and two clones side by side on two streams (the grid-share path of
    wf_setup): every render against the oracle and against a stand-alone render of the same seed.  The receive modes: the lean
    wake launches that stay at three waves (after a first launch at four)"""
    n = 1 << 12
    sd, lp, _ = _scene(kind, n)
    alone = capi.Scene(sd)
    for h, recs, waves in _rolling(kind, n, n_handles):
        assert waves == _gen_waves(kind, wake=True)
        for k, seed in enumerate(SEEDS):
            _hold_to_oracle(kind, n, seed, h[k], recs[k], f"rolling {kind} x{n_handles} render {k}")
            _same_records(recs[k], alone.render(_launch_like(lp, seed), records=True)[1])
        assert np.array_equal(recs[0]["L"].view(np.uint32), recs[3]["L"].view(np.uint32))      # same seed, same render
    alone.close()


# ---- a pool far smaller than the grid ------------------------------------------------------------------------------------------
def test_pool_far_smaller_than_the_grid(hiplib):
    """BF_WF_POOL=4096 with 2^14 paths: 64 batches for a grid of a thousand workgroups — most waves own no batch — and every
    slot regenerates three times"""
    h, r, waves = _case_small_pool()
    assert waves == _gen_waves("range")
    _hold_to_oracle("range", 1 << 14, SEEDS[0], h, r, "pool of 4096")


# ---- the old budget is still reachable and agrees -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_explicit_three_waves_agrees_with_the_default(hiplib, old_budget, case):
    """BF_SHADE_WAVES=3 means every shading launch at three waves, as before; its records are the default's bit for bit"""
    assert int(old_budget[f"{case}_waves"]) == 3
    out = CASES[case]()
    assert out[2] == _gen_waves("range")
    recs = _records_of(out)
    for k, r in enumerate(recs):
        _same_records(r, old_budget[f"{case}_{k}"])


# ---- LDS fallback --------------------------------------------------------------------------------------------------------------
def test_lds_fallback_to_three_waves(hiplib):
    """a range histogram of 12 000 bins is 12 005 floats = 48 020 B of LDS per workgroup (bf_render.cpp: lds_bytes; still below
    kMaxLdsHist, so it IS privatised), + the table copies: three workgroups fit a CU's 160 KiB, four (192 080 B) do not, so the
    first launch runs the three-wave build on the three-wave grid"""
    h, r, waves = _fresh("range", 1 << 12, bins=12000)
    assert waves == 3
    _hold_to_oracle("range", 1 << 12, SEEDS[0], h, r, "12000 bins", bins=12000)
