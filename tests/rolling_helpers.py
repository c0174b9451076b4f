"""Helpers shared by the rolling-sequence and endpoint-update tests (a plain module: no fixtures, no pytest settings).

_same_records holds two sets of per-path records to each other bit for bit, same_records_by_kind likewise up to the payload of
a NaN; _launch_like copies a launch with another
seed / flags / path count / offset; _Sequence issues K rolling renders of one handle into device buffers (torch)."""
import numpy as np

from beifong_amd import capi


def _same_records(a, b):
    for k in ("L", "aux"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert np.array_equal(a["n_rays"], b["n_rays"]) and np.array_equal(a["valid"], b["valid"])


def same_records_by_kind(a, b, what=""):
    """_same_records for renders that return non-finite radiance: bit for bit where b's L is finite; where it is not, the same KIND
    of non-finite in a (NaN for NaN, the same infinity); the sign and payload of a NaN are not part of the contract between the
    oracle's and the device's arithmetic"""
    assert np.array_equal(a["aux"].view(np.uint32), b["aux"].view(np.uint32)), what
    assert np.array_equal(a["n_rays"], b["n_rays"]) and np.array_equal(a["valid"], b["valid"]), what
    fin = np.isfinite(b["L"])
    assert np.array_equal(np.isfinite(a["L"]), fin) and np.array_equal(np.isnan(a["L"]), np.isnan(b["L"])), what
    assert np.array_equal(a["L"][fin].view(np.uint32), b["L"][fin].view(np.uint32)), what
    inf = np.isinf(b["L"])
    assert np.array_equal(a["L"][inf], b["L"][inf]), what


def _launch_like(lp, seed, flags=0, n_paths=None, path_offset=0):
    return capi.make_launch(lp.mode, int(lp.n_paths if n_paths is None else n_paths), seed=seed, path_offset=path_offset, bins=lp.bins,
                            bins_y=lp.bins_y, bin_width=lp.bin_width, color_mode=lp.color_mode, max_depth=lp.max_depth,
                            rr_depth=lp.rr_depth, time_c=lp.time_c, phase_bins=lp.phase_bins, flags=flags)


class _Sequence:
    """K rolling renders of one handle with device buffers (torch), then a flush."""

    def __init__(self, g, lp, seeds, offsets=None, extra_flags=0, records=True):
        import torch
        self.torch = torch
        self.g, self.lp, self.seeds = g, lp, list(seeds)
        K, n = len(self.seeds), g.channels(lp)
        self.hist = torch.zeros((K, n), dtype=torch.float32, device="cuda")
        self.rec = torch.zeros((K, int(lp.n_paths), 4), dtype=torch.int32, device="cuda") if records else None
        self.offsets = list(offsets) if offsets is not None else [0] * K
        self.flags = capi.BF_FLAG_ROLLING | extra_flags

    def issue(self, ks=None, stream=0):
        for k in (range(len(self.seeds)) if ks is None else ks):
            l = _launch_like(self.lp, self.seeds[k], flags=self.flags | self.lp.flags, path_offset=self.offsets[k])
            self.g.render_device(l, self.hist[k].data_ptr(), stream=stream,
                                 records_ptr=self.rec[k].data_ptr() if self.rec is not None else None)

    def results(self):
        self.torch.cuda.synchronize()
        h = self.hist.cpu().numpy()
        r = self.rec.cpu().numpy().view(np.uint32).reshape(len(self.seeds), -1, 4) if self.rec is not None else None
        recs = None
        if r is not None:
            recs = [np.ascontiguousarray(r[k]).view(capi.PATH_RECORD_DTYPE).reshape(-1) for k in range(len(self.seeds))]
        return h, recs
