"""Host model of the persistent solver's LDS window planner (fembrain_amd/csrc/pcg_pipe_mirror.h; fb_plan_mirror_model runs the functions
k_pipe_mirror_plan runs on the device) on the 56^3 cube of the headline run, against a numpy count over the same SELL layout."""
import ctypes as C

import numpy as np

from fembrain_amd import lib as fl
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube


def _plan(n):
    L = fl.lib()
    v, t = truth_cube(n, n, n, 0.1)
    fixed = np.ascontiguousarray(fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n)), np.int32)
    tt = np.ascontiguousarray(t, np.int32).reshape(-1)
    h = C.c_void_p()
    fl.check(L.fb_plan_create(C.byref(h), len(v), len(t), fl.iptr(tt), len(fixed), fl.iptr(fixed), 1, 0, None))
    info = np.zeros(12, np.int32)
    L.fb_plan_info(h, fl.iptr(info))

    def get(name):
        cnt = L.fb_plan_get(h, name.encode(), None, 0)
        a = np.zeros(cnt, np.int32)
        assert L.fb_plan_get(h, name.encode(), fl.iptr(a), cnt) == cnt
        return a
    return L, h, int(info[0]), get("slice_off"), get("colidx").reshape(-1, 64)


def _equal_deal(n_slices, nb=256):
    """pipe_slices (pcg_pipe.hip.h): XCD b & 7 keeps its contiguous eighth, shared by its nb / 8 workgroups"""
    out = []
    chunk, per = (n_slices + 7) >> 3, nb >> 3
    for b in range(nb):
        lo = (b & 7) * chunk
        ln = min(max(n_slices - lo, 0), chunk)
        base, rem = divmod(ln, per)
        j = b >> 3
        out.append((lo + j * base + min(j, rem), base + (1 if j < rem else 0)))
    return out


def test_lds_window_model_on_the_headline_cube():
    n = 56
    L, h, n_owned, so, col = _plan(n)
    n_slices = len(so) - 1
    deal = _equal_deal(n_slices)
    assert max(c for _, c in deal) == 11
    # numpy: per slice, the slot layers whose columns are a lower row of the same workgroup in at least 56 of 64 lanes
    lower_layers = np.zeros(n_slices, np.int64)
    for first, count in deal:
        lo, hi = first * 64, min((first + count) * 64, n_owned)
        for sl in range(first, first + count):
            rows = sl * 64 + np.arange(64)
            c = col[so[sl]:so[sl + 1]]
            ok = (rows[None, :] < hi) & (c >= lo) & (c < rows[None, :])
            lower_layers[sl] = int((ok.sum(1) >= 56).sum())
    assert lower_layers.mean() >= 2.5
    for c16 in (1, 0):
        out = np.zeros(4, np.int32)
        fl.check(L.fb_plan_mirror_model(h, 256, c16, 6, fl.iptr(out)))
        layers, pool, plain, wgs = out.tolist()
        assert layers <= lower_layers.sum()                 # a mirror layer is one of those (the contiguous run below the diagonal)
        assert layers / n_slices >= (2.5 if c16 else 2.0), (c16, layers / n_slices)  # (32-bit columns: 62 slots of 2,560 B, less room)
        assert plain >= 5 and wgs >= (250 if c16 else 200), (c16, plain, wgs)  # plain: the share fb_fem_persist_info reports at 11 slices per CU
        assert 0 < pool <= 128 * wgs                        # one or two pool groups per workgroup: the lanes at the edges of the mesh
    L.fb_plan_destroy(h)
