"""The shared temporary storage of the mesh-side pipelines (PlanWorkspace::temp and its neighbours) grows on a live handle.

A handle made on the smallest cube the builders take starts with every workspace buffer tiny.  Re-synced to a cube 37 times its size it
then builds a surface, cuts, merges a change and picks -- each stage's rocPRIM primitive finds the storage too small and grows it while
the stages before it may still be in flight.  A handle made fresh on the larger cube does the same with storage sized at once.  Every
result is bit for bit the same, with 32-bit sort keys and (FEMBRAIN_PLAN_KEYS64) with 64-bit ones.
"""
import numpy as np
import pytest

import cut_inputs as ci
from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, synthetic_cut, truth_cube
from test_resync_delta_gpu import _cube, _same_bits

pytestmark = pytest.mark.gpu


def _pipeline(g, fixed, strip, delta=None):
    """surface, one cut, one merged change, one box pick, in this order; (results, the change)"""
    out = {}
    s = g.surface()
    out["faces"], out["vertex_ids"], out["face_tets"] = s["faces"], s["vertex_ids"], s["face_tets"]
    out["xyz"], out["normals"], out["aabb"] = g.surface_update()
    info, _ = g.cut(strip)
    assert info["status"] == fl.FB_CUT_DONE and info["n_removed"] > 0 and info["n_new_nodes"] > 0, info
    out["cut_verts"], out["cut_tets"] = g.read_mesh()
    if delta is None:
        _, _, delta = synthetic_cut(g.verts, g.tets, axis=2, where=0.3, every_changed=3)
        assert len(delta["removed"]) and len(delta["changed_ids"]) and len(delta["added"]) and len(delta["new_xyz"])
    g.resync_delta(delta, fixed)
    lo, hi = g.verts.min(0), g.verts.max(0)
    n, ids, xyz = g.pick_box(lo + 0.2 * (hi - lo), lo + 0.7 * (hi - lo))
    assert n == len(ids) > 0
    out["picked"], out["picked_xyz"] = ids, xyz
    return out, delta


@pytest.mark.parametrize("keys64", [False, True])
def test_a_grown_workspace_gives_what_a_fresh_one_gives(gpu, monkeypatch, keys64):
    if keys64:
        monkeypatch.setenv("FEMBRAIN_PLAN_KEYS64", "1")
    v3, t3 = truth_cube(3, 3, 3, 0.1)
    v, t, fixed = _cube(10)
    _, _, strip = ci.random_planes(21, 1, centre=v.mean(0), spread=0.05)[0]
    a = FemIntegrator(v3, t3, fixed_vertices_to_dofs(cube_fixed_plane_i0(3, 3)))
    a.resync(v, t, fixed)
    b = FemIntegrator(v, t, fixed)
    try:
        got, delta = _pipeline(a, fixed, strip)
        want, _ = _pipeline(b, fixed, strip, delta)
        for name in want:
            assert np.array_equal(got[name], want[name]), name
        _same_bits(a, b, load=-300.0)
    finally:
        a.close()
        b.close()
