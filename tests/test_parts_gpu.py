"""fb_fem_parts / fb_fem_split_parts / fb_fem_read_part on the device against tests/partsref.py (itself pinned by test_parts_host.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cutref as cr
import partsref as pr
from fembrain_amd import lib as fl
from fembrain_amd.fem import Deformable, FemIntegrator
from fembrain_amd.meshgen import cube_fixed_plane_i0, delaunay_jittered, fixed_vertices_to_dofs, truth_cube

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = np.zeros(0, np.int32)
EPS = 2.0 ** -52


def _cube(n):
    v, t = truth_cube(n, n, n, 0.1)
    return v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))


def _plane_point(v, frac):
    """the middle of the grid cell at `frac` of the x extent, mid-section"""
    lo, hi = v.min(0), v.max(0)
    xs = np.unique(v[:, 0])
    k = min(max(int(np.searchsorted(xs, lo[0] + frac * (hi[0] - lo[0]))), 1), len(xs) - 1)
    return np.array([0.5 * (xs[k - 1] + xs[k]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])])


def _mid_plane(v, frac=0.47, normal=(1.0, 0.013, 0.007)):
    lo, hi = v.min(0), v.max(0)
    return cr.plane_strip(_plane_point(v, frac), normal, half=4.0 * float((hi - lo).max()))


def _all(g):
    """everything the handle reports, as partsref.parts does"""
    out = dict(g.parts())
    out.update(element_part=g.element_parts(), node_part=g.node_parts())
    out.update(g.part_table())
    return out


def _same(got, ref, volumes=True):
    for k in ("n_parts", "largest_part", "n_shared_nodes", "n_unused_nodes"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k in ("element_part", "node_part", "elements", "nodes", "first_element"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), k
    if volumes:
        err = np.abs(got["volume"] - ref["volume"])
        print("part volumes: largest error / (n eps V) = %g" % float((err / (ref["elements"] * EPS * ref["volume"])).max()))
        assert np.all(err <= ref["elements"] * EPS * ref["volume"])


def _check(g, volumes=True):
    x, t = g.read_mesh()
    ref = pr.parts(x, t)
    got = _all(g)
    _same(got, ref, volumes)
    return got, ref, x, t


X7 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [2, 0.3, 1], [0.2, 2, 1.1]], np.float64)
HAND = {
    "one tet": (X7[:4], [[0, 1, 2, 3]], dict(n_parts=1, largest_part=0, n_shared_nodes=0, n_unused_nodes=0, element_part=[0], node_part=[0, 0, 0, 0],
                                             elements=[1], nodes=[4], first_element=[0])),
    "a face": (X7[:5], [[0, 1, 2, 3], [1, 2, 3, 4]], dict(n_parts=1, largest_part=0, n_shared_nodes=0, n_unused_nodes=0, element_part=[0, 0],
                                                          node_part=[0] * 5, elements=[2], nodes=[5], first_element=[0])),
    "an edge only": (X7[:6], [[0, 1, 2, 3], [0, 1, 4, 5]], dict(n_parts=2, largest_part=0, n_shared_nodes=2, n_unused_nodes=0, element_part=[0, 1],
                                                                node_part=[0, 0, 0, 0, 1, 1], elements=[1, 1], nodes=[4, 4], first_element=[0, 1])),
    "a node only": (X7, [[0, 1, 2, 3], [0, 4, 5, 6]], dict(n_parts=2, largest_part=0, n_shared_nodes=1, n_unused_nodes=0, element_part=[0, 1],
                                                           node_part=[0, 0, 0, 0, 1, 1, 1], elements=[1, 1], nodes=[4, 4], first_element=[0, 1])),
    "three on a face and a loose tet": (np.vstack([X7[:5], [[2, 0, 1], [5, 5, 5], [6, 5, 5], [5, 6, 5], [5, 5, 6]]]), [[6, 7, 8, 9], [0, 1, 2, 3], [0, 1, 2, 4], [0, 1, 2, 5]],
                                        dict(n_parts=2, largest_part=1, n_shared_nodes=0, n_unused_nodes=0, element_part=[0, 1, 1, 1],
                                             node_part=[1] * 6 + [0] * 4, elements=[1, 3], nodes=[4, 6], first_element=[0, 1])),
    "an orphan node": (np.vstack([X7[:5], [[9, 9, 9]]])[[0, 1, 5, 2, 3, 4]], [[0, 1, 3, 4], [1, 3, 4, 5]],
                       dict(n_parts=1, largest_part=0, n_shared_nodes=0, n_unused_nodes=1, element_part=[0, 0], node_part=[0, 0, -1, 0, 0, 0],
                            elements=[2], nodes=[5], first_element=[0])),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_shapes(gpu, name):
    x, t, want = HAND[name]
    g = FemIntegrator(x, np.array(t, np.int32), NONE)
    got = _all(g)
    for k, w in want.items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(w)), (k, got[k], w)
    _same(got, pr.parts(x, t))
    g.close()


def test_cube_whole_and_cut_once(gpu):
    v, t, fixed = _cube(6)
    g = FemIntegrator(v, t, fixed)
    assert len(t) == 750 and g.parts()["n_parts"] == 1
    _check(g)
    assert g.cut(_mid_plane(v))[0]["status"] == fl.FB_CUT_DONE
    got, ref, x, t2 = _check(g)
    assert got["n_parts"] == 2
    total = g.volume()
    assert abs(got["volume"].sum() - total) <= len(t2) * EPS * total
    g.close()


def _cube12_cut_twice(**kw):
    v, t, fixed = _cube(12)
    g = FemIntegrator(v, t, fixed, **kw)
    assert g.cut(_mid_plane(v, 0.47))[0]["status"] == fl.FB_CUT_DONE
    s2 = cr.plane_strip(v.min(0) + (v.max(0) - v.min(0)) * np.array([0.5, 0.53, 0.5]), (0.013, 1.0, 0.021), half=10.0)
    assert g.cut(s2)[0]["status"] == fl.FB_CUT_DONE
    return g


def test_cube_cut_twice_and_every_part_extracted(gpu):
    g = _cube12_cut_twice()
    got, ref, x, t = _check(g)
    assert got["n_parts"] == 4
    total = g.volume()
    assert abs(got["volume"].sum() - total) <= len(t) * EPS * total
    for k in range(4):
        ids, nodes, xyz, tl = g.read_part(k)
        rids, rnodes, rxyz, rtl = pr.extract(x, t, ref["element_part"], k)
        assert np.array_equal(ids, rids) and np.array_equal(nodes, rnodes) and np.array_equal(xyz, rxyz) and np.array_equal(tl, rtl)
    g.close()


def test_long_chain(gpu):
    v, t = truth_cube(200, 2, 2, 0.1)
    g = FemIntegrator(v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(2, 2)))
    assert len(t) == 1194
    got, *_ = _check(g)
    assert got["n_parts"] == 1
    assert g.cut(_mid_plane(v, 0.5))[0]["status"] == fl.FB_CUT_DONE
    got, *_ = _check(g)
    assert got["n_parts"] == 2
    g.close()


@pytest.mark.parametrize("reverse", [False, True])
def test_order_rule_on_interleaved_cubes(gpu, reverse):
    v, t = truth_cube(4, 4, 4, 0.1)
    x = np.vstack([v, v + [5.0, 0.0, 0.0]])
    tt = np.vstack([t, t + len(v)])
    perm = np.random.default_rng(7).permutation(len(tt))
    if reverse:
        perm = perm[::-1]
    tt = np.ascontiguousarray(tt[perm])
    g = FemIntegrator(x, tt, NONE)
    got, ref, *_ = _check(g)
    assert got["n_parts"] == 2 and got["element_part"][0] == 0
    second = int(np.nonzero((perm < len(t)) != (perm[0] < len(t)))[0][0])   # the first element of the other cube
    assert got["first_element"].tolist() == [0, second]
    g.close()


def _loose_tets(n, rng):
    base = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64) * 0.1
    x = (base[None] + (np.arange(n)[:, None, None] * np.array([0.3, 0.0, 0.0])) + rng.uniform(0, 0.01, (n, 4, 3))).reshape(-1, 3)
    return x, np.arange(4 * n, dtype=np.int32).reshape(n, 4)


def test_many_parts(gpu):
    x, t = _loose_tets(5000, np.random.default_rng(3))
    g = FemIntegrator(x, t, NONE)
    got, *_ = _check(g)
    assert got["n_parts"] == 5000 and np.array_equal(got["element_part"], np.arange(5000)) and np.array_equal(got["first_element"], np.arange(5000))
    assert np.all(got["elements"] == 1) and np.all(got["nodes"] == 4)
    g.close()


def test_one_loose_tet_beside_a_long_fan_with_high_node_ids(gpu):
    # 4,999 tets in a chain (each shares a face with the next) on nodes 1000 .., one loose tet on the last four nodes; nodes 0 .. 999 unused
    n = 4999
    rng = np.random.default_rng(5)
    chain = np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2, np.arange(n) + 3], axis=1) + 1000
    t = np.vstack([chain[:2500], [[n + 1003, n + 1004, n + 1005, n + 1006]], chain[2500:]]).astype(np.int32)
    x = rng.uniform(0.0, 1.0, (n + 1007, 3)) + np.arange(n + 1007)[:, None] * [0.5, 0.0, 0.0]
    g = FemIntegrator(x, t, NONE)
    got, *_ = _check(g)
    assert got["n_parts"] == 2 and got["elements"].tolist() == [4999, 1] and got["first_element"].tolist() == [0, 2500]
    assert got["n_unused_nodes"] == 1000 and got["largest_part"] == 0
    g.close()


def test_unstructured_before_and_after_a_cut(gpu):
    v, t, fv = delaunay_jittered(7)
    g = FemIntegrator(v, t, fixed_vertices_to_dofs(fv))
    before, *_ = _check(g)
    strip = cr.plane_strip(0.5 * (v.min(0) + v.max(0)) + 0.0013, (1.0, 0.02, 0.013), half=5.0)
    info, _ = g.cut(strip)
    assert info["status"] == fl.FB_CUT_DONE
    after, *_ = _check(g)
    assert after["n_parts"] > before["n_parts"]
    g.close()


def _cut_cube_arrays(renumber=fl.FB_RENUMBER_AUTO, mesh=None):
    """the arrays of the 9^3 cube cut at mid-span; mesh: that cut mesh handed over instead (a host-built plan cannot cut)"""
    v, t, fixed = _cube(9)
    if mesh is None:
        g = FemIntegrator(v, t, fixed, renumber=renumber)
        assert g.cut(_mid_plane(v))[0]["status"] == fl.FB_CUT_DONE
    else:
        g = FemIntegrator(*mesh, fixed, renumber=renumber)
    out = _all(g)
    out["part1"] = g.read_part(1)
    out["mesh"] = g.read_mesh()
    out["wide"] = int(fl.lib().fb_fem_parts_wide(g.h))
    g.close()
    return out


def _identical(a, b):
    for k in a:
        if k in ("n_builds", "wide"):
            continue
        if k in ("part1", "mesh"):
            assert all(np.array_equal(p, q) for p, q in zip(a[k], b[k]))
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_numbering_wide_keys_and_host_plan_give_identical_arrays(gpu, monkeypatch):
    off = _cut_cube_arrays(fl.FB_RENUMBER_OFF)
    assert off["n_parts"] == 2 and off["wide"] == 0
    _identical(off, _cut_cube_arrays(fl.FB_RENUMBER_ON))
    monkeypatch.setenv("FEMBRAIN_PARTS_WIDE_KEYS", "1")
    for ren in (fl.FB_RENUMBER_OFF, fl.FB_RENUMBER_ON):
        wide = _cut_cube_arrays(ren)
        assert wide["wide"] == 1                 # the two-pass sort really ran
        _identical(off, wide)
    monkeypatch.delenv("FEMBRAIN_PARTS_WIDE_KEYS")
    monkeypatch.setenv("FEMBRAIN_PLAN_DEVICE", "0")
    host = FemIntegrator(*off["mesh"], NONE)
    assert fl.lib().fb_fem_plan_on_device(host.h) == 0
    host.close()
    _identical(off, _cut_cube_arrays(fl.FB_RENUMBER_OFF, mesh=off["mesh"]))


def test_staleness(gpu):
    v, t, fixed = _cube(6)
    g = FemIntegrator(v, t, fixed)
    assert g.element_parts().max() == 0          # read_parts before any parts(): it builds
    assert g.parts()["n_builds"] == 1
    g.set_uniform_force(1, -3000.0)
    g.do_timestep()
    q, qv, _ = g.get_q_state()
    g.set_q_state(q, qv)
    far = cr.plane_strip(v.max(0) + 5.0, (1.0, 0.0, 0.0), half=1.0)
    assert g.cut(far)[0]["status"] == fl.FB_CUT_NOTHING
    assert g.parts()["n_builds"] == 1
    assert g.cut(_mid_plane(v))[0]["status"] == fl.FB_CUT_DONE
    assert g.parts() == dict(g.parts(), n_parts=2, n_builds=2)
    g.split_parts(_mid_plane(v), 0.05)
    assert g.parts()["n_builds"] == 2
    x, t2 = g.read_mesh()
    g.resync(x, t2, fixed)
    assert g.parts()["n_builds"] == 3
    g.resync_delta(dict(removed=np.array([0], np.int32), changed_ids=NONE, changed_nodes=np.zeros((0, 4), np.int32), added=t2[:1], new_xyz=np.zeros((0, 3))), fixed)
    p = g.parts()
    assert p["n_builds"] == 4 and p["n_parts"] == 2
    g.close()


def test_bits_repeat_and_nothing_else_changes(gpu):
    v, t, fixed = _cube(9)
    g, quiet = FemIntegrator(v, t, fixed), FemIntegrator(v, t, fixed)
    for h in (g, quiet):
        assert h.cut(_mid_plane(v))[0]["status"] == fl.FB_CUT_DONE
    s0 = g.surface()
    a = _all(g)
    r0 = g.time_parts(1)                         # (a forced labelling between the two)
    b = _all(g)
    assert b["n_builds"] > a["n_builds"] and all(x > 0 and np.isfinite(x) for x in r0)
    for k in a:
        if k != "n_builds":
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    s1 = g.surface()
    assert all(np.array_equal(s0[k], s1[k]) for k in ("faces", "vertex_ids", "face_tets", "aabb")) and s0["n_builds"] == s1["n_builds"]
    for _ in range(3):
        for h in (g, quiet):
            h.set_uniform_force(1, -3000.0)
            h.do_timestep()
    assert g.get_q_state()[0].tobytes() == quiet.get_q_state()[0].tobytes()
    g.close()
    quiet.close()


def _clamped_beam(renumber=fl.FB_RENUMBER_AUTO):
    v, t = truth_cube(16, 5, 5, 0.1)
    fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(5, 5))
    g = FemIntegrator(v, t, fixed, renumber=renumber)
    point, normal = v.min(0) + (v.max(0) - v.min(0)) * np.array([0.51, 0.5, 0.5]), (1.0, 0.02, 0.013)
    strip = cr.plane_strip(point, normal, half=5.0)
    assert g.cut(strip)[0]["status"] == fl.FB_CUT_DONE
    return g, fixed, strip


def _steps_match(g, fixed, renumber):
    ref = FemIntegrator(*g.read_mesh(), fixed, renumber=renumber)
    for _ in range(3):
        for h in (g, ref):
            h.set_uniform_force(1, -3000.0)
            h.do_timestep()
    qa, qb = g.get_q_state()[0], ref.get_q_state()[0]
    ref.close()
    if renumber == fl.FB_RENUMBER_OFF:
        assert np.array_equal(qa, qb)
    else:
        assert np.abs(qa - qb).max() <= 1e-9 * np.abs(qb).max()


@pytest.mark.parametrize("renumber", [fl.FB_RENUMBER_OFF, fl.FB_RENUMBER_ON])
def test_split_opens_the_cut(gpu, renumber):
    g, fixed, strip = _clamped_beam(renumber)
    x, t = g.read_mesh()
    q = g.get_q_state()[0]
    ref = pr.split(x, q, t, strip, 0.05)
    assert ref["min_distance"] > 1e-6            # no element centroid near the plane
    assert (ref["n_front_parts"], ref["n_back_parts"], ref["n_straddling_parts"]) == (1, 1, 0)
    box0 = g.surface()["aabb"]
    labels = _all(g)
    s = g.split_parts(strip, 0.05)
    for k in ("n_front_parts", "n_back_parts", "n_straddling_parts", "n_nodes_moved"):
        assert s[k] == ref[k], k
    assert np.all(np.abs(s["shift"] - ref["shift"]) <= 4 * np.spacing(np.abs(ref["shift"])))
    x1 = g.read_mesh()[0]
    assert np.array_equal(x1[ref["sign"] > 0], x[ref["sign"] > 0] + s["shift"]) and np.array_equal(x1[ref["sign"] < 0], x[ref["sign"] < 0] - s["shift"])
    assert np.array_equal(x1[ref["sign"] == 0], x[ref["sign"] == 0]) and np.array_equal(np.any(x1 != x, axis=1), ref["moved"])
    assert np.array_equal(g.get_q_state()[0], q)
    if renumber == fl.FB_RENUMBER_ON:            # the node order was derived again from the moved positions, and the handle says so
        assert g.renumbering()[0] and g.resync_path() == fl.FB_RESYNC_DELTA_REBUILT
    after = _all(g)
    assert after["n_builds"] == labels["n_builds"] and np.array_equal(after["element_part"], labels["element_part"])
    _check(g)
    box1 = g.surface()["aabb"]
    gap = np.float32(0.999 * abs(s["shift"][0]))   # (the surface box contains the shift, either way along x)
    assert box1[1, 0] >= box0[1, 0] + gap and box1[0, 0] <= box0[0, 0] - gap
    _steps_match(g, fixed, renumber)
    # a second cut through the moved free part starts from the moved positions
    g.reset_to_rest()
    x2 = g.read_mesh()[0]
    far = x2[:, 0].max()
    strip2 = cr.plane_strip([far - 0.237, x2[:, 1].mean() + 0.003, x2[:, 2].mean() + 0.002], (1.0, 0.017, 0.011), half=5.0)
    exp = cr.cut(x2, g.read_mesh()[1], strip2, g.get_q_state()[0], "bake")
    info, d = g.cut(strip2)
    assert info["status"] == fl.FB_CUT_DONE and np.array_equal(d["new_xyz"], exp["new_xyz"]) and np.array_equal(d["added"], exp["added"])
    assert g.parts()["n_parts"] == 3
    _steps_match(g, fixed, renumber)
    g.close()


def test_split_keeps_a_shared_node_and_leaves_a_straddling_part(gpu):
    x = np.array([[0.5, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [2, 1, 0], [2, 0, 1], [3, 0, 0]], np.float64)
    t = np.array([[0, 1, 2, 3], [0, 4, 5, 6]], np.int32)
    quad = [[0.5, -5, -5], [0.5, 5, -5], [0.5, -5, 5], [0.5, 5, 5]]
    g = FemIntegrator(x, t, NONE)
    s = g.split_parts(quad, 0.25)
    assert (s["n_front_parts"], s["n_back_parts"], s["n_straddling_parts"], s["n_nodes_moved"]) == (1, 1, 0, 6) and s["shift"].tolist() == [0.25, 0.0, 0.0]
    assert np.array_equal(g.read_mesh()[0], pr.split(x, np.zeros_like(x), t, quad, 0.25)["x0"])
    assert np.array_equal(g.read_mesh()[0][0], x[0])
    g.close()
    v, t, fixed = _cube(6)
    g = FemIntegrator(v, t, fixed)
    s = g.split_parts(cr.plane_strip(0.5 * (v.min(0) + v.max(0)) + 0.003, (1.0, 0.02, 0.013), half=5.0), 0.05)
    assert (s["n_front_parts"], s["n_back_parts"], s["n_straddling_parts"], s["n_nodes_moved"]) == (0, 0, 1, 0)
    assert np.array_equal(g.read_mesh()[0], v)
    g.close()


def test_the_free_part_as_a_handle_of_its_own_falls_rigidly(gpu):
    g, fixed, strip = _clamped_beam()
    x, t = g.read_mesh()
    part = g.element_parts()
    free = int(part[np.argmax(x[t].mean(1)[:, 0])])      # the part of the element farthest from the clamp
    ids, nodes, xyz, tl = g.read_part(free)
    rids, rnodes, rxyz, rtl = pr.extract(x, t, part, free)
    assert np.array_equal(ids, rids) and np.array_equal(nodes, rnodes) and np.array_equal(xyz, rxyz) and np.array_equal(tl, rtl)
    assert not np.isin(nodes, cube_fixed_plane_i0(5, 5)).any()
    f = FemIntegrator(xyz, tl, NONE)
    for _ in range(3):
        f.set_uniform_force(1, -3000.0)
        f.do_timestep()
        assert f.last.converged == 1
    dy = f.get_q_state()[0].reshape(-1, 3)[:, 1]
    assert dy.mean() < 0 and dy.std() < 0.05 * abs(dy.mean())
    f.close()
    g.close()


def test_refusals_change_nothing(gpu):
    L = fl.lib()
    v, t, fixed = _cube(6)
    g = FemIntegrator(v, t, fixed)
    assert g.cut(_mid_plane(v))[0]["status"] == fl.FB_CUT_DONE
    before, mesh = _all(g), g.read_mesh()
    quad = _mid_plane(v).reshape(-1).copy()
    info, buf = fl.SplitInfo(), np.zeros(4 * len(mesh[1]), np.int32)
    for k in (-1, 2, 1 << 30):
        assert L.fb_fem_read_part(g.h, k, fl.iptr(buf), None, None, None) == fl.FB_EINVAL
    flat = quad.copy()
    flat[6:9] = flat[0:3] + 2.0 * (flat[3:6] - flat[0:3])        # q2 on the line q0 q1
    nan = quad.copy()
    nan[4] = np.nan
    assert L.fb_fem_split_parts(g.h, fl.dptr(flat), 0.05, C.byref(info)) == fl.FB_EINVAL
    assert L.fb_fem_split_parts(g.h, fl.dptr(nan), 0.05, C.byref(info)) == fl.FB_EINVAL
    assert L.fb_fem_split_parts(g.h, fl.dptr(quad), float("nan"), C.byref(info)) == fl.FB_EINVAL
    assert L.fb_fem_split_parts(g.h, fl.dptr(quad), float("inf"), C.byref(info)) == fl.FB_EINVAL
    assert L.fb_fem_split_parts(g.h, None, 0.05, C.byref(info)) == fl.FB_EINVAL
    pinfo = fl.PartsInfo()
    assert L.fb_fem_parts(None, C.byref(pinfo)) == fl.FB_EINVAL and L.fb_fem_read_parts(None, None, None, None, None, None, None) == fl.FB_EINVAL
    assert L.fb_fem_split_parts(None, fl.dptr(quad), 0.05, C.byref(info)) == fl.FB_EINVAL and L.fb_fem_read_part(None, 0, None, None, None, None) == fl.FB_EINVAL
    assert L.fb_fem_time_parts(None, 1, None, None) == fl.FB_EINVAL and L.fb_fem_time_parts(g.h, 0, None, None) == fl.FB_EINVAL
    after, mesh2 = _all(g), g.read_mesh()
    assert after["n_builds"] == before["n_builds"]
    _identical({k: before[k] for k in before}, after)
    assert np.array_equal(mesh[0], mesh2[0]) and np.array_equal(mesh[1], mesh2[1])
    g.close()


def _shard_child(rank, world, shm_name, q):
    try:
        from test_sharded_gpu import _mesh
        L = fl.lib()
        comm = C.c_void_p()
        fl.check(L.fb_comm_create_local(C.byref(comm), rank, world, shm_name.encode(), 8 << 20, 0))
        v, t, fixed, splits = _mesh(6, world)
        g = FemIntegrator(v, t, fixed, shard=(world, rank, splits, comm))
        quad = _mid_plane(v)
        codes = []
        for call in (g.parts, g.element_parts, lambda: g.split_parts(quad, 0.05, track=False), lambda: g.read_part(0), lambda: g.time_parts(1)):
            try:
                call()
                codes.append(fl.FB_OK)
            except fl.FbError as e:
                codes.append(e.code)
        codes.append(int(L.fb_fem_read_part(g.h, 0, None, None, None, None)))
        g.close()
        L.fb_comm_destroy(comm)
        q.put((rank, codes))
    except Exception as e:
        q.put((rank, repr(e)))
        q.close()
        q.join_thread()
        os._exit(1)


def test_sharded_handle_is_refused(gpu):
    from test_fem_surface_gpu import _run_children
    name = "fbparts%d" % os.getpid()
    got = _run_children(_shard_child, [(r, 2, name) for r in range(2)])
    assert sorted(got) == [(0, [fl.FB_EINVAL] * 6), (1, [fl.FB_EINVAL] * 6)], got


def test_python_deformable_forwards(gpu):
    v, t = truth_cube(16, 5, 5, 0.1)
    d = Deformable(v, t, fixed_vertices=cube_fixed_plane_i0(5, 5), gravity=False)
    assert d.parts()["n_parts"] == 1
    strip = cr.plane_strip(v.min(0) + (v.max(0) - v.min(0)) * np.array([0.51, 0.5, 0.5]), (1.0, 0.02, 0.013), half=5.0)
    assert d.cut(strip)[0]["status"] == fl.FB_CUT_DONE
    assert d.parts()["n_parts"] == 2
    x, tt = d.integrator.read_mesh()
    s = d.split_parts(strip, 0.05)
    ref = pr.split(x, np.zeros_like(x), tt, strip, 0.05)
    assert (s["n_front_parts"], s["n_back_parts"], s["n_nodes_moved"]) == (1, 1, ref["n_nodes_moved"])
    assert np.array_equal(d.integrator.read_mesh()[0], ref["x0"]) and np.array_equal(d.integrator.verts, ref["x0"])
    for k in range(2):
        got, want = d.read_part(k), pr.extract(ref["x0"], tt, d.integrator.element_parts(), k)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    d.timestep()
    d.integrator.close()


def test_timing_entry_point(gpu):
    v, t, fixed = _cube(6)
    g = FemIntegrator(v, t, fixed)
    x0 = g.read_mesh()[0]
    label, split = g.time_parts(3)
    assert np.isfinite(label) and label > 0 and np.isfinite(split) and split > 0
    assert np.array_equal(g.read_mesh()[0], x0)   # the timed split moves nothing
    g.close()


def test_cpp_deformable_parts(gpu, tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "parts_deformable.cpp")
    exe = str(tmp_path / "parts_deformable")
    lib_dir = os.path.join(ROOT, "fembrain_amd")
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src,
           "-L", lib_dir, "-lfembrain_hip", "-Wl,-rpath," + lib_dir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "parts_deformable ok" in r.stdout


def test_split_parts_example(gpu, tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "split_parts.py"), "--out", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "split parts ok" in out.stdout
