"""fb_fem_cut (include/fembrain_hip.h, fembrain_amd/csrc/subdivide.h): CuttableMesh::cut + cutCompleted's re-sync on the device, checked
against the numpy restatement of its rules in tests/cutref.py (cut edges, cases, node ids, pieces), against the reference's own
IntersectSegmentTriangle where its build exists, and against handles built from the cut mesh."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cutref as cr
from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator
from fembrain_amd.meshgen import apply_delta, cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    """a plane across the whole section of a box mesh, in the middle of a grid cell and tilted too little to reach a node plane: it
    passes no node"""
    lo, hi = v.min(0), v.max(0)
    return cr.plane_strip(_plane_point(v, frac), normal, half=4.0 * float((hi - lo).max()))


def _expect(g, strip, mode="bake"):
    x0, t = g.read_mesh()
    q = g.get_q_state()[0]
    return cr.cut(x0, t, strip, q, mode), x0, t, q


def _same_delta(d, e):
    assert np.array_equal(d["removed"], e["removed"])
    assert np.array_equal(d["added"], e["added"])
    assert np.array_equal(d["edge_nodes"], e["edge_nodes"])
    assert np.array_equal(d["new_xyz"], e["new_xyz"])  # bit for bit
    assert np.array_equal(d["edge_frac"], e["edge_frac"])


def _volumes(x, t):
    p = x[t]
    return np.einsum("ij,ij->i", p[:, 1] - p[:, 0], np.cross(p[:, 2] - p[:, 0], p[:, 3] - p[:, 0]))


@pytest.mark.parametrize("code", sorted(set(cr.CASE_A) | set(cr.CASE_B)))
def test_every_case_on_one_tet(gpu, code):
    from test_fem_cut_rules import TET, one_tet_strip
    t = np.array([[0, 1, 2, 3]], np.int32)
    g = FemIntegrator(TET, t, renumber=fl.FB_RENUMBER_OFF)
    strip = one_tet_strip(code)
    e = cr.cut(TET, t, strip)
    info, d = g.cut(strip)
    assert info["status"] == fl.FB_CUT_DONE and info["n_case_a"] + info["n_case_b"] == 1
    assert len(d["added"]) == (4 if code in cr.CASE_A else 6) == info["n_added"]
    _same_delta(d, e)
    x2, t2 = g.read_mesh()
    vols = _volumes(x2, t2)
    parent = _volumes(TET, t)[0]
    assert np.all(np.sign(vols) == np.sign(parent))
    assert abs(vols.sum() - parent) <= 1e-12 * abs(parent)
    for p in t2:
        new = p[p >= 4] - 4
        assert len(set(new // 2)) == len(new)  # never both copies of one cut edge
    assert info["min_volume_ratio"] == pytest.approx(e["min_volume_ratio"], rel=1e-12)
    g.close()


@pytest.mark.parametrize("n", [6, 13, 24])
@pytest.mark.parametrize("deformed", [False, True])
def test_cube_cut_through(gpu, n, deformed):
    v, t, fixed = _cube(n)
    g = FemIntegrator(v, t, fixed)
    if deformed:
        for _ in range(2):
            g.set_uniform_force(1, -3000.0)
            g.do_timestep()
    strip = _mid_plane(v)
    e, x0, t0, q = _expect(g, strip)
    assert e["status"] == 1 and e["n_unhandled"] == 0
    info, d = g.cut(strip)
    assert info["status"] == fl.FB_CUT_DONE
    assert (info["n_case_a"], info["n_case_b"], info["n_cut_edges"]) == (e["n_case_a"], e["n_case_b"], e["n_cut_edges"])
    _same_delta(d, e)
    x2, t2 = g.read_mesh()
    q = q.reshape(-1, 3)
    xe, te = apply_delta(x0 + q, t0, d)
    assert np.array_equal(t2, te) and np.array_equal(x2, xe)
    assert cr.max_face_share(t2) <= 2
    # two sides, no face path across the plane
    roots = cr.face_components(t2)
    assert len(np.unique(roots)) == 2
    side = np.sign((x2[t2].mean(1) - _plane_point(v, 0.47)) @ np.array([1.0, 0.013, 0.007])) if not deformed else None
    if side is not None:
        for r in np.unique(roots):
            assert len(np.unique(side[roots == r])) == 1
    assert abs(_volumes(x2, t2).sum() - _volumes(x0 + q, t0).sum()) <= 1e-12 * abs(_volumes(x0 + q, t0).sum())
    assert not np.any(g.get_q_state()[0])
    g.close()


@pytest.mark.skipif(not __import__("oracle.pycut", fromlist=["have_ref"]).have_ref(), reason="the reference's build is not on this machine")
def test_cut_edges_pinned_to_the_reference_routine(gpu):
    from oracle import pycut
    v, t, fixed = _cube(9)
    g = FemIntegrator(v, t, fixed, renumber=fl.FB_RENUMBER_OFF)
    g.set_uniform_force(1, -3000.0)
    g.do_timestep()
    s = _mid_plane(v, 0.41)
    s2 = _mid_plane(v, 0.63, (1.0, -0.012, 0.009))
    strip = np.concatenate([s, s2[:2], s2[2:], s[:2], s[2:]])  # quads: s, s->s2 (slanted), s2, s2->s (slanted), s (the same edges twice)
    x0, t0 = g.read_mesh()
    q = g.get_q_state()[0]
    e = cr.cut(x0, t0, strip, q)
    info, d = g.cut(strip, modify=False)
    # the reference's IntersectSegmentTriangle on every unique edge lo -> hi and both triangles of every usable quad
    pos = x0 + q.reshape(-1, 3)
    ed = np.unique(np.sort(t0[:, [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]].reshape(-1, 2), axis=1), axis=0)
    odd = np.zeros(len(ed), bool)
    tl = np.zeros(len(ed))
    for qd in cr.usable_quads(strip):
        seg = np.concatenate([pos[ed[:, 0]], pos[ed[:, 1]]], axis=1)
        h1, _, t1 = pycut.ref_segment_triangle_pairs(seg, np.tile(np.concatenate([qd[0], qd[2], qd[1]]), (len(ed), 1)), double=True)
        h2, _, t2 = pycut.ref_segment_triangle_pairs(seg, np.tile(np.concatenate([qd[2], qd[3], qd[1]]), (len(ed), 1)), double=True)
        hit = (h1 > 0) | (h2 > 0)
        odd ^= hit
        tl = np.where(hit, np.where(h1 > 0, t1, t2), tl)
    if info["status"] == fl.FB_CUT_DRY:
        got = d["edge_nodes"][::2]
        assert np.array_equal(got, ed[odd])
        k = np.lexsort((ed[odd][:, 1], ed[odd][:, 0]))
        ln = np.linalg.norm(pos[ed[odd][k][:, 1]] - pos[ed[odd][k][:, 0]], axis=1)
        np.testing.assert_allclose(d["edge_frac"][::2] * ln, tl[odd][k], rtol=1e-15)
    else:  # a pattern the subdivision refuses: the codes still follow the reference's edge set
        assert info["status"] == fl.FB_CUT_UNHANDLED and info["n_unhandled"] == e["n_unhandled"]
    assert e["codes"].any()
    # and the restatement's edge set is the reference's
    key = ed[:, 0].astype(np.int64) * (1 << 32) + ed[:, 1]
    cutm, tt = cr.cut_edges(pos, ed[:, 0], ed[:, 1], cr.usable_quads(strip))
    assert np.array_equal(cutm, odd) and np.array_equal(tt[odd], tl[odd])
    assert len(key) == len(ed)
    g.close()


@pytest.mark.parametrize("renumber", [fl.FB_RENUMBER_OFF, fl.FB_RENUMBER_ON])
def test_bake_cut_then_steps_match_a_handle_built_from_the_cut_mesh(gpu, renumber):
    v, t, fixed = _cube(12)
    g = FemIntegrator(v, t, fixed, renumber=renumber)
    g.set_uniform_force(1, -3000.0)
    g.do_timestep()
    strip = _mid_plane(v, 0.58)
    e, *_ = _expect(g, strip)
    info, d = g.cut(strip)
    assert info["status"] == fl.FB_CUT_DONE
    _same_delta(d, e)
    x2, t2 = g.read_mesh()
    ref = FemIntegrator(x2, t2, fixed, renumber=renumber)
    for _ in range(3):
        for h in (g, ref):
            h.set_uniform_force(1, -3000.0)
            h.do_timestep()
    qa, qb = g.get_q_state()[0], ref.get_q_state()[0]
    if renumber == fl.FB_RENUMBER_OFF:
        assert np.array_equal(qa, qb)
    else:
        assert np.abs(qa - qb).max() <= 1e-9 * np.abs(qb).max()
    g.close()
    ref.close()


def test_renumbered_handle_gives_the_same_delta(gpu):
    v, t, fixed = _cube(13)
    ga = FemIntegrator(v, t, fixed, renumber=fl.FB_RENUMBER_OFF)
    gb = FemIntegrator(v, t, fixed, renumber=fl.FB_RENUMBER_ON)
    strip = _mid_plane(v, 0.52)
    ia, da = ga.cut(strip)
    ib, db = gb.cut(strip)
    assert ia == ib
    _same_delta(da, db)
    xa, ta = ga.read_mesh()
    xb, tb = gb.read_mesh()
    assert np.array_equal(xa, xb) and np.array_equal(ta, tb)
    ga.close()
    gb.close()


def test_carry_keeps_rest_shape_and_state(gpu):
    v, t, fixed = _cube(10)
    g = FemIntegrator(v, t, fixed)
    g.set_uniform_force(1, -3000.0)
    g.do_timestep()
    q, qv, qa = g.get_q_state()
    x0, t0 = g.read_mesh()
    strip = _mid_plane(v, 0.55)
    e = cr.cut(x0, t0, strip, q, mode="carry")
    info, d = g.cut(strip, mode="carry")
    assert info["status"] == fl.FB_CUT_DONE
    _same_delta(d, e)
    x2, _ = g.read_mesh()
    assert np.array_equal(x2[:len(x0)], x0)
    q2, qv2, _ = g.get_q_state()
    N = len(x0)
    assert np.array_equal(q2[:3 * N], q) and np.array_equal(qv2[:3 * N], qv)
    lo, hi, f = d["edge_nodes"][:, 0], d["edge_nodes"][:, 1], d["edge_frac"]
    for a, b in ((q, q2), (qv, qv2)):
        a3 = a.reshape(-1, 3)
        want = a3[lo] + f[:, None] * (a3[hi] - a3[lo])
        assert np.array_equal(b.reshape(-1, 3)[N:], want)
    g.set_uniform_force(1, -3000.0)
    g.do_timestep()
    assert g.last.converged == 1
    g.close()


def test_refusals_change_nothing(gpu):
    v, t, fixed = _cube(10)
    g = FemIntegrator(v, t, fixed)
    twin = FemIntegrator(v, t, fixed)
    for h in (g, twin):
        h.set_uniform_force(1, -3000.0)
        h.do_timestep()
    nt = g.num_tets()
    # a blade that stops inside the mesh: cells with one or two edges cut
    lo, hi = v.min(0), v.max(0)
    p = lo + (hi - lo) * np.array([0.47, 0.5, 0.5])
    half = 0.3 * float((hi - lo).max())
    n = np.array([1.0, 0.023, 0.011])
    strip = cr.plane_strip(p, n, half=half)
    info, d = g.cut(strip)
    assert info["status"] == fl.FB_CUT_UNHANDLED and info["n_unhandled"] > 0 and info["n_added"] == 0
    x0, t0 = g.read_mesh()
    e = cr.cut(x0, t0, strip, g.get_q_state()[0])
    assert e["n_unhandled"] == info["n_unhandled"]
    assert np.array_equal(d["unhandled_ids"], e["unhandled_ids"][:len(d["unhandled_ids"])])
    assert np.array_equal(d["unhandled_codes"], e["codes"][d["unhandled_ids"]])
    assert g.num_tets() == nt
    assert np.array_equal(g.get_q_state()[0], twin.get_q_state()[0])
    # outside the mesh
    info, _ = g.cut(cr.plane_strip(hi + 5.0, n, half=0.5))
    assert info["status"] == fl.FB_CUT_NOTHING and info["n_quads"] == 1
    # degenerate quads only: skipped, nothing cut
    info, _ = g.cut(np.repeat(p[None, :], 4, axis=0))
    assert info["status"] == fl.FB_CUT_NOTHING and info["n_quads"] == 0
    # a dry run: the real cut's delta, nothing changed
    full = _mid_plane(v)
    info, d = g.cut(full, modify=False)
    assert info["status"] == fl.FB_CUT_DRY and g.num_tets() == nt
    for h in (g, twin):
        h.set_uniform_force(1, -3000.0)
        h.do_timestep()
    assert np.array_equal(g.get_q_state()[0], twin.get_q_state()[0])
    e, *_ = _expect(g, full)
    # (the state moved on a step since the dry run: compare with a dry run of the twin at the same state)
    info_t, d_t = twin.cut(full, modify=False)
    info_r, d_r = g.cut(full)
    assert info_r["status"] == fl.FB_CUT_DONE
    _same_delta(d_t, d_r)
    _same_delta(d_r, e)
    # bad arguments
    L = fl.lib()
    res = fl.CutResult()
    three = np.zeros(9)
    assert L.fb_fem_cut(g.h, 3, fl.dptr(three), fl.FB_CUT_BAKE, 1, res) == fl.FB_EINVAL
    five = np.zeros(15)
    assert L.fb_fem_cut(g.h, 5, fl.dptr(five), fl.FB_CUT_BAKE, 1, res) == fl.FB_EINVAL
    assert L.fb_fem_cut(g.h, 4, fl.dptr(full.reshape(-1)), 7, 1, res) == fl.FB_EINVAL
    assert L.fb_fem_cut(None, 4, fl.dptr(full.reshape(-1)), fl.FB_CUT_BAKE, 1, res) == fl.FB_EINVAL
    g.close()
    twin.close()


def test_host_built_plan_is_refused(gpu, monkeypatch):
    # (one check refuses sharded handles and handles whose plan was built on the host: fb_fem_resync_delta's rule)
    monkeypatch.setenv("FEMBRAIN_PLAN_DEVICE", "0")
    v, t, fixed = _cube(6)
    g = FemIntegrator(v, t, fixed)
    assert fl.lib().fb_fem_plan_on_device(g.h) == 0
    res = fl.CutResult()
    s = _mid_plane(v).reshape(-1)
    assert fl.lib().fb_fem_cut(g.h, 4, fl.dptr(s), fl.FB_CUT_BAKE, 1, res) == fl.FB_EINVAL
    assert fl.lib().fb_fem_num_tets(g.h) == len(t)
    g.close()


def test_two_successive_cuts_and_expect_cuts(gpu):
    v, t, fixed = _cube(12)
    for expect in (False, True):
        g = FemIntegrator(v, t, fixed, expect_cuts=expect)
        s1 = _mid_plane(v, 0.47)
        e1, *_ = _expect(g, s1)
        info, d = g.cut(s1)
        assert info["status"] == fl.FB_CUT_DONE
        _same_delta(d, e1)
        N1 = fl.lib().fb_fem_num_nodes(g.h)
        # across the pieces of the first cut
        s2 = cr.plane_strip(v.min(0) + (v.max(0) - v.min(0)) * np.array([0.5, 0.53, 0.5]), (0.013, 1.0, 0.021), half=10.0)
        e2, *_ = _expect(g, s2)
        info, d = g.cut(s2)
        assert info["status"] == fl.FB_CUT_DONE and e2["status"] == 1
        _same_delta(d, e2)
        assert d["edge_nodes"].max() < N1 and info["n_new_nodes"] > 0
        x2, t2 = g.read_mesh()
        assert t2.max() == N1 + info["n_new_nodes"] - 1
        assert len(np.unique(cr.face_components(t2))) == 4
        g.set_uniform_force(1, -3000.0)
        g.do_timestep()
        assert g.last.converged == 1
        g.close()


def test_the_cut_off_part_falls_freely(gpu):
    v, t = truth_cube(16, 5, 5, 0.1)
    fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(5, 5))
    g = FemIntegrator(v, t, fixed)
    strip = cr.plane_strip(v.min(0) + (v.max(0) - v.min(0)) * np.array([0.51, 0.5, 0.5]), (1.0, 0.02, 0.013), half=5.0)
    info, _ = g.cut(strip)
    assert info["status"] == fl.FB_CUT_DONE
    x2, t2 = g.read_mesh()
    for _ in range(3):
        g.set_uniform_force(1, -3000.0)
        g.do_timestep()
    q = g.get_q_state()[0].reshape(-1, 3)
    xm = 0.5 * (x2[:, 0].min() + x2[:, 0].max())
    free = x2[:, 0] > xm + 0.05
    held = x2[:, 0] < xm - 0.05
    dy_free, dy_held = q[free, 1], q[held, 1]
    assert dy_free.mean() < 0
    assert dy_free.std() < 0.05 * abs(dy_free.mean())          # rigid fall: every node of the free part moves alike
    assert dy_held.std() > 0.2 * abs(dy_held.mean())          # the clamped part bends
    g.close()


def test_scalpel_example_on_the_ventricle(gpu):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "scalpel_cut.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "scalpel cut ok" in out.stdout


def test_cpp_deformable_cut(gpu, tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "cut_deformable.cpp")
    exe = str(tmp_path / "cut_deformable")
    lib_dir = os.path.join(ROOT, "fembrain_amd")
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src,
           "-L", lib_dir, "-lfembrain_hip", "-Wl,-rpath," + lib_dir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cut_deformable ok" in r.stdout
