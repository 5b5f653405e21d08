"""fb_fem_cut where the rules that are this project's own decide the result -- the order of the caller's node ids inside an element -- and on
the paths no cube reaches: unstructured meshes, shipped meshes with their own fixed vertices, folded blades, blades that touch nodes, the
volume refusals, every kind of handle, CARRY under an active node order, and both re-sync paths.  Every cut: the device's delta equal to the
restatement (tests/cutref.py) bit for bit, the mesh read back equal to the delta applied, then the independent checker (tests/cutchecks.py)
on what the device returned.  Inputs: tests/cut_inputs.py (the same ones tests/test_fem_cut_checks.py runs without a GPU)."""
import ctypes as C

import numpy as np
import pytest

import cut_inputs as ci
import cutchecks as cc
import cutref as cr
from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator
from fembrain_amd.meshgen import apply_delta, cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube
from test_fem_cut_gpu import _same_delta

pytestmark = pytest.mark.gpu

OFF, ON, AUTO = fl.FB_RENUMBER_OFF, fl.FB_RENUMBER_ON, fl.FB_RENUMBER_AUTO
MERGED, REBUILT = fl.FB_RESYNC_DELTA_MERGED, fl.FB_RESYNC_DELTA_REBUILT
STATUS = {0: fl.FB_CUT_NOTHING, 1: fl.FB_CUT_DONE, 2: fl.FB_CUT_UNHANDLED}
LOAD = -300.0


def _load(handles, steps=1, value=LOAD):
    for _ in range(steps):
        for h in handles:
            h.set_uniform_force(1, value)
            h.do_timestep()
            assert h.last.converged == 1


def _cut(g, strip, mode="bake", plane=None, exact=True, components=None):
    """one cut of g against the restatement at the state g reports, and the checker on the device's delta.  Returns (info, delta, coverage,
    (rest, tets, q, qvel, qacc) before the cut)."""
    x0, t0 = g.read_mesh()
    q, qv, qa = g.get_q_state()
    e = cr.cut(x0, t0, strip, q, mode)
    info, d = g.cut(strip, mode=mode)
    assert info["status"] == STATUS[e["status"]]
    assert (info["n_quads"], info["n_case_a"], info["n_case_b"], info["n_unhandled"]) == (e["n_quads"], e["n_case_a"], e["n_case_b"], e["n_unhandled"])
    before = (x0, t0, q, qv, qa)
    if e["status"] != 1:
        assert info["n_added"] == info["n_removed"] == info["n_new_nodes"] == 0 and g.num_tets() == len(t0)
        return info, d, set(), before
    assert (info["n_cut_edges"], info["n_removed"], info["n_added"], info["n_new_nodes"]) == (e["n_cut_edges"], len(e["removed"]), len(e["added"]), len(e["new_xyz"]))
    _same_delta(d, e)
    assert info["min_volume_ratio"] == pytest.approx(e["min_volume_ratio"], rel=1e-9)
    pos = x0 + q.reshape(-1, 3)
    x2, t2 = g.read_mesh()
    xe, te = apply_delta(pos if mode == "bake" else x0, t0, d)
    assert np.array_equal(t2, te) and np.array_equal(x2, xe)
    cov = cc.check_cut(pos, t0, d, strip=strip if (plane is not None and exact) else None, plane=plane, rest=x0 if mode == "carry" else None,
                       components=components)
    return info, d, cov, before


def _steps_match(g, ref, bitwise, steps=3, value=LOAD):
    _load((g, ref), steps, value)
    a, b = g.get_q_state(), ref.get_q_state()
    for x, y in zip(a[:2], b[:2]):
        if bitwise:
            assert np.array_equal(x, y)
        else:
            assert np.abs(x - y).max() <= 1e-9 * np.abs(y).max()
    assert np.abs(b[0]).max() > 0


def _twin(g, fixed, **kw):
    x2, t2 = g.read_mesh()
    return FemIntegrator(x2, t2, fixed, **kw)


# ---- Delaunay meshes: every (code, id order) pair, both renumber modes, at rest and deformed ----
def test_delaunay_cuts_reach_every_code_and_id_order(gpu):
    cov, paths = set(), set()
    for n, seed, pseed, k in ci.DELAUNAY_CASES:
        v, t, fixed = ci.delaunay(n, seed)
        for renumber in (OFF, ON):
            for deformed in (False, True):
                for p, nrm, s in ci.random_planes(pseed, k):
                    g = FemIntegrator(v, t, fixed, renumber=renumber)
                    assert g.renumbering()[0] == (renumber == ON)
                    if deformed:
                        _load((g,), 2)
                    info, d, c, _ = _cut(g, s, plane=(p, nrm), components=2)
                    assert info["status"] == fl.FB_CUT_DONE
                    assert not any(np.any(x) for x in g.get_q_state())
                    cov |= c
                    paths.add((renumber, g.resync_path()))
                    g.close()
    assert len(cov) == cc.ALL_PAIRS == 168
    # a BAKE cut took both re-sync paths: merged into the caller's order, rebuilt for a fresh order (the cut adds more than 2 % nodes)
    assert paths == {(OFF, MERGED), (ON, REBUILT)}


@pytest.mark.parametrize("renumber", [OFF, ON])
def test_delaunay_bake_then_steps_match_a_handle_built_from_the_cut_mesh(gpu, renumber):
    v, t, fixed = ci.delaunay(400, 7)
    p, nrm, s = ci.random_planes(12, 2)[0]
    g = FemIntegrator(v, t, fixed, renumber=renumber)
    _load((g,), 1)
    info, *_ = _cut(g, s, plane=(p, nrm), components=2)
    assert info["status"] == fl.FB_CUT_DONE and g.resync_path() == (MERGED if renumber == OFF else REBUILT)
    ref = _twin(g, fixed, renumber=renumber)
    _steps_match(g, ref, renumber == OFF)
    g.close(); ref.close()


@pytest.mark.parametrize("prec", [fl.FB_MATRIX_F64, fl.FB_MATRIX_F32])
def test_system_after_the_cut_is_the_oracles_on_the_cut_mesh(gpu, prec):
    from test_fem_params_gpu import _check_system
    import fem_params as fp
    v, t, fixed = ci.delaunay(400, 7)
    p, nrm, s = ci.random_planes(12, 2)[1]
    g = FemIntegrator(v, t, fixed, matrix_precision=prec, **fp.handle("default"))
    _load((g,), 1)
    info, *_ = _cut(g, s, plane=(p, nrm), components=2)
    assert info["status"] == fl.FB_CUT_DONE
    x2, t2 = g.read_mesh()
    _check_system(g, x2, t2, fixed, "default", prec)
    g.close()


# ---- shipped meshes with their own fixed vertices ----
@pytest.mark.parametrize("name", ci.SHIPPED)
def test_shipped_meshes(gpu, name):
    from test_fem_cut_checks import _bodies_cut
    v, t, fixed = ci.shipped(name)
    before = len(np.unique(cr.face_components(t)))
    for i, (p, nrm, s) in enumerate(ci.shipped_planes(name, v)):
        # (the iteration cap: the oracle needs 2,249 iterations for a step of the uncut disc and 14,115 on this cut one, 4,000-5,000 on the cut
        # peanut and dumbels -- thin bodies and slivers down to 1e-11 of their parents, a property of these inputs)
        g = FemIntegrator(v, t, fixed, cg_max_iter=50000)
        info, d, _, _ = _cut(g, s, plane=(p, nrm), components=before + _bodies_cut(v, t, (p, nrm)))
        assert info["status"] == fl.FB_CUT_DONE
        # the handle keeps its fixed vertices and steps (not implicit_sphere: its unwelded cells cut down to 3.8e-12 of a parent keep the
        # oracle's PCG from converging in 200,000 iterations)
        if i == 0 and name != "implicit_sphere":
            g.set_uniform_force(1, -10.0)
            g.do_timestep()
            q = g.get_q_state()[0]
            assert g.last.converged == 1 and not np.any(q[fixed]) and np.any(q) and np.isfinite(q).all()
        g.close()


# ---- folded strips ----
def test_folded_strips_and_the_narrow_v(gpu):
    v, t, fixed = ci.delaunay(*ci.FOLD_MESH)
    done = 0
    strips = [ci.folded_strip(nq, fold, seed) for nq, fold, seed in ci.FOLDED_CASES] + [ci.v_strip(a) for a in ci.V_CASES]
    for k, s in enumerate(strips):
        g = FemIntegrator(v, t, fixed, renumber=ON if k % 2 else OFF)
        info, *_ = _cut(g, s)                      # (partition, conformity and the combinatorial side rule; no plane to take sides of)
        if k < len(ci.FOLDED_CASES):
            done += info["status"] == fl.FB_CUT_DONE
        else:
            assert info["status"] == fl.FB_CUT_DONE
        g.close()
    assert done >= 8


def test_a_blade_that_ends_inside_the_body_changes_nothing(gpu):
    v, t, fixed = ci.delaunay(*ci.FOLD_MESH)
    g, twin = FemIntegrator(v, t, fixed), FemIntegrator(v, t, fixed)
    _load((g, twin), 1)
    info, d, _, (x0, t0, q, qv, qa) = _cut(g, ci.ending_blade())
    assert info["status"] == fl.FB_CUT_UNHANDLED
    e = cr.cut(x0, t0, ci.ending_blade(), q)
    assert np.array_equal(d["unhandled_ids"], e["unhandled_ids"]) and np.array_equal(d["unhandled_codes"], e["codes"][e["unhandled_ids"]])
    x1, t1 = g.read_mesh()
    assert np.array_equal(x1, x0) and np.array_equal(t1, t0)
    _steps_match(g, twin, True, steps=2)
    g.close(); twin.close()


# ---- blades that touch nodes ----
@pytest.mark.parametrize("normal,n_unhandled", ci.TOUCHING_NORMALS)
def test_node_touching_blades(gpu, normal, n_unhandled):
    v, t = truth_cube(7, 7, 7, 0.1)
    fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(7, 7))
    g, twin = FemIntegrator(v, t, fixed), FemIntegrator(v, t, fixed)
    s = ci.touching_blade(v, normal)
    info, d, _, (x0, t0, q, _, _) = _cut(g, s)
    e = cr.cut(v, t, s)
    assert info["status"] == fl.FB_CUT_UNHANDLED and info["n_unhandled"] == n_unhandled == e["n_unhandled"]
    ids = np.nonzero((e["codes"] > 0) & ~np.isin(e["codes"], list(cr.CASE_A) + list(cr.CASE_B)))[0]
    assert len(d["unhandled_ids"]) == min(64, n_unhandled)       # the read-back's cap
    assert np.array_equal(d["unhandled_ids"], ids[:64]) and np.array_equal(d["unhandled_codes"], e["codes"][ids[:64]])
    x1, t1 = g.read_mesh()
    assert g.num_tets() == len(t) and np.array_equal(x1, v) and np.array_equal(t1, t) and not any(np.any(x) for x in g.get_q_state())
    _steps_match(g, twin, True, steps=2, value=-3000.0)
    g.close(); twin.close()


# ---- the volume refusals ----
def _raw_cut(g, strip, modify):
    res = fl.CutResult()
    pts = np.ascontiguousarray(strip, np.float64).reshape(-1)
    return fl.lib().fb_fem_cut(g.h, len(pts) // 3, fl.dptr(pts), fl.FB_CUT_BAKE, modify, C.byref(res)), res


TWO_TETS = (np.vstack([ci.UNIT_TET, [[1.0, 1.0, 1.0]]]), np.array([[0, 1, 2, 3], [1, 2, 3, 4]], np.int32))


@pytest.mark.parametrize("mesh", ["one", "two"])
@pytest.mark.parametrize("point", [(1.0, 0.0, 0.0), (0.0, 0.0, 0.0)])
def test_a_piece_without_volume_is_refused_before_anything_changes(gpu, mesh, point):
    v, t = (ci.UNIT_TET, np.array([[0, 1, 2, 3]], np.int32)) if mesh == "one" else TWO_TETS
    s = cr.plane_strip(point, (1, 0, 0), half=5.0)
    e = cr.cut(v, t, s)
    assert e["status"] == 1 and e["min_volume_ratio"] == 0.0
    g, twin = (FemIntegrator(v, t, renumber=OFF, cg_max_iter=200) for _ in range(2))
    rc, res = _raw_cut(g, s, 0)
    assert rc == fl.FB_OK and res.status == fl.FB_CUT_DRY and res.min_volume_ratio == 0.0 and res.n_added == len(e["added"])
    rc, res = _raw_cut(g, s, 1)
    assert rc == fl.FB_EINVAL
    x1, t1 = g.read_mesh()
    assert np.array_equal(x1, v) and np.array_equal(t1, t) and g.num_tets() == len(t)
    _steps_match(g, twin, True, steps=2, value=-10.0)
    g.close(); twin.close()


def test_a_piece_the_fp32_records_cannot_hold_is_refused_before_anything_changes(gpu):
    """the plane with normal (1, 1, 1) through node 0 of the unit tet: split fractions 4.9e-16, the piece at node 0 is 1.2e-46 of its parent,
    2e-47 in volume -- not zero, so k_tet_rest would take it, but zero as a float: refused (FB_EINVAL), the dry run still reports it"""
    v, t = ci.UNIT_TET, np.array([[0, 1, 2, 3]], np.int32)
    s = cr.plane_strip((0.0, 0.0, 0.0), (1, 1, 1), half=5.0)
    e = cr.cut(v, t, s)
    assert e["status"] == 1 and 0 < e["min_volume_ratio"] < 1e-45
    g, twin = (FemIntegrator(v, t, renumber=OFF, cg_max_iter=200) for _ in range(2))
    rc, res = _raw_cut(g, s, 0)
    assert rc == fl.FB_OK and res.status == fl.FB_CUT_DRY and res.min_volume_ratio == pytest.approx(e["min_volume_ratio"], rel=1e-9)
    rc, res = _raw_cut(g, s, 1)
    assert rc == fl.FB_EINVAL and b"fp32" in fl.lib().fb_last_error()
    x1, t1 = g.read_mesh()
    assert np.array_equal(x1, v) and np.array_equal(t1, t)
    _steps_match(g, twin, True, steps=2, value=-10.0)
    g.close(); twin.close()


@pytest.mark.parametrize("x", [1e-5, 1 - 1e-5])
def test_thin_pieces_the_records_hold_give_the_handle_of_the_cut_mesh(gpu, x):
    """ratios 1e-5 and 1e-15: the cut is made, and the handle is the handle of the cut mesh -- whatever a handle built from the read-back
    mesh does with a step (the oracle's PCG needs more than 10,000 iterations for the first step of the second one), this one does"""
    v, t = ci.UNIT_TET, np.array([[0, 1, 2, 3]], np.int32)
    p, nrm = np.array([x, 0.0, 0.0]), np.array([1.0, 0.0, 0.0])
    g = FemIntegrator(v, t, renumber=OFF, cg_max_iter=200)
    info, *_ = _cut(g, cr.plane_strip(p, nrm, half=5.0), plane=(p, nrm), components=2)
    assert info["status"] == fl.FB_CUT_DONE
    ref = _twin(g, (), renumber=OFF, cg_max_iter=200)
    L = fl.lib()
    for _ in range(2):
        rcs = []
        for h in (g, ref):
            h.set_uniform_force(1, -10.0)
            rcs.append(L.fb_fem_step(h.h, C.byref(h.last)))
        assert rcs[0] == rcs[1] and rcs[0] in (fl.FB_OK, fl.FB_ESOLVER)
        a, b = g.get_q_state(), ref.get_q_state()
        assert all(np.array_equal(m, n) and np.isfinite(m).all() for m, n in zip(a, b))
    g.close(); ref.close()


# ---- handle kinds ----
KINDS = dict(f64=dict(matrix_precision=fl.FB_MATRIX_F64), f32=dict(matrix_precision=fl.FB_MATRIX_F32), exact_tangent=dict(exact_tangent=True),
             linear=dict(linear=True), expect_cuts=dict(expect_cuts=True), newmark=dict(integrator=fl.FB_INTEGRATOR_NEWMARK))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_handle_kinds_bake(gpu, kind):
    v, t, fixed = ci.delaunay(400, 7)
    p, nrm, s = ci.random_planes(21, 1)[0]
    g = FemIntegrator(v, t, fixed, renumber=OFF, **KINDS[kind])
    _load((g,), 1)
    info, *_ = _cut(g, s, plane=(p, nrm), components=2)
    assert info["status"] == fl.FB_CUT_DONE and g.resync_path() == MERGED
    assert not any(np.any(x) for x in g.get_q_state())       # q, qvel and qaccel (Newmark) start again from zero
    ref = _twin(g, fixed, renumber=OFF, **KINDS[kind])
    _steps_match(g, ref, True)
    if kind == "newmark":
        assert np.array_equal(g.get_q_state()[2], ref.get_q_state()[2]) and np.any(g.get_q_state()[2])
    g.close(); ref.close()


def _carried(before, after, d):
    """CARRY: old nodes keep their values, new ones get lo + f (hi - lo), bit for bit"""
    N = len(before) // 3
    assert np.array_equal(after[:3 * N], before)
    a3 = before.reshape(-1, 3)
    lo, hi, f = d["edge_nodes"][:, 0], d["edge_nodes"][:, 1], d["edge_frac"]
    assert np.array_equal(after.reshape(-1, 3)[N:], a3[lo] + f[:, None] * (a3[hi] - a3[lo]))


def test_newmark_carry_keeps_q_qvel_and_qaccel(gpu):
    v, t, fixed = ci.delaunay(400, 7)
    p, nrm, s = ci.random_planes(21, 1)[0]
    g = FemIntegrator(v, t, fixed, renumber=OFF, integrator=fl.FB_INTEGRATOR_NEWMARK)
    _load((g,), 2)
    info, d, _, (x0, t0, q, qv, qa) = _cut(g, s, mode="carry", plane=(p, nrm), components=2)
    assert info["status"] == fl.FB_CUT_DONE and np.any(qa) and np.any(qv)
    after = g.get_q_state()
    for b, a in zip((q, qv, qa), after):
        _carried(b, a, d)
    x2, t2 = g.read_mesh()
    assert np.array_equal(x2[:len(x0)], x0)
    ref = FemIntegrator(x2, t2, fixed, renumber=OFF, integrator=fl.FB_INTEGRATOR_NEWMARK)
    ref.set_q_state(*after)
    _steps_match(g, ref, True)
    assert np.array_equal(g.get_q_state()[2], ref.get_q_state()[2])
    g.close(); ref.close()


def test_from_poly_handle(gpu):
    from fembrain_amd.blobtree import sphere_blob
    from fembrain_amd.poly import GpuPoly
    poly = GpuPoly(sphere_blob())
    xyz, tets = poly.run_tetrahedralizer(0.1)
    fixed = fixed_vertices_to_dofs(np.nonzero(xyz[:, 1] < xyz[:, 1].min() + 0.15)[0].astype(np.int32))
    g = FemIntegrator.from_poly(poly, fixed)
    p, nrm = np.array([0.013, 0.021, -0.017]), np.array([0.8, 0.1, 0.59])
    info, *_ = _cut(g, cr.plane_strip(p, nrm, half=5.0), plane=(p, nrm))
    assert info["status"] == fl.FB_CUT_DONE
    ref = _twin(g, fixed)
    _steps_match(g, ref, g.resync_path() == MERGED and not g.renumbering()[0], value=-10.0)
    g.close(); ref.close(); poly.close()


def test_persistent_solver_before_and_after_the_cut(gpu):
    n = 20
    v, t = truth_cube(n, n, n, 0.1)
    fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))
    g = FemIntegrator(v, t, fixed, pcg_variant=fl.FB_PCG_PERSISTENT)
    _load((g,), 1, -3000.0)
    assert g.pcg_path()["path"] == fl.FB_PCG_PATH_PERSISTENT
    p, nrm = v.mean(0) + [0.013, 0.021, -0.017], np.array([0.8, 0.1, 0.59])
    info, *_ = _cut(g, cr.plane_strip(p, nrm, half=10.0), plane=(p, nrm), components=2)
    assert info["status"] == fl.FB_CUT_DONE
    ref = _twin(g, fixed, pcg_variant=fl.FB_PCG_PERSISTENT)
    _steps_match(g, ref, False, value=-3000.0)
    for h in (g, ref):
        path = h.pcg_path()
        assert path["path"] == fl.FB_PCG_PATH_PERSISTENT and path["fallbacks"] == 0, path
    g.close(); ref.close()


# ---- CARRY under an active node order: both gathers, merged and across a fresh order ----
@pytest.mark.parametrize("path", [MERGED, REBUILT])
def test_carry_with_an_active_node_order(gpu, monkeypatch, path):
    if path == MERGED:
        monkeypatch.setenv("FEMBRAIN_FRESH_ORDER_PERCENT", "1000")   # (read at every call: the order is kept however many nodes come)
    else:
        monkeypatch.delenv("FEMBRAIN_FRESH_ORDER_PERCENT", raising=False)  # the default: 2 % more nodes and the order is replaced inside the cut
    v, t, fixed = ci.delaunay(1500, 5)
    p, nrm, s = ci.random_planes(11, 4)[2]
    # (cg_eps 1e-10 on both handles: the merged order and the twin's fresh one sum in different orders, and two solves stopped at the
    # default 1e-6 agree only that far)
    g = FemIntegrator(v, t, fixed, renumber=ON, cg_eps=1e-10)
    assert g.renumbering()[0]
    _load((g,), 2)
    info, d, _, (x0, t0, q, qv, _) = _cut(g, s, mode="carry", plane=(p, nrm), components=2)
    assert info["status"] == fl.FB_CUT_DONE and g.resync_path() == path and g.renumbering()[0]
    assert info["n_new_nodes"] * 100 > 2 * len(v)
    after = g.get_q_state()
    _carried(q, after[0], d)
    _carried(qv, after[1], d)
    x2, t2 = g.read_mesh()
    assert np.array_equal(x2[:len(x0)], x0)
    ref = FemIntegrator(x2, t2, fixed, renumber=ON, cg_eps=1e-10)
    ref.set_q_state(after[0], after[1])
    _steps_match(g, ref, False)
    g.close(); ref.close()


# ---- state and forces across a BAKE cut ----
@pytest.mark.parametrize("renumber,path", [(OFF, MERGED), (ON, REBUILT)])
def test_a_cut_clears_state_and_external_forces_on_both_paths(gpu, renumber, path):
    """the contract (include/fembrain_hip.h at fb_fem_cut): after a BAKE cut q, qvel (and qaccel) are zero, and in either mode the external
    forces are zero until they are set again -- on the merged and on the rebuilt path alike"""
    v, t, fixed = ci.delaunay(400, 7)
    p, nrm, s = ci.random_planes(12, 2)[0]
    g = FemIntegrator(v, t, fixed, renumber=renumber)
    f = np.zeros(3 * len(v))
    f[1::3] = LOAD
    g.set_external_forces(f)
    g.do_timestep()
    g.set_external_forces(f)            # ... left standing when the cut comes
    info, *_ = _cut(g, s, plane=(p, nrm), components=2)
    assert info["status"] == fl.FB_CUT_DONE and g.resync_path() == path
    assert not any(np.any(x) for x in g.get_q_state())
    ref = _twin(g, fixed, renumber=renumber)
    # no force call on either: both start from the same velocity field under no load.  A force vector that survived the cut, or new entries
    # read before they are written, would move g away from its twin
    x2, _ = g.read_mesh()
    vel = 0.05 * np.sin(3.0 * x2 + 0.4).reshape(-1)
    vel[fixed] = 0.0
    for h in (g, ref):
        h.set_q_state(np.zeros_like(vel), vel)
        for _ in range(2):
            h.do_timestep()
            assert h.last.converged == 1
    a, b = g.get_q_state()[0], ref.get_q_state()[0]
    assert np.any(b)
    if renumber == OFF:
        assert np.array_equal(a, b)
    else:
        assert np.abs(a - b).max() <= 1e-9 * np.abs(b).max()
    g.close(); ref.close()


# ---- a sequence of cuts ----
def _gravity_steps(handles, steps, acc=-30.0, rho=1000.0):
    """loaded steps under a weight: a force per node in proportion to its lumped mass.  (The same force on every node, as _load gives,
    sends the debris of repeated cuts -- free slivers of 1e-9 of a node's usual mass -- out of the blade's reach within a step or two.)"""
    x, t = handles[0].read_mesh()
    m = np.bincount(t.reshape(-1), weights=np.repeat(np.abs(cc.vol6(x, t)) / 6 * rho / 4, 4), minlength=len(x))
    f = np.zeros(3 * len(x))
    f[1::3] = acc * m
    for _ in range(steps):
        for h in handles:
            h.set_external_forces(f)
            h.do_timestep()
            assert h.last.converged == 1


def test_five_cuts_of_one_body(gpu):
    from test_fem_cut_checks import _bodies_cut
    # (slivers of slivers: the oracle's PCG takes 510, 2,032, 6,396, 55,038, 112,922 and 149,045 iterations for the first step after
    # 0 .. 5 such cuts under a uniform load, with every plane seed tried -- a property of cutting a Delaunay body five times, so the cap is
    # raised and the matrix kept in fp64)
    kw = dict(renumber=OFF, matrix_precision=fl.FB_MATRIX_F64, cg_max_iter=1000000)
    v, t, fixed = ci.delaunay(400, 7)
    g = FemIntegrator(v, t, fixed, **kw)
    parts = 1
    for p, nrm, s in ci.random_planes(31, 5, spread=0.25):
        _gravity_steps((g,), 2)
        x0, t0 = g.read_mesh()
        pos = x0 + g.get_q_state()[0].reshape(-1, 3)
        assert np.abs(pos).max() < 5.0        # everything within the blade's reach (its quad spans +-10)
        parts += _bodies_cut(pos, t0, (p, nrm))
        info, *_ = _cut(g, s, plane=(p, nrm), components=parts)
        assert info["status"] == fl.FB_CUT_DONE
    assert parts >= 6
    ref = _twin(g, fixed, **kw)
    _gravity_steps((g, ref), 2)
    for a, b in zip(g.get_q_state()[:2], ref.get_q_state()[:2]):
        assert np.array_equal(a, b) and np.any(b)
    g.close(); ref.close()
