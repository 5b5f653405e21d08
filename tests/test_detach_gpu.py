"""fb_fem_detach_part on the device against the host route it replaces (fb_fem_read_part + fb_fem_create + the setters, with
tests/detachref.py's arrays) and, for FB_DETACH_REMOVE, against fb_fem_resync_delta(removed = the part's elements): bit for bit."""
import ctypes as C

import numpy as np
import pytest

import cutref as cr
import detachref as dr
from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator
from fembrain_amd.meshgen import truth_cube

pytestmark = pytest.mark.gpu

NONE = np.zeros(0, np.int32)
MATS = ([1e7, 3e6], [0.46, 0.40], [1000.0, 1200.0])


def _dofs(nodes):
    return np.sort((3 * np.asarray(nodes, np.int64)[:, None] + np.arange(3)).reshape(-1)).astype(np.int32)


def _beam(permute=False):
    """the 16 x 5 x 5-node beam, both ends clamped; permute: the node ids shuffled"""
    v, t = truth_cube(16, 5, 5, 0.1)
    v, t = np.asarray(v, np.float64).reshape(-1, 3), np.asarray(t, np.int32).reshape(-1, 4)
    assert len(t) == 1440
    if permute:
        p = np.random.default_rng(11).permutation(len(v))   # new id of old node i
        v2 = np.empty_like(v)
        v2[p] = v
        v, t = v2, p[t].astype(np.int32)
    ends = np.nonzero((v[:, 0] == v[:, 0].min()) | (v[:, 0] == v[:, 0].max()))[0]
    return v, t, _dofs(ends)


def _blade(v):
    """the tilted mid-span plane of examples/split_parts.py"""
    nrm = np.array([1.0, 0.02, 0.013])
    nrm /= np.linalg.norm(nrm)
    a = np.cross(nrm, [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(nrm, a)
    p = v.min(0) + (v.max(0) - v.min(0)) * np.array([0.51, 0.5, 0.5])
    return np.array([p - 5 * a - 5 * b, p - 5 * a + 5 * b, p + 5 * a - 5 * b, p + 5 * a + 5 * b])


def _parent(permute=False, materials=True, **kw):
    """loaded, stepped twice, cut with FB_CUT_CARRY, a random external force vector, stepped once.  Returns (handle, fixed, fext)."""
    v, t, fixed = _beam(permute)
    g = FemIntegrator(v, t, fixed, **kw)
    if materials:
        g.set_materials(*MATS, element_ids=np.arange(len(t)) % 2)
    for _ in range(2):
        g.set_uniform_force(1, -3000.0)
        g.do_timestep()
    info, _ = g.cut(_blade(v), mode="carry", track=False)
    assert info["status"] == fl.FB_CUT_DONE, info
    assert g.parts()["n_parts"] == 2
    fext = np.random.default_rng(5).normal(size=3 * int(g._L.fb_fem_num_nodes(g.h))) * 40.0
    g.r = len(fext)
    g.set_external_forces(fext)
    g.do_timestep()
    assert g.last.converged == 1
    return g, fixed, fext


def _snapshot(g):
    x, t = g.read_mesh()
    return dict(x=x, t=t, state=g.get_q_state())


def _same_snapshot(a, b):
    return np.array_equal(a["x"], b["x"]) and np.array_equal(a["t"], b["t"]) and all(np.array_equal(u, w) for u, w in zip(a["state"], b["state"]))


def _twin_the_long_way(g, k, fixed, fext, materials=True, **kw):
    """read_part + fb_fem_create with detachref's fixed list + set_state + the material calls + set_external_forces"""
    ids, nodes, xyz, tl = g.read_part(k)
    q, qv, qa = g.get_q_state()
    ref = dr.detach(ids, nodes, xyz, tl, fixed_dofs=fixed, vectors=dict(q=q, qvel=qv, qaccel=qa, fext=fext),
                    material_ids=g.element_materials() if materials else None)
    twin = FemIntegrator(ref["xyz"], ref["tets"], ref["fixed"], **kw)
    twin.set_q_state(ref["q"], ref["qvel"], ref["qaccel"])
    if materials:
        twin.set_materials(*MATS)
        twin.set_element_materials(ref["materials"])
    twin.set_external_forces(ref["fext"])
    return twin, ref, ids, nodes


def _same_handles(a, b, steps=3):
    """mesh, pattern, constrained DOFs, material ids and state bit for bit; then `steps` steps of both"""
    xa, ta = a.read_mesh()
    xb, tb = b.read_mesh()
    assert np.array_equal(xa, xb) and np.array_equal(ta, tb)
    for u, w in zip(a.pattern(), b.pattern()):
        assert np.array_equal(u, w)
    assert np.array_equal(a.constrained_dofs(), b.constrained_dofs())
    assert np.array_equal(a.element_materials(), b.element_materials())
    for u, w in zip(a.get_q_state(), b.get_q_state()):
        assert np.array_equal(u, w)
    for _ in range(steps):
        assert a.do_timestep() == b.do_timestep()
        qa, va, _ = a.get_q_state()
        qb, vb, _ = b.get_q_state()
        assert np.array_equal(qa, qb) and np.array_equal(va, vb)
    assert np.abs(qa).max() > 0


def _keep_against_the_host_route(monkeypatch, piece_env=None, permute=False, **kw):
    g, fixed, fext = _parent(permute, **kw)
    assert np.array_equal(g.constrained_dofs(), fixed)
    builds = g.parts()["n_builds"]
    if piece_env is not None:
        monkeypatch.setenv("FEMBRAIN_RENUMBER", piece_env)   # (read at every build: the piece and the twin only)
    out = []
    for k in range(2):
        twin, ref, ids, nodes = _twin_the_long_way(g, k, fixed, fext, **kw)
        before = _snapshot(g)
        piece, pids, pnodes = g.detach_part(k)
        assert np.array_equal(pids, ids) and np.array_equal(pnodes, nodes)
        info = piece.detach_info
        assert (info["part"], info["n_elements"], info["n_nodes"], info["n_fixed_dofs"]) == (k, len(ids), len(nodes), len(ref["fixed"]))
        assert info["n_materials"] == 2 and info["parent_resync_path"] == -1 and info["parent_elements_left"] == len(before["t"])
        assert len(ref["fixed"]) > 0 and np.array_equal(piece.constrained_dofs(), ref["fixed"])
        assert set(np.unique(piece.element_materials())) == {0, 1}
        assert piece.renumbering()[0] == twin.renumbering()[0]
        out.append((g.renumbering()[0], piece.renumbering()[0]))
        # the parent is as it was
        assert _same_snapshot(before, _snapshot(g)) and g.parts()["n_builds"] == builds
        _same_handles(piece, twin)
        assert _same_snapshot(before, _snapshot(g))
        piece.close()
        twin.close()
    g.close()
    return out


def test_keep_against_the_host_route(gpu, monkeypatch):
    assert _keep_against_the_host_route(monkeypatch) == [(False, False)] * 2


@pytest.mark.parametrize("piece_env", [None, "0"])
def test_keep_with_the_parent_renumbered(gpu, monkeypatch, piece_env):
    got = _keep_against_the_host_route(monkeypatch, piece_env, permute=True, renumber=fl.FB_RENUMBER_ON)
    assert got == [(True, piece_env is None)] * 2


def test_keep_with_the_piece_renumbered_only(gpu, monkeypatch):
    assert _keep_against_the_host_route(monkeypatch, "1", permute=True, renumber=fl.FB_RENUMBER_OFF) == [(False, True)] * 2


def test_keep_on_a_newmark_handle(gpu, monkeypatch):
    g, fixed, fext = _parent(integrator=fl.FB_INTEGRATOR_NEWMARK)
    assert np.abs(g.get_q_state()[2]).max() > 0
    g.close()
    _keep_against_the_host_route(monkeypatch, integrator=fl.FB_INTEGRATOR_NEWMARK)


@pytest.mark.parametrize("k,renumber,rebuild", [(0, fl.FB_RENUMBER_AUTO, False), (1, fl.FB_RENUMBER_ON, False), (1, fl.FB_RENUMBER_ON, True)])
def test_remove(gpu, monkeypatch, k, renumber, rebuild):
    g, fixed, fext = _parent(renumber=renumber)
    twin, _, _ = _parent(renumber=renumber)
    if rebuild:   # the removal through the full builder: a renumbered parent comes out in a new node order
        monkeypatch.setenv("FEMBRAIN_RESYNC_DELTA", "rebuild")
    before = _snapshot(g)
    table = g.part_table()
    n_parts = g.parts()["n_parts"]
    used_by_others = np.unique(before["t"][g.element_parts() != k])
    ids, nodes, _, _ = g.read_part(k)
    piece, pids, _ = g.detach_part(k, remove=True)
    assert np.array_equal(pids, ids)
    info = piece.detach_info
    assert info["parent_elements_left"] + info["n_elements"] == len(before["t"]) and info["parent_elements_left"] == g.num_tets()
    assert info["parent_resync_path"] == g.resync_path() == (fl.FB_RESYNC_DELTA_REBUILT if rebuild else fl.FB_RESYNC_DELTA_MERGED)
    # the twin parent: the delta re-sync from the host with the same list, the carried vectors set again
    twin.resync_delta(dict(removed=ids), fixed_dofs=fixed, track=False)
    twin.set_q_state(*before["state"])
    twin.set_external_forces(fext)
    assert twin.resync_path() == g.resync_path()
    for u, w in zip(g.get_q_state(), before["state"]):
        assert np.array_equal(u, w)
    after = g.parts()
    assert after["n_parts"] == n_parts - 1
    assert after["n_unused_nodes"] == len(np.setdiff1d(nodes, used_by_others)) > 0
    vol_after = g.part_table()["volume"].sum()
    vol_before = table["volume"].sum()
    print("volume before %.17g, removed %.17g + left %.17g" % (vol_before, table["volume"][k], vol_after))
    assert abs(table["volume"][k] + vol_after - vol_before) <= 1e-12 * vol_before
    assert abs(piece.part_table()["volume"][0] - table["volume"][k]) <= 1e-12 * vol_before
    _same_handles(g, twin)
    for body in (piece,):
        body.do_timestep()
        assert body.last.converged == 1
    for h in (g, twin, piece):
        h.close()


def _cube_cut_twice():
    v, t = truth_cube(6, 6, 6, 0.1)
    v = np.asarray(v, np.float64).reshape(-1, 3)
    fixed = _dofs(np.nonzero(v[:, 0] == v[:, 0].min())[0])
    g = FemIntegrator(v, t, fixed)
    lo, hi = v.min(0), v.max(0)
    s1 = cr.plane_strip(lo + (hi - lo) * np.array([0.47, 0.5, 0.5]), (1.0, 0.013, 0.007), half=4.0)
    s2 = cr.plane_strip(lo + (hi - lo) * np.array([0.5, 0.53, 0.5]), (0.013, 1.0, 0.021), half=4.0)
    for s in (s1, s2):
        assert g.cut(s, track=False)[0]["status"] == fl.FB_CUT_DONE
    assert g.parts()["n_parts"] == 4
    return g


def test_cube_of_four_parts_detached_until_one_is_left(gpu):
    g = _cube_cut_twice()
    total = g.num_tets()
    pieces = []
    for n in (4, 3, 2):
        assert g.parts()["n_parts"] == n
        piece, ids, _ = g.detach_part(n - 1, remove=True)
        assert piece.detach_info["parent_elements_left"] == g.num_tets()
        pieces.append(piece)
    assert g.parts()["n_parts"] == 1
    pieces.append(g.detach_part(0)[0])   # the fourth call: the last part, kept
    assert pieces[-1].num_tets() == g.num_tets()
    for p in pieces:
        assert p.parts()["n_parts"] == 1
    assert sum(p.num_tets() for p in pieces) == total
    before = _snapshot(g)
    with pytest.raises(fl.FbError) as e:   # the fifth: a handle cannot be left without elements
        g.detach_part(0, remove=True)
    assert e.value.code == fl.FB_EINVAL
    assert _same_snapshot(before, _snapshot(g)) and g.parts()["n_parts"] == 1
    for p in pieces + [g]:
        p.do_timestep()
        assert p.last.converged == 1
        p.close()


def test_a_shared_node_goes_to_both_pieces(gpu):
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, -1, -1], [-2, -0.3, -1], [-0.2, -2, -1.1]], np.float64)
    t = np.array([[0, 1, 2, 3], [0, 4, 5, 6]], np.int32)
    fixed = np.array([1, 9, 10, 11, 18], np.int32)   # y of the shared node; node 3; x of node 6
    g = FemIntegrator(x, t, fixed)
    assert g.parts()["n_shared_nodes"] == 1
    rng = np.random.default_rng(2)
    q, qv, fext = rng.normal(size=21) * 1e-3, rng.normal(size=21) * 1e-2, rng.normal(size=21)
    g.set_q_state(q, qv)
    g.set_external_forces(fext)
    for k in range(2):
        ids, nodes, xyz, tl = g.read_part(k)
        ref = dr.detach(ids, nodes, xyz, tl, fixed_dofs=fixed, vectors=dict(q=q, qvel=qv))
        piece, _, pnodes = g.detach_part(k)
        assert pnodes[0] == 0 and np.array_equal(pnodes, nodes)
        pq, pv, _ = piece.get_q_state()
        assert np.array_equal(pq, ref["q"]) and np.array_equal(pv, ref["qvel"])
        assert np.array_equal(pq[:3], q[:3]) and np.array_equal(pv[:3], qv[:3])   # its own copy of node 0, the parent's state on it
        assert np.array_equal(piece.constrained_dofs(), ref["fixed"]) and 1 in piece.constrained_dofs()
        assert piece.detach_info["n_materials"] == 1 and piece.element_map_bytes() == 0
        twin = FemIntegrator(ref["xyz"], ref["tets"], ref["fixed"])
        twin.set_q_state(ref["q"], ref["qvel"])
        twin.set_external_forces(dr.gather_vector(nodes, fext))
        _same_handles(piece, twin, steps=1)
        piece.close()
        twin.close()
    g.close()


def test_a_detached_piece_is_a_full_handle(gpu):
    g, fixed, fext = _parent(expect_cuts=True)
    k = 1 - int(g.element_parts()[0])
    piece, ids, nodes = g.detach_part(k, remove=True)
    x, _ = piece.read_mesh()
    lo, hi = x.min(0), x.max(0)
    info, _ = piece.cut(cr.plane_strip(lo + (hi - lo) * np.array([0.52, 0.5, 0.5]), (1.0, 0.02, 0.013), half=4.0), mode="carry", track=False)
    assert info["status"] == fl.FB_CUT_DONE, info
    assert piece.parts()["n_parts"] == 2
    assert len(piece.surface()["faces"]) > 0
    assert piece.stress()["n_elements"] == piece.num_tets()
    assert piece.volume() > 0
    # ... and its constrained DOFs are the list a delta re-sync of it takes
    piece.r = 3 * int(piece._L.fb_fem_num_nodes(piece.h))
    piece.resync_delta(dict(removed=[0]), fixed_dofs=piece.constrained_dofs(), track=False)
    pf = piece.constrained_dofs()
    assert len(pf) > 3
    piece.set_constrained_dofs(pf[3:])
    assert np.array_equal(piece.constrained_dofs(), pf[3:])
    for body in (piece, g):
        body.do_timestep()
        assert body.last.converged == 1
    piece.close()
    g.close()


def test_refusals_change_nothing(gpu):
    g, fixed, fext = _parent()
    before = _snapshot(g)
    L = g._L
    for part, flags in ((-1, 0), (2, 0), (0, 2), (0, -1)):   # bad part, bad flags: *out is NULL afterwards
        out = C.c_void_p(12345)
        assert L.fb_fem_detach_part(g.h, part, flags, C.byref(out), None, None, None) == fl.FB_EINVAL, (part, flags)
        assert out.value is None
    assert L.fb_fem_detach_part(g.h, 0, 0, None, None, None, None) == fl.FB_EINVAL   # NULL out
    out = C.c_void_p(12345)
    assert L.fb_fem_detach_part(None, 0, 0, C.byref(out), None, None, None) == fl.FB_EINVAL and out.value is None
    for k in (-1, 2):
        with pytest.raises(fl.FbError):
            g.detach_part(k)
    assert _same_snapshot(before, _snapshot(g)) and g.parts()["n_parts"] == 2
    g.do_timestep()
    assert g.last.converged == 1
    g.close()


def test_a_host_built_plan_is_refused(gpu, monkeypatch):
    monkeypatch.setenv("FEMBRAIN_PLAN_DEVICE", "0")
    v, t = truth_cube(3, 3, 3, 0.1)
    g = FemIntegrator(v, t, NONE)
    assert g._L.fb_fem_plan_on_device(g.h) == 0 and g.parts()["n_parts"] == 1
    with pytest.raises(fl.FbError) as e:
        g.detach_part(0)
    assert e.value.code == fl.FB_EINVAL
    assert len(g.constrained_dofs()) == 0
    g.set_constrained_dofs([0, 1, 2])
    assert g.constrained_dofs().tolist() == [0, 1, 2]
    g.close()
