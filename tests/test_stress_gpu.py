"""fb_fem_stress / fb_fem_read_stress / fb_fem_surface_stress against tests/stressref.py (pinned to the oracle's force model by
tests/test_stress_ref.py), against the oracle's element forces and against the handle's own assembly.

States are set with set_q_state: no step is needed.  The restatement of a (mesh, state) is computed once and shared."""
import ctypes
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import cut_inputs as ci
import cutref as cr
import stressref as sr
from fembrain_amd import lib as fl
from fembrain_amd.fem import Deformable, FemIntegrator
from fembrain_amd.meshgen import cube_fixed_plane_i0, delaunay_jittered, fixed_vertices_to_dofs, synthetic_cut, truth_cube
from oracle.pyoracle import OrcFem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON, OFF = fl.FB_RENUMBER_ON, fl.FB_RENUMBER_OFF
E, NU = 1e7, 0.46
LAM, MU = sr.lame(E, NU)
SCALE = 3 * LAM + 2 * MU
A = np.eye(3) + np.array([[0.021, 0.004, -0.006], [0.004, -0.013, 0.009], [-0.006, 0.009, 0.017]])  # symmetric, close to I


def _cube(nx, ny, nz, cell=0.1):
    v, t = truth_cube(nx, ny, nz, cell)
    return v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(ny, nz))


def _delaunay():
    v, t, fv = delaunay_jittered(6)
    return v, t, fixed_vertices_to_dofs(fv)


MESHES = {"cube2": (lambda: _cube(2, 2, 2), {}), "cube4": (lambda: _cube(4, 4, 4), {}), "cube5": (lambda: _cube(5, 5, 5), {}),
          "cube976": (lambda: _cube(9, 7, 6), {}), "delaunay_on": (_delaunay, dict(renumber=ON)), "delaunay_off": (_delaunay, dict(renumber=OFF))}
STATES = ("rest", "smooth", "inverted", "stretch", "rotstretch")


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


Q = _rotation((0.3, -0.5, 0.8), 0.7)


def _state(name, v, t):
    if name == "rest":
        return np.zeros(3 * len(v))
    if name == "smooth":
        return ci.smooth_displacement(v, 0.03).reshape(-1)
    if name == "inverted":
        return sr.invert_element(v, t, ci.smooth_displacement(v, 0.03).reshape(-1), e=3, factor=2.2)
    if name == "stretch":
        return (v @ (A - np.eye(3)).T).reshape(-1)
    if name == "rotstretch":
        return (v @ (Q @ A - np.eye(3)).T + np.array([0.05, -0.02, 0.11])).reshape(-1)
    if name == "rigid":
        return (v @ (Q - np.eye(3)).T).reshape(-1)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _mesh(mesh):
    return MESHES[mesh][0]()


@functools.lru_cache(maxsize=None)
def _oracle(mesh, linear=False):
    v, t, _ = _mesh(mesh)
    o = OrcFem(v, t, E, NU)
    if linear:
        o.set_linear(True)
    return o


@functools.lru_cache(maxsize=None)
def _ref(mesh, state, linear=False):
    """(u, restatement in the rest frame, in the world frame, the oracle's element forces): computed once, never written to"""
    v, t, _ = _mesh(mesh)
    o = _oracle(mesh, linear)
    u = _state(state, v, t)
    fe = np.array([o.element(e, u)[2] for e in range(o.nt)])
    return u, sr.stress(o, u, LAM, MU), sr.stress(o, u, LAM, MU, world=True), fe


def _handle(mesh, **kw):
    v, t, fixed = _mesh(mesh)
    return FemIntegrator(v, t, fixed, E=E, nu=NU, **dict(MESHES[mesh][1], **kw))


def _set(g, u):
    g.set_q_state(u, np.zeros_like(u))


def _check_info(info, arr, V):
    """the summary against numpy reductions of the device's own arrays: exact"""
    vm, J, psi = arr["von_mises"], arr["J"], arr["energy_density"]
    assert info["n_elements"] == len(vm)
    assert info["max_von_mises"] == vm.max() and info["max_element"] == int(np.argmax(vm))       # bit for bit; of equal maxima the lowest
    assert info["min_J"] == J.min() and info["min_J_element"] == int(np.argmin(J))
    assert info["n_inverted"] == int((J < 0).sum())
    ref = math.fsum(V * psi)
    assert abs(info["energy"] - ref) <= len(vm) * 2.0 ** -53 * abs(ref)


def _check_arrays(arr, ref, ids=None, rest=False, what=""):
    """device arrays against the restatement (of the elements ``ids``); returns the measured maxima"""
    pick = (lambda a: a) if ids is None else (lambda a: a[ids])
    m = dict(strain=np.abs(pick(arr["strain"]) - ref["strain"]).max(), stress=np.abs(pick(arr["stress"]) - ref["stress"]).max() / SCALE,
             von_mises=np.abs(pick(arr["von_mises"]) - ref["von_mises"]).max() / SCALE,
             J=(np.abs(pick(arr["J"]) - ref["J"]) / np.abs(ref["J"])).max())
    if not rest:
        m["psi"] = np.abs(pick(arr["energy_density"]) - ref["energy_density"]).max() / np.abs(ref["energy_density"]).max()
    print("%s: %s" % (what, ", ".join("%s %.2e" % kv for kv in sorted(m.items()))))
    assert m["strain"] <= 1e-10
    assert m["stress"] <= 3 * 1e-10 and m["von_mises"] <= 3 * 1e-10
    assert m["J"] <= 1e-12
    if not rest:
        assert m["psi"] <= 1e-8
    return m


@pytest.fixture(scope="module")
def handles():
    made = {}

    def get(mesh):
        if mesh not in made:
            made[mesh] = _handle(mesh)
        return made[mesh]
    yield get
    for g in made.values():
        g.close()


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("mesh", list(MESHES))
def test_arrays_and_summary_against_the_restatement(gpu, handles, mesh, state):
    """Measured maxima over all cases: strain 7.1e-15 (bound 1e-10), stress 3.8e-15 and von Mises 1.5e-16 of 3 lambda + 2 mu (3e-10), psi
    6.5e-15 of the mesh's largest (1e-8), J 0 relative (1e-12), force identity 5.4e-12 of the largest |fe| (1e-9); at rest |strain| is at
    most 1.6e-27 (1e-13)."""
    g = handles(mesh)
    u, ref, refw, fe = _ref(mesh, state)
    _set(g, u)
    rest = state == "rest"
    for world, r in ((False, ref), (True, refw)):
        info = g.stress(world=world, tensors=True)
        assert info["flags"] == (fl.FB_STRESS_TENSORS | (fl.FB_STRESS_WORLD if world else 0))
        arr = g.element_stress()
        _check_arrays(arr, r, rest=rest, what="%s %s %s" % (mesh, state, "world" if world else "rest frame"))
        _check_info(info, arr, r["V"])
        # the inverted set is the restatement's
        assert np.array_equal(np.nonzero(arr["J"] < 0)[0], np.nonzero(r["J"] < 0)[0])
        if state == "inverted":
            assert 3 in np.nonzero(arr["J"] < 0)[0] and info["n_inverted"] >= 1
        # von Mises recomputed from the stored tensor.  In the rest frame, where the stored one is formed: 1e-13 relative.  In the world
        # frame the tensor went through R (.) R^T with the assembly's R, a Newton iterate that stops at a step of 1e-6 |R|_1 and is then
        # orthogonal to about (3e-6)^2 / 2 = 5e-12: R R^T - I moves the tensor by at most 2 * 5e-12 |sigma|_F, and von Mises is
        # sqrt(3/2)-Lipschitz in the Frobenius norm -- 3e-11 of the largest |sigma|_F in all.
        again = sr.von_mises(arr["stress"])
        if world:
            frob = np.sqrt((arr["stress"][:, :3] ** 2).sum(axis=1) + 2 * (arr["stress"][:, 3:] ** 2).sum(axis=1))
            assert np.abs(again - arr["von_mises"]).max() <= 3e-11 * frob.max()
        else:
            assert (np.abs(again - arr["von_mises"]) <= 1e-13 * np.abs(arr["von_mises"])).all()
        if rest:
            assert np.abs(arr["strain"]).max() <= 1e-13 and info["n_inverted"] == 0 and info["max_von_mises"] <= SCALE * 1e-13
            continue
        # force identity: the DEVICE's stress with the restatement's R, b and V is the oracle's element force
        f12 = sr.element_forces(arr["stress"], r["R"], r["b"], r["V"], world=world)
        err = np.abs(f12 - fe).max() / np.abs(fe).max()
        print("%s %s force identity (%s): %.2e" % (mesh, state, "world" if world else "rest frame", err))
        assert err <= 1e-9
        if not world:
            # ... and scattered over the nodes, the internal force of the handle's own assembly
            v, t, _ = _mesh(mesh)
            f = np.zeros((len(v), 3))
            np.add.at(f, t.reshape(-1), f12.reshape(-1, 3))
            fg, _ = g.assemble(u)
            assert np.abs(f.reshape(-1) - fg).max() <= 1e-9 * np.abs(fg).max()


def test_colours_only_call_keeps_no_tensors(gpu, handles):
    g = handles("cube5")
    u, ref, _, _ = _ref("cube5", "smooth")
    _set(g, u)
    full = g.stress(tensors=True)
    a = g.element_stress()
    info = g.stress()
    assert info["flags"] == 0 and {k: v for k, v in info.items() if k != "flags"} == {k: v for k, v in full.items() if k != "flags"}
    b = g.element_stress()
    assert set(b) == {"von_mises", "energy_density", "J"}
    for k in b:
        assert np.array_equal(a[k], b[k])       # the same kernel arithmetic with and without the tensor stores
    with pytest.raises(fl.FbError) as ei:
        g.element_stress(tensors=True)
    assert ei.value.code == fl.FB_EINVAL and "tensors" in str(ei.value)
    # ranges
    part = g.element_stress(first=100, count=57)
    assert np.array_equal(part["von_mises"], b["von_mises"][100:157]) and np.array_equal(part["J"], b["J"][100:157])
    g.stress(tensors=True)
    part = g.element_stress(first=380, count=4)
    assert np.array_equal(part["stress"], a["stress"][380:]) and np.array_equal(part["strain"], a["strain"][380:])


def test_refusals_change_nothing(gpu, handles):
    g = handles("cube4")
    u, _, _, _ = _ref("cube4", "smooth")
    _set(g, u)
    g.stress(tensors=True)
    before = g.element_stress()
    L = fl.lib()
    info = fl.StressInfo()
    for flags in (4, 8 | fl.FB_STRESS_TENSORS, -1):
        assert L.fb_fem_stress(g.h, flags, None) == fl.FB_EINVAL and b"flag" in L.fb_last_error()
    n = g.num_tets()
    out = np.zeros(n)
    for first, count in ((-1, 1), (0, n + 1), (n, 1), (1, n), (0, -1), (n + 1, 0)):
        assert L.fb_fem_read_stress(g.h, first, count, fl.dptr(out), None, None, None, None) == fl.FB_EINVAL
    assert L.fb_fem_read_stress(g.h, n, 0, None, None, None, None, None) == fl.FB_OK
    assert L.fb_fem_time_stress(g.h, 0, 0, None, None) == fl.FB_EINVAL and L.fb_fem_time_stress(g.h, 1, 16, None, None) == fl.FB_EINVAL
    after = g.element_stress()
    for k in before:
        assert np.array_equal(before[k], after[k])
    assert L.fb_fem_stress(g.h, fl.FB_STRESS_TENSORS, ctypes.byref(info)) == fl.FB_OK and info.n_elements == n


def test_rigid_rotation_is_stress_free_only_with_warping(gpu):
    v, t, _ = _mesh("cube4")
    u = _state("rigid", v, t)
    g1, g0 = _handle("cube4"), _handle("cube4", linear=True)
    for g in (g0, g1):
        _set(g, u)
    i1, i0 = g1.stress(tensors=True), g0.stress(tensors=True)
    a1, a0 = g1.element_stress(), g0.element_stress()
    assert np.abs(a1["strain"]).max() <= 1e-10 and i1["max_von_mises"] <= 3 * SCALE * 1e-10
    # warp = 0: R = I, strain = sym(Q) - I in every element
    want = sr.six(0.5 * (Q + Q.T) - np.eye(3))
    assert np.abs(a0["strain"] - want).max() <= 1e-10 and np.abs(want).max() > 0.1
    assert i0["max_von_mises"] > 1e-2 * SCALE
    # ... and the linear handle against the restatement with the oracle in its linear mode
    _, ref, _, fe = _ref("cube4", "rigid", True)
    _check_arrays(a0, ref, what="cube4 rigid linear")
    assert np.abs(sr.element_forces(a0["stress"], ref["R"], ref["b"], ref["V"]) - fe).max() <= 1e-9 * np.abs(fe).max()
    g0.close()
    g1.close()


def test_equal_maxima_return_the_lowest_element(gpu):
    # dyadic coordinates, a dyadic diagonal stretch and R = I: every product and sum is exact, so every element has the same bits
    v, t, fixed = _cube(5, 5, 5, 0.125)
    g = FemIntegrator(v, t, fixed, E=E, nu=NU, linear=True)
    D = np.diag([2.0 ** -5, 0.0, -(2.0 ** -6)])
    _set(g, (v @ D).reshape(-1))
    info = g.stress()
    a = g.element_stress()
    assert (a["von_mises"] == a["von_mises"].max()).sum() >= 2 and (a["J"] == a["J"].min()).sum() >= 2
    assert a["von_mises"][0] == a["von_mises"].max() and a["J"][0] == a["J"].min()
    assert info["max_element"] == 0 and info["min_J_element"] == 0
    # an element made the only maximum moves it; one more equal to it further up does not
    u = (v @ D).reshape(-1, 3).copy()
    u[t[200][0]] += [0.0, 2.0 ** -7, 0.0]
    _set(g, u.reshape(-1))
    info = g.stress()
    a = g.element_stress()
    assert info["max_element"] == int(np.argmax(a["von_mises"])) and info["max_von_mises"] == a["von_mises"].max()
    g.close()


def test_energy_bits_repeat_and_do_not_depend_on_the_numbering(gpu, handles):
    u, ref, _, _ = _ref("delaunay_on", "smooth")
    got = []
    for mesh in ("delaunay_on", "delaunay_off"):
        g = handles(mesh)
        assert g.renumbering()[0] == (mesh == "delaunay_on")
        _set(g, u)
        i1 = g.stress(tensors=True)
        a1 = g.element_stress()
        i2 = g.stress(tensors=True)
        assert i1 == i2
        got.append((i1, a1))
    assert got[0][0] == got[1][0]                      # the summary, energy bits included
    for k in got[0][1]:
        assert np.array_equal(got[0][1][k], got[1][1][k]), k


def test_host_built_plan_gives_the_same_arrays(gpu, handles, monkeypatch):
    u, _, _, _ = _ref("delaunay_on", "inverted")
    g = handles("delaunay_on")
    _set(g, u)
    want_info = g.stress(tensors=True)
    want = g.element_stress()
    assert fl.lib().fb_fem_plan_on_device(g.h) == 1
    monkeypatch.setenv("FEMBRAIN_PLAN_DEVICE", "0")
    gh = _handle("delaunay_on")
    monkeypatch.delenv("FEMBRAIN_PLAN_DEVICE")
    assert fl.lib().fb_fem_plan_on_device(gh.h) == 0
    _set(gh, u)
    assert gh.stress(tensors=True) == want_info
    got = gh.element_stress()
    for k in want:
        assert np.array_equal(want[k], got[k]), k
    assert np.array_equal(g.surface_stress(), gh.surface_stress())
    gh.close()


MATS = ((1e7, 0.46, 1000.0), (2e5, 0.45, 1000.0), (3e6, 0.40, 1100.0))


def _three_materials(t, v):
    c = v[t].mean(axis=1)
    return ((c[:, 0] > v[:, 0].mean()).astype(np.uint8) + (c[:, 1] > v[:, 1].mean()).astype(np.uint8)).astype(np.uint8)


def test_every_element_follows_its_own_material(gpu):
    v, t, _ = _mesh("cube5")
    ids = _three_materials(t, v)
    assert set(ids) == {0, 1, 2}
    lam, mu = (np.array([sr.lame(m[0], m[1])[k] for m in MATS])[ids] for k in (0, 1))
    u, _, _, _ = _ref("cube5", "smooth")
    o = _oracle("cube5")
    ref = sr.stress(o, u, lam, mu)
    g = _handle("cube5")
    g.set_materials(*zip(*MATS), element_ids=ids)
    _set(g, u)
    info = g.stress(tensors=True)
    a = g.element_stress()
    scale = 3 * lam + 2 * mu
    assert np.abs(a["strain"] - ref["strain"]).max() <= 1e-10
    assert (np.abs(a["stress"] - ref["stress"]).max(axis=1) <= 3 * scale * 1e-10).all()
    assert (np.abs(a["von_mises"] - ref["von_mises"]) <= 3 * scale * 1e-10).all()
    assert np.abs(a["energy_density"] - ref["energy_density"]).max() <= 1e-8 * ref["energy_density"].max()
    _check_info(info, a, ref["V"])
    # twice the force scaling: twice the stress, the same strain
    g.set_internal_force_scaling_factor(2.0)
    g.stress(tensors=True)
    b = g.element_stress()
    assert np.array_equal(b["strain"], a["strain"]) and np.array_equal(b["J"], a["J"])
    assert np.abs(b["stress"] - 2 * a["stress"]).max() <= 1e-15 * np.abs(a["stress"]).max() * 8
    g.close()


def test_force_scaling_on_a_uniform_handle_doubles_the_stress_and_leaves_the_strain(gpu):
    """the handle without an element map takes the scaling through its own lambda / mu, not through the table"""
    u, ref, _, _ = _ref("cube5", "smooth")
    g = _handle("cube5")
    assert g.element_map_bytes() == 0
    _set(g, u)
    i1 = g.stress(tensors=True)
    a = g.element_stress()
    g.set_internal_force_scaling_factor(2.0)
    i2 = g.stress(tensors=True)
    b = g.element_stress()
    assert np.array_equal(b["strain"], a["strain"]) and np.array_equal(b["J"], a["J"])
    # (doubling E doubles lambda and mu exactly: a power of two)
    assert np.array_equal(b["stress"], 2 * a["stress"]) and np.array_equal(b["von_mises"], 2 * a["von_mises"])
    assert np.array_equal(b["energy_density"], 2 * a["energy_density"])
    assert i2["max_von_mises"] == 2 * i1["max_von_mises"] and i2["max_element"] == i1["max_element"] and i2["energy"] == 2 * i1["energy"]
    assert np.abs(b["stress"] - 2 * ref["stress"]).max() <= 2 * 3 * SCALE * 1e-10
    g.set_internal_force_scaling_factor(1.0)
    g.stress(tensors=True)
    assert np.array_equal(g.element_stress()["stress"], a["stress"])
    g.close()


def test_a_map_of_copies_of_material_zero_gives_the_uniform_bytes(gpu, handles):
    v, t, _ = _mesh("cube5")
    u, _, _, _ = _ref("cube5", "inverted")
    gu = handles("cube5")
    _set(gu, u)
    iu = gu.stress(tensors=True)
    au = gu.element_stress()
    g = _handle("cube5")
    g.set_materials([E, E, E], [NU, NU, NU], [1000.0] * 3, element_ids=_three_materials(t, v))
    assert g.element_map_bytes() > 0
    _set(g, u)
    im = g.stress(tensors=True)
    am = g.element_stress()
    assert im == iu
    for k in au:
        assert np.array_equal(au[k], am[k]), k
    g.close()


def _surface_check(g, what):
    s = g.surface()
    a = g.element_stress()
    want = sr.surface_mean(a["von_mises"], s["faces"], s["vertex_ids"], s["face_tets"])
    got = g.surface_stress()
    assert got.dtype == np.float32 and len(got) == len(s["vertex_ids"]) > 0
    err = np.abs(got.astype(np.float64) - want)
    print("%s: surface stress on %d vertices, worst %.2e of its value" % (what, len(got), (err / np.maximum(np.abs(want), 1e-300)).max()))
    assert (err <= 2.0 ** -23 * np.abs(want)).all()
    return s


def _after_the_change(g, what):
    """stale after a change of the mesh; a new stress() has the new element count and matches the restatement on the read-back mesh"""
    for call in (g.element_stress, g.surface_stress):
        with pytest.raises(fl.FbError) as ei:
            call()
        assert ei.value.code == fl.FB_EINVAL and "current mesh" in str(ei.value)
    x, tt = g.read_mesh()
    u = ci.smooth_displacement(x, 0.02).reshape(-1)
    _set(g, u)
    info = g.stress(tensors=True)
    a = g.element_stress()
    assert info["n_elements"] == len(tt) == len(a["von_mises"])
    o = OrcFem(x, tt, E, NU)
    _check_arrays(a, sr.stress(o, u, LAM, MU), what=what)
    _surface_check(g, what)


def test_stale_until_asked_and_after_every_change_of_the_mesh(gpu):
    v, t, fixed = _mesh("cube5")
    g = FemIntegrator(v, t, fixed, E=E, nu=NU, expect_cuts=True)
    for call in (g.element_stress, g.surface_stress):          # nothing asked yet
        with pytest.raises(fl.FbError) as ei:
            call()
        assert ei.value.code == fl.FB_EINVAL
    _set(g, _ref("cube5", "smooth")[0])
    g.stress()
    _surface_check(g, "cube5 before the changes")
    # full re-sync
    g.resync(v, t, fixed)
    _after_the_change(g, "cube5 after resync")
    # a cut that does nothing leaves the arrays valid; one that cuts does not
    g.stress()
    info, _ = g.cut(cr.plane_strip((50.0, 0.0, 0.0), (1.0, 0.0, 0.0), half=1.0))
    assert info["status"] == fl.FB_CUT_NOTHING
    g.element_stress()
    lo, hi = v.min(0), v.max(0)
    xs = np.unique(v[:, 0])
    strip = cr.plane_strip(np.array([0.5 * (xs[1] + xs[2]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])]), (1.0, 0.013, 0.007), half=4.0 * float((hi - lo).max()))
    info, _ = g.cut(strip, mode="carry")
    assert info["status"] == fl.FB_CUT_DONE
    _after_the_change(g, "cube5 after the cut")
    # delta re-sync
    g.stress()
    _, _, d = synthetic_cut(g.verts, g.tets, axis=1, where=0.4)
    g.resync_delta(d, fixed)
    _after_the_change(g, "cube5 after resync_delta")
    g.close()


def test_surface_stress_on_the_delaunay_mesh_before_and_after_a_cut(gpu):
    v, t, fixed = _mesh("delaunay_on")
    g = FemIntegrator(v, t, fixed, E=E, nu=NU, renumber=ON, expect_cuts=True)
    _set(g, _ref("delaunay_on", "smooth")[0])
    g.stress()
    before = _surface_check(g, "delaunay before the cut")
    c = 0.5 * (v.min(0) + v.max(0))
    info, _ = g.cut(cr.plane_strip(c, (1.0, 0.021, 0.013), half=4.0), mode="carry")
    assert info["status"] == fl.FB_CUT_DONE
    g.stress()
    after = _surface_check(g, "delaunay after the cut")
    assert len(after["faces"]) > len(before["faces"])
    g.close()


def test_more_partials_than_a_workgroup_folds_at_once(gpu):
    """374,166 elements in 1,462 workgroups: the single-workgroup folds walk their partials in strides"""
    v, t, fixed = _cube(42, 40, 40)
    assert len(t) == 374166 and -(-len(t) // 256) > 256
    g = FemIntegrator(v, t, fixed, E=E, nu=NU, renumber=ON)
    u = sr.invert_element(v, t, ci.smooth_displacement(v, 0.03).reshape(-1), e=len(t) - 7, factor=2.2)
    _set(g, u)
    info = g.stress(tensors=True)
    a = g.element_stress()
    pick = np.sort(np.random.default_rng(7).choice(len(t), 2000, replace=False))
    pick[-1] = len(t) - 7
    o = OrcFem(v, t[pick], E, NU)             # the sampled elements as a mesh of their own over the same nodes
    ref = sr.stress(o, u, LAM, MU)
    _check_arrays(a, ref, ids=pick, what="cube 42 x 40 x 40, 2000 sampled elements")
    x, tt = g.read_mesh()
    assert np.array_equal(tt, t)
    p = x[tt]
    V = np.abs(np.einsum("ij,ij->i", p[:, 0] - p[:, 3], np.cross(p[:, 1] - p[:, 3], p[:, 2] - p[:, 3]))) / 6.0
    assert np.abs(V[pick] - ref["V"]).max() <= 1e-15 * V.max()
    _check_info(info, a, V)
    assert info["n_inverted"] >= 1 and a["J"][len(t) - 7] < 0
    assert info == g.stress(tensors=True)
    g.close()


def test_a_handle_that_asks_steps_to_the_same_bytes_as_one_that_does_not(gpu):
    v, t, fixed = _mesh("cube976")
    ga, gb = FemIntegrator(v, t, fixed, E=E, nu=NU), FemIntegrator(v, t, fixed, E=E, nu=NU)
    for k in range(3):
        for g in (ga, gb):
            g.set_uniform_force(1, -3000.0)
            g.do_timestep()
        gb.stress(tensors=bool(k % 2), world=bool(k // 2))
        gb.surface_stress()
    for a, b in zip(ga.get_q_state(), gb.get_q_state()):
        assert np.array_equal(a, b)
    ga.close()
    gb.close()


def test_deformable_forwards_and_the_timing_entry_point_answers(gpu):
    v, t, _ = _mesh("cube4")
    d = Deformable(v, t, fixed_vertices=cube_fixed_plane_i0(4, 4), E=E, nu=NU)
    d.timestep()
    info = d.stress(tensors=True)
    a = d.element_stress()
    assert info["max_von_mises"] == a["von_mises"].max() > 0 and a["stress"].shape == (len(t), 6)
    assert len(d.surface_stress()) == len(d.surface_mesh()["vertex_ids"])
    se, ss = d.integrator.time_stress(reps=3, tensors=True)
    assert 0 < se < 1 and 0 < ss < 1
    d.integrator.close()


def test_stress_map_example_runs(gpu, tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "stress_map.py"), "--n", "8", "--out", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "largest von Mises stress before the cut" in out.stdout and "after the cut" in out.stdout
    obj = (tmp_path / "stress_after.obj").read_text().splitlines()
    nv, nf = sum(ln.startswith("v ") for ln in obj), sum(ln.startswith("f ") for ln in obj)
    assert nv > 0 and nf > 0 and sum(ln.startswith("# vm ") for ln in obj) == nv
