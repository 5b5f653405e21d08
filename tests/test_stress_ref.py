"""tests/stressref.py pinned to the oracle's force model without a GPU: the reference has no stress output, but its element force
E B (R^T x - x0) (corotationalLinearFEM.cpp:107-137, 270-286) pins the stress exactly.  What tests/test_stress_gpu.py compares the
device against."""
import numpy as np
import pytest

import stressref as sr
from cut_inputs import smooth_displacement
from fembrain_amd.meshgen import delaunay_jittered, truth_cube
from oracle.pyoracle import OrcFem

E, NU = 1e7, 0.46
LAM, MU = sr.lame(E, NU)


def _mesh(name):
    if name == "cube":
        return truth_cube(4, 4, 4, 0.1)
    v, t, _ = delaunay_jittered(6)
    return v, t


def _forces(o, u):
    return np.array([o.element(e, u)[2] for e in range(o.nt)])


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


A = np.eye(3) + np.array([[0.021, 0.004, -0.006], [0.004, -0.013, 0.009], [-0.006, 0.009, 0.017]])  # symmetric, close to I


@pytest.mark.parametrize("name", ["cube", "delaunay"])
def test_stress_reproduces_the_element_force(name):
    v, t = _mesh(name)
    o = OrcFem(v, t, E, NU)
    u = smooth_displacement(v, 0.03).reshape(-1)
    r = sr.stress(o, u, LAM, MU)
    fe = _forces(o, u)
    mine = sr.element_forces(r["stress"], r["R"], r["b"], r["V"])
    err = np.abs(mine - fe).max() / np.abs(fe).max()
    print("force identity on %s: %.2e of max |fe|" % (name, err))
    assert err < 1e-11
    w = sr.stress(o, u, LAM, MU, world=True)
    assert np.abs(sr.element_forces(w["stress"], w["R"], w["b"], w["V"], world=True) - fe).max() / np.abs(fe).max() < 1e-11


@pytest.mark.parametrize("name", ["cube", "delaunay"])
def test_inverted_element_keeps_the_identity_with_the_flipped_rotation(name):
    v, t = _mesh(name)
    o = OrcFem(v, t, E, NU)
    u = sr.invert_element(v, t, smooth_displacement(v, 0.03).reshape(-1))
    r = sr.stress(o, u, LAM, MU)
    inv = np.nonzero(r["J"] < 0)[0]
    assert 3 in inv
    fe = _forces(o, u)
    mine = sr.element_forces(r["stress"], r["R"], r["b"], r["V"])
    err = np.abs(mine[inv] - fe[inv]).max() / np.abs(fe[inv]).max()
    print("inverted elements %s on %s: %.2e of their max |fe|" % (inv.tolist(), name, err))
    assert err < 1e-12
    for e in inv:
        assert abs(np.linalg.det(r["R"][e]) - 1.0) < 1e-9   # the flipped R the oracle returns is a proper rotation


@pytest.mark.parametrize("name", ["cube", "delaunay"])
def test_energy_density_is_the_quadratic_form_of_K0(name):
    """V psi = d^T K0 d / 2 with d = R^T x - X, to 1e-12 relative in every element -- except where the quadratic form itself cancels
    further than that.  Its twelve-term sums in fp64 are good to gamma_14 = 14 * 2^-53 = 1.6e-15 of S = |d|^T |K0| |d| / 2, and V psi is
    formed from the same products; so an element passes at max(1e-12 |ref|, 4e-15 S): twice gamma_14 and a rounding up.  On the cube S is
    at most 934 |ref| and the second term never decides: every element is held to 1e-12 relative alone.  On the jittered Delaunay mesh
    slivers with |b| up to 6.6e3 take S to 7.7e6 |ref| (K0 entries of 4e8 against a V psi of 10); in extended precision the oracle's own
    K0 moves d^T K0 d by 1.5e-10 relative there.  Measured: per element 6.1e-14 relative on the cube; on the Delaunay mesh 5.5e-11
    relative (73 of 1230 elements past 1e-12) and 6.4e-16 of S."""
    v, t = _mesh(name)
    o = OrcFem(v, t, E, NU)
    u = smooth_displacement(v, 0.03).reshape(-1)
    r = sr.stress(o, u, LAM, MU)
    ref, S = np.zeros(o.nt), np.zeros(o.nt)
    for e in range(o.nt):
        n = o.tets[e]
        d = ((o.verts[n] + u.reshape(-1, 3)[n]) @ r["R"][e] - o.verts[n]).reshape(-1)  # R^T x - X, node by node
        K0 = o.K0(e)
        ref[e] = 0.5 * d @ K0 @ d
        S[e] = 0.5 * np.abs(d) @ np.abs(K0) @ np.abs(d)
    err = np.abs(r["V"] * r["energy_density"] - ref)
    print("V psi against d^T K0 d / 2 on %s: %.2e relative, %.2e of S, %d elements past 1e-12 relative, largest S / |ref| %.3g"
          % (name, (err / np.abs(ref)).max(), (err / S).max(), int((err > 1e-12 * np.abs(ref)).sum()), (S / np.abs(ref)).max()))
    if name == "cube":
        assert (err <= 1e-12 * np.abs(ref)).all()
    else:
        assert (err <= np.maximum(1e-12 * np.abs(ref), 4e-15 * S)).all()
        assert (err <= 1e-12 * np.abs(ref))[S <= 100 * np.abs(ref)].all()     # (where the form is well conditioned, the plain bound)


@pytest.mark.parametrize("name", ["cube", "delaunay"])
def test_linear_energy_is_half_the_work_of_the_internal_force(name):
    v, t = _mesh(name)
    o = OrcFem(v, t, E, NU)
    o.set_linear(True)
    u = smooth_displacement(v, 0.03).reshape(-1)
    r = sr.stress(o, u, LAM, MU)
    assert np.array_equal(r["R"], np.broadcast_to(np.eye(3), r["R"].shape))
    f, _ = o.assemble(u, want_K=False)
    total, ref = float(np.sum(r["V"] * r["energy_density"])), 0.5 * float(u @ f)
    print("linear energy on %s: %.17g against %.17g" % (name, total, ref))
    assert abs(total - ref) <= 1e-12 * abs(ref)


@pytest.mark.parametrize("name", ["cube", "delaunay"])
def test_homogeneous_stretch_gives_the_closed_formulas(name):
    """x = A X gives strain = A - I in every element to 1e-13, and the stress, von Mises, psi and J of the closed formulas.  The jittered
    Delaunay mesh has a sliver with |b| = 6.6e3 (element 784): H summed node by node as sum_j (R^T P_j - X_j) b_j^T multiplies the
    rounding of X + u (5.5e-17) by it and gave 1.04e-13 there; through the displacement gradient (stressref.element) the rounding that
    is left is u's own."""
    v, t = _mesh(name)
    o = OrcFem(v, t, E, NU)
    u = (v @ (A - np.eye(3)).T).reshape(-1)       # x - X, formed without the cancellation of A X - X
    r = sr.stress(o, u, LAM, MU)
    eps = A - np.eye(3)
    sig = LAM * np.trace(eps) * np.eye(3) + 2 * MU * eps
    err = np.abs(r["strain"] - sr.six(eps)).max()
    print("homogeneous stretch on %s: strain error %.2e" % (name, err))
    assert err < 1e-13
    scale = 3 * LAM + 2 * MU
    assert np.abs(r["stress"] - sr.six(sig)).max() < scale * 1e-13
    assert np.abs(r["von_mises"] - sr.von_mises(sr.six(sig))).max() < scale * 1e-13
    # psi = sigma : eps / 2 over nine entries: its error is at most |d sigma| |eps| + |sigma| |d eps| per entry, each within scale * 1e-13 * max |eps|
    assert np.abs(r["energy_density"] - 0.5 * np.sum(sig * eps)).max() < 9 * scale * 1e-13 * np.abs(eps).max()
    assert np.abs(r["J"] - np.linalg.det(A)).max() < 1e-13


@pytest.mark.parametrize("name", ["cube", "delaunay"])
def test_rotation_leaves_the_rest_frame_tensors_and_turns_the_world_ones(name):
    v, t = _mesh(name)
    o = OrcFem(v, t, E, NU)
    Q = _rotation((0.3, -0.5, 0.8), 0.7)
    c = np.array([0.05, -0.02, 0.11])
    u0 = (v @ (A - np.eye(3)).T).reshape(-1)
    u1 = (v @ (Q @ A - np.eye(3)).T + c).reshape(-1)
    r0, r1, w1 = sr.stress(o, u0, LAM, MU), sr.stress(o, u1, LAM, MU), sr.stress(o, u1, LAM, MU, world=True)
    scale = 3 * LAM + 2 * MU
    assert np.abs(r1["strain"] - r0["strain"]).max() < 1e-10      # (the Newton loop stops at a 1e-6 step: R to ~1e-12)
    assert np.abs(r1["stress"] - r0["stress"]).max() < scale * 1e-10
    eps = A - np.eye(3)
    assert np.abs(w1["strain"] - sr.six(Q @ eps @ Q.T)).max() < 1e-10
    sig = LAM * np.trace(eps) * np.eye(3) + 2 * MU * eps
    assert np.abs(w1["stress"] - sr.six(Q @ sig @ Q.T)).max() < scale * 1e-10
    assert np.abs(w1["von_mises"] - r0["von_mises"]).max() < scale * 1e-10


def test_surface_mean_walks_the_faces_of_a_vertex():
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 1, 0]])
    vm = np.array([1.0, 10.0, 100.0])
    got = sr.surface_mean(vm, faces, np.array([0, 1, 2, 3, 4]), np.array([2, 0, 1]))
    assert np.array_equal(got, [(100.0 + 1.0 + 10.0) / 3, (100.0 + 10.0) / 2, (100.0 + 1.0) / 2, 1.0, 10.0])
