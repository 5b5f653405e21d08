"""CPU: the C restatement (oracle/fem_oracle.c) against the golden vectors produced by the reference's own VegaFEM
build (tests/golden/make_fem_golden.py) and, where oracle/_ref is present, against that build live."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import fem_params as fp
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube
from oracle import pyoracle
from oracle.pyoracle import OrcFem

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def cube5():
    g = np.load(os.path.join(GOLD, "fem_cube5.npz"))
    n = int(g["n"])
    v, t = truth_cube(n, n, n, 0.1)
    return g, v, t


def test_elements_pattern_mass(cube5):
    g, v, t = cube5
    o = OrcFem(v, t)
    for k, e in enumerate(g["els"]):
        assert np.abs(o.K0(int(e)) - g["K0"][k]).max() <= 1e-12 * np.abs(g["K0"][k]).max()
        assert np.abs(o.Minv(int(e)) - g["Minv"][k]).max() <= 1e-12 * np.abs(g["Minv"][k]).max()
    ia, ja = o.csr()
    assert np.array_equal(ia, g["ia"]) and np.array_equal(ja, g["ja"])  # bit-exact pattern and column order
    M = sp.csr_matrix((o.mass_on_pattern(), ja, ia), shape=(o.r, o.r))
    Mref = sp.csr_matrix((g["mass_a"], g["mass_ja"], g["mass_ia"]), shape=(o.r, o.r))
    assert abs(M - Mref).max() <= 1e-15 * abs(Mref).max()


def test_assembly(cube5):
    g, v, t = cube5
    o = OrcFem(v, t)
    f, K = o.assemble(g["u"])
    assert np.abs(f - g["f"]).max() <= 1e-12 * np.abs(g["f"]).max()
    assert np.abs(K - g["K"]).max() <= 1e-12 * np.abs(g["K"]).max()


def test_step_system_and_solution(cube5):
    g, v, t = cube5
    o = OrcFem(v, t)
    o.integrator(g["fixed"])
    o.set_state(g["q0"], g["v0"])
    fext = np.zeros(o.r)
    fext[1::3] = -10.0
    o.set_external_forces(fext)
    info, keff, rhs, dv = o.step(cg_eps=1e-12, cg_maxiter=20000, want=True)
    assert np.abs(keff - g["keff"]).max() <= 1e-12 * np.abs(g["keff"]).max()
    assert np.abs(rhs - g["rhs"]).max() <= 1e-11 * np.abs(g["rhs"]).max()
    assert abs(info - int(g["cg_info"])) <= 2
    assert np.abs(dv - g["dv"]).max() <= 1e-9 * np.abs(g["dv"]).max()
    q1, v1 = o.get_state()
    assert np.abs(q1 - g["q1"]).max() <= 1e-9 * np.abs(g["q1"]).max()


@pytest.mark.parametrize("load,key", [(-10000.0, "ref_load"), (-10.0, "gentle")])
def test_three_steps(cube5, load, key):
    g, v, t = cube5
    o = OrcFem(v, t)
    o.integrator(g["fixed"])
    f = np.zeros(o.r)
    f[1::3] = load
    for k in range(3):
        o.set_external_forces(f)
        it = o.step()
        q, qv = o.get_state()
        assert abs(it - int(g["it_" + key][k])) <= 2
        # both runs stop at the reference's 1e-6 residual: agreement far below that tolerance is not implied
        assert np.abs(q - g["q_" + key][k]).max() <= 2e-6 * np.abs(g["q_" + key][k]).max()
        assert np.abs(qv - g["v_" + key][k]).max() <= 2e-5 * np.abs(g["v_" + key][k]).max()


def test_beam3_mass_file_and_steps():
    """beam3_tet.mass is a mass matrix shipped BY the reference for beam3_tet.veg: a known answer for a5."""
    g = np.load(os.path.join(GOLD, "fem_beam3.npz"))
    o = OrcFem(g["verts"], g["tets"], E=1e7, nu=0.46, rho=1000.0)
    ia, ja = o.csr()
    M = sp.csr_matrix((o.mass_on_pattern(), ja, ia), shape=(o.r, o.r))
    Mv = M[0::3][:, 0::3].tocsr()  # the vertex-level matrix sits on the xx entries of every 3x3 block
    n = int(g["mass_n"])
    Mref = sp.csr_matrix((g["mass_v"], (g["mass_i"], g["mass_j"])), shape=(n, n))
    assert abs(Mv - Mref).max() <= 1e-12 * abs(Mref).max()
    o.integrator(fixed_vertices_to_dofs(g["fixed_vertices"]))
    f = np.zeros(o.r)
    f[1::3] = -10.0
    for k in range(3):
        o.set_external_forces(f)
        it = o.step()
        q, _ = o.get_state()
        assert abs(it - int(g["iters"][k])) <= 3
        assert np.abs(q - g["q"][k]).max() <= 5e-6 * np.abs(g["q"][k]).max()


def test_polar_decomposition_properties():
    o = OrcFem(*truth_cube(2, 2, 2, 0.1))
    rng = np.random.default_rng(0)
    for _ in range(50):
        F = np.eye(3) + 0.4 * rng.normal(size=(3, 3))
        det, R, S = o.polar(F)
        if det < 0:
            continue
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9
        assert np.abs(R @ S - F).max() < 1e-9 and np.abs(S - S.T).max() < 1e-15


@pytest.mark.skipif(not pyoracle.have_ref(), reason="oracle/_ref (reference build) not present")
def test_live_reference_build_matches_and_survey_norms():
    """The harness + reference TUs reproduce the norms SURVEY.md 8c recorded from the FULL reference build
    (27^3 cube, |q|_2 = 730.25, 875.31, 531.02 after steps 1..3) -- this pins the restated DoTimestep sequence."""
    from oracle.pyoracle import RefFem
    n = 27
    v, t = truth_cube(n, n, n, 0.1)
    fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))
    r = RefFem(v, t)
    r.integrator(fixed)
    f = np.zeros(r.r)
    f[1::3] = -10000.0
    want = [730.25, 875.31, 531.02]
    for k in range(3):
        r.set_external_forces(f)
        r.step()
        q, _ = r.get_state()
        assert abs(np.linalg.norm(q) - want[k]) < 0.006


def test_linear_elasticity_mode_against_reference_vectors():
    """warp = 0 (corotationalLinearFEM.cpp:429-453): K = K0, f = K0 u -- golden vectors of the reference build with
    ComputeForceAndStiffnessMatrix(.., warp = 0) (tests/golden/make_fem_golden.py linear)"""
    g = np.load(os.path.join(GOLD, "fem_cube5_linear.npz"))
    n = int(g["n"])
    v, t = truth_cube(n, n, n, 0.1)
    o = OrcFem(v, t)
    o.set_linear(True)
    f, K = o.assemble(g["u"])
    assert np.abs(f - g["f"]).max() <= 1e-12 * np.abs(g["f"]).max()
    assert np.abs(K - g["K"]).max() <= 1e-12 * np.abs(g["K"]).max()
    # K does not depend on u, and f is linear in it
    f2, K2 = o.assemble(2.0 * g["u"])
    assert np.array_equal(K2, K) and np.abs(f2 - 2.0 * f).max() <= 1e-12 * np.abs(f).max()
    o.integrator(g["fixed"])
    fext = np.zeros(o.r)
    fext[1::3] = -10.0
    for k in range(2):
        o.set_external_forces(fext)
        it = o.step()
        q, _ = o.get_state()
        assert abs(abs(it) - g["it"][k]) <= 2
        assert np.abs(q - g["q"][k]).max() <= 1e-5 * np.abs(g["q"][k]).max()


def test_warp2_exact_tangent_against_reference_golden_and_finite_differences():
    """warp = 2 (corotationalLinearFEM.cpp:296-428): the oracle's f and K against the reference build's golden vectors; and the
    reference's own self-check idea (ForceModel::TestStiffnessMatrix, forceModel.cpp:47-109): K is the derivative of f"""
    g = np.load(os.path.join(GOLD, "fem_cube5_warp2.npz"))
    n = int(g["n"])
    v, t = truth_cube(n, n, n, 0.1)
    o = OrcFem(v, t)
    o.set_warp(2)
    f, K = o.assemble(g["u"])
    assert np.abs(f - g["f"]).max() <= 1e-12 * np.abs(g["f"]).max()
    assert np.abs(K - g["K"]).max() <= 1e-11 * np.abs(g["K"]).max()
    import scipy.sparse as sp
    ia, ja = o.csr()
    A = sp.csr_matrix((K, ja, ia), shape=(o.r, o.r))
    assert abs(A - A.T).max() <= 1e-12 * abs(A).max()          # the exact tangent of this model is symmetric (to rounding)
    rng = np.random.default_rng(3)
    dq = rng.normal(size=o.r)
    eps = 1e-7
    fp, _ = o.assemble(g["u"] + eps * dq, want_K=False)
    fm, _ = o.assemble(g["u"] - eps * dq, want_K=False)
    fd = (fp - fm) / (2 * eps)
    assert np.abs(fd - A @ dq).max() <= 2e-5 * np.abs(A @ dq).max()
    o.set_warp(1)                                              # warp = 1 leaves the rotation's derivative out: not the derivative of f
    _, K1 = o.assemble(g["u"])
    A1 = sp.csr_matrix((K1, ja, ia), shape=(o.r, o.r))
    assert np.abs(fd - A1 @ dq).max() > 1e-3 * np.abs(A @ dq).max()


def test_newmark_step_against_reference_golden():
    g = np.load(os.path.join(GOLD, "fem_cube5_newmark.npz"))
    n = int(g["n"])
    v, t = truth_cube(n, n, n, 0.1)
    for mx in (1, 3):
        o = OrcFem(v, t)
        o.integrator(g["fixed"])
        f = np.zeros(o.r)
        f[1::3] = -10000.0
        for k in range(3):
            o.set_external_forces(f)
            newton, pcg = o.newmark_step(max_newton=mx)
            assert newton == g["iters_%d" % mx][k][0] and abs(pcg - g["iters_%d" % mx][k][1]) <= 3
            q, qv = o.get_state()
            for got, want in ((q, g["q_%d" % mx][k]), (qv, g["qvel_%d" % mx][k]), (o.get_accel(), g["qaccel_%d" % mx][k])):
                assert np.abs(got - want).max() <= 5e-6 * np.abs(want).max()   # two solves that both stop at 1e-6


@pytest.mark.parametrize("name", ["disc", "pyramid"])
def test_shipped_disc_and_pyramid_meshes(name):
    """The other two tet meshes the reference ships (data/models/disc/disc.1.veg, pyramid/pyramid.1.veg) through the oracle against
    the reference build's vectors (tests/golden/fem_<name>.npz, make_fem_golden.py shipped): f and K at a seeded displacement, three
    gentle steps.  The disc is a thin plate of slivers: 2,000+ PCG iterations on 204 DOFs, counts agree to a few per cent."""
    g = np.load(os.path.join(GOLD, "fem_%s.npz" % name))
    o = OrcFem(g["verts"], g["tets"])
    ia, ja = o.csr()
    assert np.array_equal(ia, g["ia"]) and np.array_equal(ja, g["ja"])
    f, K = o.assemble(g["u"])
    assert np.abs(f - g["f"]).max() <= 1e-9 * np.abs(g["f"]).max()
    assert np.abs(K - g["K"]).max() <= 1e-9 * np.abs(g["K"]).max()
    o.integrator(fixed_vertices_to_dofs(g["fixed_vertices"]))
    fe = np.zeros(o.r)
    fe[1::3] = -10.0
    eps = float(g["cg_eps"])  # 1e-9 for the disc: at 1e-6 two correct solvers of this plate agree only to ~1e-3
    for k in range(3):
        o.set_external_forces(fe)
        it = abs(o.step(cg_eps=eps))
        q, _ = o.get_state()
        assert abs(it - int(g["iters"][k])) <= max(5, 0.1 * int(g["iters"][k])), (k, it, int(g["iters"][k]))
        assert np.abs(q - g["q"][k]).max() <= 5e-6 * np.abs(g["q"][k]).max()


def test_peanut_veg_steps_against_reference_build():
    """data/models/blobtree/peanut.veg -- a mesh FemBrain itself simulates (its polygonizer's surface, tetrahedralized by TetGen;
    3,224 nodes / 12,947 tets) -- through the oracle against the reference build (tests/golden/fem_peanut.npz): two steps under the
    reference load and two under a gentle one"""
    g = np.load(os.path.join(GOLD, "fem_peanut.npz"))
    v = g["verts"].astype(np.float64)
    fixed = fixed_vertices_to_dofs(g["fixed_vertices"])
    for load, key in ((-10000.0, "ref_load"), (-10.0, "gentle")):
        o = OrcFem(v, g["tets"])
        o.integrator(fixed)
        fe = np.zeros(o.r)
        fe[1::3] = load
        for k in range(2):
            o.set_external_forces(fe)
            it = abs(o.step())
            q, _ = o.get_state()
            assert abs(it - int(g["it_" + key][k])) <= max(3, 0.02 * int(g["it_" + key][k]))
            assert np.abs(q - g["q_" + key][k]).max() <= 5e-6 * np.abs(g["q_" + key][k]).max()


# --- away from the default parameters (tests/fem_params.py) ------------------------------------------------------------------------------

def _param_mesh(mesh):
    if mesh == "cube5":
        v, t = truth_cube(5, 5, 5, 0.1)
        return v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(5, 5))
    g = np.load(os.path.join(GOLD, "fem_beam3.npz"))
    return g["verts"], g["tets"], fixed_vertices_to_dofs(g["fixed_vertices"])


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()


@pytest.mark.skipif(not pyoracle.have_ref(), reason="oracle/_ref (reference build) not present")
@pytest.mark.parametrize("mesh", ["cube5", "beam3"])
@pytest.mark.parametrize("name", fp.NAMES)
def test_oracle_matches_the_reference_build_at_every_parameter_set(mesh, name):
    """OrcFem against RefFem (the reference's own CorotationalLinearFEM, GenerateMassMatrix, SparseMatrix, CGSolver) at each set of
    tests/fem_params.py: f and K at a seeded displacement, the mass on the pattern (rho), Keff and rhs of a backward-Euler step from a
    live state (h, c_M, c_K, lambda < 0 or >> mu), and q, qdot after three steps.  Same arithmetic in both up to summation order: 1e-12
    on the matrices; both solves stop at the reference's 1e-6 residual, iteration counts within max(2, 5 %) (the long solves of near_incomp
    and of beam3 part on summation order alone: 386 against 400 at stiff_long on beam3)."""
    from oracle.pyoracle import RefFem
    v, t, fixed = _param_mesh(mesh)
    o, r = OrcFem(v, t, **fp.material(name)), RefFem(v, t, **fp.material(name))
    ia, ja = o.csr()
    ria, rja = r.csr()
    assert np.array_equal(ia, ria) and np.array_equal(ja, rja)
    u = np.random.default_rng(11).normal(size=o.r) * 0.003
    (fo, Ko), (fr, Kr) = o.assemble(u), r.assemble(u)
    assert _rel(fo, fr) <= 1e-12 and _rel(Ko, Kr) <= 1e-12
    M = sp.csr_matrix((o.mass_on_pattern(), ja, ia), shape=(o.r, o.r))
    mia, mja, ma = r.mass_csr()
    Mr = sp.csr_matrix((ma, mja, mia), shape=(o.r, o.r))
    assert abs(M - Mr).max() <= 1e-15 * abs(Mr).max()
    for x in (o, r):
        x.integrator(fixed, **fp.integrator(name))
        x.set_state(*fp.live_state(x.r, fixed))
        x.set_external_forces(fp.load(name, x.r))
    (io, ko, bo, _), (ir, kr, br, _) = o.step(want=True), r.step(want=True)
    assert _rel(ko, kr) <= 1e-12 and _rel(bo, br) <= 1e-12 and abs(io - ir) <= max(2, 0.05 * abs(ir)), (io, ir)
    for x in (o, r):
        x.set_state(np.zeros(x.r), np.zeros(x.r))
    for k in range(3):
        io, ir = o.step(), r.step()
        assert abs(io - ir) <= max(2, 0.05 * abs(ir)), (k, io, ir)
        (qo, vo), (qr, vr) = o.get_state(), r.get_state()
        assert _rel(qo, qr) <= 2e-6 and _rel(vo, vr) <= 2e-5, (k, _rel(qo, qr), _rel(vo, vr))


@pytest.mark.skipif(not pyoracle.have_ref(), reason="oracle/_ref (reference build) not present")
@pytest.mark.parametrize("mesh", ["cube5", "beam3"])
@pytest.mark.parametrize("name", fp.NAMES)
def test_oracle_newmark_matches_the_reference_build_off_the_control_pair(mesh, name):
    """ImplicitNewmarkSparse::DoTimestep, oracle against the reference build, for every (beta, gamma) of tests/fem_params.py -- the two
    with gamma != 2 beta make a6 = (1 - gamma / 2 beta) h, a3 and a5 live -- with 1 and 3 Newton iterations: q, qdot, qddot after three
    steps, the same Newton counts and PCG totals within max(2 per solve, 5 %) (two solves that both stop at 1e-6, as in
    test_newmark_step_against_reference_golden)"""
    from oracle.pyoracle import RefFem
    v, t, fixed = _param_mesh(mesh)
    for beta, gamma in fp.NEWMARK:
        for mx in (1, 3):
            o, r = OrcFem(v, t, **fp.material(name)), RefFem(v, t, **fp.material(name))
            for x in (o, r):
                x.integrator(fixed, **fp.integrator(name))
            f = fp.load(name, o.r)
            for k in range(3):
                for x in (o, r):
                    x.set_external_forces(f)
                (no, po), (nr, pr) = o.newmark_step(beta, gamma, max_newton=mx), r.newmark_step(beta, gamma, max_newton=mx)
                assert no == nr and abs(po - pr) <= max(2 * mx, 0.05 * pr), (beta, gamma, mx, k, po, pr)
                (qo, vo), (qr, vr) = o.get_state(), r.get_state()
                for a, b, tol in ((qo, qr, 5e-6), (vo, vr, 5e-5), (o.get_accel(), r.get_accel(), 5e-5)):
                    assert _rel(a, b) <= tol, (beta, gamma, mx, k, _rel(a, b))


def test_parameter_golden_is_the_oracle_at_those_parameters():
    """tests/golden/fem_cube5_params.npz (make_fem_golden.py params: the reference build's vectors at four sets of tests/fem_params.py)
    through the oracle: Keff applied to a seeded vector, its diagonal, rhs from a live state, q / qdot after three steps; the Newmark
    step with (beta, gamma) = (0.4, 0.6) at soft_damped; the step tolerances of the live comparisons above.  The same file pins the
    device in tests/test_fem_params_gpu.py."""
    g = np.load(os.path.join(GOLD, "fem_cube5_params.npz"))
    v, t, fixed = _param_mesh("cube5")
    ia, ja = OrcFem(v, t).csr()
    for name in [str(s) for s in g["names"]]:
        o = OrcFem(v, t, **fp.material(name))
        o.integrator(fixed, **fp.integrator(name))
        o.set_state(*fp.live_state(o.r, fixed))
        o.set_external_forces(fp.load(name, o.r))
        _, keff, rhs, _ = o.step(want=True)
        A = sp.csr_matrix((keff, ja, ia), shape=(o.r, o.r))
        assert _rel(A @ g["w"], g[name + "_keff_w"]) <= 1e-12 and _rel(A.diagonal(), g[name + "_keff_diag"]) <= 1e-12
        assert _rel(rhs, g[name + "_rhs"]) <= 1e-12
        o.set_state(np.zeros(o.r), np.zeros(o.r))
        for k in range(3):
            it = o.step()
            assert abs(it - int(g[name + "_its"][k])) <= max(2, 0.05 * it), (name, k, it)
        q, qv = o.get_state()
        assert _rel(q, g[name + "_q3"]) <= 2e-6 and _rel(qv, g[name + "_v3"]) <= 2e-5, name
    beta, gamma = g["newmark_pair"]
    o = OrcFem(v, t, **fp.material("soft_damped"))
    o.integrator(fixed, **fp.integrator("soft_damped"))
    for k in range(3):
        o.set_external_forces(fp.load("soft_damped", o.r))
        newton, pcg = o.newmark_step(beta, gamma, max_newton=1)
        assert newton == g["newmark_its"][k][0] and abs(pcg - g["newmark_its"][k][1]) <= 2, (k, pcg)
    q, qv = o.get_state()
    assert _rel(q, g["newmark_q3"]) <= 5e-6 and _rel(qv, g["newmark_v3"]) <= 5e-5 and _rel(o.get_accel(), g["newmark_a3"]) <= 5e-5
