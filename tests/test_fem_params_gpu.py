"""The device FEM path away from the default parameters, at the sets of tests/fem_params.py: the system (Keff, rhs) and the mass of
every assembly kernel against the oracle, the states of every solver path, and the parameters through a handle's life cycle.

Tolerances.  System: those of test_fem_gpu.py::test_system_spmv_pcg (1e-9 / 5e-7 on Keff, 1e-9 / 2e-7 on rhs) -- rounding of single
entries, independent of the conditioning.  States of an FB_MATRIX_F32 handle: tools/params_f32_spread.py runs the oracle's three steps
once with every Keff entry rounded to fp32 before its solve; the largest spread it prints on 9^3 .. 20^3 cubes is 4.3e-4 of max|q| and
max|qdot| at near_incomp (lambda / mu = 33), 2.7e-4 at default, 1.8e-6 at stiff_long and below 6e-7 at soft_damped, auxetic and
tiny_step.  STATE_TOL is about five times that, never below 1e-5 (two solves that stop at the same 1e-6 residual a few iterations
apart differ by up to 1.5e-6 at tiny_step: the oracle at 1e-6 against its own solve at 1e-12)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import cutref as cr
import fem_params as fp
from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator, bsr_to_scipy
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, synthetic_cut, truth_cube
from oracle.pyoracle import OrcFem

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
F32, F64 = fl.FB_MATRIX_F32, fl.FB_MATRIX_F64
STATE_TOL = {"near_incomp": 2.5e-3}     # FB_MATRIX_F32, q; every other set and every FB_MATRIX_F64 handle: 1e-5
KERNELS = ("rows", "tets1", "tets")                        # FEMBRAIN_ASM_KERNEL: k_assemble_rows, k_assemble_tets, the default


def _tol(name, prec):
    return STATE_TOL.get(name, 1e-5) if prec == F32 else 1e-5


def _cube(n):
    v, t = truth_cube(n, n, n, 0.1)
    return v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))


def _delaunay(seed=42, n=300):
    """Delaunay tetrahedra of random points with the mixed orientations scipy returns them in (slivers below 1e-7 dropped)"""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0, 1, size=(n, 3))
    t = Delaunay(pts).simplices.astype(np.int32)
    vol = np.einsum("ij,ij->i", pts[t[:, 1]] - pts[t[:, 0]], np.cross(pts[t[:, 2]] - pts[t[:, 0]], pts[t[:, 3]] - pts[t[:, 0]])) / 6
    t = np.ascontiguousarray(t[np.abs(vol) > 1e-7])
    assert (vol > 1e-7).any() and (vol < -1e-7).any()
    return pts, t, fixed_vertices_to_dofs(np.nonzero(pts[:, 0] < 0.1)[0])


def _mesh(kind):
    if kind == "hub":
        from test_fem_gpu import _wide_mesh
        return _wide_mesh()
    if kind == "delaunay":
        return _delaunay()
    return _cube(int(kind[4:]))


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()


def _oracle(v, t, fixed, name, **integ):
    o = OrcFem(v, t, **fp.material(name))
    o.integrator(fixed, **(integ or fp.integrator(name)))
    return o


def _check_system(g, v, t, fixed, name, prec, seed=7, **integ):
    """g.system() and g.mass() from a live state against the oracle's Keff / rhs / mass at the same parameters (free DOFs), A = A^T bit
    for bit, identity rows and a zero right-hand side on the clamped DOFs.  Returns (Keff blocks, rhs, mass) for bit comparisons."""
    o = _oracle(v, t, fixed, name, **integ)
    q0, v0 = fp.live_state(o.r, fixed, seed)
    fext = fp.load(name, o.r)
    o.set_state(q0, v0)
    o.set_external_forces(fext)
    g.set_q_state(q0, v0)
    g.set_external_forces(fext)
    _, keff, rhs, _ = o.step(cg_eps=1e-12, cg_maxiter=20000, want=True)
    Kg, rhs_g = g.system()
    free = np.ones(o.r, bool)
    free[fixed] = False
    ia, ja = o.csr()
    Ko = sp.csr_matrix((keff, ja, ia), shape=(o.r, o.r))
    bptr, bcol = g.pattern()
    Kgs = bsr_to_scipy(bptr, bcol, Kg)
    assert abs(Kgs - Kgs.T).max() == 0, name     # the persistent solver's LDS window reads lower blocks as transposes: A = A^T exactly
    tol_k, tol_b = (1e-9, 1e-9) if prec == F64 else (5e-7, 2e-7)
    dk = abs((Kgs - Ko)[free][:, free]).max() / abs(Ko).max()
    db = np.abs(rhs_g[free] - rhs[free]).max() / np.abs(rhs).max()
    assert dk <= tol_k and db <= tol_b, (name, dk, db)
    assert not rhs_g[~free].any() and abs(Kgs[~free] - sp.identity(o.r, format="csr")[~free]).max() == 0
    mo = o.mass_on_pattern()
    m_blk = np.empty(len(bcol))
    for node in range(len(bptr) - 1):          # the xx entry of every block of row 3 node (the mass is the same on the three DOFs)
        seg = mo[ia[3 * node]:ia[3 * node + 1]].reshape(-1, 3)[:, 0]
        m_blk[bptr[node]:bptr[node + 1]] = seg
    assert np.abs(g.mass() - m_blk).max() <= (1e-12 if prec == F64 else 1e-7) * m_blk.max(), name
    return Kg, rhs_g, g.mass()


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("name", fp.NAMES)
def test_system_of_every_assembly_kernel_at_every_parameter_set(gpu, monkeypatch, name, prec):
    """Keff, rhs and mass of k_assemble_rows, k_assemble_tets and the default kernel (k_assemble_tets_st for fp32 records) on a 9^3 cube
    from a random (q, qdot) against the oracle at each set -- c_M > 0 makes the g_m m qdot term and the s_m scale live, rho != 1000 the
    mass, nu < 0 a negative lambda -- and the three kernels write the same bits"""
    v, t, fixed = _cube(9)
    out = []
    for kern in KERNELS:
        monkeypatch.setenv("FEMBRAIN_ASM_KERNEL", kern)
        g = FemIntegrator(v, t, fixed, matrix_precision=prec, **fp.handle(name))
        out.append(_check_system(g, v, t, fixed, name, prec))
        g.close()
    for a in out[:2]:
        assert all(np.array_equal(x, y) for x, y in zip(a, out[2])), name


@pytest.mark.parametrize("name", ["soft_damped", "near_incomp", "auxetic"])
@pytest.mark.parametrize("kind", ["hub", "delaunay"])
def test_system_on_wide_rows_and_mixed_orientations(gpu, monkeypatch, kind, name):
    """The hub mesh (a row of more than 32 blocks: k_assemble_wide) and a Delaunay mesh of mixed orientations, fp32 records: every
    kernel against the oracle and bit for bit against the others"""
    v, t, fixed = _mesh(kind)
    out = []
    for kern in KERNELS:
        monkeypatch.setenv("FEMBRAIN_ASM_KERNEL", kern)
        g = FemIntegrator(v, t, fixed, matrix_precision=F32, **fp.handle(name))
        if kind == "hub":
            assert (fl.lib().fb_fem_assembly_wide_slices(g.h) > 0) == (kern != "rows")
        out.append(_check_system(g, v, t, fixed, name, F32))
        g.close()
    for a in out[:2]:
        assert all(np.array_equal(x, y) for x, y in zip(a, out[2])), name


def test_system_against_the_reference_build_golden(gpu):
    """tests/golden/fem_cube5_params.npz (the reference's own build at four sets): Keff applied to a seeded vector, its diagonal and
    rhs of the device, fp64 records"""
    g0 = np.load(os.path.join(GOLD, "fem_cube5_params.npz"))
    v, t, fixed = _cube(int(g0["n"]))
    free = np.ones(3 * len(v), bool)
    free[fixed] = False
    for name in [str(s) for s in g0["names"]]:
        g = FemIntegrator(v, t, fixed, matrix_precision=F64, **fp.handle(name))
        g.set_q_state(*fp.live_state(g.r, fixed))
        g.set_external_forces(fp.load(name, g.r))
        K, rhs = g.system()
        A = bsr_to_scipy(*g.pattern(), K)
        assert _rel((A @ g0["w"])[free], g0[name + "_keff_w"][free]) <= 1e-9, name
        assert _rel(A.diagonal()[free], g0[name + "_keff_diag"][free]) <= 1e-9, name
        assert _rel(rhs[free], g0[name + "_rhs"][free]) <= 1e-9, name
        g.close()


def test_newmark_off_the_control_pair_writes_the_same_bits_in_every_assembly_kernel(gpu, monkeypatch):
    """soft_damped with (beta, gamma) = (0.4, 0.6), three Newton iterations: Keff, rhs and the states after two steps, bit for bit across
    the assembly kernels"""
    v, t, fixed = _cube(12)
    out = []
    for kern in KERNELS:
        monkeypatch.setenv("FEMBRAIN_ASM_KERNEL", kern)
        g = FemIntegrator(v, t, fixed, matrix_precision=F32, integrator=fl.FB_INTEGRATOR_NEWMARK, **fp.handle("soft_damped"))
        g.set_newmark(0.4, 0.6, 3, 1e-6)
        its = []
        for _ in range(2):
            g.set_external_forces(fp.load("soft_damped", g.r))
            its.append((g.do_timestep(), g.last.newton_iterations))
        out.append((its, *g.system(), *g.get_q_state()))
        g.close()
    for a in out[:2]:
        assert a[0] == out[2][0] and all(np.array_equal(x, y) for x, y in zip(a[1:], out[2][1:]))


def _handle(monkeypatch, path, v, t, fixed, **kw):
    """a handle on solver path `path`, and what pcg_path() must say after a step"""
    if path in ("merged", "reference"):
        monkeypatch.setenv("FEMBRAIN_PCG_PERSIST", "0")
        g = FemIntegrator(v, t, fixed, pcg_variant=fl.FB_PCG_MERGED if path == "merged" else fl.FB_PCG_REFERENCE, **kw)
        monkeypatch.delenv("FEMBRAIN_PCG_PERSIST")
        return g, fl.FB_PCG_PATH_TWO_LAUNCH, ""
    monkeypatch.setenv("FEMBRAIN_PERSIST_MIN_WAVES", "1")
    if path == "pipe2":
        monkeypatch.setenv("FEMBRAIN_PERSIST_ROWS", "2")
    g = FemIntegrator(v, t, fixed, pcg_variant=fl.FB_PCG_PERSISTENT, **kw)
    monkeypatch.delenv("FEMBRAIN_PERSIST_ROWS", raising=False)
    return g, fl.FB_PCG_PATH_PERSISTENT, "k_pcg_pipe2<c16>" if path == "pipe2" else "k_pcg_pipe<float,c16,8,8>"


@pytest.mark.parametrize("path,prec", [("merged", F64), ("merged", F32), ("reference", F32), ("persistent", F32), ("pipe2", F32)])
@pytest.mark.parametrize("name", ["soft_damped", "near_incomp", "auxetic", "tiny_step"])
def test_three_steps_on_every_solver_path(gpu, monkeypatch, name, path, prec):
    """Three steps of a 14^3 cube against the oracle on the two-launch merged and reference solvers and the persistent k_pcg_pipe /
    k_pcg_pipe2 (forced); pcg_path() says which ran.  Iteration counts within max(3, 2 %); at tiny_step (Keff ~ M, fewer than 30
    iterations: the persistent solver never reaches its first exact-residual refresh) the oracle's count exactly."""
    v, t, fixed = _cube(14)
    o = _oracle(v, t, fixed, name)
    g, want_path, want_kernel = _handle(monkeypatch, path, v, t, fixed, matrix_precision=prec, **fp.handle(name))
    assert g.pcg_path()["kernel"] == want_kernel, g.pcg_path()
    f = fp.load(name, o.r)
    tol = _tol(name, prec)
    for k in range(3):
        o.set_external_forces(f)
        g.set_external_forces(f)
        io, ig = abs(o.step()), g.do_timestep()
        if name == "tiny_step":
            assert io < fp.FIRST_REFRESH and ig == io, (k, ig, io)
        else:
            assert abs(ig - io) <= max(3, 0.02 * io), (k, ig, io)
        assert g.last.pcg_path == want_path
        (qo, vo), (qg, vg, _) = o.get_state(), g.get_q_state()
        assert _rel(qg, qo) <= tol and _rel(vg, vo) <= 5 * tol, (k, _rel(qg, qo), _rel(vg, vo))
        assert not qg[fixed].any() and not vg[fixed].any()
    g.close()


@pytest.mark.parametrize("name", ["soft_damped", "near_incomp", "auxetic", "tiny_step"])
def test_block_jacobi_steps_solve_the_same_systems(gpu, name):
    """FB_PCG_BLOCK_JACOBI (another preconditioner: another stopping point) with both solves at 1e-10: the oracle's states to 1e-7"""
    v, t, fixed = _cube(14)
    o = _oracle(v, t, fixed, name)
    g = FemIntegrator(v, t, fixed, matrix_precision=F64, pcg_variant=fl.FB_PCG_BLOCK_JACOBI, cg_eps=1e-10, cg_max_iter=20000, **fp.handle(name))
    f = fp.load(name, o.r)
    for k in range(3):
        o.set_external_forces(f)
        g.set_external_forces(f)
        assert o.step(cg_eps=1e-10, cg_maxiter=20000) > 0 and g.do_timestep() > 0
        (qo, vo), (qg, vg, _) = o.get_state(), g.get_q_state()
        assert _rel(qg, qo) <= 1e-7 and _rel(vg, vo) <= 1e-7, (k, _rel(qg, qo), _rel(vg, vo))
    g.close()


@pytest.mark.parametrize("max_newton", [1, 3])
@pytest.mark.parametrize("path,prec", [("merged", F64), ("persistent", F32)])
def test_newmark_off_the_control_pair_against_the_oracle(gpu, monkeypatch, path, prec, max_newton):
    """ImplicitNewmarkSparse at soft_damped (c_M > 0) with (beta, gamma) = (0.4, 0.6): a6 = (1 - gamma / 2 beta) h, a3 and a5 live; on the
    persistent path every solve starts from the previous solution (the unsharded warm start).  q, qdot, qddot after three steps against
    the oracle, PCG totals within max(3 per solve, 2 %)."""
    v, t, fixed = _cube(14)
    o = _oracle(v, t, fixed, "soft_damped")
    g, want_path, want_kernel = _handle(monkeypatch, path, v, t, fixed, matrix_precision=prec, integrator=fl.FB_INTEGRATOR_NEWMARK,
                                        **fp.handle("soft_damped"))
    assert g.pcg_path()["kernel"] == want_kernel, g.pcg_path()
    g.set_newmark(0.4, 0.6, max_newton, 1e-6)
    f = fp.load("soft_damped", o.r)
    for k in range(3):
        o.set_external_forces(f)
        g.set_external_forces(f)
        its = g.do_timestep()
        newton, pcg = o.newmark_step(0.4, 0.6, max_newton=max_newton)
        assert g.last.newton_iterations == newton and abs(its - pcg) <= max(3 * newton, 0.02 * pcg), (k, its, pcg)
        assert g.last.pcg_path == want_path
        q, qv, qa = g.get_q_state()
        for got, w in zip((q, qv, qa), (*o.get_state(), o.get_accel())):
            assert _rel(got, w) <= 1e-5, (k, _rel(got, w))
    g.close()


def test_mirror_window_at_soft_damped(gpu, monkeypatch):
    """The 12-wave kernel with its LDS mirror window on a 52^3 cube at soft_damped: three steps bit for bit those of the same kernel
    without the window (FEMBRAIN_PIPE_MIRROR=0), and within the state tolerance of the two-launch solver"""
    v, t, fixed = _cube(52)
    monkeypatch.setenv("FEMBRAIN_PIPE_MIRROR", "0")
    g0 = FemIntegrator(v, t, fixed, **fp.handle("soft_damped"))
    monkeypatch.delenv("FEMBRAIN_PIPE_MIRROR")
    g1 = FemIntegrator(v, t, fixed, **fp.handle("soft_damped"))
    monkeypatch.setenv("FEMBRAIN_PCG_PERSIST", "0")
    g2 = FemIntegrator(v, t, fixed, matrix_precision=F32, **fp.handle("soft_damped"))
    monkeypatch.delenv("FEMBRAIN_PCG_PERSIST")
    assert g1.persist_mirror()[0] and not g0.persist_mirror()[0] and g0.pcg_path()["kernel"] == g1.pcg_path()["kernel"]
    assert ",12," in g1.pcg_path()["kernel"], g1.pcg_path()
    f = fp.load("soft_damped", g1.r)
    for k in range(3):
        its = []
        for g in (g0, g1, g2):
            g.set_external_forces(f)
            its.append(g.do_timestep())
        assert g1.last.pcg_path == fl.FB_PCG_PATH_PERSISTENT and g2.last.pcg_path == fl.FB_PCG_PATH_TWO_LAUNCH
        assert its[0] == its[1] and abs(its[1] - its[2]) <= max(3, 0.02 * its[2]), its
        s0, s1, s2 = g0.get_q_state(), g1.get_q_state(), g2.get_q_state()
        assert all(np.array_equal(a, b) for a, b in zip(s0, s1)), k
        assert _rel(s1[0], s2[0]) <= 1e-5 and _rel(s1[1], s2[1]) <= 5e-5, k
    for g in (g0, g1, g2):
        g.close()


# --- the parameters through a handle's life cycle (soft_damped) ---------------------------------------------------------------------

def test_parameters_survive_resync_and_resync_delta(gpu):
    """A full re-sync onto another mesh and a delta re-sync (synthetic cut) rebuild with the handle's lambda, mu, rho, h, c_M, c_K"""
    v, t, fixed = _cube(7)
    g = FemIntegrator(v, t, fixed, matrix_precision=F64, **fp.handle("soft_damped"))
    _check_system(g, v, t, fixed, "soft_damped", F64)
    v2, t2, fixed2 = _cube(8)
    g.resync(v2, t2, fixed2)
    _check_system(g, v2, t2, fixed2, "soft_damped", F64)
    v3, t3, delta = synthetic_cut(v2, t2)
    g.resync_delta(delta, fixed2)
    _check_system(g, v3, t3, fixed2, "soft_damped", F64)
    g.close()


@pytest.mark.parametrize("mode", ["bake", "carry"])
def test_parameters_survive_a_cut(gpu, mode):
    """fb_fem_cut (BAKE / CARRY) through a deformed 9^3 cube: the handle's system afterwards is the oracle's on the mesh it reads back,
    at soft_damped"""
    v, t, fixed = _cube(9)
    g = FemIntegrator(v, t, fixed, matrix_precision=F64, **fp.handle("soft_damped"))
    g.set_external_forces(fp.load("soft_damped", g.r))
    g.do_timestep()
    lo, hi = v.min(0), v.max(0)
    xs = np.unique(v[:, 0])
    point = np.array([0.5 * (xs[4] + xs[5]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])])
    info, _ = g.cut(cr.plane_strip(point, (1.0, 0.013, 0.007), half=4.0 * float((hi - lo).max())), mode=mode)
    assert info["status"] == fl.FB_CUT_DONE and info["n_added"] > 0, info
    x2, t2 = g.read_mesh()
    _check_system(g, x2, t2, fixed, "soft_damped", F64)
    g.close()


def test_parameters_reach_a_handle_made_from_the_polygonizer(gpu):
    """fb_fem_create_from_poly takes E, nu, rho, h, c_M and c_K from its parameters as fb_fem_create does"""
    from fembrain_amd.blobtree import sphere_blob
    from fembrain_amd.poly import GpuPoly
    p = GpuPoly(sphere_blob())
    p.run_tetrahedralizer(0.1)
    xyz, tets = p.read_tetmesh()
    v, t = xyz.astype(np.float64), tets.astype(np.int32)
    fixed = fixed_vertices_to_dofs(np.nonzero(v[:, 1] < v[:, 1].min() + 0.15)[0])
    g = FemIntegrator.from_poly(p, fixed, matrix_precision=F64, **fp.handle("soft_damped"))
    _check_system(g, g.verts, g.tets, fixed, "soft_damped", F64)
    g.close()


@pytest.mark.parametrize("name", ["soft_damped", "auxetic"])
def test_parameters_reach_a_renumbered_handle(gpu, name):
    """FB_RENUMBER_ON (an internal node order) on a Delaunay mesh: the system in the caller's order is the oracle's at the set"""
    v, t, fixed = _delaunay()
    g = FemIntegrator(v, t, fixed, matrix_precision=F64, renumber=fl.FB_RENUMBER_ON, **fp.handle(name))
    assert g.renumbering()[0]
    _check_system(g, v, t, fixed, name, F64)
    g.close()


def test_setters_after_creation_and_after_a_resync(gpu):
    """set_timestep / set_damping / set_internal_force_scaling_factor on a handle made at the defaults (and twice soft_damped's E):
    the system is the oracle's at soft_damped; they hold through a re-sync; called again after it, the new values hold.  Non-finite
    damping or time step is refused and leaves the handle as it was."""
    v, t, fixed = _cube(7)
    p = fp.PARAMS["soft_damped"]
    g = FemIntegrator(v, t, fixed, matrix_precision=F64, E=2 * p["E"], nu=p["nu"], rho=p["rho"])
    g.set_timestep(p["h"])
    g.set_damping(p["cM"], p["cK"])
    g.set_internal_force_scaling_factor(0.5)
    _check_system(g, v, t, fixed, "soft_damped", F64)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(fl.FbError):
            g.set_damping(bad, p["cK"])
        with pytest.raises(fl.FbError):
            g.set_damping(p["cM"], bad)
        with pytest.raises(fl.FbError):
            g.set_timestep(bad)
    _check_system(g, v, t, fixed, "soft_damped", F64)
    v2, t2, fixed2 = _cube(8)
    g.resync(v2, t2, fixed2)
    _check_system(g, v2, t2, fixed2, "soft_damped", F64)
    g.set_timestep(0.02)
    g.set_damping(-0.05, 0.004)          # (finite negative damping is accepted, as the reference accepts it)
    _check_system(g, v2, t2, fixed2, "soft_damped", F64, timestep=0.02, cM=-0.05, cK=0.004)
    g.close()
