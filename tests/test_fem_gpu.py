"""Parity of the HIP FEM path (through the C ABI) against the CPU oracle on the same inputs.

Tolerances (stated per test): FB_MATRIX_F64 storage reproduces the fp64 oracle up to summation order
(<= 1e-9 relative); the default FB_MATRIX_F32 storage rounds every stiffness entry to fp32 (6e-8 relative),
everything else (geometry, polar decomposition, vectors, dots) stays fp64.
"""
import os

import numpy as np
import pytest

from fembrain_amd import lib as fl
from fembrain_amd.fem import Deformable, FemIntegrator, bsr_to_scipy
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube
from oracle.pyoracle import OrcFem
from product_inputs import _delaunay_lattice

pytestmark = pytest.mark.gpu


def _cube(n):
    v, t = truth_cube(n, n, n, 0.1)
    fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))
    return v, t, fixed


def _oracle_bsr(o):
    """oracle scalar CSR values -> [nblk,3,3] in block order"""
    ia, ja = o.csr()

    def conv(a):
        bptr, bcol = o.blocks()
        out = np.empty((len(bcol), 3, 3))
        for k in range(3):
            rows = np.arange(o.nv) * 3 + k
            for r, node in zip(rows, range(o.nv)):
                seg = a[ia[r]:ia[r + 1]].reshape(-1, 3)
                out[bptr[node]:bptr[node + 1], k, :] = seg
        return out
    return conv


@pytest.mark.parametrize("prec,tol", [(fl.FB_MATRIX_F64, 1e-10), (fl.FB_MATRIX_F32, 5e-7)])
def test_pattern_elements_assembly(gpu, prec, tol):
    n = 6
    v, t, fixed = _cube(n)
    o = OrcFem(v, t)
    g = FemIntegrator(v, t, fixed, matrix_precision=prec)
    # a2: pattern bit-exact
    obptr, obcol = o.blocks()
    bptr, bcol = g.pattern()
    assert np.array_equal(bptr, obptr) and np.array_equal(bcol, obcol)
    # a1: K0 / M^-1 (MFMA fp64 kernel): tight in both modes
    K0, Mi = g.element_stiffness(0, len(t))
    for e in (0, 1, 77, len(t) - 1):
        assert np.abs(K0[e] - o.K0(e)).max() <= 1e-11 * np.abs(o.K0(e)).max()
        assert np.abs(Mi[e] - o.Minv(e)).max() <= 1e-11 * np.abs(o.Minv(e)).max()
    # ... the cube's gradient matrices are mostly zeros, so a transposed or permuted MFMA operand can pass there: EVERY element of the
    # 400-point Delaunay mesh, both orientations, dense gradients
    pts, td, fixed_d, _ = _random_delaunay()
    od = OrcFem(pts, td)
    gd = FemIntegrator(pts, td, fixed_d, matrix_precision=prec)
    K0d, Mid = gd.element_stiffness(0, len(td))
    worst = [0.0, 0.0]
    for e in range(len(td)):
        ko, mo_ = od.K0(e), od.Minv(e)
        worst = [max(worst[0], np.abs(K0d[e] - ko).max() / np.abs(ko).max()), max(worst[1], np.abs(Mid[e] - mo_).max() / np.abs(mo_).max())]
    print("k_element_K0_mfma on %d Delaunay elements: worst relative error K0 %.2e, Minv %.2e" % (len(td), worst[0], worst[1]))
    assert worst[0] <= 1e-11 and worst[1] <= 1e-11, worst
    # a range of elements is the same rows of the full call, bit for bit
    for first, count in ((1, 1), (3, 5), (len(td) - 2, 2)):
        Kr, Mr = gd.element_stiffness(first, count)
        assert np.array_equal(Kr, K0d[first:first + count]) and np.array_equal(Mr, Mid[first:first + count]), (first, count)
    gd.close()
    # a5: mass
    conv = _oracle_bsr(o)
    mo = conv(o.mass_on_pattern())[:, 0, 0]
    assert np.abs(g.mass() - mo).max() <= (1e-12 if prec == fl.FB_MATRIX_F64 else 1e-7) * mo.max()  # V travels in the fp32 record
    # a3: warped assembly at a random displacement
    rng = np.random.default_rng(5)
    u = rng.normal(size=o.r) * 0.01
    fo, Ko = o.assemble(u)
    fg, Kg = g.assemble(u)
    Ko = conv(Ko)
    assert np.abs(Kg - Ko).max() <= tol * np.abs(Ko).max()
    assert np.abs(fg - fo).max() <= 1e-9 * np.abs(fo).max()  # element forces never pass through the fp32 matrix


@pytest.mark.parametrize("spmv", [fl.FB_SPMV_ROWS, fl.FB_SPMV_SPLIT])  # the row kernel of large meshes / the split kernel of small ones
@pytest.mark.parametrize("prec,tol", [(fl.FB_MATRIX_F64, 1e-9), (fl.FB_MATRIX_F32, 5e-7)])
def test_system_spmv_pcg(gpu, prec, tol, spmv):
    n = 7
    v, t, fixed = _cube(n)
    o = OrcFem(v, t)
    o.integrator(fixed)
    g = FemIntegrator(v, t, fixed, matrix_precision=prec, spmv_kernel=spmv)
    rng = np.random.default_rng(7)
    q0 = rng.normal(size=o.r) * 0.005
    v0 = rng.normal(size=o.r) * 0.1
    q0[fixed] = 0
    v0[fixed] = 0
    fext = np.zeros(o.r)
    fext[1::3] = -10.0
    o.set_state(q0, v0)
    o.set_external_forces(fext)
    g.set_q_state(q0, v0)
    g.set_external_forces(fext)
    info, keff, rhs, dv = o.step(cg_eps=1e-12, cg_maxiter=20000, want=True)
    Kg, rhs_g = g.system()
    # constrained rows/cols: oracle removes them; here they are identity rows -> compare on the free DOFs
    free = np.ones(o.r, bool)
    free[fixed] = False
    ia, ja = o.csr()
    import scipy.sparse as sp
    Ko = sp.csr_matrix((keff, ja, ia), shape=(o.r, o.r))
    bptr, bcol = g.pattern()
    Kgs = bsr_to_scipy(bptr, bcol, Kg)
    assert abs(Kgs - Kgs.T).max() == 0  # stored operator exactly symmetric (fp32 rounding included): CG needs A = A^T
    D = (Kgs - Ko)[free][:, free]
    assert abs(D).max() <= tol * abs(Ko).max()
    # in fp32 mode the (hK+D)qvel term sees the rotated gradients through their fp32 record
    assert np.abs(rhs_g[free] - rhs[free]).max() <= (1e-9 if prec == fl.FB_MATRIX_F64 else 2e-7) * np.abs(rhs).max()
    assert np.all(rhs_g[~free] == 0)
    # identity rows
    Kc = Kgs[~free]
    assert abs(Kc - sp.identity(o.r, format="csr")[~free]).max() == 0
    # a9: SpMV against the same matrix multiplied on host
    x = rng.normal(size=o.r)
    y = g.spmv(x)
    assert np.abs(y - Kgs @ x).max() <= 1e-12 * np.abs(Kgs @ x).max()
    # a8: PCG with a tight tolerance reproduces the oracle's solution, in both formulations
    it, xg = g.pcg(rhs_g, eps=1e-12, max_iter=20000)
    assert it > 0
    assert np.abs(xg - dv).max() <= max(50 * tol, 1e-8) * np.abs(dv).max()
    for variant in (fl.FB_PCG_REFERENCE, fl.FB_PCG_PERSISTENT):
        if variant == fl.FB_PCG_PERSISTENT and prec == fl.FB_MATRIX_F64:
            continue    # the persistent solver keeps part of the matrix in LDS as fp32 words: FB_MATRIX_F32 only
        g2 = FemIntegrator(v, t, fixed, matrix_precision=prec, pcg_variant=variant)
        g2.set_q_state(q0, v0)
        g2.set_external_forces(fext)
        g2.system()
        it2, xg2 = g2.pcg(rhs_g, eps=1e-12, max_iter=20000)
        assert abs(it2 - it) <= max(2, 0.02 * it), variant
        assert np.abs(xg2 - xg).max() <= 1e-8 * np.abs(xg).max(), variant
        itz, xz = g2.pcg(np.zeros(o.r), eps=1e-6, max_iter=100)   # zero right-hand side: no iteration, x = 0
        assert itz == 0 and not xz.any()
        itm, _ = g2.pcg(rhs_g, eps=1e-12, max_iter=7)             # iteration cap: -7 as the reference returns
        assert itm == -7, (variant, itm)


@pytest.mark.parametrize("spmv", [fl.FB_SPMV_ROWS, fl.FB_SPMV_SPLIT])
@pytest.mark.parametrize("variant", [fl.FB_PCG_MERGED, fl.FB_PCG_REFERENCE, fl.FB_PCG_PERSISTENT])
@pytest.mark.parametrize("prec", [fl.FB_MATRIX_F64, fl.FB_MATRIX_F32])
def test_three_steps_reference_load(gpu, prec, variant, spmv):
    """q, qvel after 3 steps under the reference load (-10000 per y DOF, plane i=0 clamped, CG eps 1e-6).

    Stated tolerance: both solvers stop at a 1e-6 relative (Jacobi-weighted) residual, so the two converged
    solutions may differ by O(cond * 1e-6); measured against the reference build itself the oracle differs by
    1e-6..1e-7 after 3 steps (tests/test_oracle_ref.py).  Bound used here: 2e-4 of max|q| (fp32 matrix),
    2e-5 (fp64 matrix)."""
    n = 9
    v, t, fixed = _cube(n)
    if variant == fl.FB_PCG_PERSISTENT and prec == fl.FB_MATRIX_F64:
        with pytest.raises(fl.FbError, match="FB_MATRIX_F32"):
            FemIntegrator(v, t, fixed, matrix_precision=prec, pcg_variant=variant, spmv_kernel=spmv)
        return
    o = OrcFem(v, t)
    o.integrator(fixed)
    g = FemIntegrator(v, t, fixed, matrix_precision=prec, pcg_variant=variant, spmv_kernel=spmv)
    fext = np.zeros(o.r)
    fext[1::3] = -10000.0
    tol = 2e-5 if prec == fl.FB_MATRIX_F64 else 2e-4
    for k in range(3):
        o.set_external_forces(fext)
        g.set_external_forces(fext)
        io = o.step()
        ig = g.do_timestep()
        qo, vo = o.get_state()
        qg, vg, _ = g.get_q_state()
        assert abs(ig - abs(io)) <= max(3, 0.02 * abs(io)), (ig, io)
        assert np.abs(qg - qo).max() <= tol * np.abs(qo).max(), k
        assert np.abs(vg - vo).max() <= 10 * tol * np.abs(vo).max(), k
        assert np.all(qg[fixed] == 0) and np.all(vg[fixed] == 0)


def test_deformable_driver(gpu):
    n = 6
    v, t, _ = _cube(n)
    d = Deformable(v, t, fixed_vertices=cube_fixed_plane_i0(n, n), floor_y=-0.05)
    seen = []
    d.set_deform_callback(lambda dof, q: seen.append((dof, float(np.abs(q).max()))))
    it1 = d.timestep()
    assert it1 > 0 and len(seen) == 1 and seen[0][0] == 3 * len(v)
    q, qv, _ = d.integrator.get_q_state()
    # after the floor clamp no node sits below the floor
    assert (v[:, 1] + q[1::3]).min() >= -0.05 - 1e-12
    assert d.ct_collided > 0
    it2 = d.timestep()  # gravity is withheld after a collision step (Deformable.cpp:331)
    assert it2 > 0


def test_solver_failure_is_reported(gpu):
    n = 5
    v, t, fixed = _cube(n)
    g = FemIntegrator(v, t, fixed, cg_max_iter=3)
    g.set_uniform_force(1, -10000.0)
    q_before = g.get_q_state()[0].copy()
    with pytest.raises(fl.FbError) as ei:
        g.do_timestep()
    assert ei.value.code == fl.FB_ESOLVER
    assert np.array_equal(g.get_q_state()[0], q_before)  # state untouched, as the reference exits before the update


def test_bad_arguments(gpu):
    v, t, fixed = _cube(4)
    with pytest.raises(fl.FbError):
        FemIntegrator(v, t, fixed[::-1])  # not ascending
    bad = t.copy()
    bad[0, 0] = len(v)
    with pytest.raises(fl.FbError, match="tet 0 references node %d outside" % len(v)):
        FemIntegrator(v, bad, fixed)
    bad[0, 0], bad[5, 2] = 0, -3
    with pytest.raises(fl.FbError, match="tet 5 references node -3 outside"):
        FemIntegrator(v, bad, fixed)


def test_one_rank_rccl_communicator_runs_the_collective_path(gpu):
    """RCCL plumbing on one GPU: a real one-rank communicator (dlopen, unique id, ncclCommInitRank) drives the sharded
    code path -- partial fold kernel + ncclAllReduce on the handle's stream every iteration -- and must reproduce the
    unsharded result bit for bit (a one-rank all-reduce is the identity)."""
    import ctypes as C
    L = fl.lib()
    buf = (C.c_ubyte * 128)()
    fl.check(L.fb_comm_unique_id(buf))
    comm = C.c_void_p()
    fl.check(L.fb_comm_create(C.byref(comm), 0, 1, buf, 0))
    n = 8
    v, t, fixed = _cube(n)
    a = FemIntegrator(v, t, fixed)
    b = FemIntegrator(v, t, fixed, shard=(1, 0, None, comm))
    for g in (a, b):
        g.set_uniform_force(1, -10000.0)
    ia = [a.do_timestep() for _ in range(2)]
    ib = [b.do_timestep() for _ in range(2)]
    assert ia == ib
    assert np.array_equal(a.get_q_state()[0], b.get_q_state()[0])
    b.close()
    fl.check(L.fb_comm_destroy(comm))


def test_config1_sphere_tetmesh_one_step(gpu):
    """BASELINE config 1: sphere.blob polygonized at cellsize 0.1 (3,744 tets, the golden-pinned mesh), nodes with
    y < -0.35 clamped, reference gravity, one step -- an UNSTRUCTURED pattern (ragged rows, SELL padding)."""
    from fembrain_amd.blobtree import sphere_blob
    from fembrain_amd.poly import GpuPoly
    xyz, tets = GpuPoly(sphere_blob()).run_tetrahedralizer(0.1)
    assert len(tets) == 3744
    v = xyz.astype(np.float64)
    t = tets.astype(np.int32)
    fixed = fixed_vertices_to_dofs(np.nonzero(v[:, 1] < -0.35)[0])
    o = OrcFem(v, t)
    o.integrator(fixed)
    g = FemIntegrator(v, t, fixed)
    obptr, obcol = o.blocks()
    bptr, bcol = g.pattern()
    assert np.array_equal(bptr, obptr) and np.array_equal(bcol, obcol)
    f = np.zeros(o.r)
    f[1::3] = -10000.0
    o.set_external_forces(f)
    g.set_external_forces(f)
    io, ig = abs(o.step()), g.do_timestep()
    qo, _ = o.get_state()
    qg, _, _ = g.get_q_state()
    assert abs(io - ig) <= max(3, 0.02 * io)
    assert np.abs(qg - qo).max() <= 2e-4 * np.abs(qo).max()


def test_beam3_against_reference_golden(gpu):
    """Vega's own beam (208 nodes / 450 tets, TetGen-style unstructured) with the q after 3 steps of the step sequence restated on
    reference objects (oracle/ref_harness.cpp over the reference's own force model, matrix and solver code)."""
    import os
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "fem_beam3.npz"))
    fixed = fixed_vertices_to_dofs(gold["fixed_vertices"])
    for prec, tol in ((fl.FB_MATRIX_F64, 2e-5), (fl.FB_MATRIX_F32, 3e-4)):
        g = FemIntegrator(gold["verts"], gold["tets"], fixed, matrix_precision=prec)
        f = np.zeros(g.r)
        f[1::3] = -10.0
        for k in range(3):
            g.set_external_forces(f)
            it = g.do_timestep()
            q, _, _ = g.get_q_state()
            assert abs(it - int(gold["iters"][k])) <= max(5, 0.03 * int(gold["iters"][k]))
            assert np.abs(q - gold["q"][k]).max() <= tol * np.abs(gold["q"][k]).max()
        # mass against the matrix file the reference ships (beam3_tet.mass)
        bptr, bcol = g.pattern()
        m = g.mass()
        import scipy.sparse as sp
        M = sp.csr_matrix((m, bcol, bptr), shape=(len(gold["verts"]),) * 2)
        Mref = sp.csr_matrix((gold["mass_v"], (gold["mass_i"], gold["mass_j"])), shape=M.shape)
        assert abs(M - Mref).max() <= (1e-12 if prec == fl.FB_MATRIX_F64 else 1e-7) * abs(Mref).max()


@pytest.mark.parametrize("name", ["disc", "pyramid"])
def test_shipped_disc_and_pyramid_meshes_against_reference_golden(gpu, name):
    """data/models/disc/disc.1.veg (a thin plate of slivers) and pyramid/pyramid.1.veg, the other tet meshes the reference ships:
    pattern, f and K at a seeded displacement and three gentle steps against the reference build's vectors"""
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "fem_%s.npz" % name))
    fixed = fixed_vertices_to_dofs(gold["fixed_vertices"])
    # fp32 matrix storage on the disc: every entry rounded to 6e-8 times a condition number of ~1e5 (2,800 PCG iterations on 204 DOFs)
    # The DEFAULT handle (FB_MATRIX_AUTO) stores a mesh this small as fp64 -- below the persistent solver's range fp32 values buy no
    # speed -- and is held to the fp64 tolerance; fp32 storage asked for by name keeps its measured 1e-2 on the disc.
    for prec, tol_k, tol_q in ((fl.FB_MATRIX_AUTO, 1e-9, 2e-5), (fl.FB_MATRIX_F64, 1e-9, 2e-5), (fl.FB_MATRIX_F32, 5e-7, 1e-2 if name == "disc" else 3e-4)):
        g = FemIntegrator(gold["verts"], gold["tets"], fixed, matrix_precision=prec, cg_eps=float(gold["cg_eps"]))  # (disc: 1e-9, see make_fem_golden.py)
        assert g.matrix_precision() == (fl.FB_MATRIX_F32 if prec == fl.FB_MATRIX_F32 else fl.FB_MATRIX_F64)
        f, K = g.assemble(gold["u"])
        bptr, bcol = g.pattern()
        # the golden K is the reference's scalar CSR: compare through a sparse matrix
        import scipy.sparse as sp
        n = len(gold["verts"])
        A = sp.bsr_matrix((K, bcol, bptr), shape=(3 * n, 3 * n)).tocsr()
        Aref = sp.csr_matrix((gold["K"], gold["ja"], gold["ia"]), shape=(3 * n, 3 * n))
        assert abs(A - Aref).max() <= tol_k * abs(Aref).max()
        assert np.abs(f - gold["f"]).max() <= (1e-9 if prec == fl.FB_MATRIX_F64 else 1e-9) * np.abs(gold["f"]).max()
        fe = np.zeros(g.r)
        fe[1::3] = -10.0
        for k in range(3):
            g.set_external_forces(fe)
            it = g.do_timestep()
            q, _, _ = g.get_q_state()
            assert abs(it - int(gold["iters"][k])) <= max(5, 0.15 * int(gold["iters"][k])), (name, k, it, int(gold["iters"][k]))
            assert np.abs(q - gold["q"][k]).max() <= tol_q * np.abs(gold["q"][k]).max(), (name, k, prec, np.abs(q - gold["q"][k]).max() / np.abs(gold["q"][k]).max())
        g.close()


def test_peanut_veg_steps_against_reference_golden(gpu):
    """data/models/blobtree/peanut.veg, a mesh FemBrain itself simulates (3,224 nodes / 12,947 TetGen tets), against the reference
    build's q after two steps under the reference load and under a gentle one; both matrix widths"""
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "fem_peanut.npz"))
    v = gold["verts"].astype(np.float64)
    fixed = fixed_vertices_to_dofs(gold["fixed_vertices"])
    for prec, tol in ((fl.FB_MATRIX_F64, 2e-5), (fl.FB_MATRIX_F32, 3e-4)):
        for load, key in ((-10000.0, "ref_load"), (-10.0, "gentle")):
            g = FemIntegrator(v, gold["tets"], fixed, matrix_precision=prec)
            f = np.zeros(g.r)
            f[1::3] = load
            for k in range(2):
                g.set_external_forces(f)
                it = g.do_timestep()
                q, _, _ = g.get_q_state()
                ref = gold["q_" + key][k]
                assert abs(it - int(gold["it_" + key][k])) <= max(5, 0.03 * int(gold["it_" + key][k])), (key, k, it)
                assert np.abs(q - ref).max() <= tol * np.abs(ref).max(), (prec, key, k, np.abs(q - ref).max() / np.abs(ref).max())
            g.close()


@pytest.mark.parametrize("name", ["dumbel", "dumbelclose", "eggshell", "implicit_sphere"])
def test_remaining_shipped_tet_meshes_against_reference_golden(gpu, name):
    """The other tet meshes the reference ships as polygonizer output (round 3, tests/golden/make_fem_golden.py round3):
    data/models/blobtree/{dumbel,dumbelclose,eggshell}.veg -- GPUPoly surfaces tetrahedralized by TetGen, 18-22k slivery tets -- and
    data/models/sphere/implicit_sphere.veg, the tet polygonizer's own output (624 unwelded cells: 624 separate bodies, most of them
    free-floating).  q after two steps of the reference build under the reference load and under -10 per y-DOF, both matrix widths;
    iteration counts of both steps."""
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "fem_%s.npz" % name))
    v = gold["verts"].astype(np.float64)
    fixed = fixed_vertices_to_dofs(gold["fixed_vertices"])
    for prec, tol in ((fl.FB_MATRIX_F64, 5e-5), (fl.FB_MATRIX_F32, 5e-4)):
        for load, key in ((-10000.0, "ref_load"), (-10.0, "gentle")):
            g = FemIntegrator(v, gold["tets"], fixed, matrix_precision=prec)
            f = np.zeros(g.r)
            f[1::3] = load
            for k in range(2):
                g.set_external_forces(f)
                it = g.do_timestep()
                # (implicit_sphere is 624 separate bodies, most of them in free fall: the iteration at which the LAST of them passes the
                # tolerance moves with rounding -- 114 for 105 with the fp64 matrix, 218 for 151 with the fp32-stored one in the
                # second step under the reference load, where the cells have fallen 266 units; q is held to its tolerance all the same)
                rel = (0.1 if prec == fl.FB_MATRIX_F64 else 0.5) if name == "implicit_sphere" else 0.03
                assert abs(it - int(gold["it_" + key][k])) <= max(5, rel * int(gold["it_" + key][k])), (name, key, k, it, int(gold["it_" + key][k]))
            q = g.get_q_state()[0]
            ref = gold["q_" + key]
            assert np.abs(q - ref).max() <= tol * np.abs(ref).max(), (name, prec, key, np.abs(q - ref).max() / np.abs(ref).max())
            g.close()


def test_tumor_veg_is_refused_where_the_reference_goes_nan(gpu):
    """data/models/blobtree/tumor.veg: two of its 32,303 tets have exactly zero volume at the six digits the file prints.  The
    reference's inverse4x4 (corotationalLinearFEM.cpp:529-572) divides by zero there: its K and f are NaN from the first assembly on
    (recorded in tests/golden/fem_tumor.npz by the reference build itself) and its PCG 'converges' in 0 iterations.  Here the handle
    is refused and the element named (decided deviation)."""
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "fem_tumor.npz"))
    assert not bool(gold["reference_K_finite"]) and int(gold["n_flat_tets"]) == 2
    with pytest.raises(fl.FbError, match="rest volume") as e:
        FemIntegrator(gold["verts"].astype(np.float64), gold["tets"], fixed_vertices_to_dofs(gold["fixed_vertices"]))
    assert e.value.code == fl.FB_EINVAL


def test_ragged_inputs(gpu):
    """Edge cases: a node no element references (kept at rest), a single tet, no constraints at all (singular K but
    Keff = M + ... is SPD), arbitrary (not node-aligned) constrained DOFs."""
    v, t, fixed = _cube(4)
    v2 = np.vstack([v, [[9.0, 9.0, 9.0]]])  # isolated extra node
    g = FemIntegrator(v2, t, fixed)
    g.set_uniform_force(1, -100.0)
    it = g.do_timestep()
    q, qv, _ = g.get_q_state()
    assert it > 0 and np.isfinite(q).all() and np.isfinite(qv).all()
    o = OrcFem(v, t)
    o.integrator(fixed)
    f = np.zeros(o.r)
    f[1::3] = -100.0
    o.set_external_forces(f)
    o.step()
    qo, _ = o.get_state()
    assert np.abs(q[:-3] - qo).max() <= 2e-4 * np.abs(qo).max()
    # single tet, free floating
    v1 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], float) * 0.1
    t1 = np.array([[0, 1, 2, 3]], np.int32)
    g1 = FemIntegrator(v1, t1, [])
    g1.set_uniform_force(1, -1.0)
    assert g1.do_timestep() > 0
    o1 = OrcFem(v1, t1)
    o1.integrator(np.zeros(0, np.int32))
    f1 = np.zeros(12)
    f1[1::3] = -1.0
    o1.set_external_forces(f1)
    o1.step()
    assert np.abs(g1.get_q_state()[0] - o1.get_state()[0]).max() <= 1e-6 * np.abs(o1.get_state()[0]).max()
    # constrained DOFs that do not cover whole nodes
    odd = np.array([0, 4, 5, 17, 30], np.int32)
    g3 = FemIntegrator(v, t, odd)
    o3 = OrcFem(v, t)
    o3.integrator(odd)
    g3.set_external_forces(f)
    o3.set_external_forces(f)
    g3.do_timestep()
    o3.step()
    q3 = g3.get_q_state()[0]
    assert np.all(q3[odd] == 0) and np.abs(q3 - o3.get_state()[0]).max() <= 2e-4 * np.abs(q3).max()
    # changing the constraints later takes effect at the next step
    g3.set_constrained_dofs(fixed)
    g3.reset_to_rest()
    g3.set_external_forces(f)
    g3.do_timestep()
    assert np.abs(g3.get_q_state()[0] - qo).max() <= 2e-4 * np.abs(qo).max()


def test_integrator_surface_semantics(gpu):
    """IntegratorBase-level calls behave as the reference's: force setters, state copies, reset, timestep / damping
    changes, resync after a topology change (Deformable::syncForceModel) and the per-step element rebuild."""
    n = 5
    v, t, fixed = _cube(n)
    g = FemIntegrator(v, t, fixed)
    o = OrcFem(v, t)
    o.integrator(fixed, timestep=0.02, cM=0.1, cK=0.02)
    g.set_timestep(0.02)
    g.set_damping(0.1, 0.02)
    f1 = np.zeros(g.r)
    f1[1::3] = -40.0
    f2 = np.zeros(g.r)
    f2[0::3] = 15.0
    g.set_external_forces_to_zero()
    g.add_external_forces(f1)
    g.add_external_forces(f2)          # AddExternalForces accumulates
    o.set_external_forces(f1 + f2)
    rng = np.random.default_rng(2)
    q0 = rng.normal(size=g.r) * 1e-3
    v0 = rng.normal(size=g.r) * 1e-2
    q0[fixed] = 0
    v0[fixed] = 0
    g.set_q_state(q0, v0)
    qa, va, aa = g.get_q_state()
    assert np.array_equal(qa, q0) and np.array_equal(va, v0) and not aa.any()   # copy semantics, qaccel forced 0
    o.set_state(q0, v0)
    g.rebuild_elements()               # same rest state: must not change the result
    ig, io = g.do_timestep(), abs(o.step())
    assert abs(ig - io) <= max(3, 0.02 * io)
    assert np.abs(g.get_q_state()[0] - o.get_state()[0]).max() <= 2e-4 * np.abs(o.get_state()[0]).max()
    assert g.get_force_assembly_time() > 0 and g.get_system_solve_time() > 0
    g.reset_to_rest()
    assert not g.get_q_state()[0].any() and not g.get_q_state()[1].any()
    # resync with a different mesh (as after a cut): same handle, new topology, state reset
    v2, t2, fixed2 = _cube(6)
    g.resync(v2, t2, fixed2)
    o2 = OrcFem(v2, t2)
    o2.integrator(fixed2, timestep=0.02, cM=0.1, cK=0.02)
    bptr, bcol = g.pattern()
    obptr, obcol = o2.blocks()
    assert np.array_equal(bptr, obptr) and np.array_equal(bcol, obcol)
    f = np.zeros(g.r)
    f[1::3] = -100.0
    g.set_external_forces(f)
    o2.set_external_forces(f)
    g.do_timestep()
    o2.step()
    assert np.abs(g.get_q_state()[0] - o2.get_state()[0]).max() <= 2e-4 * np.abs(o2.get_state()[0]).max()
    # moved rest positions + rebuild_elements == a fresh handle on the moved mesh (the per-step K0 rebuild path)
    with pytest.raises(fl.FbError):
        g.set_timestep(0.0)
    with pytest.raises(ValueError):
        g.set_external_forces(np.zeros(5))


def test_floor_collision_kernel_matches_reference_loop(gpu):
    """Deformable.cpp:350-402 restated on the host vs fb_fem_floor_collision."""
    n = 5
    v, t, fixed = _cube(n)
    g = FemIntegrator(v, t, fixed)
    rng = np.random.default_rng(4)
    q = rng.normal(size=g.r) * 0.05
    qv = rng.normal(size=g.r)
    g.set_q_state(q, qv)
    floor_y = 0.03
    hit = g.floor_collision(floor_y, 0.4)
    pc = v[:, 1] + q[1::3]
    assert hit == int((pc <= floor_y).sum())
    q_ref, v_ref = q.copy(), qv.copy()
    v_ref[1::3] = qv[1::3] - 1.4 * qv[1::3]          # vr = vp - 0.4 vn with n = +y
    m = pc <= floor_y
    q_ref[1::3][m] = floor_y - v[m, 1]
    qg, vg, _ = g.get_q_state()
    assert np.allclose(qg, q_ref, rtol=0, atol=1e-15) and np.allclose(vg, v_ref, rtol=1e-15, atol=1e-15)


def test_config2_105k_tets_one_step(gpu):
    """BASELINE config 2 canonical mesh (27^3 nodes, 105,456 tets): one reference-load step against the oracle."""
    n = 27
    v, t, fixed = _cube(n)
    o = OrcFem(v, t)
    o.integrator(fixed)
    g = FemIntegrator(v, t, fixed)
    f = np.zeros(o.r)
    f[1::3] = -10000.0
    o.set_external_forces(f)
    g.set_uniform_force(1, -10000.0)
    io, ig = abs(o.step()), g.do_timestep()
    qo, vo = o.get_state()
    qg, vg, _ = g.get_q_state()
    assert abs(io - ig) <= max(3, 0.02 * io), (io, ig)      # 1029 iterations in the reference build
    assert abs(np.linalg.norm(qg) - 730.25) < 0.05          # |q|_2 after step 1 of the full reference
    assert np.abs(qg - qo).max() <= 2e-4 * np.abs(qo).max()
    assert np.abs(vg - vo).max() <= 2e-3 * np.abs(vo).max()


def test_full_size_1M_tet_properties(gpu):
    """BASELINE config 4 mesh (998,250 tets): size-independent properties of the assembled operator and the solve."""
    n = 56
    v, t, fixed = _cube(n)
    g = FemIntegrator(v, t, fixed)
    assert g.num_blocks() == 2559646
    rng = np.random.default_rng(11)
    # mass: sum over all blocks = rho * volume (each tet contributes rho V /20 * (4*2 + 12*1) = rho V)
    assert abs(g.mass().sum() - 1000.0 * (0.1 * (n - 1)) ** 3) <= 1e-6 * 1000.0 * (0.1 * (n - 1)) ** 3
    # internal forces of any displacement field sum to zero (translation invariance of every element)
    u = rng.normal(size=g.r) * 1e-3
    fint, _ = g.assemble(u)
    assert np.abs(fint.reshape(-1, 3).sum(0)).max() <= 1e-9 * np.abs(fint).sum()
    # a rigid translation produces no internal force at all
    ft, _ = g.assemble(np.tile([0.3, -0.2, 0.1], len(v)))
    assert np.abs(ft).max() <= 1e-6 * np.abs(fint).max()
    # SpMV of the assembled Keff: linear and symmetric
    g.set_uniform_force(1, -10000.0)
    g.system()
    x, y = rng.normal(size=g.r), rng.normal(size=g.r)
    Ax, Ay = g.spmv(x), g.spmv(y)
    assert np.abs(g.spmv(2.0 * x - 3.0 * y) - (2.0 * Ax - 3.0 * Ay)).max() <= 1e-12 * np.abs(Ax).max()
    assert abs(y @ Ax - x @ Ay) <= 1e-12 * abs(y @ Ax)
    assert np.array_equal(Ax[fixed], x[fixed])              # identity rows on the clamped plane
    # one full step: converged, and the returned dv really solves the system to the reference tolerance
    K, rhs = g.system()
    it, dv = g.pcg(rhs, eps=1e-6, max_iter=10000)
    assert 1000 < it < 3000
    res = rhs - g.spmv(dv)
    bptr, bcol = g.pattern()
    diag = np.empty(g.r)
    isdiag = bcol == np.repeat(np.arange(len(v)), np.diff(bptr))
    diag.reshape(-1, 3)[:] = np.stack([K[isdiag][:, k, k] for k in range(3)], 1)
    assert (res * res / diag).sum() <= 1.5e-12 * (rhs * rhs / diag).sum()   # sum r^2/D <= eps^2 sum r0^2/D
    assert not dv[fixed].any()


def test_full_size_8M_tet_properties(gpu):
    """BASELINE config 5 mesh (111^3 nodes, 7,986,000 tets) on one GPU: the block count of SURVEY.md section 8, the
    non-temporal SpMV with 16-bit column ids (what systems this large run) linear and symmetric, one step from rest
    converged with the residual the reference's stopping rule asks for."""
    n = 111
    v, t, fixed = _cube(n)
    assert len(t) == 7986000
    g = FemIntegrator(v, t, fixed)
    assert g.num_blocks() == 20220091
    assert fl.lib().fb_fem_plan_on_device(g.h) == 1
    rng = np.random.default_rng(12)
    assert abs(g.mass().sum() - 1000.0 * (0.1 * (n - 1)) ** 3) <= 1e-6 * 1000.0 * (0.1 * (n - 1)) ** 3
    g.set_uniform_force(1, -10000.0)
    K, rhs = g.system()
    x, y = rng.normal(size=g.r), rng.normal(size=g.r)
    Ax, Ay = g.spmv(x), g.spmv(y)
    assert np.abs(g.spmv(2.0 * x - 3.0 * y) - (2.0 * Ax - 3.0 * Ay)).max() <= 1e-12 * np.abs(Ax).max()
    assert abs(y @ Ax - x @ Ay) <= 1e-12 * abs(y @ Ax)
    assert np.array_equal(Ax[fixed], x[fixed])
    it, dv = g.pcg(rhs, eps=1e-6, max_iter=10000)
    assert 1500 < it < 5000
    res = rhs - g.spmv(dv)
    bptr, bcol = g.pattern()
    diag = np.empty(g.r)
    isdiag = bcol == np.repeat(np.arange(len(v)), np.diff(bptr))
    diag.reshape(-1, 3)[:] = np.stack([K[isdiag][:, k, k] for k in range(3)], 1)
    assert (res * res / diag).sum() <= 1.5e-12 * (rhs * rhs / diag).sum()
    assert not dv[fixed].any()
    # and the step itself (rebuild + assembly + PCG + state update) agrees with that solve
    g.rebuild_elements()
    its = g.do_timestep()
    assert abs(its - it) <= max(3, 0.02 * it)
    q, qv, _ = g.get_q_state()
    assert np.abs(qv - dv).max() <= 1e-6 * np.abs(dv).max()     # q_vel = 0 + dv from rest
    g.close()


def test_device_is_an_mi355x(gpu):
    import ctypes as C
    L = fl.lib()
    name, arch, ncu = C.create_string_buffer(128), C.create_string_buffer(64), C.c_int(0)
    fl.check(L.fb_device_info(0, name, 128, arch, 64, C.byref(ncu)))
    assert arch.value.decode().startswith("gfx950") and ncu.value == 256, (name.value, arch.value, ncu.value)


def test_inverted_and_strongly_rotated_elements(gpu):
    """a3/a4 edge cases: elements turned inside out (det F < 0: the reference flips the polar factors,
    corotationalLinearFEM.cpp:270-283) and a rigid rotation by 170 degrees (R far from I, zero elastic force)."""
    n = 4
    v, t, fixed = _cube(n)
    o = OrcFem(v, t)
    g = FemIntegrator(v, t, fixed, matrix_precision=fl.FB_MATRIX_F64)
    conv = _oracle_bsr(o)
    # push one interior node through the opposite faces of the tets around it
    u = np.zeros(o.r)
    node = (1 * n + 1) * n + 1
    u[3 * node:3 * node + 3] = [0.25, 0.22, 0.27]
    x = v + u.reshape(-1, 3)
    vol = np.einsum("ij,ij->i", x[t[:, 1]] - x[t[:, 0]], np.cross(x[t[:, 2]] - x[t[:, 0]], x[t[:, 3]] - x[t[:, 0]]))
    vol0 = np.einsum("ij,ij->i", v[t[:, 1]] - v[t[:, 0]], np.cross(v[t[:, 2]] - v[t[:, 0]], v[t[:, 3]] - v[t[:, 0]]))
    assert (np.sign(vol) != np.sign(vol0)).sum() >= 3   # several inverted elements
    fo, Ko = o.assemble(u)
    fg, Kg = g.assemble(u)
    assert np.abs(Kg - conv(Ko)).max() <= 1e-9 * np.abs(Ko).max()
    assert np.abs(fg - fo).max() <= 1e-9 * np.abs(fo).max()
    # rigid rotation about the cube centre: internal forces vanish, K = R K0 R^T block-wise
    a = np.deg2rad(170.0)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    c = v.mean(0)
    u = ((v - c) @ R.T + c - v).reshape(-1)
    fo, Ko = o.assemble(u)
    fg, Kg = g.assemble(u)
    assert np.abs(fg).max() <= 1e-6 * np.abs(Ko).max() * 0.1 and np.abs(fo).max() <= 1e-6 * np.abs(Ko).max() * 0.1
    assert np.abs(Kg - conv(Ko)).max() <= 1e-9 * np.abs(Ko).max()
    _, K0 = o.assemble(np.zeros(o.r))
    K0 = conv(K0)
    assert np.abs(Kg - np.einsum("ab,kbc,dc->kad", R, K0, R)).max() <= 1e-8 * np.abs(K0).max()


def test_every_dof_constrained_and_degenerate_input(gpu):
    v, t, _ = _cube(3)
    allfixed = np.arange(3 * len(v), dtype=np.int32)
    g = FemIntegrator(v, t, allfixed)
    g.set_uniform_force(1, -1000.0)
    it = g.do_timestep()                      # nothing to solve: x = 0 at once
    q, qv, _ = g.get_q_state()
    assert it >= 0 and not q.any() and not qv.any()
    with pytest.raises(fl.FbError):
        FemIntegrator(v, np.array([[0, 1, 2, 2]], np.int32), [])           # repeated vertex: zero volume
    flat = v.copy()
    flat[:, 2] = 0.0
    with pytest.raises(fl.FbError):
        FemIntegrator(flat, t, [])                                         # all elements flat


def test_config2_blobtree_model_100k_tets_end_to_end(gpu):
    """BASELINE config 2 on a reference model (no brain BlobTree exists; ventricle.blob, 17 primitives, stands in):
    field sweep -> tetrahedral polygonizer at the cellsize that gives 100k +- 10 % tets (0.115 -> 107,820) -> FEM handle
    on that welded mesh, lowest 5 % of the nodes in y clamped, reference gravity, one step.  Tet mesh bit-exact against the
    oracle; displacements within the stated fp32-matrix tolerance; PCG iteration count within 2 %."""
    import os
    from fembrain_amd.blobtree import read_blob
    from fembrain_amd.poly import GpuPoly
    from oracle.pyfield import OrcPoly
    blob = read_blob(os.path.join(os.path.dirname(__file__), "golden", "blob", "ventricle.blob"))
    xyz, tets = GpuPoly(blob).run_tetrahedralizer(0.115)
    oxyz, otets, _ = OrcPoly(blob).run_tetrahedralizer(0.115)
    assert 90000 <= len(tets) <= 110000
    assert np.array_equal(tets, otets) and np.abs(xyz - oxyz).max() <= 1e-6
    v, t = xyz.astype(np.float64), tets.astype(np.int32)
    ycut = np.sort(v[:, 1])[len(v) // 20]
    fixed = fixed_vertices_to_dofs(np.nonzero(v[:, 1] <= ycut)[0])
    o = OrcFem(v, t)
    o.integrator(fixed)
    g = FemIntegrator(v, t, fixed)
    f = np.zeros(o.r)
    f[1::3] = -10000.0
    o.set_external_forces(f)
    g.set_external_forces(f)
    io, ig = abs(o.step()), g.do_timestep()
    qo, _ = o.get_state()
    qg, _, _ = g.get_q_state()
    assert abs(io - ig) <= max(3, 0.02 * io), (io, ig)
    assert np.abs(qg - qo).max() <= 2e-4 * np.abs(qo).max()


def _random_delaunay():
    """400 random points, Delaunay tetrahedra in both orientations as scipy returns them (slivers below 1e-7 volume dropped)"""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(42)
    pts = rng.uniform(0, 1, size=(400, 3))
    t = Delaunay(pts).simplices.astype(np.int32)
    vol = np.einsum("ij,ij->i", pts[t[:, 1]] - pts[t[:, 0]], np.cross(pts[t[:, 2]] - pts[t[:, 0]], pts[t[:, 3]] - pts[t[:, 0]])) / 6
    t = np.ascontiguousarray(t[np.abs(vol) > 1e-7])
    assert len(t) > 1500 and (vol > 0).any() and (vol < 0).any()
    return pts, t, fixed_vertices_to_dofs(np.nonzero(pts[:, 0] < 0.1)[0]), rng


def test_random_delaunay_mesh(gpu):
    """An unstructured mesh with no grid regularity at all: Delaunay tetrahedra of random points (slivers below 1e-7 volume
    dropped), mixed orientations as scipy returns them, irregular valences (row lengths 5..40).  Pattern bit-exact, warped
    assembly to the fp64 tolerance, two steps against the oracle."""
    pts, t, fixed, rng = _random_delaunay()
    o = OrcFem(pts, t)
    o.integrator(fixed)
    g = FemIntegrator(pts, t, fixed, matrix_precision=fl.FB_MATRIX_F64)
    obptr, obcol = o.blocks()
    bptr, bcol = g.pattern()
    assert np.array_equal(bptr, obptr) and np.array_equal(bcol, obcol)
    u = rng.normal(size=o.r) * 0.003
    fo, Ko = o.assemble(u)
    fg, Kg = g.assemble(u)
    assert np.abs(Kg - _oracle_bsr(o)(Ko)).max() <= 1e-9 * np.abs(Ko).max()
    assert np.abs(fg - fo).max() <= 1e-9 * np.abs(fo).max()
    f = np.zeros(o.r)
    f[1::3] = -200.0
    for _ in range(2):
        o.set_external_forces(f)
        g.set_external_forces(f)
        io, ig = abs(o.step()), g.do_timestep()
        assert abs(io - ig) <= max(3, 0.02 * io), (io, ig)
    qo, vo = o.get_state()
    qg, vg, _ = g.get_q_state()
    assert np.abs(qg - qo).max() <= 2e-5 * np.abs(qo).max()
    assert np.abs(vg - vo).max() <= 2e-4 * np.abs(vo).max()


def test_internal_force_scaling_factor(gpu):
    """IntegratorBase::SetInternalForceScalingFactor: f_int and K times s == a body of Young's modulus s E."""
    v, t, fixed = _cube(5)
    rng = np.random.default_rng(2)
    u = rng.normal(size=3 * len(v)) * 0.004
    g = FemIntegrator(v, t, fixed, matrix_precision=fl.FB_MATRIX_F64)
    f1, K1 = g.assemble(u)
    g.set_internal_force_scaling_factor(0.25)
    f2, K2 = g.assemble(u)
    assert np.abs(f2 - 0.25 * f1).max() <= 1e-12 * np.abs(f1).max() and np.abs(K2 - 0.25 * K1).max() <= 1e-12 * np.abs(K1).max()
    soft = FemIntegrator(v, t, fixed, matrix_precision=fl.FB_MATRIX_F64, E=0.25e7)
    for h in (g, soft):
        h.set_uniform_force(1, -500.0)
        h.do_timestep()
    assert np.abs(g.get_q_state()[0] - soft.get_q_state()[0]).max() <= 1e-9 * np.abs(soft.get_q_state()[0]).max()
    with pytest.raises(fl.FbError):
        g.set_internal_force_scaling_factor(0.0)


def test_nontemporal_value_stream_gives_identical_iterates(gpu, monkeypatch):
    """k_spmv<.., NT> (picked by size for systems beyond the Infinity Cache; forced here through FEMBRAIN_SPMV_NT) only
    changes the cache policy of the matrix loads: states after 2 steps are bitwise those of the default kernel."""
    v, t, fixed = _cube(12)
    out = []
    for nt in ("0", "1"):
        monkeypatch.setenv("FEMBRAIN_SPMV_NT", nt)
        g = FemIntegrator(v, t, fixed, spmv_kernel=fl.FB_SPMV_ROWS)
        its = []
        for _ in range(2):
            g.set_uniform_force(1, -10000.0)
            its.append(g.do_timestep())
        q, qv, _ = g.get_q_state()
        out.append((its, q, qv))
        g.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


@pytest.mark.parametrize("prec,tol", [(fl.FB_MATRIX_F64, 1e-10), (fl.FB_MATRIX_F32, 5e-7)])
def test_linear_elasticity_mode(gpu, prec, tol):
    """fb_fem_params.linear = warp 0 of the reference's force model (corotationalLinearFEM.cpp:429-453): K = K0 whatever
    the displacement, f = K0 u; assembled values and two steps against the oracle (pinned for this mode by
    tests/golden/fem_cube5_linear.npz, vectors of the reference build) and against those vectors directly"""
    g5 = np.load(os.path.join(os.path.dirname(__file__), "golden", "fem_cube5_linear.npz"))
    n = int(g5["n"])
    v, t, fixed = _cube(n)
    o = OrcFem(v, t)
    o.set_linear(True)
    g = FemIntegrator(v, t, fixed, matrix_precision=prec, linear=True)
    conv = _oracle_bsr(o)
    fg, Kg = g.assemble(g5["u"])
    assert np.abs(fg - g5["f"]).max() <= 1e-9 * np.abs(g5["f"]).max()
    Kref = conv(g5["K"])
    assert np.abs(Kg - Kref).max() <= tol * np.abs(Kref).max()
    # a large rigid-looking displacement changes nothing in K (no rotation extraction in this mode)
    big = np.tile([0.3, -0.2, 0.1], len(v)) + 0.5 * np.cross(v, [0.0, 0.0, 1.0]).reshape(-1)
    _, K2 = g.assemble(big)
    assert np.array_equal(K2, Kg)
    o.integrator(fixed)
    fext = np.zeros(o.r)
    fext[1::3] = -10.0
    for k in range(2):
        o.set_external_forces(fext)
        g.set_external_forces(fext)
        io, ig = abs(o.step()), g.do_timestep()
        qg = g.get_q_state()[0]
        assert abs(ig - io) <= 3 and abs(ig - g5["it"][k]) <= 3
        assert np.abs(qg - g5["q"][k]).max() <= (2e-5 if prec == fl.FB_MATRIX_F64 else 2e-4) * np.abs(g5["q"][k]).max()


def _device_plan(g, name):
    L = fl.lib()
    n = L.fb_fem_device_plan_get(g.h, name.encode(), None, 0)
    assert n >= 0, (name, L.fb_last_error())
    a = np.zeros(n, np.int32)
    assert L.fb_fem_device_plan_get(g.h, name.encode(), fl.iptr(a), n) == n
    return a


def _host_plan(v, t, fixed):
    import ctypes as C
    L = fl.lib()
    h = C.c_void_p()
    tt = np.ascontiguousarray(t, np.int32).reshape(-1)
    fd = np.ascontiguousarray(fixed, np.int32)
    fl.check(L.fb_plan_create(C.byref(h), len(v), len(t), fl.iptr(tt), len(fd), fl.iptr(fd), 1, 0, None))

    def get(name):
        cnt = L.fb_plan_get(h, name.encode(), None, 0)
        a = np.zeros(cnt, np.int32)
        assert L.fb_plan_get(h, name.encode(), fl.iptr(a), cnt) == cnt
        return a
    return get, (L, h)


@pytest.mark.parametrize("mesh", ["cube7", "cube20", "delaunay", "isolated"])
def test_device_plan_equals_host_plan(gpu, mesh):
    """plan_device.hip (radix sort of the 16 vertex pairs of every tet, run-length encoding, SELL-64 layout, contribution
    lists) against fem_plan.cpp, array by array, bit for bit"""
    if mesh.startswith("cube"):
        n = int(mesh[4:])
        v, t, fixed = _cube(n)
    else:
        from scipy.spatial import Delaunay
        rng = np.random.default_rng(3)
        v = rng.uniform(0, 1, size=(3000, 3))
        t = Delaunay(v).simplices.astype(np.int32)
        vol = np.einsum("ij,ij->i", v[t[:, 1]] - v[t[:, 0]], np.cross(v[t[:, 2]] - v[t[:, 0]], v[t[:, 3]] - v[t[:, 0]])) / 6
        t = np.ascontiguousarray(t[np.abs(vol) > 1e-9])
        rng.shuffle(t)   # element order is part of the contribution lists
        fixed = fixed_vertices_to_dofs(np.nonzero(v[:, 0] < 0.1)[0])
        if mesh == "isolated":   # nodes no element references (identity rows), in the middle and at the end
            v = np.concatenate([v[:1500], rng.uniform(2, 3, size=(70, 3)), v[1500:], rng.uniform(2, 3, size=(5, 3))])
            t = np.where(t >= 1500, t + 70, t).astype(np.int32)
            fixed = fixed_vertices_to_dofs(np.nonzero(v[:, 0] < 0.1)[0])
    g = FemIntegrator(v, t, fixed)
    assert fl.lib().fb_fem_plan_on_device(g.h) == 1
    get, (L, hp) = _host_plan(v, t, fixed)
    for name in ("bptr", "bcol", "blk_slot", "slice_off", "colidx", "slot_coff", "slot_ccnt", "contrib"):
        assert np.array_equal(_device_plan(g, name), get(name)), name
    bptr, bcol = g.pattern()   # fetched from the device on demand
    assert np.array_equal(bptr, get("bptr")) and np.array_equal(bcol, get("bcol"))
    L.fb_plan_destroy(hp)
    # and a handle on the host plan gives the same step, bit for bit
    f = np.zeros(g.r)
    f[1::3] = -50.0
    g.set_external_forces(f)
    it = g.do_timestep()
    os.environ["FEMBRAIN_PLAN_DEVICE"] = "0"
    try:
        g2 = FemIntegrator(v, t, fixed)
    finally:
        del os.environ["FEMBRAIN_PLAN_DEVICE"]
    assert fl.lib().fb_fem_plan_on_device(g2.h) == 0
    g2.set_external_forces(f)
    assert g2.do_timestep() == it > 0
    assert np.array_equal(g2.get_q_state()[0], g.get_q_state()[0])
    # a re-sync (Deformable::syncForceModel) with fewer elements goes through the device builder again
    g.resync(v, t[: len(t) // 2], fixed)
    get, (L, hp) = _host_plan(v, t[: len(t) // 2], fixed)
    for name in ("bptr", "bcol", "slice_off", "colidx", "contrib"):
        assert np.array_equal(_device_plan(g, name), get(name)), name
    L.fb_plan_destroy(hp)


def test_fem_handle_straight_from_the_polygonizer(gpu):
    """fb_fem_create_from_poly: field grid -> tets -> FEM without a host copy.  Same plan, same steps (bit for bit) as
    fb_fem_create on the arrays fb_poly_read_tetmesh returns."""
    from fembrain_amd.blobtree import read_blob
    from fembrain_amd.poly import GpuPoly
    blob = read_blob(os.path.join(os.path.dirname(__file__), "golden", "blob", "tumor.blob"))
    p = GpuPoly(blob)
    xyz, tets = p.run_tetrahedralizer(0.11)
    assert len(tets) > 3000
    fixed = fixed_vertices_to_dofs(np.nonzero(xyz[:, 1] < np.percentile(xyz[:, 1], 10))[0])
    a = FemIntegrator.from_poly(p, fixed)
    b = FemIntegrator(xyz.astype(np.float64), tets.astype(np.int32), fixed)
    assert fl.lib().fb_fem_plan_on_device(a.h) == 1
    for name in ("bptr", "bcol", "slice_off", "colidx", "contrib"):
        assert np.array_equal(_device_plan(a, name), _device_plan(b, name)), name
    for g in (a, b):
        g.set_uniform_force(1, -50.0)
    for _ in range(2):
        assert a.do_timestep() == b.do_timestep()
    assert np.array_equal(a.get_q_state()[0], b.get_q_state()[0])
    p.close()   # the FEM handle owns its copy of the mesh
    a.set_uniform_force(1, -50.0)
    assert a.do_timestep() > 0
    # a polygonizer without a tet mesh is refused
    q = GpuPoly(blob)
    with pytest.raises(fl.FbError):
        FemIntegrator.from_poly.__func__(FemIntegrator, _NoMesh(q))


class _NoMesh:
    """a GpuPoly stand-in whose read_tetmesh would fail: from_poly must fail in the C call, not earlier"""
    def __init__(self, poly):
        self.h = poly.h

    def read_tetmesh(self):
        return np.zeros((4, 3), np.float32), np.zeros((1, 4), np.uint32)


def _wide_mesh():
    """a hub node shared by 40 tets: one row of more than 32 blocks"""
    rng = np.random.default_rng(3)
    pts = rng.normal(size=(60, 3))
    pts /= np.linalg.norm(pts, axis=1)[:, None]
    from scipy.spatial import ConvexHull
    hull = ConvexHull(pts)
    v = np.concatenate([[[0.0, 0.0, 0.0]], pts])
    t = np.array([[0, a + 1, b + 1, c + 1] for a, b, c in hull.simplices], np.int32)
    # ... next to an ordinary body (a 7^3 cube, separate): slices of ordinary width beside the one that is too wide for the element-major
    # kernel, which then takes all but that one (round 5; alone, the star is one slice and the slot-major kernel's)
    vc, tc, fc = _cube(7)
    vv = np.concatenate([v + np.array([5.0, 0.0, 0.0]), vc])
    tt = np.concatenate([t, tc + len(v)]).astype(np.int32)
    return vv, np.ascontiguousarray(tt), np.sort(np.concatenate([fixed_vertices_to_dofs(np.array([1, 2, 3])), fc + 3 * len(v)])).astype(np.int32)


def _jittered_lattice():
    """Delaunay tetrahedra of a 9^3 lattice with jittered points: irregular valences, longest block row 29 (slices of 16..29
    slots: the element-major kernel with one workgroup per CU)"""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(1)
    n = 9
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(float)
    pts = (g + rng.uniform(-0.3, 0.3, size=g.shape)) * 0.1
    t = Delaunay(pts).simplices.astype(np.int32)
    vol = np.einsum("ij,ij->i", pts[t[:, 1]] - pts[t[:, 0]], np.cross(pts[t[:, 2]] - pts[t[:, 0]], pts[t[:, 3]] - pts[t[:, 0]])) / 6
    t = np.ascontiguousarray(t[np.abs(vol) > 1e-10])
    return pts, t, fixed_vertices_to_dofs(np.nonzero(g[:, 0] == 0)[0])


@pytest.mark.parametrize("case", ["cube14", "cube14_f64", "cube14_tangent", "cube14_newmark", "cube14_block_jacobi", "beam3", "jitter", "jitter_f64", "hub",
                                  "hub_f64", "hub_tangent", "hub_newmark", "hub_newmark3", "hub_block_jacobi", "hub_delaunay", "hub_delaunay_three_workgroups"])
def test_element_major_assembly_writes_the_bits_of_the_slot_major_kernel(gpu, monkeypatch, case):
    """k_assemble_tets_st / k_assemble_tets (lane walks its row's elements, blocks accumulated in LDS) against k_assemble_rows (FEMBRAIN_ASM_KERNEL=rows):
    raw f and K at a seeded displacement, Keff and rhs of a step, the states after two steps -- all bit for bit, for both matrix
    widths, the exact tangent, the Newmark step and the block-Jacobi inverse blocks; a mesh with a row wider than 32 slots keeps the
    slot-major kernel by itself.  hub*: the slices wider than 31 slots go through k_assemble_wide (a workgroup per slice, slots dealt to its
    wavefronts, the running sums by one of them) -- the same bits again, also when one workgroup takes all of them in turn"""
    kw = {}
    hub = case.startswith("hub")
    if case == "hub_delaunay_three_workgroups":
        monkeypatch.setenv("FEMBRAIN_ASM_WIDE_GRID", "3")
    if case == "beam3":
        g0 = np.load(os.path.join(GOLD, "fem_beam3.npz"))
        v, t, fixed = g0["verts"], g0["tets"], fixed_vertices_to_dofs(g0["fixed_vertices"])
    elif hub:
        v, t, fixed = _delaunay_lattice(12) if "delaunay" in case else _wide_mesh()       # (delaunay: dozens of hull slices of 32..60 slots)
        if case.endswith("f64"):
            kw["matrix_precision"] = fl.FB_MATRIX_F64
        if case.endswith("tangent"):
            kw["exact_tangent"] = True
        if case.endswith("newmark") or case.endswith("newmark3"):
            kw["integrator"] = fl.FB_INTEGRATOR_NEWMARK
        if case.endswith("block_jacobi"):
            kw["pcg_variant"] = fl.FB_PCG_BLOCK_JACOBI
    elif case.startswith("jitter"):
        v, t, fixed = _jittered_lattice()
        if case.endswith("f64"):
            kw["matrix_precision"] = fl.FB_MATRIX_F64
    else:
        v, t, fixed = _cube(14)
        if case.endswith("f64"):
            kw["matrix_precision"] = fl.FB_MATRIX_F64
        if case.endswith("tangent"):
            kw["exact_tangent"] = True
        if case.endswith("newmark"):
            kw["integrator"] = fl.FB_INTEGRATOR_NEWMARK
        if case.endswith("block_jacobi"):
            kw["pcg_variant"] = fl.FB_PCG_BLOCK_JACOBI
    u = np.random.default_rng(5).normal(size=3 * len(v)) * 0.003
    out = []
    # "tets": the default -- k_assemble_tets_st (2: records staged in LDS by one wavefront, mass entries from k_mass_blocks) for fp32
    # records and the plain tangent, else k_assemble_tets (1); "tets1": k_assemble_tets; "rows": k_assemble_rows (0)
    staged = not case.endswith("f64") and not case.endswith("tangent")
    kw.setdefault("matrix_precision", fl.FB_MATRIX_F32)       # (the fp32 kernels are the subject; FB_MATRIX_AUTO would store these small meshes as fp64)
    for kern in ("tets", "tets1", "rows"):
        monkeypatch.setenv("FEMBRAIN_ASM_KERNEL", kern)
        g = FemIntegrator(v, t, fixed, **kw)
        # (a hub node makes ONE slice too wide for the element-major kernel: that slice alone goes through the slot-major kernel, round 5)
        assert fl.lib().fb_fem_assembly_kernel(g.h) == (0 if kern == "rows" else (2 if kern == "tets" and staged else 1))
        assert (fl.lib().fb_fem_assembly_wide_slices(g.h) > 0) == (hub and kern != "rows")
        if case.endswith("newmark3"):    # (several Newton iterations: every kernel also leaves the residual of ALL DOFs for the error quotient)
            g.set_newmark(0.25, 0.5, 3, 0.5)
        f, K = g.assemble(u)
        its = []
        for k in range(2):
            if k:
                g.rebuild_elements()     # (the rest data again: the mass entries are formed again with it)
            g.set_uniform_force(1, -2000.0 if not hub and case not in ("jitter", "jitter_f64") else -1.0)
            its.append(g.do_timestep())
            its.append(g.last.newton_iterations)
        Keff, rhs = g.system()
        out.append((f, K, its, Keff, rhs, g.get_q_state()[0], g.mass()))
        g.close()
    b = out[2]
    for a in out[:2]:
        assert a[2] == b[2]
        for x, y in zip(a, b):
            if not isinstance(x, list):
                assert np.array_equal(x, y)
    assert np.abs(b[1]).max() > 0 and np.abs(b[5]).max() > 0


def test_16bit_column_differences_give_identical_iterates(gpu, monkeypatch):
    """k_spmv<.., C16> reads column - row as 16-bit values (device-built plans whose differences all fit); the products are
    the same, so are the states -- bit for bit against the 32-bit index kernel (FEMBRAIN_SPMV_C16=0); a mesh whose node
    numbering makes a difference too wide falls back by itself"""
    v, t, fixed = _cube(14)
    out = []
    for c16 in ("1", "0"):
        monkeypatch.setenv("FEMBRAIN_SPMV_C16", c16)
        g = FemIntegrator(v, t, fixed, spmv_kernel=fl.FB_SPMV_ROWS, matrix_precision=fl.FB_MATRIX_F32)
        its = []
        for _ in range(2):
            g.set_uniform_force(1, -10000.0)
            its.append(g.do_timestep())
        out.append((its, g.get_q_state()[0], g.spmv_bytes()))
        g.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])
    assert out[0][2] < out[1][2]    # 2 bytes less per block in the 16-bit form
    monkeypatch.delenv("FEMBRAIN_SPMV_C16")
    # 40,000 isolated nodes between two halves of the numbering: differences beyond 16 bits -> 32-bit kernel, same answer
    half = len(v) // 2
    pad = np.random.default_rng(1).uniform(5, 6, size=(40000, 3))
    v2 = np.concatenate([v[:half], pad, v[half:]])
    t2 = np.where(t >= half, t + 40000, t).astype(np.int32)
    fixed2 = fixed_vertices_to_dofs(np.nonzero(v2[:, 0] < v[:, 0].min() + 1e-9)[0])
    g2 = FemIntegrator(v2, t2, fixed2, spmv_kernel=fl.FB_SPMV_ROWS, matrix_precision=fl.FB_MATRIX_F32, renumber=fl.FB_RENUMBER_OFF)

    def index_bytes(g):
        n, nb = g.n_nodes, g.num_blocks()
        return (g.spmv_bytes() - (n + 1) * 4 - 24 * n - 96 * n) / nb - 36

    assert index_bytes(g2) == 4.0
    # (round 4) left to itself the handle renumbers such a mesh (fembrain_amd/csrc/renumber.h) and the differences fit again
    g4 = FemIntegrator(v2, t2, fixed2, spmv_kernel=fl.FB_SPMV_ROWS, matrix_precision=fl.FB_MATRIX_F32)
    assert g4.renumbering()[0] and index_bytes(g4) == 2.0
    g4.close()
    g3 = FemIntegrator(v, t, fixed, spmv_kernel=fl.FB_SPMV_ROWS, matrix_precision=fl.FB_MATRIX_F32)
    assert index_bytes(g3) == 2.0
    g2.set_uniform_force(1, -1000.0)
    assert g2.do_timestep() > 0
    q2 = g2.get_q_state()[0].reshape(-1, 3)
    assert np.isfinite(q2).all() and np.abs(q2[:half]).max() > 0


def test_resync_through_meshes_of_different_sizes(gpu):
    """Deformable::syncForceModel on one handle through meshes that grow and shrink (the plan builder's workspace is reused):
    after every re-sync the handle steps exactly like a fresh one"""
    meshes = [_cube(8), _cube(13), _cube(5), _cube(10)]
    v0, t0, f0 = meshes[0]
    g = FemIntegrator(v0, t0, f0)
    for v, t, fixed in meshes[1:] + meshes[:2]:
        g.resync(v, t, fixed)
        fresh = FemIntegrator(v, t, fixed)
        for h in (g, fresh):
            h.set_uniform_force(1, -3000.0)
        assert g.do_timestep() == fresh.do_timestep()
        assert np.array_equal(g.get_q_state()[0], fresh.get_q_state()[0])
        fresh.close()


def test_failed_resync_poisons_the_handle_until_a_good_one(gpu):
    """a re-sync that fails half way (node id out of range after a bad subdivision; a flat element) must not leave a handle
    that steps over buffers of two meshes: every call returns an error until a valid re-sync recovers it"""
    v, t, fixed = _cube(6)
    g = FemIntegrator(v, t, fixed)
    g.set_uniform_force(1, -3000.0)
    g.do_timestep()
    v2, t2, fixed2 = _cube(9)
    bad = t2.copy()
    bad[17, 2] = len(v2) + 5                      # out of range
    with pytest.raises(fl.FbError, match="outside"):
        g.resync(v2, bad, fixed2)
    for call in (g.do_timestep, g.rebuild_elements, lambda: g.set_uniform_force(1, -1.0), g.get_q_state):
        with pytest.raises(fl.FbError, match="unusable after a failed"):
            call()
    flat = v2.copy()
    flat[t2[3]] = flat[t2[3, 0]]                  # a degenerate element
    with pytest.raises(fl.FbError, match="rest volume"):
        g.resync(flat, t2, fixed2)
    with pytest.raises(fl.FbError, match="unusable after a failed"):
        g.do_timestep()
    g.resync(v2, t2, fixed2)                      # recovery
    fresh = FemIntegrator(v2, t2, fixed2)
    for h in (g, fresh):
        h.set_uniform_force(1, -3000.0)
    assert g.do_timestep() == fresh.do_timestep()
    assert np.array_equal(g.get_q_state()[0], fresh.get_q_state()[0])


# ---- the persistent pipelined solver (pcg_pipe.hip.h): every instantiation the dispatch can select ------------------------------
# k_pcg_pipe<float, c16 | c32, (8, 8) | (12, 6)>: 16- or 32-bit column words; up to 8 slices per CU with up to 8 LDS-resident slots per
# slice, 9..12 with up to 6 (the CU's 60 wavefront-slots dealt to the workgroup's slices); k_pcg_pipe2<c16 | c32> for 13..24.  Each is checked against the oracle or a reference-built golden (fem_cube56_step1.npz / fem_cube58_step1.npz: the
# reference's own CorotationalLinearFEM + CGSolver, tests/golden/make_fem_golden.py) AND against the two-launch solver of the same
# library; fb_fem_pcg_path says which kernel ran.
def _two_launch(monkeypatch, *a, **kw):
    kw.setdefault("matrix_precision", fl.FB_MATRIX_F32)   # (the partner of a persistent handle, whose values are fp32; FB_MATRIX_AUTO would store a small mesh as fp64)
    monkeypatch.setenv("FEMBRAIN_PCG_PERSIST", "0")
    g = FemIntegrator(*a, **kw)
    monkeypatch.delenv("FEMBRAIN_PCG_PERSIST")
    assert not g.persist_info()[0] and g.pcg_path()["kernel"] == ""
    return g


def _persistent(monkeypatch, kernel, *a, c16=True, **kw):
    monkeypatch.setenv("FEMBRAIN_PERSIST_MIN_WAVES", "1")   # (read once per process: the default starts at 4 slices per CU)
    if not c16:
        monkeypatch.setenv("FEMBRAIN_SPMV_C16", "0")
    if ",5,16" in kernel:
        monkeypatch.setenv("FEMBRAIN_PIPE_SMALL", "1")      # (opt-in: whole slices in LDS up to 4 slices per CU; measured no faster than (8, 8))
    g = FemIntegrator(*a, pcg_variant=fl.FB_PCG_PERSISTENT, **kw)
    if ",5,16" in kernel:
        monkeypatch.delenv("FEMBRAIN_PIPE_SMALL")
    if not c16:
        monkeypatch.delenv("FEMBRAIN_SPMV_C16")
    assert g.persist_info()[0] and g.pcg_path()["kernel"] == kernel, g.pcg_path()
    return g


@pytest.mark.parametrize("n,c16,kernel", [(14, True, "k_pcg_pipe<float,c16,8,8>"), (14, False, "k_pcg_pipe<float,c32,8,8>"),
                                          (26, True, "k_pcg_pipe<float,c16,8,8>"), (26, False, "k_pcg_pipe<float,c32,8,8>"),
                                          (14, True, "k_pcg_pipe<float,c16,5,16>"), (26, True, "k_pcg_pipe<float,c16,5,16>"), (26, False, "k_pcg_pipe<float,c32,5,16>")])
def test_persistent_solver_against_the_oracle(gpu, monkeypatch, n, c16, kernel):
    """One and two slices per workgroup (2,744 / 17,576 nodes): the solution of a tight solve and three reference-load steps against
    the CPU oracle (CGSolver.cpp:129-190 restated), iteration counts within max(3, 2 %)."""
    v, t, fixed = _cube(n)
    o = OrcFem(v, t)
    o.integrator(fixed)
    g = _persistent(monkeypatch, kernel, v, t, fixed, c16=c16)
    fext = np.zeros(o.r)
    fext[1::3] = -10000.0
    o.set_external_forces(fext)
    g.set_external_forces(fext)
    info, keff, rhs, dv = o.step(cg_eps=1e-8, cg_maxiter=20000, want=True)
    o.set_state(np.zeros(o.r), np.zeros(o.r))
    _, rhs_g = g.system()
    free = np.ones(o.r, bool)
    free[fixed] = False          # (the oracle removes the clamped DOFs, here they are identity rows with a zero right-hand side)
    assert np.abs(rhs_g[free] - rhs[free]).max() <= 2e-7 * np.abs(rhs).max() and not rhs_g[~free].any()
    it, xg = g.pcg(rhs_g, eps=1e-8, max_iter=20000)
    assert g.pcg_path()["path"] == fl.FB_PCG_PATH_PERSISTENT
    assert abs(it - abs(info)) <= max(3, 0.02 * abs(info)), (it, info)
    assert np.abs(xg - dv).max() <= 5e-6 * np.abs(dv).max()       # fp32-stored matrix: K entries rounded to 6e-8, cond ~ 1e2
    # a tolerance below 1e-8 is within three orders of where the pipelined recurrences stall (~1e-11): the two-launch solver takes it
    # (1e-10: the true residual b - A x, taken every 30th iteration as the reference does, has its own floor near 1e-12 at this size)
    it10, x10 = g.pcg(rhs_g, eps=1e-10, max_iter=20000)
    assert g.pcg_path()["path"] == fl.FB_PCG_PATH_TWO_LAUNCH and it10 > it and np.abs(x10 - xg).max() <= 1e-6 * np.abs(xg).max()
    for k in range(3):
        o.set_external_forces(fext)
        io, ig = abs(o.step()), g.do_timestep()
        assert abs(ig - io) <= max(3, 0.02 * io), (k, ig, io)
        qo, qg = o.get_state()[0], g.get_q_state()[0]
        assert np.abs(qg - qo).max() <= 2e-4 * np.abs(qo).max(), k
        assert g.last.pcg_path == fl.FB_PCG_PATH_PERSISTENT and g.last.persist_fallbacks == 0
    p = g.pcg_path()
    assert p["path"] == fl.FB_PCG_PATH_PERSISTENT and p["launches"] >= 4 and p["fallbacks"] == 0 and 0 < p["max_producers"] <= 64
    g.close()


@pytest.mark.parametrize("kind,m,rows", [("cube", 20, 1), ("delaunay", 16, 1), ("delaunay", 22, 1), ("cube", 20, 2), ("delaunay", 22, 2)])
def test_published_vector_node_by_node_gives_the_same_iterates(gpu, monkeypatch, kind, m, rows):
    """Round 5: on a mesh whose columns are scattered the persistent solver publishes the vector its products gather from node by node
    (x, y, z side by side: one cache line per lane and slot instead of three; k_pcg_pipe<..., XYZ>, two gathers per slot in the hand-written
    stream instead of three).  The library decides from the lines the gathers touch (fb_fem_persist_gather); forced both ways here
    (FEMBRAIN_PIPE_XYZ), helpers off (their partial sums would be cut at other slots: with the node-by-node vector a slice keeps up to 12
    slots in LDS instead of 6): the sums of a row and their order are the same, so iterations and solution are -- bit for bit, also across
    launch cuts, against the plain kernel with planes."""
    v, t, fixed = _cube(m) if kind == "cube" else _delaunay_lattice(m)
    monkeypatch.setenv("FEMBRAIN_PERSIST_MIN_WAVES", "1")
    monkeypatch.setenv("FEMBRAIN_PIPE_HELPERS", "0")
    if rows == 2:
        monkeypatch.setenv("FEMBRAIN_PERSIST_ROWS", "2")          # (the two-row kernel, k_pcg_pipe2<..., XYZ>, on a mesh far below its range)
    out = []
    for xyz in ("1", "0"):
        monkeypatch.setenv("FEMBRAIN_PIPE_XYZ", xyz)
        # (12 LDS slots of a slice is the library's choice from 6 slices per CU on; asked for here, on meshes of a slice or two per CU)
        monkeypatch.setenv("FEMBRAIN_PIPE_LDS_CAP", "12" if xyz == "1" else "6")
        g = FemIntegrator(v, t, fixed, pcg_variant=fl.FB_PCG_PERSISTENT, matrix_precision=fl.FB_MATRIX_F32)
        assert g.persist_gather()[0] == (xyz == "1") and g.persist_gather()[1] > 0
        if rows == 1:
            assert (g.persist_info()[3] > 8) == (xyz == "1"), g.persist_info()      # (these meshes have a slice or two per CU: 12 slots against 8)
        g.set_uniform_force(1, -100.0)
        _, rhs = g.system()
        it, x = g.pcg(rhs, eps=1e-6, max_iter=20000)
        assert g.pcg_path()["path"] == fl.FB_PCG_PATH_PERSISTENT and g.pcg_path()["fallbacks"] == 0 and it > 30
        assert g.pcg_path()["kernel"].startswith("k_pcg_pipe2<" if rows == 2 else "k_pcg_pipe<")
        if xyz == "1":
            for run in ("1", "7"):
                monkeypatch.setenv("FEMBRAIN_PERSIST_MAX_RUN", run)
                itc, xc = g.pcg(rhs, eps=1e-6, max_iter=20000)
                assert itc == it and np.array_equal(xc, x), run
            monkeypatch.delenv("FEMBRAIN_PERSIST_MAX_RUN")
        out.append((it, x))
        g.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("kind,m,force,minlen,even", [("cube", 14, "1", "4", True), ("cube", 26, "1", "4", True), ("cube", 26, "1", None, False), ("cube", 40, "1", None, False),
                                                      ("delaunay", 16, "1", None, True), ("delaunay", 22, None, None, True), ("delaunay", 22, None, None, False)])
def test_persistent_solver_with_helper_wavefronts(gpu, monkeypatch, kind, m, force, minlen, even):
    """Round 5: where a few slices are much wider than the rest (hull nodes of a Delaunay mesh) wavefronts without a slice of their own
    multiply the upper part of a wide slice's slots and hand the partial sums over in LDS (pcg_pipe.hip.h, PipeArgs::tasks), and the
    slices are dealt to the workgroups by slots (PipeArgs::wg_first).  The library decides from the widths (delaunay 22) or is told
    (FEMBRAIN_PIPE_HELPERS=1; on the well-conditioned cubes with streams as short as 4 slots, so that hundreds of helpers work).
    Against the same kernel WITHOUT helpers: on the cubes the SAME iteration count and the solution to 1e-10 (only the order of three
    additions per row differs); on the sliver meshes, whose pipelined recurrences answer every change of rounding with a few per cent
    of iterations, within 4 % and to the solver's tolerance.  Against ITSELF cut into launches of 1, 7 and 30 iterations: bit for bit.
    Against the two-launch solver: three steps to the parity tolerance of the step tests."""
    if kind == "cube":
        v, t, fixed = _cube(m)
        load, eps = -10000.0, 1e-8
    else:
        v, t, fixed = _delaunay_lattice(m)
        load, eps = -100.0, 1e-6
    gm = _two_launch(monkeypatch, v, t, fixed)
    monkeypatch.setenv("FEMBRAIN_PERSIST_MIN_WAVES", "1")
    if force:
        monkeypatch.setenv("FEMBRAIN_PIPE_HELPERS", force)
    if minlen:
        monkeypatch.setenv("FEMBRAIN_PIPE_HELP_MINLEN", minlen)
    if not even:
        # the LDS dealt to the slices of a workgroup by WIDTH instead of in equal shares (opt-in: measured slower, pcg_pipe_plan.h pipe_deal_lds): every
        # slice streams the same number of slots as far as the LDS goes.  The small cubes are then resident as a whole, up to 15 slots of a
        # slice where the unrolled loop takes 6, nothing is streamed and nobody helps: bit for bit the plain kernel
        monkeypatch.setenv("FEMBRAIN_PIPE_LDS_BY_WIDTH", "1")
    gp = FemIntegrator(v, t, fixed, pcg_variant=fl.FB_PCG_PERSISTENT)
    monkeypatch.delenv("FEMBRAIN_PIPE_HELP_MINLEN", raising=False)
    monkeypatch.delenv("FEMBRAIN_PIPE_LDS_BY_WIDTH", raising=False)
    monkeypatch.setenv("FEMBRAIN_PIPE_HELPERS", "0")
    g0 = FemIntegrator(v, t, fixed, pcg_variant=fl.FB_PCG_PERSISTENT)
    monkeypatch.delenv("FEMBRAIN_PIPE_HELPERS")
    L = fl.lib()
    cnt = L.fb_fem_device_plan_get(gp.h, b"slice_off", None, 0)
    so = np.zeros(cnt, np.int32)
    L.fb_fem_device_plan_get(gp.h, b"slice_off", fl.iptr(so), cnt)
    wd = np.diff(so)
    # the library's own rule where it was left to decide: widest slice wider than 24 slots and half again as wide as the average
    expect = True if force else bool(wd.max() > 24 and wd.max() >= 1.5 * wd.mean())
    n_help = L.fb_fem_persist_helpers(gp.h)
    assert L.fb_fem_persist_helpers(g0.h) == 0
    if even:
        assert (n_help > 0) == expect, (n_help, wd.max(), wd.mean(), gp.pcg_path())
    else:       # (these meshes are small: whole slices resident, more slots than the unrolled loop takes; helpers only where something is still streamed)
        assert gp.persist_info()[3] > 6 and g0.persist_info()[3] <= 8, (gp.persist_info(), g0.persist_info())
    deep = n_help == 0
    # (round 5: where the columns of a slot are scattered the published vector lies node by node -- decided from the cache lines the gathers
    # touch, sampled on the device: the Delaunay lattices yes, the cubes no; both forms give the same sums in the same order)
    xyz, lp, lr = gp.persist_gather()
    assert lp > 0 and lr > 0 and xyz == (kind == "delaunay" and lp >= 30 and lp >= 1.5 * lr), (xyz, lp, lr)
    assert not (kind == "cube" and xyz), (kind, m, xyz, lp, lr)   # (these lattices are small: 27-30 lines against 21-23, planes; the 91,125-node probe has 80 against 44)
    if expect:
        assert gp.pcg_path()["kernel"].startswith("k_pcg_pipe<float,") and gp.pcg_path()["kernel"].endswith(",12,6>")
    for g in (gm, gp, g0):
        g.set_uniform_force(1, load)
    _, rhs = gm.system()
    gp.system(); g0.system()
    itp, xp = gp.pcg(rhs, eps=eps, max_iter=20000)
    it0, x0 = g0.pcg(rhs, eps=eps, max_iter=20000)
    assert gp.pcg_path()["path"] == fl.FB_PCG_PATH_PERSISTENT and gp.pcg_path()["fallbacks"] == 0 and it0 > 30
    if deep:
        assert itp == it0 and np.array_equal(xp, x0), (itp, it0)      # (no helper: the sums of a row in the plain kernel's order)
    elif kind == "cube":
        assert itp == it0 and np.abs(xp - x0).max() <= 1e-10 * np.abs(x0).max(), (itp, it0)
    else:
        assert abs(itp - it0) <= 0.04 * it0 and np.abs(xp - x0).max() <= 2e-4 * np.abs(x0).max(), (itp, it0)
    assert not xp[fixed].any()
    for run in ("1", "7", "30"):
        monkeypatch.setenv("FEMBRAIN_PERSIST_MAX_RUN", run)
        itc, xc = gp.pcg(rhs, eps=eps, max_iter=20000)
        assert itc == itp and np.array_equal(xc, xp), run
    monkeypatch.delenv("FEMBRAIN_PERSIST_MAX_RUN")
    for g in (gm, gp):
        g.reset_to_rest()
    for k in range(3):
        its = []
        for g in (gm, gp):
            g.set_uniform_force(1, load)
            its.append(g.do_timestep())
        assert abs(its[0] - its[1]) <= max(3, (0.02 if kind == "cube" else 0.05) * its[0]), (k, its)
        qa, qb = gm.get_q_state()[0], gp.get_q_state()[0]
        assert np.abs(qa - qb).max() <= 2e-4 * np.abs(qa).max()
    for g in (gm, gp, g0):
        g.close()


@pytest.mark.parametrize("n,kname", [(14, "k_pcg_pipe<float,c16,8,8>"), (31, "k_pcg_pipe<float,c16,8,8>"), (40, "k_pcg_pipe<float,c16,8,8>"),
                                     (14, "k_pcg_pipe<float,c16,5,16>"), (31, "k_pcg_pipe<float,c16,5,16>"), (40, "k_pcg_pipe<float,c16,5,16>")])
def test_persistent_solver_matches_two_launch_and_itself(gpu, n, kname, monkeypatch):
    """The persistent solver against the two-launch solver (k_spmv + k_cg_fused, an independent code path: the handle is created
    with FEMBRAIN_PCG_PERSIST=0 and says so): same iteration counts to max(3, 2 %), same solution to the solver tolerance; and
    against ITSELF cut into launches of 1 and 7 iterations -- every state vector goes through memory at a cut, every hand-off
    around it is a kernel boundary -- bit for bit: a stale read inside the launch would show here.  Slices per workgroup: 1
    (n = 14), 2 (n = 31), 4 (n = 40), with (8, 8) and with the opt-in whole-slice-in-LDS instantiation (5, 16).
    Also the poll-all form of the neighbour wait (what an unstructured numbering gets)."""
    v, t, fixed = _cube(n)
    gm = _two_launch(monkeypatch, v, t, fixed)
    gp = _persistent(monkeypatch, kname, v, t, fixed)
    monkeypatch.setenv("FEMBRAIN_PERSIST_POLL_ALL", "1")
    ga = _persistent(monkeypatch, kname, v, t, fixed)
    monkeypatch.delenv("FEMBRAIN_PERSIST_POLL_ALL")
    assert ga.pcg_path()["max_producers"] == -1 and gp.pcg_path()["max_producers"] > 0
    for g in (gm, gp, ga):
        g.set_uniform_force(1, -10000.0)
    _, rhs = gm.system()
    gp.system(); ga.system()
    itm, xm = gm.pcg(rhs, eps=1e-8, max_iter=20000)
    itp, xp = gp.pcg(rhs, eps=1e-8, max_iter=20000)
    ita, xa = ga.pcg(rhs, eps=1e-8, max_iter=20000)
    assert gm.pcg_path()["path"] == fl.FB_PCG_PATH_TWO_LAUNCH and gp.pcg_path()["path"] == fl.FB_PCG_PATH_PERSISTENT
    assert itm > 60 and abs(itp - itm) <= max(3, 0.02 * itm), (itp, itm)
    assert np.abs(xp - xm).max() <= 1e-6 * np.abs(xm).max()
    assert ita == itp and np.array_equal(xa, xp)            # which flags are polled changes no bit
    assert not xp[fixed].any()
    for run in ("1", "7", "30", "31"):
        monkeypatch.setenv("FEMBRAIN_PERSIST_MAX_RUN", run)
        itc, xc = gp.pcg(rhs, eps=1e-8, max_iter=20000)
        assert itc == itp and np.array_equal(xc, xp), run
    monkeypatch.delenv("FEMBRAIN_PERSIST_MAX_RUN")
    for cap in (1, 29, 30, 37):
        # iteration cap (also on and next to an exact-residual iteration): -cap as the reference returns, with the iterate the launch has --
        # after ONE exact residual has confirmed what its recurrences carried (it was repeated in full by the two-launch solver)
        itl, xl = gp.pcg(rhs, eps=1e-8, max_iter=cap)
        itk, xk = gm.pcg(rhs, eps=1e-8, max_iter=cap)
        assert itl == -cap and itk == -cap and gp.pcg_path()["path"] == fl.FB_PCG_PATH_PERSISTENT, cap
        assert np.abs(xl - xk).max() <= 1e-9 * np.abs(xk).max() and not xl[fixed].any(), cap
        # ... and with the check switched off the literal recurrences have the last word (FB_PCG_PATH_RESOLVED), bit for bit
        monkeypatch.setenv("FEMBRAIN_PERSIST_CAP_CHECK", "0")
        itr, xr = gp.pcg(rhs, eps=1e-8, max_iter=cap)
        monkeypatch.delenv("FEMBRAIN_PERSIST_CAP_CHECK")
        assert itr == -cap and np.array_equal(xr, xk) and gp.pcg_path()["path"] == fl.FB_PCG_PATH_RESOLVED, cap
    itz, xz = gp.pcg(np.zeros_like(rhs), eps=1e-6, max_iter=100)
    assert itz == 0 and not xz.any()
    # full steps: three reference-load steps against the two-launch solver
    for k in range(3):
        im, ip = gm.do_timestep(), gp.do_timestep()
        assert abs(im - ip) <= max(3, 0.02 * im)
        qm, qp = gm.get_q_state()[0], gp.get_q_state()[0]
        assert np.abs(qm - qp).max() <= 2e-5 * np.abs(qm).max()
    gm.close(); gp.close(); ga.close()


def _check_against_big_golden(g, gold, tol_q=2e-4):
    g.set_uniform_force(1, -10000.0)
    it = g.do_timestep()
    q, qv, _ = g.get_q_state()
    want = int(abs(gold["iters"]))
    assert abs(it - want) <= max(3, 0.02 * want), (it, want)
    assert np.abs(q[gold["idx"]] - gold["q"]).max() <= tol_q * float(gold["q_maxabs"])
    assert np.abs(qv[gold["idx"]] - gold["qvel"]).max() <= tol_q * float(gold["qvel_maxabs"])
    assert abs(np.linalg.norm(q) - float(gold["q_norm"])) <= tol_q * float(gold["q_norm"])
    assert abs(np.linalg.norm(qv) - float(gold["qvel_norm"])) <= tol_q * float(gold["qvel_norm"])
    return it, q


@pytest.mark.parametrize("n,c16,kernel,slices_per_cu", [(56, True, "k_pcg_pipe<float,c16,12,6>", 11), (56, False, "k_pcg_pipe<float,c32,12,6>", 11),
                                                        (58, True, "k_pcg_pipe<float,c16,12,6>", 12)])
def test_default_handle_at_1M_tets_against_the_reference_built_golden(gpu, monkeypatch, n, c16, kernel, slices_per_cu):
    """BASELINE config 4 (56^3 nodes, 998,250 tets: 11 slices per CU) and the largest cube the persistent solver takes (58^3, 1.11M
    tets: 12 per CU): the DEFAULT handle -- no variant asked for -- runs the persistent kernel and reproduces the first reference-load
    step of the reference's own CorotationalLinearFEM + CGSolver (tests/golden/fem_cube5x_step1.npz): iteration count within
    max(3, 2 %), q and qvel at 2,000 seeded DOFs and their norms within 2e-4 (fp32-stored matrix, both solvers stop at 1e-6); the same
    step by the two-launch solver of this library agrees as well."""
    gold = np.load(os.path.join(GOLD, "fem_cube%d_step1.npz" % n))
    v, t, fixed = _cube(n)
    if not c16:
        monkeypatch.setenv("FEMBRAIN_SPMV_C16", "0")
    g = FemIntegrator(v, t, fixed)
    monkeypatch.delenv("FEMBRAIN_SPMV_C16", raising=False)
    on, waves, wgs, slots = g.persist_info()
    assert on and waves == slices_per_cu and wgs == 256 and slots == 5 and g.pcg_path()["kernel"] == kernel
    it, q = _check_against_big_golden(g, gold)
    p = g.pcg_path()
    assert p["path"] == fl.FB_PCG_PATH_PERSISTENT and p["launches"] == 1 and p["fallbacks"] == 0 and 0 < p["max_producers"] <= 64
    g.close()
    if c16:
        g2 = _two_launch(monkeypatch, v, t, fixed)
        it2, q2 = _check_against_big_golden(g2, gold)
        assert abs(it2 - it) <= max(3, 0.02 * it) and np.abs(q2 - q).max() <= 2e-5 * np.abs(q).max()
        g2.close()


@pytest.mark.parametrize("n,c16,kernel", [(14, True, "k_pcg_pipe2<c16>"), (26, False, "k_pcg_pipe2<c32>"), (31, True, "k_pcg_pipe2<c16>")])
def test_two_row_persistent_solver_against_the_oracle_and_itself(gpu, monkeypatch, n, c16, kernel):
    """k_pcg_pipe2 (a wavefront owns two slices, x / p / z in LDS; the form of 13..24 slices per CU) forced onto small cubes
    (FEMBRAIN_PERSIST_ROWS=2): three reference-load steps against the CPU oracle, a tight solve against the two-launch solver, and
    itself cut into launches of 1 and 7 iterations bit for bit.  n = 14: one wavefront with one row set in use; 26 / 31: two row
    sets, one or two wavefronts per workgroup."""
    v, t, fixed = _cube(n)
    o = OrcFem(v, t)
    o.integrator(fixed)
    monkeypatch.setenv("FEMBRAIN_PERSIST_ROWS", "2")
    g = _persistent(monkeypatch, kernel, v, t, fixed, c16=c16)
    monkeypatch.delenv("FEMBRAIN_PERSIST_ROWS")
    gm = _two_launch(monkeypatch, v, t, fixed)
    for h in (g, gm):
        h.set_uniform_force(1, -10000.0)
    _, rhs = gm.system()
    g.system()
    itm, xm = gm.pcg(rhs, eps=1e-8, max_iter=20000)
    itp, xp = g.pcg(rhs, eps=1e-8, max_iter=20000)
    assert g.pcg_path()["path"] == fl.FB_PCG_PATH_PERSISTENT and abs(itp - itm) <= max(3, 0.02 * itm)
    assert np.abs(xp - xm).max() <= 1e-6 * np.abs(xm).max() and not xp[fixed].any()
    for run in ("1", "7", "30"):
        monkeypatch.setenv("FEMBRAIN_PERSIST_MAX_RUN", run)
        itc, xc = g.pcg(rhs, eps=1e-8, max_iter=20000)
        assert itc == itp and np.array_equal(xc, xp), run
    monkeypatch.delenv("FEMBRAIN_PERSIST_MAX_RUN")
    itl, xl = g.pcg(rhs, eps=1e-8, max_iter=37)
    assert itl == -37 and g.pcg_path()["path"] == fl.FB_PCG_PATH_PERSISTENT   # (the capped iterate stands after one exact residual)
    itk, xk = gm.pcg(rhs, eps=1e-8, max_iter=37)
    assert itk == -37 and np.abs(xl - xk).max() <= 1e-9 * np.abs(xk).max()
    monkeypatch.setenv("FEMBRAIN_PERSIST_CAP_CHECK", "0")
    itl, xl = g.pcg(rhs, eps=1e-8, max_iter=37)
    monkeypatch.delenv("FEMBRAIN_PERSIST_CAP_CHECK")
    assert itl == -37 and g.pcg_path()["path"] == fl.FB_PCG_PATH_RESOLVED and np.array_equal(xl, xk)
    fext = np.zeros(o.r)
    fext[1::3] = -10000.0
    for k in range(3):
        o.set_external_forces(fext)
        g.set_external_forces(fext)
        io, ig = abs(o.step()), g.do_timestep()
        assert abs(ig - io) <= max(3, 0.02 * io), (k, ig, io)
        qo, qg = o.get_state()[0], g.get_q_state()[0]
        assert np.abs(qg - qo).max() <= 2e-4 * np.abs(qo).max(), k
        assert g.last.pcg_path == fl.FB_PCG_PATH_PERSISTENT
    g.close(); gm.close()


@pytest.mark.parametrize("n,c16,kernel,slices_per_cu", [(60, True, "k_pcg_pipe2<c16>", 14), (60, False, "k_pcg_pipe2<c32>", 14), (73, True, "k_pcg_pipe2<c16>", 24)])
def test_default_handle_between_1M_and_2M_tets_against_the_reference_built_golden(gpu, monkeypatch, n, c16, kernel, slices_per_cu):
    """13..24 slices per CU: 60^3 nodes (1,232,274 tets, 14 per CU) and 73^3 (2,239,488 tets, 24 per CU, the largest the persistent
    solver takes).  The DEFAULT handle runs the two-row persistent kernel and reproduces the first reference-load step of the
    reference's own CorotationalLinearFEM + CGSolver (tests/golden/fem_cube60_step1.npz / fem_cube73_step1.npz)."""
    gold = np.load(os.path.join(GOLD, "fem_cube%d_step1.npz" % n))
    v, t, fixed = _cube(n)
    if not c16:
        monkeypatch.setenv("FEMBRAIN_SPMV_C16", "0")
    g = FemIntegrator(v, t, fixed)
    monkeypatch.delenv("FEMBRAIN_SPMV_C16", raising=False)
    on, waves, wgs, slots = g.persist_info()
    # (round 5: what the vectors of the workgroup's slices leave of the 160 KB holds the first slots of every slice: 1 at 14 slices per CU, 0 at 24)
    pool = (160 * 1024 - 4416 - (slices_per_cu + 1) * 6144) // (2432 if c16 else 2560)
    assert on and waves == slices_per_cu and wgs == 256 and slots == min(4, pool // slices_per_cu) and slots == (1 if n == 60 else 0) and g.pcg_path()["kernel"] == kernel
    _check_against_big_golden(g, gold)
    p = g.pcg_path()
    assert p["path"] == fl.FB_PCG_PATH_PERSISTENT and p["launches"] == 1 and p["fallbacks"] == 0
    g.close()


@pytest.mark.parametrize("n,slices_per_cu", [(52, 9), (54, 10)])
def test_nine_and_ten_slices_per_cu_keep_seven_slots_of_a_slice_in_lds(gpu, monkeypatch, n, slices_per_cu):
    """Round 5: at 9 and 10 slices per CU the LDS has room for 7 slots of a slice, one more than the (12, 6) instantiation's loop takes;
    k_pcg_pipe<float,c16,12,7> is the same kernel with that bound (52^3: 13.6 -> 13.0 us per iteration).  The sums of a row do not depend
    on where its slots live: iterations and state bit for bit those of (12, 6) (FEMBRAIN_PIPE_KLT7=0), launch cuts included."""
    v, t, fixed = _cube(n)
    out = []
    for k7 in ("1", "0"):
        monkeypatch.setenv("FEMBRAIN_PIPE_KLT7", k7)
        g = FemIntegrator(v, t, fixed)
        on, waves, wgs, slots = g.persist_info()
        assert on and waves == slices_per_cu and g.pcg_path()["kernel"] == "k_pcg_pipe<float,c16,12,%d>" % (7 if k7 == "1" else 6)
        g.set_uniform_force(1, -10000.0)
        it = g.do_timestep()
        q = g.get_q_state()[0]
        if k7 == "1":
            g.reset_to_rest()
            monkeypatch.setenv("FEMBRAIN_PERSIST_MAX_RUN", "400")
            g.set_uniform_force(1, -10000.0)
            assert g.do_timestep() == it and np.array_equal(g.get_q_state()[0], q)
            monkeypatch.delenv("FEMBRAIN_PERSIST_MAX_RUN")
        assert g.pcg_path()["fallbacks"] == 0 and g.last.pcg_path == fl.FB_PCG_PATH_PERSISTENT
        out.append((it, q))
        g.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])


def test_persistent_solver_limits_are_refused_not_degraded(gpu, monkeypatch):
    """FB_PCG_PERSISTENT asked for explicitly where it cannot run is an error, not a silent other solver: fp64 storage, more than 24
    slices per CU.  The default (FB_PCG_MERGED) falls to the two-launch solver there and says so."""
    v, t, fixed = _cube(9)
    with pytest.raises(fl.FbError, match="FB_MATRIX_F32"):
        FemIntegrator(v, t, fixed, pcg_variant=fl.FB_PCG_PERSISTENT, matrix_precision=fl.FB_MATRIX_F64)
    with pytest.raises(fl.FbError, match="unknown pcg_variant"):
        FemIntegrator(v, t, fixed, pcg_variant=2)           # the removed FB_PCG_FUSED
    v, t, fixed = _cube(75)                                # 421,875 nodes = 6,592 slices: 26 per CU
    with pytest.raises(fl.FbError, match="slices per CU"):
        FemIntegrator(v, t, fixed, pcg_variant=fl.FB_PCG_PERSISTENT)
    g = FemIntegrator(v, t, fixed)
    assert not g.persist_info()[0]
    g.set_uniform_force(1, -10000.0)
    g.do_timestep()
    assert g.last.pcg_path == fl.FB_PCG_PATH_TWO_LAUNCH
    g.close()


@pytest.mark.parametrize("mask", ["0:128", "24:96", "5:64"])
def test_plain_store_publish_does_not_trust_the_dispatch_order(gpu, monkeypatch, mask):
    """workgroups whose consumers all share their XCD publish with plain stores (the line stays in the shared L2) -- but
    which workgroups share an XCD is only OBSERVED to follow blockIdx & 7, and a CU-masked stream deals them otherwise.  The kernel
    therefore asks the hardware (HW_REG_XCC_ID) and stores plainly only where every producer / consumer announced the same id.  With
    plain stores forced on and the stream confined to odd sets of CUs the solve must be, bit for bit, the solve with write-through
    stores only (the arithmetic is the same; a stale gather would change it)."""
    n = 30
    v, t, fixed = _cube(n)
    monkeypatch.setenv("FEMBRAIN_CU_MASK", mask)
    monkeypatch.setenv("FEMBRAIN_PERSIST_MIN_WAVES", "1")
    out = []
    for plain in ("1", "0"):
        monkeypatch.setenv("FEMBRAIN_PIPE_PLAIN_STORES", plain)
        g = FemIntegrator(v, t, fixed, pcg_variant=fl.FB_PCG_PERSISTENT)
        its = []
        for _ in range(3):
            g.set_uniform_force(1, -10000.0)
            its.append(g.do_timestep())
        assert g.pcg_path()["path"] == fl.FB_PCG_PATH_PERSISTENT and g.pcg_path()["fallbacks"] == 0
        out.append((its, g.get_q_state()[0]))
        g.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])
    monkeypatch.delenv("FEMBRAIN_CU_MASK")
    ref = _two_launch(monkeypatch, v, t, fixed)
    for _ in range(3):
        ref.set_uniform_force(1, -10000.0)
        ref.do_timestep()
    assert np.abs(out[0][1] - ref.get_q_state()[0]).max() <= 2e-5 * np.abs(ref.get_q_state()[0]).max()
    ref.close()


def test_persistent_timeout_falls_back_visibly_or_fails_strictly(gpu):
    """A wait inside the persistent launch that times out (here: FEMBRAIN_PERSIST_TIMEOUT_MS tiny, read when the handle is made;
    in production: workgroups that are not all resident).  Non-strict: the step is repeated by the two-launch solver, the result is
    the two-launch result, fb_step_info says FALLBACK and counts it, the handle stays with the two-launch solver -- and a Newmark
    step keeps its warm start.  Strict (FEMBRAIN_PERSIST_STRICT=1): FB_EDEVICE.  Re-arm (round 4): after FEMBRAIN_PERSIST_REARM clean
    two-launch solves, or at a re-sync, the persistent solver is tried again.  In subprocesses: the knobs are process-wide."""
    import subprocess
    import sys
    code = r"""
import os, sys
import numpy as np
sys.path.insert(0, %r)
from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube
mode = sys.argv[1]
L = fl.lib()
if mode == "rearm":
    os.environ["FEMBRAIN_PERSIST_REARM"] = "2"
n = 40
v, t = truth_cube(n, n, n, 0.1)
fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))
kw = dict(integrator=fl.FB_INTEGRATOR_NEWMARK) if mode == "newmark" else {}
os.environ["FEMBRAIN_PCG_PERSIST"] = "0"
ref = FemIntegrator(v, t, fixed, **kw)
del os.environ["FEMBRAIN_PCG_PERSIST"]
os.environ["FEMBRAIN_PERSIST_TIMEOUT_MS"] = "0.0001"     # 10 ticks of the 100 MHz clock: a wait that is not over at its first poll gives up
g = FemIntegrator(v, t, fixed, **kw)
assert g.persist_info()[0] and not ref.persist_info()[0]
for h in (ref, g):
    h.set_uniform_force(1, -10000.0)
if mode == "rearm":
    # round 4: the fallback is not for life.  After FEMBRAIN_PERSIST_REARM clean two-launch solves the handle launches the persistent
    # solver again (with the time-out the environment holds THEN), and a re-sync re-arms it at once.
    assert g.do_timestep() > 0 and g.last.pcg_path == fl.FB_PCG_PATH_FALLBACK and L.fb_fem_persist_rearms(g.h) == 0
    os.environ["FEMBRAIN_PERSIST_TIMEOUT_MS"] = "50"
    for k in range(2):
        g.do_timestep()
        assert g.last.pcg_path == fl.FB_PCG_PATH_TWO_LAUNCH and not g.persist_info()[0]
    ref.do_timestep(); ref.do_timestep(); ref.do_timestep()
    ir, ig = ref.do_timestep(), g.do_timestep()
    assert g.last.pcg_path == fl.FB_PCG_PATH_PERSISTENT and g.persist_info()[0] and L.fb_fem_persist_rearms(g.h) == 1, (g.last.pcg_path, g.pcg_path())
    assert abs(ir - ig) <= max(3, 0.02 * ir) and np.abs(ref.get_q_state()[0] - g.get_q_state()[0]).max() <= 2e-5 * np.abs(ref.get_q_state()[0]).max()
    assert g.last.persist_fallbacks == 1
    # a re-sync re-arms at once: time out again (tiny bound, read at the re-sync), fall back, re-sync with a sane bound
    os.environ["FEMBRAIN_PERSIST_TIMEOUT_MS"] = "0.0001"
    g.resync(v, t, fixed)
    g.set_uniform_force(1, -10000.0)
    g.do_timestep()
    assert g.last.pcg_path == fl.FB_PCG_PATH_FALLBACK and g.last.persist_fallbacks == 2
    os.environ["FEMBRAIN_PERSIST_TIMEOUT_MS"] = "50"
    g.resync(v, t, fixed)
    g.set_uniform_force(1, -10000.0)
    g.do_timestep()
    assert g.last.pcg_path == fl.FB_PCG_PATH_PERSISTENT and L.fb_fem_persist_rearms(g.h) == 1
    print("REARM-OK")
    sys.exit(0)
if mode == "strict":
    os.environ["FEMBRAIN_PERSIST_STRICT"] = "1"
    try:
        g.do_timestep()
    except fl.FbError as e:
        assert e.code == fl.FB_EDEVICE and "timed out" in str(e), e
        print("STRICT-OK")
    sys.exit(0)
its = []
for k in range(2):          # Newmark: the second step's solve starts from the first one's solution
    ir, ig = ref.do_timestep(), g.do_timestep()
    assert ir == ig, (k, ir, ig)
    assert np.array_equal(ref.get_q_state()[0], g.get_q_state()[0]), k
    its.append(ig)
    assert g.last.pcg_path == (fl.FB_PCG_PATH_FALLBACK if k == 0 else fl.FB_PCG_PATH_TWO_LAUNCH), (k, g.last.pcg_path)
    assert g.last.persist_fallbacks == 1
p = g.pcg_path()
assert p["fallbacks"] == 1 and p["kernel"] == "" and not g.persist_info()[0]
print("FALLBACK-OK", its)
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),)
    for mode in ("fallback", "newmark", "strict", "rearm"):
        r = subprocess.run([sys.executable, "-c", code, mode], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and {"strict": "STRICT-OK", "rearm": "REARM-OK"}.get(mode, "FALLBACK-OK") in r.stdout, (mode, r.stdout[-2000:], r.stderr[-2000:])
        if mode != "strict":
            assert "falls back to the two-launch iteration" in r.stderr
        if mode == "rearm":
            assert "re-armed after 2 two-launch solves" in r.stderr


# ---- exact tangent stiffness (warp = 2) and the Newmark step ---------------------------------------------------------
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("prec,tol", [(fl.FB_MATRIX_F64, 1e-10), (fl.FB_MATRIX_F32, 5e-7)])
def test_exact_tangent_assembly_matches_reference_golden_and_oracle(gpu, prec, tol):
    """warp = 2 (corotationalLinearFEM.cpp:296-428): f and K at the golden displacement against the reference build's vectors
    (tests/golden/fem_cube5_warp2.npz), then on a larger cube against the oracle; K differs from the warp = 1 stiffness."""
    gold = np.load(os.path.join(GOLD, "fem_cube5_warp2.npz"))
    for n, u, want in ((int(gold["n"]), gold["u"], (gold["f"], gold["K"])), (8, None, None)):
        v, t, fixed = _cube(n)
        o = OrcFem(v, t)
        o.set_warp(2)
        if u is None:
            u = np.random.default_rng(n).normal(size=o.r) * 0.01
            want = o.assemble(u)
        conv = _oracle_bsr(o)
        g = FemIntegrator(v, t, fixed, matrix_precision=prec, exact_tangent=True)
        fg, Kg = g.assemble(u)
        Kw = conv(want[1])
        assert np.abs(fg - want[0]).max() <= 1e-9 * np.abs(want[0]).max()
        assert np.abs(Kg - Kw).max() <= tol * np.abs(Kw).max()
        g1 = FemIntegrator(v, t, fixed, matrix_precision=prec)
        _, K1 = g1.assemble(u)
        assert np.abs(Kg - K1).max() > 1e-3 * np.abs(Kw).max()      # the rotation-derivative terms are not small
        bptr, bcol = g.pattern()
        A = bsr_to_scipy(bptr, bcol, Kg)
        assert abs(A - A.T).max() == 0                              # stored symmetric, bitwise
        g.close(); g1.close()


def test_exact_tangent_steps_match_oracle(gpu):
    n = 7
    v, t, fixed = _cube(n)
    o = OrcFem(v, t)
    o.set_warp(2)
    o.integrator(fixed)
    g = FemIntegrator(v, t, fixed, exact_tangent=True)
    fext = np.zeros(o.r)
    fext[1::3] = -100.0   # (under the reference's -10000 the cube folds over itself and the exact tangent loses definiteness:
    #                       CG iteration counts then depend on the last bit; SURVEY 8c advises a gentle load for parity)
    for k in range(3):
        o.set_external_forces(fext)
        g.set_external_forces(fext)
        io, ig = abs(o.step()), g.do_timestep()
        qo, vo = o.get_state()
        qg, vg, _ = g.get_q_state()
        assert abs(ig - io) <= max(3, 0.02 * io), (ig, io)
        assert np.abs(qg - qo).max() <= 2e-4 * np.abs(qo).max(), k
    g.close()


@pytest.mark.parametrize("prec,tol", [(fl.FB_MATRIX_F64, 2e-5), (fl.FB_MATRIX_F32, 2e-4)])
@pytest.mark.parametrize("max_newton", [1, 3])
def test_newmark_step_matches_reference_golden_and_oracle(gpu, prec, tol, max_newton):
    """ImplicitNewmarkSparse::DoTimestep (implicitNewmarkSparse.cpp:183-379; beta 1/4, gamma 1/2): q, qvel, qaccel after each of
    3 steps against tests/golden/fem_cube5_newmark.npz -- ImplicitNewmarkSparse::DoTimestep RESTATED ON REFERENCE OBJECTS (oracle/ref_harness.cpp drives the
    reference's own CorotationalLinearFEM / SparseMatrix / CGSolver; its integrator translation units need PARDISO and do not build here),
    then 3 steps of a 9^3 cube against the oracle.  PCG iteration totals within max(3, 2 %) (each solve starts from the
    previous solution, as there)."""
    gold = np.load(os.path.join(GOLD, "fem_cube5_newmark.npz"))
    for n in (int(gold["n"]), 9):
        v, t, fixed = _cube(n)
        g = FemIntegrator(v, t, fixed, matrix_precision=prec, integrator=fl.FB_INTEGRATOR_NEWMARK)
        g.set_newmark(0.25, 0.5, max_newton, 1e-6)
        o = OrcFem(v, t)
        o.integrator(fixed)
        f = np.zeros(g.r)
        f[1::3] = -10000.0
        for k in range(3):
            g.set_external_forces(f)
            o.set_external_forces(f)
            its = g.do_timestep()
            newton, pcg = o.newmark_step(max_newton=max_newton)
            q, qv, qa = g.get_q_state()
            if n == int(gold["n"]):
                want = (gold["q_%d" % max_newton][k], gold["qvel_%d" % max_newton][k], gold["qaccel_%d" % max_newton][k])
                pcg_want = int(gold["iters_%d" % max_newton][k][1])
            else:
                want = (*o.get_state(), o.get_accel())
                pcg_want = pcg
            assert abs(its - pcg_want) <= max(3 * max_newton, 0.02 * pcg_want), (n, k, its, pcg_want)
            for got, w, scale in zip((q, qv, qa), want, (1, 10, 10)):
                assert np.abs(got - w).max() <= scale * tol * np.abs(w).max(), (n, k)
            assert not q[fixed].any() and not qv[fixed].any() and not qa[fixed].any()
        g.close()


@pytest.mark.parametrize("epsilon", [0.9, 0.7, 0.5, 0.1])
def test_newmark_newton_loop_stops_where_the_reference_stops(gpu, epsilon):
    """implicitNewmarkSparse.cpp:258-274: the Newton loop ends when |qresidual|^2 / |first qresidual|^2 < epsilon^2, the sum taken over ALL r
    DOFs before RemoveRows -- the reaction forces at the clamped nodes included (VERDICT r4 "what's missing" 4: rounds 2-4 summed the free
    DOFs only and could stop an iteration early).  With a clamped face the reactions do not vanish at equilibrium, so the reference's
    quotient levels off above 0.5 and its loop runs to the cap of 8 solves at any usual epsilon (the oracle: 8, 8, 1 solves in three steps at
    0.9 and 0.7; 8, 8, 8 from 0.5 down) where the sum over the free DOFs ends it after two or three.  The same NUMBER of linear solves per
    step as the oracle, PCG totals within max(3 per solve, 2 %), and the states."""
    v, t, fixed = _cube(7)
    g = FemIntegrator(v, t, fixed, matrix_precision=fl.FB_MATRIX_F64, integrator=fl.FB_INTEGRATOR_NEWMARK)
    g.set_newmark(0.25, 0.5, 8, epsilon)
    o = OrcFem(v, t)
    o.integrator(fixed)
    f = np.zeros(g.r)
    f[1::3] = -20000.0
    for k in range(3):
        g.set_external_forces(f)
        o.set_external_forces(f)
        its = g.do_timestep()
        newton, pcg = o.newmark_step(max_newton=8, epsilon=epsilon)
        assert g.last.newton_iterations == newton, (k, g.last.newton_iterations, newton)
        assert abs(its - pcg) <= max(3 * newton, 0.02 * pcg), (k, its, pcg)
        q, qv, qa = g.get_q_state()
        for got, w, scale in zip((q, qv, qa), (*o.get_state(), o.get_accel()), (1, 10, 10)):
            assert np.abs(got - w).max() <= scale * 2e-5 * np.abs(w).max(), k
    g.close()


def test_newmark_needs_its_integrator_and_resets(gpu):
    v, t, fixed = _cube(5)
    g = FemIntegrator(v, t, fixed)
    with pytest.raises(fl.FbError, match="NEWMARK"):
        g.set_newmark()
    gn = FemIntegrator(v, t, fixed, integrator=fl.FB_INTEGRATOR_NEWMARK)
    gn.set_uniform_force(1, -10000.0)
    a = gn.do_timestep()
    q1 = gn.get_q_state()
    gn.reset_to_rest()
    assert not any(x.any() for x in gn.get_q_state())
    gn.set_uniform_force(1, -10000.0)
    assert gn.do_timestep() == a and all(np.array_equal(x, y) for x, y in zip(gn.get_q_state(), q1))


@pytest.mark.parametrize("n,renumber,kernel", [(27, fl.FB_RENUMBER_OFF, "k_pcg_pipe<float,c16,8,8,bj>"), (56, fl.FB_RENUMBER_OFF, "k_pcg_pipe<float,c16,12,6,bj>"),
                                              (30, fl.FB_RENUMBER_ON, "k_pcg_pipe<float,c16,8,8,bj>")])
def test_block_jacobi_inside_the_persistent_kernel(gpu, monkeypatch, n, renumber, kernel):
    """FB_PCG_BLOCK_JACOBI (opt-in, outside the parity claim) runs inside k_pcg_pipe<.., BJ> where the handle is eligible for the
    one-row persistent kernel: the steps agree with the two-launch block-Jacobi solver (FEMBRAIN_PCG_PERSIST=0) to the solver
    tolerance, in about the same number of iterations, fewer than Jacobi; a tight tolerance leaves the persistent kernel"""
    v, t, fixed = _cube(n)
    gp = FemIntegrator(v, t, fixed, pcg_variant=fl.FB_PCG_BLOCK_JACOBI, renumber=renumber)
    assert gp.persist_info()[0] and gp.pcg_path()["kernel"] == kernel, gp.pcg_path()
    monkeypatch.setenv("FEMBRAIN_PCG_PERSIST", "0")
    g2 = FemIntegrator(v, t, fixed, pcg_variant=fl.FB_PCG_BLOCK_JACOBI, renumber=renumber)
    monkeypatch.delenv("FEMBRAIN_PCG_PERSIST")
    assert not g2.persist_info()[0] and g2.pcg_path()["kernel"] == ""
    gj = FemIntegrator(v, t, fixed, renumber=renumber)
    for k in range(3):
        its = []
        for g in (gp, g2, gj):
            g.set_uniform_force(1, -1000.0)
            its.append(g.do_timestep())
        assert gp.last.pcg_path == fl.FB_PCG_PATH_PERSISTENT and g2.last.pcg_path == fl.FB_PCG_PATH_TWO_LAUNCH
        assert 0 < its[0] < its[2] and abs(its[0] - its[1]) <= max(3, its[1] // 20), its
        qp, q2, qj = (g.get_q_state()[0] for g in (gp, g2, gj))
        assert np.abs(qp - q2).max() <= 2e-5 * np.abs(q2).max()
        if k == 0:   # (another preconditioner stops on another norm: the trajectories part at the solver tolerance per step)
            assert np.abs(qp - qj).max() <= 1e-4 * np.abs(qj).max()
        assert not qp[fixed].any()
    _, rhs = gp.system()
    itp, xp = gp.pcg(rhs, eps=1e-8, max_iter=20000)
    assert itp > 0 and gp.pcg_path()["path"] == fl.FB_PCG_PATH_PERSISTENT
    for run in ("1", "7", "30"):                     # the solve cut into shorter launches: the same bits
        monkeypatch.setenv("FEMBRAIN_PERSIST_MAX_RUN", run)
        itc, xc = gp.pcg(rhs, eps=1e-8, max_iter=20000)
        assert itc == itp and np.array_equal(xc, xp), run
    monkeypatch.delenv("FEMBRAIN_PERSIST_MAX_RUN")
    itl, xl = gp.pcg(rhs, eps=1e-8, max_iter=17)     # the iteration cap: repeated by the two-launch block-Jacobi solver
    assert itl == -17 and gp.pcg_path()["path"] == fl.FB_PCG_PATH_RESOLVED
    it, x = gp.pcg(rhs, eps=1e-10, max_iter=20000)   # below the persistent solver's tolerance floor: the literal two-launch sequence
    assert it > 0 and gp.pcg_path()["path"] == fl.FB_PCG_PATH_TWO_LAUNCH
    res = rhs - gp.spmv(x)
    assert np.abs(res).max() <= 1e-6 * np.abs(rhs).max()
    for g in (gp, g2, gj):
        g.close()


def test_block_jacobi_option_solves_the_same_system_in_fewer_iterations(gpu):
    """FB_PCG_BLOCK_JACOBI (opt-in, not the reference's preconditioner): same solution of the same Keff to the solver tolerance,
    the constrained rows stay put, and it needs fewer iterations than Jacobi on the reference-load cantilever"""
    n = 16
    v, t, fixed = _cube(n)
    gj = FemIntegrator(v, t, fixed, pcg_variant=fl.FB_PCG_REFERENCE)
    gb = FemIntegrator(v, t, fixed, pcg_variant=fl.FB_PCG_BLOCK_JACOBI)
    for g in (gj, gb):
        g.set_uniform_force(1, -10000.0)
    _, rhs = gj.system()
    gb.system()
    itj, xj = gj.pcg(rhs, eps=1e-10, max_iter=20000)
    itb, xb = gb.pcg(rhs, eps=1e-10, max_iter=20000)
    assert 0 < itb < itj, (itb, itj)
    assert np.abs(xb - xj).max() <= 1e-7 * np.abs(xj).max()
    assert not xb[fixed].any()
    res = rhs - gb.spmv(xb)
    assert np.abs(res).max() <= 1e-6 * np.abs(rhs).max()
    for k in range(2):   # full steps agree with the Jacobi solver to the step tolerance
        ij, ib = gj.do_timestep(), gb.do_timestep()
        assert ib < ij
        assert np.abs(gb.get_q_state()[0] - gj.get_q_state()[0]).max() <= 2e-5 * np.abs(gj.get_q_state()[0]).max()
