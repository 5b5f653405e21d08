"""GPU: per-element materials (fb_fem_set_materials / fb_fem_set_element_materials) against the restatement of tests/matref.py -- the
heterogeneous system as a sum of uniform oracle terms, pinned on the CPU by tests/test_materials_ref.py.

Bounds are those of tests/test_fem_gpu.py for the uniform handle: K 1e-10 / 5e-7 of max|K| (fp64 / fp32 storage), f 1e-9, mass
1e-12 / 1e-7, Keff 1e-9 / 5e-7, rhs 1e-9 / 2e-7, dv max(50 tol, 1e-8), PCG iterations within max(3, 2 %) of orc_pcg on the restated
system, three steps 2e-5 / 2e-4 of max|q| (ten times that on qvel).  The K bound holds a second time on the block rows whose
elements all have the softest material, against the largest |K| of THOSE rows: such rows are a uniform assembly, for which the bound
is established, and a stiff region's scale cannot hide a soft region's error."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import cut_inputs as ci
import cutref as cr
import fem_params as fp
import product_inputs as pi
from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator, bsr_to_scipy
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube
from matref import MatRef, region_ids, three_materials

pytestmark = pytest.mark.gpu

MATS = three_materials()
SOFTEST = int(np.argmin([m[0] for m in MATS]))
STEP = dict(timestep=0.01, damping_mass=0.4, damping_stiffness=0.003)   # (c_M > 0: the mass terms of every assembly kernel are live)
WARPS = {"linear": dict(linear=True), "warp1": dict(), "tangent": dict(exact_tangent=True)}
WARP_NO = {"linear": 0, "warp1": 1, "tangent": 2}


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name.startswith("cube"):
        n = int(name[4:])
        v, t = truth_cube(n, n, n, 0.1)
        return v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))
    if name == "hub":   # one node of degree 100: a slice wider than the element-major kernels take (k_assemble_wide)
        v, t, fv = pi.hub(100)
        return v, t, fixed_vertices_to_dofs(fv)
    if name == "delaunay":   # a jittered lattice's Delaunay tetrahedra, node ids shuffled
        v, t, fv0 = pi.delaunay_lattice(6)
        perm = np.random.default_rng(11).permutation(len(v))   # new id of old node
        v2 = np.empty_like(v)
        v2[perm] = v
        fv = np.sort(perm[fv0])
        return v2, np.ascontiguousarray(perm[t].astype(np.int32)), fixed_vertices_to_dofs(fv)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _ref(name, warp):
    v, t, _ = _mesh(name)
    return MatRef(v, t, MATS, region_ids(v, t), warp=WARP_NO[warp])


@functools.lru_cache(maxsize=None)
def _state(name):
    v, t, fixed = _mesh(name)
    q, qv = fp.live_state(3 * len(v), fixed, q_scale=0.005 if name.startswith("cube") else 0.002)
    fext = np.zeros(3 * len(v))
    fext[1::3] = -10.0
    u = np.random.default_rng(12345).normal(size=3 * len(v)) * (0.01 if name.startswith("cube") else 0.002)
    return q, qv, fext, u


@functools.lru_cache(maxsize=None)
def _expected(name, warp):
    """(f, K blocks, mass blocks, Keff csr values, rhs, direct dv, orc_pcg info at 1e-6) of the restatement: computed once, shared"""
    ref = _ref(name, warp)
    q, qv, fext, u = _state(name)
    fixed = _mesh(name)[2]
    f, Kb = ref.assemble(u)
    keff, rhs, _ = ref.system(q, qv, fext, STEP["timestep"], STEP["damping_mass"], STEP["damping_stiffness"])
    dv = ref.solve(keff, rhs, fixed)
    info, _ = ref.pcg_iterations(keff, rhs, fixed, eps=1e-6)
    for a in (f, Kb, keff, rhs, dv):
        a.setflags(write=False)
    return f, Kb, ref.mass_blocks(), keff, rhs, dv, info


def _handle(name, prec=fl.FB_MATRIX_F32, warp="warp1", materials=True, **kw):
    v, t, fixed = _mesh(name)
    d = MATS[0]
    a = dict(E=d[0], nu=d[1], rho=d[2], matrix_precision=prec)
    a.update(STEP)
    a.update(WARPS[warp])
    a.update(kw)
    g = FemIntegrator(v, t, fixed, **a)
    if materials:
        g.set_materials(*zip(*MATS), element_ids=region_ids(v, t))
    return g


def _soft_rows(ref):
    """block rows (nodes) every element of which has the softest material"""
    touched = np.zeros(ref.nv, bool)
    other = np.zeros(ref.nv, bool)
    touched[ref.t.reshape(-1)] = True
    other[ref.t[ref.ids != SOFTEST].reshape(-1)] = True
    return np.nonzero(touched & ~other)[0]


def _check_K(Kg, Kb, tol, ref, what):
    err = np.abs(Kg - Kb)
    print("%s: max|dK| / max|K| = %.2e (bound %.0e)" % (what, err.max() / np.abs(Kb).max(), tol))
    assert err.max() <= tol * np.abs(Kb).max(), what
    rows = _soft_rows(ref)
    if len(rows):
        blk = np.concatenate([np.arange(ref.bptr[a], ref.bptr[a + 1]) for a in rows])
        print("%s: %d rows of the softest material only: max|dK| / max|K rows| = %.2e" % (what, len(rows), err[blk].max() / np.abs(Kb[blk]).max()))
        assert err[blk].max() <= tol * np.abs(Kb[blk]).max(), what
    else:
        print("%s: no block row touches the softest material only: the second bound does not apply to this mesh" % what)
    return len(rows)


CASES = [("cube5", {}), ("cube6", {}), ("hub", {}), ("delaunay", dict(renumber=fl.FB_RENUMBER_ON)), ("delaunay", dict(renumber=fl.FB_RENUMBER_OFF))]


@pytest.mark.parametrize("warp", list(WARPS))
@pytest.mark.parametrize("kernel", ["default", "rows", "tets1"])
@pytest.mark.parametrize("prec", [fl.FB_MATRIX_F64, fl.FB_MATRIX_F32])
@pytest.mark.parametrize("mesh,kw", CASES, ids=["cube5", "cube6", "hub", "delaunay_renumbered", "delaunay_caller_order"])
def test_three_materials_against_the_restatement(gpu, monkeypatch, mesh, kw, prec, kernel, warp):
    if kernel != "default":
        monkeypatch.setenv("FEMBRAIN_ASM_KERNEL", kernel)
    f64 = prec == fl.FB_MATRIX_F64
    ref = _ref(mesh, warp)
    f, Kb, mb, keff, rhs, dv, info = _expected(mesh, warp)
    q, qv, fext, u = _state(mesh)
    fixed = _mesh(mesh)[2]
    g = _handle(mesh, prec, warp, **kw)
    L = fl.lib()
    assert g.element_map_bytes() >= ref.nt and np.array_equal(g.element_materials(), ref.ids)
    staged = not f64 and warp != "tangent"
    assert L.fb_fem_assembly_kernel(g.h) == (0 if kernel == "rows" else (2 if kernel == "default" and staged else 1))
    if mesh == "hub":
        assert (L.fb_fem_assembly_wide_slices(g.h) > 0) == (kernel != "rows")
    if "renumber" in kw:
        assert g.renumbering()[0] == (kw["renumber"] == fl.FB_RENUMBER_ON)
    bptr, bcol = g.pattern()
    assert np.array_equal(bptr, ref.bptr) and np.array_equal(bcol, ref.bcol)
    # raw f, K (the slot-major kernel whatever FEMBRAIN_ASM_KERNEL says) and the mass
    fg, Kg = g.assemble(u)
    n_soft = _check_K(Kg, Kb, 1e-10 if f64 else 5e-7, ref, "K")
    assert n_soft > 0   # (every mesh of this test has such rows: the second bound applied)
    assert np.abs(fg - f).max() <= 1e-9 * np.abs(f).max()
    assert np.abs(g.mass() - mb).max() <= (1e-12 if f64 else 1e-7) * mb.max()
    # the element stiffness of every material (the MFMA inspection kernel): tight whatever the storage
    K0, _ = g.element_stiffness(0, ref.nt)
    for e in (0, ref.nt // 3, ref.nt // 2, ref.nt - 1):
        want = ref.orc[int(ref.ids[e])].K0(e)
        assert np.abs(K0[e] - want).max() <= 1e-11 * np.abs(want).max(), e
    # the system of a step at a live state: the kernel FEMBRAIN_ASM_KERNEL names
    g.set_q_state(q, qv)
    g.set_external_forces(fext)
    Keff_g, rhs_g = g.system()
    free = ref.free(fixed)
    tol = 1e-9 if f64 else 5e-7
    Kgs = bsr_to_scipy(bptr, bcol, Keff_g)
    D = (Kgs - ref.csr(keff))[free][:, free]
    print("Keff: %.2e of max (bound %.0e); rhs %.2e" % (abs(D).max() / np.abs(keff).max(), tol, np.abs(rhs_g[free] - rhs[free]).max() / np.abs(rhs).max()))
    assert abs(D).max() <= tol * np.abs(keff).max()
    assert abs(Kgs - Kgs.T).max() == 0
    assert np.abs(rhs_g[free] - rhs[free]).max() <= (1e-9 if f64 else 2e-7) * np.abs(rhs).max() and not rhs_g[~free].any()
    if warp == "tangent":
        g.close()
        return   # (the exact tangent's Keff is symmetrised here and is not the oracle's step matrix: tests/test_fem_gpu.py solves at warp 0 / 1)
    it12, xg = g.pcg(rhs_g, eps=1e-12, max_iter=20000)
    assert it12 > 0 and np.abs(xg - dv).max() <= max(50 * tol, 1e-8) * np.abs(dv).max()
    it6, _ = g.pcg(rhs_g, eps=1e-6, max_iter=20000)
    assert info > 0 and abs(it6 - info) <= max(3, 0.02 * info), (it6, info)
    g.close()


@pytest.mark.parametrize("prec,tol", [(fl.FB_MATRIX_F64, 2e-5), (fl.FB_MATRIX_F32, 2e-4)])
def test_three_steps_with_three_materials(gpu, prec, tol):
    """q, qvel after three steps of the 6^3 cube under a y load, against the restatement stepping with the oracle's PCG at the same
    tolerance (1e-6): the bound of the uniform three-step parity test of that precision (tests/test_fem_gpu.py), unchanged."""
    ref = _ref("cube6", "warp1")
    fixed = _mesh("cube6")[2]
    g = _handle("cube6", prec)
    fext = np.zeros(ref.r)
    fext[1::3] = -1000.0
    q, qv = np.zeros(ref.r), np.zeros(ref.r)
    for k in range(3):
        g.set_external_forces(fext)
        ig = g.do_timestep()
        q, qv, _, info = ref.step(q, qv, fext, fixed, STEP["timestep"], STEP["damping_mass"], STEP["damping_stiffness"], pcg_eps=1e-6)
        qg, vg, _ = g.get_q_state()
        print("step %d: iterations %d / %d, q %.2e, qvel %.2e" % (k, ig, info, np.abs(qg - q).max() / np.abs(q).max(), np.abs(vg - qv).max() / np.abs(qv).max()))
        assert abs(ig - abs(info)) <= max(3, 0.02 * abs(info)), (ig, info)
        assert np.abs(qg - q).max() <= tol * np.abs(q).max(), k
        assert np.abs(vg - qv).max() <= 10 * tol * np.abs(qv).max(), k
        assert not qg[fixed].any() and not vg[fixed].any()
    g.close()


def _three_steps(g):
    f = np.zeros(g.r)
    f[1::3] = -1000.0
    out = []
    for _ in range(3):
        g.set_external_forces(f)
        g.do_timestep()
        out.append(g.get_q_state()[0])
    return out


@pytest.mark.parametrize("warp", ["warp1", "tangent"])
@pytest.mark.parametrize("kernel", ["default", "rows", "tets1"])
@pytest.mark.parametrize("prec", [fl.FB_MATRIX_F64, fl.FB_MATRIX_F32])
@pytest.mark.parametrize("mesh", ["cube6", "hub"])
def test_a_map_of_equal_materials_is_the_uniform_handle_bit_for_bit(gpu, monkeypatch, mesh, prec, kernel, warp):
    if kernel != "default":
        monkeypatch.setenv("FEMBRAIN_ASM_KERNEL", kernel)
    v, t, fixed = _mesh(mesh)
    q, qv, fext, u = _state(mesh)
    out = []
    for mapped in (False, True):
        g = _handle(mesh, prec, warp, materials=False)
        if mapped:   # three entries equal to the params', every element names a non-zero one: the map exists and is read
            d = MATS[0]
            g.set_materials([d[0]] * 3, [d[1]] * 3, [d[2]] * 3, element_ids=1 + (np.arange(len(t)) & 1))
        assert (g.element_map_bytes() > 0) == mapped
        g.set_q_state(q, qv)
        g.set_external_forces(fext)
        Keff, rhs = g.system()
        fa, Ka = g.assemble(u)
        K0, _ = g.element_stiffness(0, len(t))
        g.reset_to_rest()
        out.append([Keff, rhs, g.mass(), fa, Ka, K0] + _three_steps(g))
        g.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert np.abs(out[0][-1]).max() > 0


NEWMARK_CASES = [(m, p, k, w, False) for m in ("cube6", "hub") for p in (fl.FB_MATRIX_F64, fl.FB_MATRIX_F32) for k in ("default", "rows", "tets1")
                 for w in ("warp1", "tangent")] + [("hub", fl.FB_MATRIX_F32, "default", "warp1", True)]


@pytest.mark.parametrize("mesh,prec,kernel,warp,newton", NEWMARK_CASES,
                         ids=["%s-%s-%s-%s%s" % (m, "f64" if p == fl.FB_MATRIX_F64 else "f32", k, w, "-newton3" if n else "") for m, p, k, w, n in NEWMARK_CASES])
def test_a_map_of_equal_materials_is_the_uniform_newmark_handle_bit_for_bit(gpu, monkeypatch, mesh, prec, kernel, warp, newton):
    """The Newmark sibling of the test above: the material-aware instantiations that take qacc (k_assemble_tets<.., NEWMARK, MAT>,
    k_assemble_tets_st<NEWMARK, MAT>) against the uniform ones, and -- a Newmark handle assembles without qacc too -- mass() and the raw
    assemble().  newton: three Newton iterations per step at a loose tolerance, so that the residual of every DOF (res_all) is written."""
    if kernel != "default":
        monkeypatch.setenv("FEMBRAIN_ASM_KERNEL", kernel)
    v, t, fixed = _mesh(mesh)
    q, qv, fext, u = _state(mesh)
    L = fl.lib()
    staged = prec == fl.FB_MATRIX_F32 and warp != "tangent"
    out = []
    for mapped in (False, True):
        g = _handle(mesh, prec, warp, materials=False, integrator=fl.FB_INTEGRATOR_NEWMARK)
        if newton:
            g.set_newmark(0.25, 0.5, 3, 0.5)
        if mapped:   # three entries equal to the params', every element names a non-zero one: the map exists and is read
            d = MATS[0]
            g.set_materials([d[0]] * 3, [d[1]] * 3, [d[2]] * 3, element_ids=1 + (np.arange(len(t)) & 1))
        assert (g.element_map_bytes() > 0) == mapped
        assert L.fb_fem_assembly_kernel(g.h) == (0 if kernel == "rows" else (2 if kernel == "default" and staged else 1))
        if mesh == "hub":
            assert (L.fb_fem_assembly_wide_slices(g.h) > 0) == (kernel != "rows")
        g.set_q_state(q, qv)
        g.set_external_forces(fext)
        Keff, rhs = g.system()
        fa, Ka = g.assemble(u)
        g.reset_to_rest()
        out.append([Keff, rhs, g.mass(), fa, Ka] + _three_steps(g))
        g.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert np.abs(out[0][-1]).max() > 0


def test_a_handle_that_never_sets_a_map_allocates_none(gpu):
    """... and steps to the bytes of a handle that was never asked anything about materials: a one-entry table, or ids that are all 0,
    change the params' material and nothing else."""
    v, t, fixed = _mesh("cube6")
    soft = MATS[1]
    plain = _handle("cube6", materials=False, E=soft[0], nu=soft[1], rho=soft[2])
    g = _handle("cube6", materials=False)
    assert g.element_map_bytes() == 0 and [len(a) for a in g.materials()] == [1, 1, 1] and not g.element_materials().any()
    g.set_materials(soft[0], soft[1], soft[2])              # n = 1, no map: lambda, mu, rho replaced
    g.set_element_materials(np.zeros(len(t), np.uint8))     # every id 0: still no map
    assert g.element_map_bytes() == 0 and [a[0] for a in g.materials()] == list(soft)
    for a, b in zip(_three_steps(g), _three_steps(plain)):
        assert np.array_equal(a, b)
    assert np.array_equal(g.mass(), plain.mass())
    g.close()
    plain.close()


def test_internal_force_scaling_scales_every_material(gpu):
    ref = _ref("cube5", "warp1")
    _, Kb = _expected("cube5", "warp1")[:2]
    u = _state("cube5")[3]
    g = _handle("cube5", fl.FB_MATRIX_F64)
    g.set_internal_force_scaling_factor(0.25)
    f2, K2 = g.assemble(u)
    assert np.abs(K2 - 0.25 * Kb).max() <= 1e-10 * np.abs(0.25 * Kb).max()
    E, nu, rho = g.materials()    # the table reads back as set
    assert np.array_equal(np.stack([E, nu, rho], 1), np.asarray(MATS))
    g.set_materials(*zip(*MATS))  # ... and a table set afterwards is scaled too
    f3, K3 = g.assemble(u)
    assert np.array_equal(K3, K2) and np.array_equal(f3, f2)
    g.close()


def test_every_refusal_leaves_the_handle_as_it_was(gpu):
    v, t, fixed = _mesh("cube5")
    ids = region_ids(v, t)
    want = _three_steps(_handle("cube5"))
    g = _handle("cube5")
    L = fl.lib()
    E, nu, rho = (np.array(a) for a in zip(*MATS))

    def refused(call, *a):
        with pytest.raises(fl.FbError) as e:
            call(*a)
        assert e.value.code == fl.FB_EINVAL

    for bad in (0.0, -1.0, np.nan, np.inf):
        refused(g.set_materials, [E[0], bad, E[2]], nu, rho)                        # E > 0, finite
    for bad in (0.5, -1.0, 0.7, np.nan):
        refused(g.set_materials, E, [nu[0], nu[1], bad], rho)                       # -1 < nu < 0.5
    for bad in (0.0, -3.0, np.inf, np.nan):
        refused(g.set_materials, E, nu, [bad, rho[1], rho[2]])                      # rho > 0, finite
    refused(g.set_materials, np.ones(257), np.zeros(257), np.ones(257))             # 1..256 entries
    z = np.zeros(0)
    assert L.fb_fem_set_materials(g.h, 0, fl.dptr(z), fl.dptr(z), fl.dptr(z)) == fl.FB_EINVAL
    assert L.fb_fem_set_materials(g.h, 3, None, fl.dptr(nu), fl.dptr(rho)) == fl.FB_EINVAL
    refused(g.set_materials, E[:2], nu[:2], rho[:2])                                # ids up to 2 are in use: the table cannot shrink below them
    refused(g.set_materials, E[0], nu[0], rho[0])
    refused(g.set_element_materials, [0, 1, 3, 0])                                  # id >= n_materials (checked on the host, nothing uploaded)
    refused(g.set_element_materials, [0], -1)                                       # bad ranges
    refused(g.set_element_materials, [0, 0], len(t) - 1)
    refused(g.set_element_materials, [0], len(t))
    b = np.zeros(4, np.uint8)
    assert L.fb_fem_set_element_materials(g.h, 0, -1, fl.bptr(b)) == fl.FB_EINVAL
    assert L.fb_fem_set_element_materials(g.h, 0, 4, None) == fl.FB_EINVAL
    assert L.fb_fem_read_element_materials(g.h, len(t) - 1, 2, fl.bptr(b)) == fl.FB_EINVAL
    assert L.fb_fem_set_element_materials(g.h, 2 ** 31 - 1, 2, fl.bptr(b)) == fl.FB_EINVAL   # (first + count past an int)
    # nothing changed: the table, the map, and three steps to the bytes of a handle that was never refused anything
    assert np.array_equal(np.stack(g.materials(), 1), np.asarray(MATS)) and np.array_equal(g.element_materials(), ids)
    for a, b in zip(_three_steps(g), want):
        assert np.array_equal(a, b)
    # a table that GROWS is fine, and so is a range of ids
    g.set_materials(np.append(E, 1e6), np.append(nu, 0.1), np.append(rho, 900.0))
    g.set_element_materials([3, 3], first=5)
    assert g.element_materials()[4:8].tolist() == [ids[4], 3, 3, ids[7]]
    g.close()


def test_resync_returns_the_ids_to_zero_and_keeps_the_table(gpu):
    v, t, fixed = _mesh("cube5")
    g = _handle("cube5")
    v6, t6, fixed6 = _mesh("cube6")
    g.resync(v6, t6, fixed6)
    assert g.element_map_bytes() >= len(t6) and not g.element_materials().any() and len(g.element_materials()) == len(t6)
    assert np.array_equal(np.stack(g.materials(), 1), np.asarray(MATS))
    d = MATS[0]
    plain = _handle("cube6", materials=False)
    for a, b in zip(_three_steps(g), _three_steps(plain)):   # every element material 0 = the params': the uniform handle's bytes
        assert np.array_equal(a, b)
    g.set_materials(d[0], d[1], d[2])    # no id above 0 in use any more: the table may shrink to one entry
    g.close()
    plain.close()


# ---- the map through cuts and delta re-syncs ----
def _cut_setup(mode, **kw):
    """the 5^3 cube, region planes through its nodes at the middle of every axis, a blade in the middle of a cell across the y and z planes"""
    v, t, fixed = _mesh("cube5")
    mean = v.mean(axis=0)
    g = _handle("cube5", fl.FB_MATRIX_F64, expect_cuts=True, cg_eps=1e-9, **kw)
    lo, hi = v.min(0), v.max(0)
    xs = np.unique(v[:, 0])
    point = np.array([0.5 * (xs[1] + xs[2]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])])
    strip = cr.plane_strip(point, (1.0, 0.013, 0.007), half=4.0 * float((hi - lo).max()))
    return g, mean, strip


def _check_against_restatement(g, mean, what):
    """every element's id is the region of its rest centroid (a piece lies inside its parent: no piece-to-parent map needed), and
    assemble() is the restatement on the mesh and the ids the handle reads back"""
    x, t = g.read_mesh()
    ids = g.element_materials()
    assert len(ids) == len(t) and np.array_equal(ids, region_ids(x, t, mean)), what
    assert len(np.unique(ids)) == 3
    ref = MatRef(x, t, MATS, ids)
    u = np.random.default_rng(3).normal(size=ref.r) * 0.002
    f, Kb = ref.assemble(u)
    bptr, bcol = g.pattern()
    assert np.array_equal(bptr, ref.bptr) and np.array_equal(bcol, ref.bcol)
    fg, Kg = g.assemble(u)
    assert np.abs(Kg - Kb).max() <= 1e-10 * np.abs(Kb).max(), what
    assert np.abs(fg - f).max() <= 1e-9 * np.abs(f).max(), what
    assert np.abs(g.mass() - ref.mass_blocks()).max() <= 1e-12 * ref.mass_blocks().max(), what
    return ids


@pytest.mark.parametrize("mode", ["bake", "carry"])
def test_pieces_of_a_cut_inherit_their_parents_material(gpu, mode):
    g, mean, strip = _cut_setup(mode)
    before = g.element_materials()
    nt = len(before)
    # a dry run, a blade that misses, and a blade through the lattice's middle node (unhandled cells) touch nothing
    info, _ = g.cut(strip, mode=mode, modify=False)
    assert info["status"] == fl.FB_CUT_DRY and np.array_equal(g.element_materials(), before)
    info, _ = g.cut(strip + np.array([50.0, 0.0, 0.0]), mode=mode)
    assert info["status"] == fl.FB_CUT_NOTHING and np.array_equal(g.element_materials(), before)
    info, _ = g.cut(ci.touching_blade(_mesh("cube5")[0], (1.0, 1.0, 0.0)), mode=mode)
    assert info["status"] == fl.FB_CUT_UNHANDLED and np.array_equal(g.element_materials(), before) and g.num_tets() == nt
    if mode == "carry":   # a deformed body: the rest shape, and with it the regions, stay
        g.set_uniform_force(1, -200.0)
        g.do_timestep()
    info, delta = g.cut(strip, mode=mode)
    assert info["status"] == fl.FB_CUT_DONE and info["n_removed"] > 0
    ids = _check_against_restatement(g, mean, mode)
    keep = np.ones(nt, bool)
    keep[delta["removed"]] = False
    assert np.array_equal(ids[:keep.sum()], before[keep])   # kept elements keep their id, in order
    g.do_timestep()                                          # ... and the cut body steps
    g.close()


def _delta_of(t, n_nodes):
    """remove elements 3 and 200, change element 10 in place (two of its nodes swapped twice = itself, re-pointed), append two copies
    of removed elements: the change fb_fem_resync_delta takes"""
    removed = np.array([3, 200], np.int32)
    changed_ids = np.array([10], np.int32)
    changed_nodes = t[[10]].copy()
    added = t[[200, 3]].copy()
    return dict(removed=removed, changed_ids=changed_ids, changed_nodes=changed_nodes, added=added, new_xyz=np.zeros((0, 3)))


@pytest.mark.parametrize("path", ["merged", "rebuild", "realloc"])
def test_resync_delta_keeps_the_ids_of_what_stays(gpu, monkeypatch, path):
    """Removed elements drop out, kept and changed ones keep their id in order, appended ones get 0 until the caller sets them; the
    merged path, FEMBRAIN_RESYNC_DELTA=rebuild and a handle whose element buffers must grow (reserve_elements small) give the same array"""
    if path == "rebuild":
        monkeypatch.setenv("FEMBRAIN_RESYNC_DELTA", "rebuild")
    v, t, fixed = _mesh("cube5")
    mean = v.mean(axis=0)
    g = _handle("cube5", fl.FB_MATRIX_F64, **(dict(reserve_elements=1) if path == "realloc" else dict(expect_cuts=True)))
    before = g.element_materials()
    d = _delta_of(t, len(v))
    g.resync_delta(d, fixed)
    assert g.resync_path() == (fl.FB_RESYNC_DELTA_REBUILT if path == "rebuild" else fl.FB_RESYNC_DELTA_MERGED)
    keep = np.ones(len(t), bool)
    keep[d["removed"]] = False
    ids = g.element_materials()
    assert np.array_equal(ids, np.concatenate([before[keep], [0, 0]]))
    g.set_element_materials(before[[200, 3]], first=len(ids) - 2)   # the caller names the appended elements' materials
    _check_against_restatement(g, mean, path)
    if path == "realloc":   # growth by far more than the slack: many appended elements, the map re-allocated with the element buffers
        x, tt = g.read_mesh()
        now = g.element_materials()
        big = dict(removed=np.zeros(0, np.int32), changed_ids=np.zeros(0, np.int32), changed_nodes=np.zeros((0, 4), np.int32),
                   added=np.tile(tt, (3, 1)), new_xyz=np.zeros((0, 3)))
        g.resync_delta(big, fixed)
        ids = g.element_materials()
        assert len(ids) == 4 * len(tt) and np.array_equal(ids[:len(tt)], now) and not ids[len(tt):].any()
        assert g.element_map_bytes() >= len(ids)
    g.close()


@pytest.mark.parametrize("path", ["merged", "rebuild", "realloc"])
def test_cut_by_every_resync_path(gpu, monkeypatch, path):
    """fb_fem_cut re-syncs through fb_fem_resync_delta's paths: the pieces inherit on each of them, and across a re-allocation"""
    if path == "rebuild":
        monkeypatch.setenv("FEMBRAIN_RESYNC_DELTA", "rebuild")
    else:
        monkeypatch.setenv("FEMBRAIN_FRESH_ORDER_PERCENT", "100000")   # (read at every call: the node order is kept however many nodes a cut adds)
    v, t, fixed = _mesh("cube5")
    if path == "realloc":
        g = _handle("cube5", fl.FB_MATRIX_F64, reserve_elements=1, cg_eps=1e-9)
        mean = v.mean(axis=0)
        lo, hi = v.min(0), v.max(0)
        xs = np.unique(v[:, 0])
        strip = cr.plane_strip(np.array([0.5 * (xs[1] + xs[2]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])]), (1.0, 0.013, 0.007), half=4.0 * float((hi - lo).max()))
    else:
        g, mean, strip = _cut_setup("bake")
    bytes_before = g.element_map_bytes()
    info, _ = g.cut(strip, mode="bake")
    assert info["status"] == fl.FB_CUT_DONE
    assert g.resync_path() == (fl.FB_RESYNC_DELTA_REBUILT if path == "rebuild" else fl.FB_RESYNC_DELTA_MERGED)
    _check_against_restatement(g, mean, path)
    # a second cut, across the first: pieces of pieces
    x, _ = g.read_mesh()
    ys = np.unique(_mesh("cube5")[0][:, 1])
    strip2 = cr.plane_strip(np.array([0.2, 0.5 * (ys[2] + ys[3]), 0.2]), (0.011, 1.0, 0.006), half=4.0)
    info, _ = g.cut(strip2, mode="bake")
    assert info["status"] == fl.FB_CUT_DONE
    _check_against_restatement(g, mean, path + " second cut")
    assert g.element_map_bytes() >= g.num_tets() and (path != "realloc" or g.element_map_bytes() > bytes_before)
    g.close()


# ---- sharded handles: one material, no map ----
def _shard_worker(rank, world, shm_name, q):
    try:
        from fembrain_amd import lib as fl_
        from fembrain_amd.fem import FemIntegrator as Fem
        L = fl_.lib()
        comm = C.c_void_p()
        fl_.check(L.fb_comm_create_local(C.byref(comm), rank, world, shm_name.encode(), 8 << 20, 0))
        n = 8
        v, t = truth_cube(n, n, n, 0.1)
        fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))
        splits = np.array([(n * r // world) * n * n for r in range(world + 1)], np.int32)
        g = Fem(v, t, fixed, shard=(world, rank, splits, comm))
        codes = []
        for call in (lambda: g.set_materials([1e7, 2e6], [0.46, 0.3], [1000.0, 900.0]), lambda: g.set_element_materials([0, 0, 0]),
                     lambda: g.set_element_materials([1])):
            try:
                call()
                codes.append(0)
            except fl_.FbError as e:
                codes.append(e.code)
        f = np.zeros(g.r)
        f[1::3] = -10000.0
        g.set_external_forces(f)
        it = g.do_timestep()
        qq = g.get_q_state()[0]
        own = g.owned_nodes()
        dofs = (3 * own[:, None].astype(np.int64) + np.arange(3)[None, :]).reshape(-1)
        q.put((rank, codes, it, dofs, qq[dofs].copy(), g.element_map_bytes(), int(L.fb_fem_num_materials(g.h))))
        g.close()
        L.fb_comm_destroy(comm)
    except Exception as e:   # surface the failure instead of hanging the peer
        q.put((rank, repr(e), 0, None, None, 0, 0))
        q.close()
        q.join_thread()
        os._exit(1)


def test_a_sharded_handle_refuses_a_second_material_and_a_map(gpu):
    import multiprocessing as mp
    world, n = 2, 8
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "/fembrain_test_%d_mat" % os.getpid()
    procs = [ctx.Process(target=_shard_worker, args=(r, world, name, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    v, t = truth_cube(n, n, n, 0.1)
    fixed = fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))
    one = FemIntegrator(v, t, fixed)
    f = np.zeros(one.r)
    f[1::3] = -10000.0
    one.set_external_forces(f)
    it1 = one.do_timestep()
    q1 = one.get_q_state()[0]
    for rank, codes, it, dofs, qq, map_bytes, n_mat in got:
        assert codes == [fl.FB_EINVAL] * 3, (rank, codes)      # every one refused -- also the ids that are all 0: a map is a map
        assert map_bytes == 0 and n_mat == 1
        assert abs(it - it1) <= max(3, 0.02 * it1)               # ... and the handle steps as the unsharded one does
        assert np.abs(qq - q1[dofs]).max() <= 2e-4 * np.abs(q1).max()
    one.close()
