"""Constrained motion on the device (include/fembrain_hip.h, "Constrained motion"; fembrain_amd/csrc/motion.hip) against its NumPy
restatement on the oracle's matrices (tests/motionref.py).

Tolerances are the suite's own.  State after a step: the step-parity bounds of test_three_steps_reference_load, 2e-5 of max|q| with fp64
storage and 2e-4 with fp32, ten times that for velocities (a PCG at 1e-6 against a direct solve).  Right-hand side: the bounds of
test_system_spmv_pcg, 1e-9 (fp64) and 2e-7 (fp32) of max|rhs|.  Reactions: the right-hand-side bound scaled by max|lambda|, against the
rule evaluated at the DEVICE's own dv (the two solvers' dv differ by the PCG tolerance, which is not the reactions' error).

The rule's solve is direct.  A handle that is compared with it solves to 1e-10 (TIGHT), not to the default 1e-6: the states here are
millimetres of displacement, and where a PCG stops at 1e-6 of the residual is by itself 0.9 .. 7e-5 of max|q| away from the direct
solution (measured on these cases with the right-hand sides agreeing to 1e-15) -- the state bounds are to measure the rule, not that.
The handles compared with each other (persistent against reference, twins, zero motion) keep the default."""
import ctypes as C
import os

import numpy as np
import pytest

import adversarial_inputs as ai
import cutref as cr
from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube
from motionref import MotionRef, momentum_terms, reactions_at

pytestmark = pytest.mark.gpu

H = 0.0333   # FemIntegrator's and MotionRef's default step
TIGHT = dict(cg_eps=1e-10, cg_max_iter=20000)
PRECS = [(fl.FB_MATRIX_F64, 2e-5, 1e-9), (fl.FB_MATRIX_F32, 2e-4, 2e-7)]   # storage, state bound, rhs bound


def _dofs(nodes):
    return fixed_vertices_to_dofs(np.asarray(nodes, np.int32))


def _cube(nx, ny=None, nz=None):
    ny, nz = ny or nx, nz or nx
    v, t = truth_cube(nx, ny, nz, 0.1)
    far = np.arange(nx * ny * nz - ny * nz, nx * ny * nz, dtype=np.int32)   # plane i = nx - 1
    return v, t, _dofs(cube_fixed_plane_i0(ny, nz)), far


def _stretch_shear(v, nodes):
    """targets of the nodes' DOFs (ascending): pulled along x, sheared along y by the height z, a little twist in z"""
    p = np.asarray(v, np.float64).reshape(-1, 3)[nodes]
    u = np.stack([np.full(len(nodes), 0.004), 0.03 * (p[:, 2] - p[:, 2].mean()) + 0.002, 0.02 * (p[:, 1] - p[:, 1].mean())], axis=1)
    return u.reshape(-1)


def _state(r, zero, seed=7):
    """a random state, zero on the DOFs ``zero`` (the clamp) and non-zero everywhere else -- on the moved DOFs too"""
    rng = np.random.default_rng(seed)
    q, qv = rng.normal(size=r) * 0.003, rng.normal(size=r) * 0.05
    q[zero] = 0
    qv[zero] = 0
    fext = rng.normal(size=r) * 5.0
    return q, qv, fext


def _close(a, b, tol, what=""):
    err, scale = np.abs(np.asarray(a) - np.asarray(b)).max(), np.abs(b).max()
    print("%s: max error %.3e of %.3e (%.2e relative, bound %.1e)" % (what, err, scale, err / scale if scale else 0.0, tol))
    assert err <= tol * scale, (what, err, scale)


def _steps(g, ref, fixed, dofs, u, q, qv, fext, steps, tol):
    """``steps`` steps of the handle and of the rule, each from its own state; returns the last (out, q_before, qvel_before) of the handle"""
    fixed, dofs = np.asarray(fixed, np.int64), np.asarray(dofs, np.int64)
    held = np.setdiff1d(fixed, dofs)
    g.set_q_state(q, qv)
    last = None
    for k in range(steps):
        g.set_external_forces(fext)
        qb, vb, _ = g.get_q_state()
        out = ref.step(q, qv, fext, fixed, dofs, u)
        g.do_timestep()
        qg, vg, _ = g.get_q_state()
        _close(qg, out["q"], tol, "q after step %d" % k)
        _close(vg, out["qvel"], 10 * tol, "qvel after step %d" % k)
        assert np.array_equal(qg[dofs], u), k                              # the target's bits
        vs = (np.asarray(u, np.float64) - qb[dofs]) / ref.h
        assert np.all(np.abs(vg[dofs] - vs) <= 4 * np.spacing(np.abs(vs))), k   # (u - q_before) / h to 4 ulp
        assert not qg[held].any() and not vg[held].any(), k                # every other constrained DOF is nailed as ever
        q, qv = out["q"], out["qvel"]
        last = (out, qb, vb)
    return last


@pytest.mark.parametrize("prec,tol,rtol", PRECS)
def test_cube_stretch_and_shear(gpu, prec, tol, rtol):
    """4 x 4 x 4, plane i = 0 clamped at 0, plane i = 3 in the set: three steps from a random state that is non-zero on the moved DOFs"""
    v, t, clamp, far = _cube(4)
    moved = _dofs(far)
    fixed = np.sort(np.concatenate([clamp, moved]))
    u = _stretch_shear(v, far)
    ref = MotionRef(v, t)
    q, qv, fext = _state(ref.r, clamp)
    g = FemIntegrator(v, t, fixed, matrix_precision=prec, **TIGHT)
    plain = FemIntegrator(v, t, fixed, matrix_precision=prec, **TIGHT)
    assert g.motion_info()["table_builds"] == 0
    g.set_constrained_motion(moved, u)
    d, uu = g.constrained_motion()
    assert np.array_equal(d, moved) and np.array_equal(uu, u)
    assert not g.reactions()[0].any() and not g.reactions()[1].any()     # zeros before a step with the set
    for h in (g, plain):
        h.set_q_state(q, qv)
        h.set_external_forces(fext)
    # the system: the matrix is that of a handle without a set, bit for bit; the right-hand side carries the correction
    K, rhs = g.system()
    K0, rhs0 = plain.system()
    assert np.array_equal(K, K0)
    out = ref.step(q, qv, fext, fixed, moved, u)
    assert not rhs[fixed].any()
    _close(rhs, out["rhs"], rtol, "rhs")
    assert np.abs(rhs - rhs0).max() > 1e-2 * np.abs(rhs).max()            # the correction is not small change
    assert g.motion_info()["table_builds"] == 1
    _steps(g, ref, fixed, moved, u, q, qv, fext, 3, tol)
    # new targets build nothing
    g.set_constrained_motion(moved, 0.5 * u)
    g.set_external_forces(fext)
    g.do_timestep()
    assert np.array_equal(g.get_q_state()[0][moved], 0.5 * u)
    mi = g.motion_info()
    assert mi["table_builds"] == 1 and mi["n_dofs"] == len(moved) and mi["n_touched_nodes"] >= len(far) and mi["longest_run"] >= 1
    assert plain.motion_info()["table_builds"] == 0
    g.close(); plain.close()


@pytest.mark.parametrize("prec,tol,rtol", PRECS)
def test_one_dof_of_a_node(gpu, prec, tol, rtol):
    """Only the y DOF of an interior node is constrained and moved, its x and z are free: the coupling inside the node's own diagonal
    block.  A correction formed per node instead of per DOF misses it."""
    v, t, clamp, _ = _cube(4)
    node = 1 * 16 + 2 * 4 + 1
    dof = np.array([3 * node + 1], np.int32)
    fixed = np.sort(np.concatenate([clamp, dof]))
    u = np.array([0.006])
    ref = MotionRef(v, t)
    q, qv, fext = _state(ref.r, clamp, seed=3)
    g = FemIntegrator(v, t, fixed, matrix_precision=prec, **TIGHT)
    g.set_constrained_motion(dof, u)
    g.set_q_state(q, qv)
    g.set_external_forces(fext)
    _, rhs = g.system()
    out = ref.step(q, qv, fext, fixed, dof, u)
    _close(rhs, out["rhs"], rtol, "rhs")
    # what the node's own x and z rows get from its moved y DOF, in the rule: far above the bound
    same_node = np.array([3 * node, 3 * node + 2])
    plain = ref.step(q, qv, fext, fixed)["rhs"]
    # (without the set the DOF would be nailed: the rule's right-hand sides differ by exactly the correction)
    dv_c = (u[0] - q[dof[0]]) / H - qv[dof[0]]
    corr = -(out["keff"][same_node][:, dof].toarray().reshape(-1)) * dv_c
    assert np.abs(corr).max() > 1e3 * rtol * np.abs(rhs).max()
    assert np.abs((out["rhs"] - plain)[same_node] - corr).max() <= 1e-12 * np.abs(out["rhs"]).max()
    _steps(g, ref, fixed, dof, u, q, qv, fext, 2, tol)
    mi = g.motion_info()
    assert mi["n_dofs"] == 1 and mi["n_listed_elements"] == mi["longest_run"] > 0
    g.close()


def test_bighub_scrambled_walks_a_long_run(gpu):
    """bighub under permuted ids: 120 of the hub's 1,100 neighbours are held and moved, so the records of the hub's centre -- a free node in
    every listed element -- are one run of hundreds"""
    v, t, fixed0 = ai.mesh("bighub", True)
    nodes = np.sort(ai.caller_ids("bighub", np.arange(2, 122), True)).astype(np.int32)
    moved = _dofs(nodes)
    fixed = np.union1d(fixed0, moved).astype(np.int32)
    rng = np.random.default_rng(5)
    u = rng.normal(size=len(moved)) * 2e-4
    ref = MotionRef(v, t)
    zero = np.setdiff1d(fixed, moved)
    q, qv, fext = _state(ref.r, zero, seed=9)
    q *= 0.05
    qv *= 0.05
    g = FemIntegrator(v, t, fixed, matrix_precision=fl.FB_MATRIX_F64, **TIGHT)
    g.set_constrained_motion(moved, u)
    g.set_q_state(q, qv)
    g.set_external_forces(fext)
    _, rhs = g.system()
    mi = g.motion_info()
    print("bighub:", mi)
    assert mi["longest_run"] > 64 and mi["n_listed_elements"] >= mi["longest_run"]
    out = ref.step(q, qv, fext, fixed, moved, u)
    _close(rhs, out["rhs"], 1e-9, "rhs")
    _steps(g, ref, fixed, moved, u, q, qv, fext, 1, 2e-5)
    lam, s3 = g.reactions()
    assert np.array_equal(np.array([lam[moved % 3 == a].sum() for a in range(3)]) != 0, s3 != 0)
    g.close()


def test_permuted_ids_under_forced_renumbering(gpu):
    """the same body under permuted caller ids in a handle that renumbers behind the ABI, against the unpermuted run in the caller's order"""
    v, t, clamp, far = _cube(5)
    moved = _dofs(far)
    fixed = np.sort(np.concatenate([clamp, moved]))
    u = _stretch_shear(v, far)
    perm = np.random.default_rng(3).permutation(len(v))      # ai.scrambled's: new id of old node
    v2, t2, fixed2 = ai.scrambled(v, t, fixed)
    dmap = (3 * perm[:, None] + np.arange(3)[None]).reshape(-1)          # new DOF of old DOF
    order = np.argsort(dmap[moved])
    moved2, u2 = dmap[moved][order].astype(np.int32), u[order]
    ref = MotionRef(v, t)
    q, qv, fext = _state(ref.r, clamp, seed=13)
    q2, qv2, fext2 = np.zeros_like(q), np.zeros_like(qv), np.zeros_like(fext)
    q2[dmap], qv2[dmap], fext2[dmap] = q, qv, fext
    a = FemIntegrator(v, t, fixed, matrix_precision=fl.FB_MATRIX_F64, renumber=fl.FB_RENUMBER_OFF, **TIGHT)
    b = FemIntegrator(v2, t2, fixed2, matrix_precision=fl.FB_MATRIX_F64, renumber=fl.FB_RENUMBER_ON, **TIGHT)
    assert b.renumbering()[0] and not a.renumbering()[0]
    a.set_constrained_motion(moved, u)
    b.set_constrained_motion(moved2, u2)
    assert np.array_equal(b.constrained_motion()[0], moved2)
    b.set_q_state(q2, qv2)
    for k in range(2):
        b.set_external_forces(fext2)
        b.do_timestep()
    _steps(a, ref, fixed, moved, u, q, qv, fext, 2, 2e-5)
    (qa, va, _), (qb, vb, _) = a.get_q_state(), b.get_q_state()
    _close(qb[dmap], qa, 2e-5, "q, permuted against unpermuted")
    _close(vb[dmap], va, 2e-4, "qvel, permuted against unpermuted")
    assert np.array_equal(qb[moved2], u2)
    la, lb = a.reactions()[0], b.reactions()[0]
    inv = np.empty_like(order)
    inv[order] = np.arange(len(order))
    _close(lb[inv], la, 2e-5, "reactions, permuted against unpermuted")
    assert a.motion_info()["n_listed_elements"] == b.motion_info()["n_listed_elements"]
    a.close(); b.close()


def test_two_materials(gpu):
    """a soft half and a stiff, heavy half through set_materials: the correction and the reactions take each element's own material"""
    v, t, clamp, far = _cube(4)
    moved = _dofs(far)
    fixed = np.sort(np.concatenate([clamp, moved]))
    u = _stretch_shear(v, far)
    mats = [(1e7, 0.46, 1000.0), (4e7, 0.3, 2500.0)]
    cz = np.asarray(v, np.float64).reshape(-1, 3)[np.asarray(t).reshape(-1, 4)].mean(axis=1)[:, 2]
    ids = (cz > np.median(cz)).astype(np.uint8)
    assert 0 < ids.sum() < len(ids)
    ref = MotionRef(v, t, materials=mats, ids=ids)
    q, qv, fext = _state(ref.r, clamp, seed=21)
    g = FemIntegrator(v, t, fixed, matrix_precision=fl.FB_MATRIX_F64, **TIGHT)
    g.set_materials(*zip(*mats), element_ids=ids)
    g.set_constrained_motion(moved, u)
    g.set_q_state(q, qv)
    g.set_external_forces(fext)
    _, rhs = g.system()
    _close(rhs, ref.step(q, qv, fext, fixed, moved, u)["rhs"], 1e-9, "rhs")
    out, qb, vb = _steps(g, ref, fixed, moved, u, q, qv, fext, 2, 2e-5)
    _check_reactions(g, ref, fixed, moved, u, qb, vb, fext, 1e-9)
    g.close()


@pytest.mark.parametrize("warp,kw", [(0, dict(linear=True)), (2, dict(exact_tangent=True))])
def test_warp_0_and_2(gpu, warp, kw):
    v, t, clamp, far = _cube(4)
    moved = _dofs(far)
    fixed = np.sort(np.concatenate([clamp, moved]))
    u = _stretch_shear(v, far)
    ref = MotionRef(v, t, warp=warp)
    q, qv, fext = _state(ref.r, clamp, seed=31)
    g = FemIntegrator(v, t, fixed, matrix_precision=fl.FB_MATRIX_F64, **TIGHT, **kw)
    g.set_constrained_motion(moved, u)
    g.set_q_state(q, qv)
    g.set_external_forces(fext)
    _, rhs = g.system()
    _close(rhs, ref.step(q, qv, fext, fixed, moved, u)["rhs"], 1e-9, "rhs")
    out, qb, vb = _steps(g, ref, fixed, moved, u, q, qv, fext, 2, 2e-5)
    _check_reactions(g, ref, fixed, moved, u, qb, vb, fext, 1e-9)
    g.close()


def test_persistent_solver_against_the_reference_sequence(gpu):
    """FB_PCG_PERSISTENT (fp32) against FB_PCG_REFERENCE: the solvers see only a different right-hand side"""
    v, t, clamp, far = _cube(7)
    moved = _dofs(far)
    fixed = np.sort(np.concatenate([clamp, moved]))
    u = _stretch_shear(v, far)
    q, qv, fext = _state(3 * len(v), clamp, seed=41)
    res = []
    for variant in (fl.FB_PCG_PERSISTENT, fl.FB_PCG_REFERENCE):
        g = FemIntegrator(v, t, fixed, matrix_precision=fl.FB_MATRIX_F32, pcg_variant=variant)
        g.set_constrained_motion(moved, u)
        g.set_q_state(q, qv)
        for _ in range(3):
            g.set_external_forces(fext)
            g.do_timestep()
        print("variant %d ran PCG path %s" % (variant, g.pcg_path()))
        res.append(g.get_q_state()[:2] + (g.reactions()[0],))
        g.close()
    (qp, vp, lp), (qr, vr, lr) = res
    assert np.array_equal(qp[moved], u) and np.array_equal(qr[moved], u)
    _close(qp, qr, 2e-4, "q, persistent against reference")
    _close(vp, vr, 2e-3, "qvel, persistent against reference")
    _close(lp, lr, 2e-4, "reactions, persistent against reference")


def test_two_identical_handles_give_the_same_bits(gpu):
    v, t, clamp, far = _cube(5)
    moved = _dofs(far)
    fixed = np.sort(np.concatenate([clamp, moved]))
    u = _stretch_shear(v, far)
    q, qv, fext = _state(3 * len(v), clamp, seed=51)
    res = []
    for _ in range(2):
        g = FemIntegrator(v, t, fixed)
        g.set_constrained_motion(moved, u)
        g.set_q_state(q, qv)
        for k in range(3):
            g.set_external_forces(fext)
            g.do_timestep()
        res.append(g.get_q_state()[:2] + g.reactions() + (g.system()[1],))
        g.close()
    for x, y in zip(*res):
        assert np.array_equal(x, y)
    assert np.abs(res[0][2]).max() > 0


@pytest.mark.parametrize("prec", [fl.FB_MATRIX_F64, fl.FB_MATRIX_F32])
def test_zero_motion_is_the_plain_step(gpu, prec):
    """the set is the clamp with targets 0, from rest: the state is that of a plain handle after 3 steps, bit for bit"""
    v, t, clamp, _ = _cube(5)
    g = FemIntegrator(v, t, clamp, matrix_precision=prec)
    plain = FemIntegrator(v, t, clamp, matrix_precision=prec)
    g.set_constrained_motion(clamp, np.zeros(len(clamp)))
    for k in range(3):
        for h in (g, plain):
            h.set_uniform_force(1, -10000.0)
            h.do_timestep()
        (qa, va, _), (qb, vb, _) = g.get_q_state(), plain.get_q_state()
        assert np.array_equal(qa, qb) and np.array_equal(va, vb), k
    assert np.abs(qa).max() > 0
    assert g.motion_info()["table_builds"] == 1 and plain.motion_info()["table_builds"] == 0
    # the clamp's reactions hold the body against the load: their y sum is the load on the free nodes minus what accelerates them
    lam, s3 = g.reactions()
    assert s3[1] > 0 and np.abs(lam).max() > 0
    g.close(); plain.close()


def _check_reactions(g, ref, fixed, dofs, u, qb, vb, fext, rtol, momentum=False):
    """the handle's reactions of the step it just made from (qb, vb) against the rule at the handle's own dv"""
    fixed, dofs = np.asarray(fixed, np.int64), np.asarray(dofs, np.int64)
    qa, va, _ = g.get_q_state()
    free = np.ones(ref.r, bool)
    free[fixed] = False
    dv = np.zeros(ref.r)
    dv[free] = (va - vb)[free]
    dv[dofs] = (np.asarray(u, np.float64) - qb[dofs]) / ref.h - vb[dofs]
    lam_ref = reactions_at(ref, qb, vb, fext, dofs, dv)
    lam, s3 = g.reactions()
    _close(lam, lam_ref, rtol, "reactions")
    s3_np = np.array([lam[dofs % 3 == a].sum() for a in range(3)])
    assert np.all(np.abs(s3 - s3_np) <= 1e-12 * np.abs(lam).sum())       # one fixed tree against numpy's order
    if momentum:
        assert len(dofs) == len(fixed)   # every constrained DOF is in the set: sum(lambda) is the whole constraint force
        keff, rhs0, _ = ref.system(qb, vb, fext)
        r = np.zeros(ref.r)
        r[free] = (keff @ dv)[free] - rhs0[free]
        terms = momentum_terms(ref, qb, vb, fext, fixed, dv, r, lam=lam)
        gap, big = np.abs(terms.sum(axis=1)).max(), np.abs(terms).max()
        # each of the n reactions is within rtol * max|lambda| of the rule's, and the rule closes the balance to 1e-10 of its largest term
        bound = len(dofs) * rtol * np.abs(lam).max() + 1e-10 * big
        print("momentum: gap %.3e, largest term %.3e, bound %.3e" % (gap, big, bound))
        assert gap <= bound, terms
    return lam


@pytest.mark.parametrize("prec,tol,rtol", PRECS)
def test_reactions_and_momentum(gpu, prec, tol, rtol):
    """every constrained DOF in the set (the clamp at target 0, the far plane moved), cM = 0: the reactions against the rule, and
    sum(lambda) + sum(fext) - (1/h) sum_b m_b dv_b = -(1/h) sum_f r_f with the device's own dv and reactions"""
    v, t, clamp, far = _cube(4)
    moved = _dofs(far)
    fixed = np.sort(np.concatenate([clamp, moved]))
    u = np.zeros(len(fixed))
    u[np.isin(fixed, moved)] = _stretch_shear(v, far)
    ref = MotionRef(v, t)
    q, qv, fext = _state(ref.r, clamp, seed=61)
    g = FemIntegrator(v, t, fixed, matrix_precision=prec, **TIGHT)
    g.set_constrained_motion(fixed, u)
    for steps in (1, 1):
        out, qb, vb = _steps(g, ref, fixed, fixed, u, q, qv, fext, steps, tol)
        lam = _check_reactions(g, ref, fixed, fixed, u, qb, vb, fext, rtol, momentum=True)
        _close(lam, out["lam"], 50 * tol, "reactions against the rule's own solve")   # (the two dv differ by the PCG tolerance)
        q, qv = g.get_q_state()[:2]
    g.close()


def _mid_plane(v, frac=0.47, normal=(1.0, 0.013, 0.007)):
    """test_fem_cut_gpu's: a plane across the whole section, in the middle of a grid cell, tilted too little to reach a node plane"""
    lo, hi = v.min(0), v.max(0)
    xs = np.unique(v[:, 0])
    k = min(max(int(np.searchsorted(xs, lo[0] + frac * (hi[0] - lo[0]))), 1), len(xs) - 1)
    point = np.array([0.5 * (xs[k - 1] + xs[k]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])])
    return cr.plane_strip(point, normal, half=4.0 * float((hi - lo).max()))


def test_cut_through_a_held_beam(gpu):
    """fb_fem_cut (state carried) through a beam clamped at one end and held at the other: the set survives, the table is built again,
    and the next step is the rule's on the mesh the handle reads back"""
    v, t, clamp, far = _cube(7, 3, 3)
    moved = _dofs(far)
    fixed = np.sort(np.concatenate([clamp, moved]))
    u = _stretch_shear(v, far)
    g = FemIntegrator(v, t, fixed, matrix_precision=fl.FB_MATRIX_F64, expect_cuts=True, **TIGHT)
    g.set_constrained_motion(moved, u)
    q, qv, fext = _state(3 * len(v), clamp, seed=71)
    g.set_q_state(q, qv)
    g.set_external_forces(fext)
    g.do_timestep()
    assert g.motion_info()["table_builds"] == 1
    listed_before = g.motion_info()["n_listed_elements"]
    info, _ = g.cut(_mid_plane(np.asarray(v, np.float64).reshape(-1, 3)), mode="carry")
    assert info["status"] == fl.FB_CUT_DONE and info["n_new_nodes"] > 0
    d, uu = g.constrained_motion()
    assert np.array_equal(d, moved) and np.array_equal(uu, u)            # the set survived, targets and all
    mi = g.motion_info()
    assert mi["table_builds"] == 1 and not mi["table_valid"]
    x0, t2 = g.read_mesh()
    fixed2 = g.constrained_dofs()
    assert np.array_equal(fixed2, fixed)
    ref = MotionRef(x0, t2)
    qb, vb, _ = g.get_q_state()
    assert np.array_equal(qb[moved], u)
    fext2 = np.zeros(ref.r)
    fext2[1::3] = -20.0
    _steps(g, ref, fixed2, moved, u, qb, vb, fext2, 1, 2e-5)
    mi = g.motion_info()
    assert mi["table_builds"] == 2 and mi["table_valid"] and mi["n_listed_elements"] == listed_before   # (the cut is far from the held face)
    _check_reactions(g, ref, fixed2, moved, u, qb, vb, fext2, 1e-9)
    g.close()


def test_freeing_a_moved_dof(gpu):
    """set_constrained_dofs without one of the moved DOFs: it leaves the set with its q and qvel, and the next step is the rule's with it free"""
    v, t, clamp, far = _cube(4)
    moved = _dofs(far)
    fixed = np.sort(np.concatenate([clamp, moved]))
    u = _stretch_shear(v, far)
    ref = MotionRef(v, t)
    q, qv, fext = _state(ref.r, clamp, seed=81)
    g = FemIntegrator(v, t, fixed, matrix_precision=fl.FB_MATRIX_F64, **TIGHT)
    g.set_constrained_motion(moved, u)
    _steps(g, ref, fixed, moved, u, q, qv, fext, 1, 2e-5)
    qb, vb, _ = g.get_q_state()
    gone = moved[7]
    keep = moved != gone
    g.set_constrained_dofs(fixed[fixed != gone])
    d, uu = g.constrained_motion()
    assert np.array_equal(d, moved[keep]) and np.array_equal(uu, u[keep])
    qa, va, _ = g.get_q_state()
    assert np.array_equal(qa, qb) and np.array_equal(va, vb) and qa[gone] == u[7] and va[gone] != 0
    _steps(g, ref, fixed[fixed != gone], moved[keep], u[keep], qb, vb, fext, 1, 2e-5)
    assert g.motion_info()["table_builds"] == 2
    assert g.get_q_state()[0][gone] != u[7]                                # it moves as a free DOF now
    # ... and an empty list clears the set
    g.set_constrained_motion([], [])
    assert g.motion_info()["n_dofs"] == 0 and len(g.reactions()[0]) == 0
    g.close()


def test_grasp_layer(gpu):
    v, t, clamp, far = _cube(5, 3, 3)
    x = np.asarray(v, np.float64).reshape(-1, 3)
    ref = MotionRef(v, t)
    q, qv, fext = _state(ref.r, clamp, seed=91)
    g = FemIntegrator(v, t, clamp, matrix_precision=fl.FB_MATRIX_F64, **TIGHT)
    g.set_q_state(q, qv)
    with pytest.raises(fl.FbError):
        g.grasp_move()                                                     # nothing is held
    info = g.grasp(far)
    fixed = g.constrained_dofs()
    assert len(fixed) == len(clamp) + 3 * len(far) and np.array_equal(fixed, np.union1d(clamp, _dofs(far)))
    assert info["n_dofs"] == 3 * len(far) and info["n_grasp_nodes"] == len(far)
    d, u0 = g.constrained_motion()
    assert np.array_equal(d, _dofs(far)) and np.array_equal(u0, q[d])      # targets = the current q, bit for bit
    # a rotation about a pivot and a shift, against numpy to 1e-14 of the body's size
    th = 0.3
    R = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
    tr, pivot = np.array([0.01, -0.02, 0.005]), np.array([0.2, 0.1, 0.0])
    g.grasp_move(R, tr, pivot)
    p = x[far] + q.reshape(-1, 3)[far]
    want = ((p - pivot) @ R.T + pivot + tr - x[far]).reshape(-1)
    size = float((x.max(0) - x.min(0)).max())
    got = g.constrained_motion()[1]
    assert np.abs(got - want).max() <= 1e-14 * size
    # a gentle move, a step against the rule, the force on the tool
    g.grasp_move(None, (0.003, 0.0, 0.0), (0.0, 0.0, 0.0))
    u = g.constrained_motion()[1]
    out, qb, vb = _steps(g, ref, fixed, d, u, q, qv, fext, 1, 2e-5)
    _check_reactions(g, ref, fixed, d, u, qb, vb, fext, 1e-9)
    with pytest.raises(fl.FbError):
        g.grasp(far[:2])                                                   # one grasp per handle
    qa, va, _ = g.get_q_state()
    g.release()
    assert np.array_equal(g.constrained_dofs(), clamp) and g.motion_info()["n_dofs"] == 0 and g.motion_info()["n_grasp_nodes"] == 0
    qr, vr, _ = g.get_q_state()
    assert np.array_equal(qr, qa) and np.array_equal(vr, va)              # the state is kept
    g.set_external_forces(fext)
    g.do_timestep()
    assert np.abs(g.get_q_state()[0][d] - u).max() > 0                     # and the tissue springs back as free DOFs
    g.reset_to_rest()
    g.close()


def test_resets_clear_the_set(gpu):
    v, t, clamp, far = _cube(4)
    g = FemIntegrator(v, t, clamp)
    g.grasp(far)
    assert g.motion_info()["n_dofs"] == 3 * len(far)
    g.reset_to_rest()
    assert g.motion_info()["n_dofs"] == 0 and g.motion_info()["n_grasp_nodes"] == 0
    g.set_constrained_motion(clamp[:3], [0.0, 0.0, 0.0])
    g.resync(v, t, clamp)
    assert g.motion_info()["n_dofs"] == 0
    g.close()


def test_bad_arguments_change_nothing(gpu):
    v, t, clamp, far = _cube(4)
    moved = _dofs(far)
    fixed = np.sort(np.concatenate([clamp, moved]))
    u = _stretch_shear(v, far)
    g = FemIntegrator(v, t, fixed)
    g.set_constrained_motion(moved, u)

    def refused(call):
        with pytest.raises(fl.FbError) as e:
            call()
        assert e.value.code == fl.FB_EINVAL
        d, uu = g.constrained_motion()
        assert np.array_equal(d, moved) and np.array_equal(uu, u)

    free_dof = 3 * 20 + 1
    assert free_dof not in fixed
    refused(lambda: g.set_constrained_motion([free_dof], [0.0]))                     # not a constrained DOF
    refused(lambda: g.set_constrained_motion(moved[::-1], u))                        # not ascending
    refused(lambda: g.set_constrained_motion(moved[[0, 0]], u[:2]))                  # twice
    bad = u.copy()
    bad[3] = np.nan
    refused(lambda: g.set_constrained_motion(moved, bad))                            # a target that is not finite
    bad[3] = np.inf
    refused(lambda: g.set_constrained_motion(moved, bad))
    refused(lambda: fl.check(g._L.fb_fem_set_constrained_motion(g.h, 3, None, None)))  # null arrays with a count
    refused(lambda: fl.check(g._L.fb_fem_set_constrained_motion(g.h, -1, None, None)))
    refused(lambda: g.grasp_move([[np.nan] * 3] * 3))                                # (and no grasp)
    g.close()
    nm = FemIntegrator(v, t, fixed, integrator=fl.FB_INTEGRATOR_NEWMARK)
    for call in (lambda: nm.set_constrained_motion(moved, u), lambda: nm.grasp(far), lambda: nm.time_motion()):
        with pytest.raises(fl.FbError) as e:
            call()
        assert e.value.code == fl.FB_EINVAL
    assert nm.motion_info()["n_dofs"] == 0
    nm.set_uniform_force(1, -50.0)
    nm.do_timestep()
    nm.close()


def _sharded_worker(rank, world, shm_name, q):
    try:
        L = fl.lib()
        comm = C.c_void_p()
        fl.check(L.fb_comm_create_local(C.byref(comm), rank, world, shm_name.encode(), 8 << 20, 0))
        v, t = truth_cube(6, 4, 4, 0.1)
        fixed = np.arange(3 * 16, dtype=np.int32)
        splits = np.array([0, 48, 96], np.int32)
        g = FemIntegrator(v, t, fixed, shard=(world, rank, splits, comm))
        codes = []
        for call in (lambda: g.set_constrained_motion(fixed[:3], [0.0, 0.0, 0.0]), lambda: g.grasp([90, 91])):
            try:
                call()
                codes.append(0)
            except fl.FbError as e:
                codes.append(e.code)
        g.set_uniform_force(1, -50.0)   # it still steps
        g.do_timestep()
        codes.append(g.last.converged)
        q.put((rank, codes))
        g.close()
        L.fb_comm_destroy(comm)
    except Exception as e:  # surface the failure instead of hanging the peer
        q.put((rank, repr(e)))
        q.close()
        q.join_thread()
        os._exit(1)


def test_a_sharded_handle_is_refused():
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, "/fembrain_test_mo_%d" % os.getpid(), q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=120) for _ in procs]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for rank, codes in res:
        assert codes == [fl.FB_EINVAL, fl.FB_EINVAL, 1], (rank, codes)


def test_time_motion_leaves_everything_as_it_was(gpu):
    v, t, clamp, far = _cube(5)
    moved = _dofs(far)
    fixed = np.sort(np.concatenate([clamp, moved]))
    u = _stretch_shear(v, far)
    g = FemIntegrator(v, t, fixed)
    with pytest.raises(fl.FbError):
        g.time_motion()                                                    # no set
    g.set_constrained_motion(moved, u)
    q, qv, fext = _state(3 * len(v), clamp, seed=95)
    g.set_q_state(q, qv)
    g.set_external_forces(fext)
    g.do_timestep()
    before = g.get_q_state()[:2] + g.reactions() + (g.motion_info()["table_builds"],)
    sec = g.time_motion(reps=3)
    assert sec.shape == (4,) and np.all(sec > 0) and np.all(sec < 1.0)
    after = g.get_q_state()[:2] + g.reactions() + (g.motion_info()["table_builds"],)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    g.close()
