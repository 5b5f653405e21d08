"""Constrained motion and the grasp (fembrain_amd/csrc/motion.hip) where tests/test_motion_gpu.py does not reach: every parameter set of
tests/fem_params.py (c_M != 0: the mass-damping terms of the correction and of the reactions), the three assembly kernels with a set,
sets and tables past one workgroup of 256, cuts through the held elements, FB_CUT_BAKE, a caller's own fb_fem_resync_delta,
fb_fem_detach_part, the grasp's bookkeeping under overlap and renumbering, and an inverted listed element.

The reference is tests/motionref.py (the rule in NumPy on the oracle's matrices, a direct solve), pinned on the CPU at every parameter
set by tests/test_motion_ref.py.  Helpers and tolerances are those of tests/test_motion_gpu.py: state 2e-5 of max|q| with fp64 storage
(qvel ten times that), right-hand side and reactions 1e-9 (fp64) and 2e-7 (fp32); every handle compared with the direct solve runs
TIGHT.  With fp32 storage the state bound is max(2e-4, test_fem_params_gpu._tol(name, F32)): near_incomp is conditioning-bound there.

Every liveness condition -- that a case reaches what it is written for -- is asserted from the reference or from numpy alone."""
import numpy as np
import pytest

import adversarial_inputs as ai
import fem_params as fp
from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator, bsr_to_scipy
from fembrain_amd.meshgen import synthetic_cut
from motionref import MotionRef, reactions_at
from test_fem_params_gpu import _tol as _params_tol
from test_motion_gpu import PRECS, TIGHT, _check_reactions, _close, _cube, _dofs, _mid_plane, _state, _steps, _stretch_shear

pytestmark = pytest.mark.gpu

F32, F64 = fl.FB_MATRIX_F32, fl.FB_MATRIX_F64
KERNELS = ["rows", "tets1", "tets"]


def _ref(name, v, t):
    return MotionRef(v, t, **fp.material(name), **fp.integrator(name))


def _held_cube(nx, ny=None, nz=None, whole_clamp=False):
    """_cube with the far plane moved by _stretch_shear: (v, t, clamp, far, moved DOFs, every constrained DOF, set DOFs, targets);
    whole_clamp: the clamp is in the set too, at target 0 (every constrained DOF is then in the set)"""
    v, t, clamp, far = _cube(nx, ny, nz)
    moved = _dofs(far)
    fixed = np.sort(np.concatenate([clamp, moved]))
    u = _stretch_shear(v, far)
    if not whole_clamp:
        return v, t, clamp, far, moved, fixed, moved, u
    u_all = np.zeros(len(fixed))
    u_all[np.isin(fixed, moved)] = u
    return v, t, clamp, far, moved, fixed, fixed, u_all


def _xyz(v):
    return np.asarray(v, np.float64).reshape(-1, 3)


# ---- 1. parameter sets ------------------------------------------------------------------------------------------------------------------

def _param_case(name):
    v, t, clamp, far, moved, fixed, dofs, u = _held_cube(4, whole_clamp=True)
    ref = _ref(name, v, t)
    q, qv, fext = _state(ref.r, clamp, seed=7)
    fext = fext * (fp.PARAMS[name]["E"] / 1e7)
    return v, t, clamp, moved, fixed, u, ref, q, qv, fext


def _mass_damping_shares(name):
    """(share of max|rhs| that reaches the free rows through the moved columns by mass damping, h cM M_fc v*_c; share of max|lambda|
    that goes when cM is set to 0 in the rule at the same dv) -- from the rule alone"""
    v, t, clamp, moved, fixed, u, ref, q, qv, fext = _param_case(name)
    out = ref.step(q, qv, fext, fixed, fixed, u)
    free = np.ones(ref.r, bool)
    free[fixed] = False
    w = np.zeros(ref.r)
    w[fixed] = (u - q[fixed]) / ref.h
    rhs_share = np.abs((ref.h * ref.cM * (ref.M @ w))[free]).max() / np.abs(out["rhs"]).max()
    p = dict(fp.integrator(name), cM=0.0)
    lam0 = reactions_at(MotionRef(v, t, **fp.material(name), **p), q, qv, fext, fixed, out["dv"])
    lam = reactions_at(ref, q, qv, fext, fixed, out["dv"])
    return rhs_share, np.abs(lam - lam0).max() / np.abs(lam).max()


@pytest.mark.parametrize("prec,tol,rtol", PRECS)
@pytest.mark.parametrize("name", fp.NAMES)
def test_every_parameter_set(gpu, name, prec, tol, rtol):
    """4^3, the clamp in the set at 0 and the far plane moved, from a state that is non-zero on the moved DOFs: right-hand side,
    two steps, reactions at the device's own dv and the five-term momentum balance, at each set of fem_params"""
    v, t, clamp, moved, fixed, u, ref, q, qv, fext = _param_case(name)
    if name in ("soft_damped", "tiny_step"):
        # what a wrong or missing c_M term would change, a hundred times above the fp32 bound (measured: 4.9e-5 and 8.2e-4 at
        # soft_damped, 8.8e-5 and 9.4e-5 at tiny_step)
        shares = _mass_damping_shares(name)
        print("%s: mass-damping share of the right-hand side %.2e, of the reactions %.2e" % ((name,) + shares))
        assert min(shares) >= 100 * 2e-7, shares
    if prec == F32:
        tol = max(tol, _params_tol(name, F32))
    g = FemIntegrator(v, t, fixed, matrix_precision=prec, **fp.handle(name), **TIGHT)
    g.set_constrained_motion(fixed, u)
    g.set_q_state(q, qv)
    g.set_external_forces(fext)
    _, rhs = g.system()
    out = ref.step(q, qv, fext, fixed, fixed, u)
    assert not rhs[fixed].any()
    _close(rhs, out["rhs"], rtol, "%s rhs" % name)
    q1, v1 = q, qv
    for k in range(2):      # (one step at a time: the reactions of each)
        _, qb, vb = _steps(g, ref, fixed, fixed, u, q1, v1, fext, 1, tol)
        _check_reactions(g, ref, fixed, fixed, u, qb, vb, fext, rtol, momentum=True)
        q1, v1 = g.get_q_state()[:2]
    assert g.motion_info()["table_builds"] == 1
    g.close()


@pytest.mark.parametrize("prec,tol,rtol", PRECS)
def test_setters_on_a_handle_with_a_set(gpu, prec, tol, rtol):
    """set_timestep / set_damping on a live handle with a set: the next system() and step are the rule's at the new values (soft_damped's
    h, c_M, c_K on the default material), and the table is not built again"""
    v, t, clamp, far, moved, fixed, dofs, u = _held_cube(4, whole_clamp=True)
    q, qv, fext = _state(3 * len(_xyz(v)), clamp, seed=17)
    g = FemIntegrator(v, t, fixed, matrix_precision=prec, **TIGHT)
    g.set_constrained_motion(dofs, u)
    _steps(g, MotionRef(v, t), fixed, dofs, u, q, qv, fext, 1, tol)
    assert g.motion_info()["table_builds"] == 1
    p = fp.integrator("soft_damped")
    g.set_timestep(p["timestep"])
    g.set_damping(p["cM"], p["cK"])
    ref = MotionRef(v, t, **p)
    qb, vb, _ = g.get_q_state()
    g.set_external_forces(fext)
    _, rhs = g.system()
    _close(rhs, ref.step(qb, vb, fext, fixed, dofs, u)["rhs"], rtol, "rhs after the setters")
    for k in range(2):
        _, qb, vb = _steps(g, ref, fixed, dofs, u, qb, vb, fext, 1, tol)
        _check_reactions(g, ref, fixed, dofs, u, qb, vb, fext, rtol, momentum=True)
        qb, vb = g.get_q_state()[:2]
    assert g.motion_info()["table_builds"] == 1
    g.close()


@pytest.mark.parametrize("prec,tol,rtol", PRECS)
@pytest.mark.parametrize("name", ["soft_damped", "default"])
def test_assembly_kernels_with_a_set(gpu, monkeypatch, name, prec, tol, rtol):
    """FEMBRAIN_ASM_KERNEL = rows | tets1 | tets from a state that is non-zero on constrained DOFs: system() with the set gives the same
    bits from all three, within the rule's bound"""
    v, t, clamp, moved, fixed, u, ref, q, qv, fext = _param_case(name)
    want = ref.step(q, qv, fext, fixed, fixed, u)["rhs"]
    out = []
    for kern in KERNELS:
        monkeypatch.setenv("FEMBRAIN_ASM_KERNEL", kern)
        g = FemIntegrator(v, t, fixed, matrix_precision=prec, **fp.handle(name), **TIGHT)
        g.set_constrained_motion(fixed, u)
        g.set_q_state(q, qv)
        g.set_external_forces(fext)
        K, rhs = g.system()
        _close(rhs, want, rtol, "%s rhs of %s" % (name, kern))
        g.do_timestep()
        out.append((K, rhs) + g.get_q_state()[:2] + g.reactions())
        g.close()
    for a in out[:2]:
        assert all(np.array_equal(x, y) for x, y in zip(a, out[2])), name


# ---- 2. past one workgroup ----------------------------------------------------------------------------------------------------------------

def _second_trip(lam, dofs, first=256):
    """the largest share of sum(|lambda|) that the entries from ``first`` on carry in one axis' sum"""
    dofs = np.asarray(dofs)
    tail = np.arange(len(dofs)) >= first
    return max(abs(lam[tail & (dofs % 3 == a)].sum()) for a in range(3)) / np.abs(lam).sum()


@pytest.mark.parametrize("n_set", [432, 255, 256, 257, 300])
def test_sets_across_the_workgroup_edges(gpu, n_set):
    """truth_cube(3, 12, 12), the first n_set DOFs of the far plane in the set (432: the whole plane; below that some nodes are partly
    in the set): right-hand side, a step, reactions and their sum against the rule, with entries past the 256th that carry weight"""
    v, t, clamp, far = _cube(3, 12, 12)
    moved = _dofs(far)[:n_set]
    u = _stretch_shear(v, far)[:n_set]
    fixed = np.sort(np.concatenate([clamp, moved]))
    ref = MotionRef(v, t)
    q, qv, fext = _state(ref.r, clamp, seed=101)
    g = FemIntegrator(v, t, fixed, matrix_precision=F64, **TIGHT)
    g.set_constrained_motion(moved, u)
    g.set_q_state(q, qv)
    g.set_external_forces(fext)
    _, rhs = g.system()
    out = ref.step(q, qv, fext, fixed, moved, u)
    _close(rhs, out["rhs"], 1e-9, "rhs")
    mi = g.motion_info()
    print("n_set %d:" % n_set, mi)
    assert mi["n_dofs"] == n_set
    if n_set == 432:    # every 1-D launch of the unit has a second workgroup
        assert len(far) == 144 and mi["n_listed_elements"] >= 605 and mi["n_touched_nodes"] == 288
    if n_set > 256:
        # the second trip of the sum's strided loop carries weight in the rule's reactions: a million times the bound of the sum
        assert np.abs(out["lam"][256:]).max() > 0
        assert _second_trip(out["lam"], moved) > 1e6 * 1e-12
    _, qb, vb = _steps(g, ref, fixed, moved, u, q, qv, fext, 1, 2e-5)
    lam = _check_reactions(g, ref, fixed, moved, u, qb, vb, fext, 1e-9)    # (sum3 within 1e-12 sum|lambda| of numpy in there)
    if n_set > 256:
        assert np.abs(lam[256:]).max() > 0
    g.close()


# ---- 3. cuts ----------------------------------------------------------------------------------------------------------------------------

def _beam(**kw):
    """the 7 x 3 x 3 beam clamped at i = 0 and held at i = 6, after one step from a random state: (handle, v, t, clamp, far, moved,
    fixed, targets)"""
    v, t, clamp, far, moved, fixed, dofs, u = _held_cube(7, 3, 3)
    g = FemIntegrator(v, t, fixed, matrix_precision=F64, expect_cuts=True, **TIGHT, **kw)
    g.set_constrained_motion(moved, u)
    q, qv, fext = _state(3 * len(_xyz(v)), clamp, seed=71)
    g.set_q_state(q, qv)
    g.set_external_forces(fext)
    g.do_timestep()
    assert np.array_equal(g.get_q_state()[0][moved], u)
    return g, v, t, clamp, far, moved, fixed, u


def _gravity(r):
    f = np.zeros(r)
    f[1::3] = -20.0
    return f


def _carry_cut_run(v, t, fixed, moved, u, q, qv, f0, strip, renumber):
    """a held beam stepped once, cut (state carried) and stepped again against the rule on the mesh it reads back; returns
    (q, qvel, reactions, cut info, motion info, listed elements before the cut)"""
    g = FemIntegrator(v, t, fixed, matrix_precision=F64, expect_cuts=True, renumber=renumber, **TIGHT)
    assert bool(g.renumbering()[0]) == (renumber == fl.FB_RENUMBER_ON)
    g.set_constrained_motion(moved, u)
    g.set_q_state(q, qv)
    g.set_external_forces(f0)
    g.do_timestep()
    listed_before = g.motion_info()["n_listed_elements"]
    n_old = g.n_nodes
    info, _ = g.cut(strip, mode="carry")
    assert info["status"] == fl.FB_CUT_DONE and info["n_new_nodes"] > 0
    d, uu = g.constrained_motion()
    assert np.array_equal(d, moved) and np.array_equal(uu, u)             # the set survived, targets and all
    x0, t2 = g.read_mesh()
    fixed2 = g.constrained_dofs()
    assert len(x0) == n_old + info["n_new_nodes"] and np.array_equal(fixed2, fixed)   # the new nodes are free
    ref = MotionRef(x0, t2)
    qb, vb, _ = g.get_q_state()
    assert np.array_equal(qb[moved], u)
    fext = _gravity(ref.r)
    _steps(g, ref, fixed2, moved, u, qb, vb, fext, 1, 2e-5)
    mi = g.motion_info()
    assert mi["table_builds"] == 2 and mi["table_valid"]
    lam = _check_reactions(g, ref, fixed2, moved, u, qb, vb, fext, 1e-9)
    qa, va, _ = g.get_q_state()
    g.close()
    return qa, va, lam, info, mi, listed_before


def test_carry_cut_through_the_held_elements(gpu):
    """FB_CUT_CARRY with the blade inside the last layer of cells, through the elements of the held face: the set and its targets
    survive bit for bit, the new nodes are free, the table is built again with another element list, and the next step and its
    reactions are the rule's on the mesh read back.  The same under FB_RENUMBER_ON on permuted ids: against the rule on its own mesh,
    and to 2e-5 against a FB_RENUMBER_OFF handle on the same permuted ids.

    Against the run on UNPERMUTED ids the old nodes' q differs by 6.1e-4 of max|q| (measured; printed below, not asserted): the cut
    triangulates each prism by the lowest caller id (subdivide.hip), so permuted ids give another, equally valid, element list and the
    two runs differ by the discretisation, which no arithmetic bound covers.  Every run is held to 2e-5 of the rule on its own mesh."""
    v, t, clamp, far, moved, fixed, dofs, u = _held_cube(7, 3, 3)
    x, tt = _xyz(v), np.asarray(t).reshape(-1, 4)
    n_old = len(x)
    xs = np.unique(x[:, 0])
    assert np.searchsorted(xs, xs[0] + 0.9 * (xs[-1] - xs[0])) == len(xs) - 1    # _mid_plane's cell at frac = 0.9: the last layer
    strip = _mid_plane(x, frac=0.9)
    q, qv, f0 = _state(3 * n_old, clamp, seed=71)
    qa, va, lam_a, info, mi, listed_before = _carry_cut_run(v, t, fixed, moved, u, q, qv, f0, strip, fl.FB_RENUMBER_OFF)
    assert mi["n_listed_elements"] != listed_before                        # the cut went through the listed elements
    # ... permuted ids, with and without an internal order behind the ABI
    perm = np.random.default_rng(3).permutation(n_old)                    # ai.scrambled's: new id of old node
    v2, t2p, fixed_p = ai.scrambled(x, tt, fixed)
    dmap = (3 * perm[:, None] + np.arange(3)[None]).reshape(-1)           # new DOF of old DOF
    order = np.argsort(dmap[moved])
    moved_p, u_p = dmap[moved][order].astype(np.int32), u[order]
    q2, qv2, f2 = np.zeros_like(q), np.zeros_like(qv), np.zeros_like(f0)
    q2[dmap], qv2[dmap], f2[dmap] = q, qv, f0
    on = _carry_cut_run(v2, t2p, fixed_p, moved_p, u_p, q2, qv2, f2, strip, fl.FB_RENUMBER_ON)
    off = _carry_cut_run(v2, t2p, fixed_p, moved_p, u_p, q2, qv2, f2, strip, fl.FB_RENUMBER_OFF)
    _close(on[0], off[0], 2e-5, "q, renumbered against not, permuted ids")
    _close(on[1], off[1], 2e-4, "qvel, renumbered against not, permuted ids")
    _close(on[2], off[2], 2e-5, "reactions, renumbered against not, permuted ids")
    for r in (on, off):
        assert r[3]["n_new_nodes"] == info["n_new_nodes"] and r[4]["n_listed_elements"] != r[5]
    assert on[4]["n_listed_elements"] == off[4]["n_listed_elements"]
    err = np.abs(on[0][dmap] - qa[:3 * n_old]).max() / np.abs(qa).max()
    print("q of the old nodes, permuted against unpermuted ids (another triangulation of the cut prisms): %.2e of max|q|" % err)


def test_bake_cut_keeps_the_world_space_targets(gpu):
    """FB_CUT_BAKE (Deformable.cut's default) adds q to the rest positions and zeroes the state.  A cut does not move a held node's
    world-space target: the targets come back as u - q_c, here exactly 0, the held nodes stay where they are and end the step with
    qvel = 0."""
    g, v, t, clamp, far, moved, fixed, u = _beam()
    x_old = g.read_mesh()[0]
    q_before = g.get_q_state()[0]
    info, _ = g.cut(_mid_plane(_xyz(v)), mode="bake")
    assert info["status"] == fl.FB_CUT_DONE and info["n_new_nodes"] > 0
    x0, t2 = g.read_mesh()
    assert np.array_equal(x0[:len(x_old)], x_old + q_before.reshape(-1, 3))          # x0 += q, bit for bit: the held nodes at x0_old + u
    assert np.array_equal(x0[far], x_old[far] + u.reshape(-1, 3))
    qc, vc, _ = g.get_q_state()
    assert not qc.any() and not vc.any()
    d, uu = g.constrained_motion()
    assert np.array_equal(d, moved)
    assert np.array_equal(uu, u - q_before[moved]) and not uu.any()                  # exactly 0.0
    fixed2 = g.constrained_dofs()
    assert np.array_equal(fixed2, fixed)
    # a step under no load: the rule from rest on the mesh read back.  Everything stays at rest up to the rounding of the forces of an
    # undeformed element, so the bounds are taken of the distance a kept target would have moved the held nodes by, max|u| (and /h)
    ref = MotionRef(x0, t2)
    zero = np.zeros(ref.r)
    out = ref.step(zero, zero, zero, fixed2, moved, uu)
    g.set_external_forces(zero)
    g.do_timestep()
    qa, va, _ = g.get_q_state()
    eq, ev = np.abs(qa - out["q"]).max(), np.abs(va - out["qvel"]).max()
    print("after the baked cut: q off by %.3e (bound 2e-5 of %.3e), qvel by %.3e (bound 2e-4 of %.3e)" % (eq, np.abs(u).max(), ev, np.abs(u).max() / ref.h))
    assert eq <= 2e-5 * np.abs(u).max() and ev <= 2e-4 * np.abs(u).max() / ref.h
    assert not qa[moved].any() and not va[moved].any()                               # exactly 0
    assert g.motion_info()["table_builds"] == 2
    g.close()


def test_bake_cut_with_targets_ahead_of_the_state(gpu):
    """The targets are changed to u / 2 after the step and before the baked cut: they come back as u / 2 - u, the next step is the
    rule's from rest on the mesh read back, and the held nodes reach the world position they reach in a twin that was not cut."""
    g, v, t, clamp, far, moved, fixed, u = _beam()
    twin, *_ = _beam()
    for h in (g, twin):
        h.set_constrained_motion(moved, 0.5 * u)
    x_old = g.read_mesh()[0]
    info, _ = g.cut(_mid_plane(_xyz(v)), mode="bake")
    assert info["status"] == fl.FB_CUT_DONE
    d, uu = g.constrained_motion()
    want = 0.5 * u - u
    assert np.array_equal(d, moved) and np.all(np.abs(uu - want) <= np.spacing(np.abs(want))) and np.abs(uu).max() > 1e-3
    x0, t2 = g.read_mesh()
    ref = MotionRef(x0, t2)
    zero = np.zeros(ref.r)
    fixed2 = g.constrained_dofs()
    _, qb, vb = _steps(g, ref, fixed2, moved, uu, zero, zero, zero, 1, 2e-5)
    _check_reactions(g, ref, fixed2, moved, uu, qb, vb, zero, 1e-9)
    twin.set_external_forces(np.zeros(twin.r))
    twin.do_timestep()
    world = (x0 + g.get_q_state()[0].reshape(-1, 3))[far]
    world_twin = (x_old + twin.get_q_state()[0].reshape(-1, 3))[far]
    err = np.abs(world - world_twin).max()
    print("held nodes, cut against uncut: %.3e apart (bound 2e-5 of %.3e)" % (err, np.abs(u).max()))
    assert err <= 2e-5 * np.abs(u).max()
    g.close(); twin.close()


def _rotation(th):
    return np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])


def _grasp_targets(p_grab, x0, R, tr, pivot):
    return ((p_grab - pivot) @ R.T + pivot + tr - x0).reshape(-1)


def test_bake_cut_under_a_grasp(gpu):
    """grasp, grasp_move, a step, a baked cut, grasp_move again: the targets are R (p_grab - pivot) + pivot + t - x0 with the rest
    positions the handle reads back, to 1e-14 of the body's size"""
    v, t, clamp, far = _cube(7, 3, 3)
    x = _xyz(v)
    size = float((x.max(0) - x.min(0)).max())
    q, qv, fext = _state(3 * len(x), clamp, seed=91)
    g = FemIntegrator(v, t, clamp, matrix_precision=F64, expect_cuts=True, **TIGHT)
    g.set_q_state(q, qv)
    g.grasp(far)
    p_grab = x[far] + q.reshape(-1, 3)[far]
    R, tr, pivot = _rotation(0.02), np.array([0.003, -0.001, 0.002]), np.array([0.6, 0.1, 0.1])
    g.grasp_move(R, tr, pivot)
    u1 = g.constrained_motion()[1]
    assert np.abs(u1 - _grasp_targets(p_grab, x[far], R, tr, pivot)).max() <= 1e-14 * size
    g.set_external_forces(fext)
    g.do_timestep()
    info, _ = g.cut(_mid_plane(x), mode="bake")
    assert info["status"] == fl.FB_CUT_DONE
    x0, _ = g.read_mesh()
    assert np.array_equal(x0[far], x[far] + u1.reshape(-1, 3))
    d, uu = g.constrained_motion()
    assert np.array_equal(d, _dofs(far)) and not uu.any()                   # held where they are
    assert g.motion_info()["n_grasp_nodes"] == len(far)
    R2, tr2 = _rotation(-0.03), np.array([0.001, 0.002, -0.001])
    g.grasp_move(R2, tr2, pivot)
    u2 = g.constrained_motion()[1]
    want = _grasp_targets(p_grab, x0[far], R2, tr2, pivot)
    assert np.abs(u2 - want).max() <= 1e-14 * size and np.abs(want).max() > 1e-4
    g.set_external_forces(np.zeros(3 * len(x0)))
    g.do_timestep()
    assert np.array_equal(g.get_q_state()[0][d], u2)
    g.close()


def test_a_callers_own_resync_delta(gpu):
    """fb_fem_resync_delta with the same constrained list: the set and its targets are kept, the state is zero, the step is the
    rule's from rest on the new mesh; with a list that drops two moved DOFs those entries leave the set"""
    for drop in ((), (4, 11)):
        g, v, t, clamp, far, moved, fixed, u = _beam()
        v2, t2, delta = synthetic_cut(_xyz(v), np.asarray(t).reshape(-1, 4))
        gone = moved[list(drop)]
        keep = ~np.isin(moved, gone)
        fixed2 = fixed[~np.isin(fixed, gone)]
        g.resync_delta(delta, fixed2)
        d, uu = g.constrained_motion()
        assert np.array_equal(d, moved[keep]) and np.array_equal(uu, u[keep]), drop
        qc, vc, _ = g.get_q_state()
        assert not qc.any() and not vc.any()
        x0, tt = g.read_mesh()
        assert len(x0) == len(v2) and len(tt) == len(t2)
        ref = MotionRef(x0, tt)
        zero = np.zeros(ref.r)
        fext = _gravity(ref.r)
        _, qb, vb = _steps(g, ref, fixed2, moved[keep], u[keep], zero, zero, fext, 1, 2e-5)
        _check_reactions(g, ref, fixed2, moved[keep], u[keep], qb, vb, fext, 1e-9)
        assert g.motion_info()["table_builds"] == 2 and g.motion_info()["n_dofs"] == keep.sum()
        if drop:
            assert np.abs(g.get_q_state()[0][gone]).min() > 0               # free now: they moved under the load
        g.close()


# ---- 4. detach --------------------------------------------------------------------------------------------------------------------------

def _cut_beam():
    """_beam cut in the middle (state carried): (handle, far, moved, fixed, targets, part of the held face, part of the clamp)"""
    g, v, t, clamp, far, moved, fixed, u = _beam()
    info, _ = g.cut(_mid_plane(_xyz(v)), mode="carry")
    assert info["status"] == fl.FB_CUT_DONE
    assert g.parts()["n_parts"] == 2
    part = g.node_parts()
    held, clamped = int(part[far[0]]), int(part[clamp[0] // 3])
    assert held != clamped and np.all(part[far] == held) and np.all(part[clamp // 3] == clamped)
    return g, far, moved, fixed, u, held, clamped


def _orphan_step(g, fixed, moved, u, tol=2e-5):
    """a step of the handle under a load against the rule on the mesh it reads back, the DOFs of nodes without an element constrained in
    the rule and skipped in the comparison unless the handle constrains them; returns (rule, fext, the step's output, q and qvel before)"""
    x0, tt = g.read_mesh()
    ref = MotionRef(x0, tt)
    fixed, moved = np.asarray(fixed, np.int64), np.asarray(moved, np.int64)
    look = np.ones(ref.r, bool)
    look[np.setdiff1d(ref.orphan_dofs, fixed)] = False
    rng = np.random.default_rng(23)
    fext = _gravity(ref.r) + rng.normal(size=ref.r) * 2.0
    qb, vb, _ = g.get_q_state()
    out = ref.step(qb, vb, fext, fixed, moved, u, orphans_constrained=True)
    g.set_external_forces(fext)
    g.do_timestep()
    qa, va, _ = g.get_q_state()
    _close(qa[look], out["q"][look], tol, "q")
    _close(va[look], out["qvel"][look], 10 * tol, "qvel")
    assert np.array_equal(qa[moved], u)
    # reactions at the handle's own dv (orphan rows are empty in the rule: lambda = -fext there)
    free = look.copy()
    free[fixed] = False
    dv = np.zeros(ref.r)
    dv[free] = (va - vb)[free]
    dv[moved] = (np.asarray(u, np.float64) - qb[moved]) / ref.h - vb[moved]
    lam_ref = reactions_at(ref, qb, vb, fext, moved, dv)
    lam, s3 = g.reactions()
    _close(lam, lam_ref, 1e-9, "reactions")
    s3_np = np.array([lam[moved % 3 == a].sum() for a in range(3)])
    assert np.all(np.abs(s3 - s3_np) <= 1e-12 * np.abs(lam).sum())
    return ref, fext, lam


def test_detach_keep_leaves_the_parent_alone(gpu):
    g, far, moved, fixed, u, held, clamped = _cut_beam()
    twin, *_ = _cut_beam()
    piece, ids, nodes = g.detach_part(held, remove=False)
    assert piece.motion_info()["n_dofs"] == 0 and piece.motion_info()["n_grasp_nodes"] == 0
    local = np.array([int(np.flatnonzero(nodes == f)[0]) for f in far])     # the piece's ids of the held nodes
    assert np.isin(_dofs(np.sort(local)), piece.constrained_dofs()).all()
    assert len(piece.reactions()[0]) == 0
    piece.close()
    for h in (g, twin):
        d, uu = h.constrained_motion()
        assert np.array_equal(d, moved) and np.array_equal(uu, u)
        h.set_external_forces(_gravity(h.r))
        h.do_timestep()
    for x, y in zip(g.get_q_state()[:2] + g.reactions(), twin.get_q_state()[:2] + twin.reactions()):
        assert np.array_equal(x, y)
    assert np.abs(g.reactions()[0]).max() > 0
    g.close(); twin.close()


def test_detach_remove_of_the_held_part(gpu):
    """every DOF of the set sits on a node without elements afterwards: the step succeeds, the held DOFs end at their targets, the
    reactions are -fext there (an empty row of the rule) and the rest of the body steps as the rule says"""
    g, far, moved, fixed, u, held, clamped = _cut_beam()
    piece, _, _ = g.detach_part(held, remove=True)
    piece.close()
    d, uu = g.constrained_motion()
    assert np.array_equal(d, moved) and np.array_equal(uu, u)
    new_u = u + 0.001                                                      # (the held DOFs move: v* != 0)
    g.set_constrained_motion(moved, new_u)
    ref, fext, lam = _orphan_step(g, fixed, moved, new_u)
    assert np.isin(moved, ref.orphan_dofs).all()
    assert g.motion_info()["n_listed_elements"] == 0 and g.motion_info()["table_valid"]
    assert np.array_equal(lam, -fext[moved]) and np.abs(lam).min() > 0
    g.close()


def test_detach_remove_of_the_clamped_part(gpu):
    """the parent is the free-floating held half: step and reactions are the rule's on the mesh read back"""
    g, far, moved, fixed, u, held, clamped = _cut_beam()
    piece, _, _ = g.detach_part(clamped, remove=True)
    piece.close()
    new_u = u + 0.001
    g.set_constrained_motion(moved, new_u)
    ref, fext, lam = _orphan_step(g, fixed, moved, new_u)
    assert not np.isin(moved, ref.orphan_dofs).any() and np.isin(np.setdiff1d(fixed, moved), ref.orphan_dofs).all()
    assert g.motion_info()["n_listed_elements"] > 0
    g.close()


# ---- 5. the grasp's bookkeeping ---------------------------------------------------------------------------------------------------------

def test_grasp_over_the_clamp_and_an_existing_set(gpu):
    v, t, clamp, far = _cube(4)
    extra = np.array([3 * far[0], 3 * far[0] + 1, 3 * far[1], 3 * far[1] + 1], np.int32)
    fixed0 = np.sort(np.concatenate([clamp, extra])).astype(np.int32)
    q, qv, _ = _state(3 * len(_xyz(v)), clamp, seed=111)
    g = FemIntegrator(v, t, fixed0, matrix_precision=F64)
    g.set_q_state(q, qv)
    d0 = np.array([3 * far[0] + 1], np.int32)
    g.set_constrained_motion(d0, [0.002])
    g.grasp(far)
    mine = _dofs(far)
    assert np.array_equal(g.constrained_dofs(), np.union1d(fixed0, mine))
    d, uu = g.constrained_motion()
    assert np.array_equal(d, mine)
    was = d == d0[0]
    assert uu[was][0] == 0.002 and np.array_equal(uu[~was], q[d[~was]]) and np.abs(q[d0[0]] - 0.002) > 0
    assert g.motion_info()["n_grasp_nodes"] == len(far)
    g.release()
    assert np.array_equal(g.constrained_dofs(), fixed0)
    d, uu = g.constrained_motion()
    assert np.array_equal(d, d0) and np.array_equal(uu, [0.002])
    qa, va, _ = g.get_q_state()
    assert np.array_equal(qa, q) and np.array_equal(va, qv)
    assert g.motion_info()["n_grasp_nodes"] == 0
    g.close()


def test_grasp_under_forced_renumbering(gpu):
    """grasp, grasp_move and two steps on permuted ids in a handle that renumbers behind the ABI, against the unpermuted twin"""
    v, t, clamp, far = _cube(5)
    x = _xyz(v)
    size = float((x.max(0) - x.min(0)).max())
    perm = np.random.default_rng(3).permutation(len(x))
    v2, t2, clamp2 = ai.scrambled(x, np.asarray(t).reshape(-1, 4), clamp)
    dmap = (3 * perm[:, None] + np.arange(3)[None]).reshape(-1)
    ref = MotionRef(v, t)
    q, qv, fext = _state(ref.r, clamp, seed=121)
    q2, qv2, fext2 = np.zeros_like(q), np.zeros_like(qv), np.zeros_like(fext)
    q2[dmap], qv2[dmap], fext2[dmap] = q, qv, fext
    a = FemIntegrator(v, t, clamp, matrix_precision=F64, renumber=fl.FB_RENUMBER_OFF, **TIGHT)
    b = FemIntegrator(v2, t2, clamp2, matrix_precision=F64, renumber=fl.FB_RENUMBER_ON, **TIGHT)
    assert b.renumbering()[0] and not a.renumbering()[0]
    a.set_q_state(q, qv)
    b.set_q_state(q2, qv2)
    far2 = np.sort(perm[far]).astype(np.int32)
    a.grasp(far)
    b.grasp(far2)
    moved, moved2 = _dofs(far), _dofs(far2)
    order = np.argsort(dmap[moved])
    assert np.array_equal(dmap[moved][order], moved2)
    (da, ua), (db, ub) = a.constrained_motion(), b.constrained_motion()
    assert np.array_equal(da, moved) and np.array_equal(db, moved2) and np.array_equal(ub, ua[order]) and np.array_equal(ua, q[moved])
    R, tr, pivot = _rotation(0.05), np.array([0.003, -0.002, 0.001]), np.array([0.4, 0.2, 0.2])
    a.grasp_move(R, tr, pivot)
    b.grasp_move(R, tr, pivot)
    want = _grasp_targets(x[far] + q.reshape(-1, 3)[far], x[far], R, tr, pivot)
    ua, ub = a.constrained_motion()[1], b.constrained_motion()[1]
    assert np.abs(ua - want).max() <= 1e-14 * size and np.abs(ub - want[order]).max() <= 1e-14 * size
    fixed = a.constrained_dofs()
    for k in range(2):
        b.set_external_forces(fext2)
        b.do_timestep()
    _, qb_, vb_ = _steps(a, ref, fixed, moved, ua, q, qv, fext, 2, 2e-5)
    _check_reactions(a, ref, fixed, moved, ua, qb_, vb_, fext, 1e-9)
    (qa, va, _), (qb, vb, _) = a.get_q_state(), b.get_q_state()
    _close(qb[dmap], qa, 2e-5, "q, permuted against unpermuted")
    _close(vb[dmap], va, 2e-4, "qvel, permuted against unpermuted")
    inv = np.empty_like(order)
    inv[order] = np.arange(len(order))
    _close(b.reactions()[0][inv], a.reactions()[0], 2e-5, "reactions, permuted against unpermuted")
    a.close(); b.close()


def test_set_constrained_dofs_while_a_grasp_is_held(gpu):
    v, t, clamp, far = _cube(5, 3, 3)
    x = _xyz(v)
    size = float((x.max(0) - x.min(0)).max())
    q, qv, _ = _state(3 * len(x), clamp, seed=131)
    g = FemIntegrator(v, t, clamp, matrix_precision=F64)
    g.set_q_state(q, qv)
    g.grasp(far)
    lost = _dofs(far[2:3])
    own = np.array([3 * 20 + 2], np.int32)                                 # a DOF the caller constrains besides
    assert not np.isin(own, np.union1d(clamp, _dofs(far))).any()
    fixed = np.union1d(np.setdiff1d(g.constrained_dofs(), lost), own).astype(np.int32)
    g.set_constrained_dofs(fixed)
    rest = np.setdiff1d(_dofs(far), lost)
    d, uu = g.constrained_motion()
    assert np.array_equal(d, rest) and np.array_equal(uu, q[rest])
    assert g.motion_info()["n_dofs"] == 3 * len(far) - 3
    R, tr, pivot = _rotation(0.2), np.array([0.01, 0.0, -0.01]), np.array([0.2, 0.1, 0.1])
    g.grasp_move(R, tr, pivot)
    want = _grasp_targets(x[far] + q.reshape(-1, 3)[far], x[far], R, tr, pivot)
    d, uu = g.constrained_motion()
    assert np.array_equal(d, rest) and np.abs(uu - want[np.isin(_dofs(far), rest)]).max() <= 1e-14 * size
    qa, va, _ = g.get_q_state()
    assert np.array_equal(qa, q) and np.array_equal(va, qv)
    g.release()
    assert np.array_equal(g.constrained_dofs(), np.union1d(clamp, own)) and g.motion_info()["n_dofs"] == 0
    g.close()


# ---- 6. an inverted listed element ----------------------------------------------------------------------------------------------------------

def _det_f(x0, t, q):
    X, P = x0[t], (x0 + q.reshape(-1, 3))[t]
    return np.linalg.det(np.transpose(P[:, 1:] - P[:, :1], (0, 2, 1))) / np.linalg.det(np.transpose(X[:, 1:] - X[:, :1], (0, 2, 1)))


def _inverted_case():
    """4^3 with the far plane held: a free node of an element at the held face pushed through the element's opposite face, so that
    det F is -0.5 there and every other element keeps det F > 0.2.  Returns (v, t, clamp, moved, fixed, targets, q, element)"""
    v, t, clamp, far, moved, fixed, dofs, u = _held_cube(4)
    x0, tt = _xyz(v), np.asarray(t, np.int64).reshape(-1, 4)
    free_node = np.ones(len(x0), bool)
    free_node[np.asarray(fixed) // 3] = False
    q0 = _state(3 * len(x0), clamp, seed=143)[0] * 0.3
    q0[moved] = u
    for e in np.flatnonzero(np.isin(tt, far).any(axis=1)):
        for k in range(4):
            n = tt[e, k]
            if not free_node[n]:
                continue
            a, b, c = x0[tt[e, [j for j in range(4) if j != k]]]
            nrm = np.cross(b - a, c - a)
            nrm /= np.linalg.norm(nrm)
            height = (x0[n] - a) @ nrm
            q = q0.copy()
            q[3 * n:3 * n + 3] += -1.5 * height * nrm                      # det F of e: 1 - 1.5
            det = _det_f(x0, tt, q)
            if det[e] < -0.2 and np.all(np.delete(det, e) > 0.2):
                return v, t, clamp, moved, fixed, u, q, int(e)
    raise AssertionError("no element of the held face can be inverted alone")


def test_an_inverted_listed_element(gpu):
    """det F < 0 in one listed element: the negated rotation of k_motion_elements<., true> against k_tet_warp's and the oracle's"""
    v, t, clamp, moved, fixed, u, q, e = _inverted_case()
    x0, tt = _xyz(v), np.asarray(t, np.int64).reshape(-1, 4)
    det = _det_f(x0, tt, q)
    assert det[e] < 0 and abs(det[e]) > 0.2 and (det < 0).sum() == 1 and np.isin(tt[e], moved // 3).any()
    ref = MotionRef(v, t)
    _, qv, fext = _state(ref.r, clamp, seed=141)
    g = FemIntegrator(v, t, fixed, matrix_precision=F64, **TIGHT)
    g.set_constrained_motion(moved, u)
    g.set_q_state(q, qv)
    g.set_external_forces(fext)
    _, rhs = g.system()
    _close(rhs, ref.step(q, qv, fext, fixed, moved, u)["rhs"], 1e-9, "rhs")
    g.do_timestep()
    lam = _check_reactions(g, ref, fixed, moved, u, q, qv, fext, 1e-9)
    # ... and inside the device: the reactions formed from the rest records against those formed from the matrices of a handle without
    # constraints at the same state (its system() is the unmasked Keff and -h g)
    free = np.ones(ref.r, bool)
    free[fixed] = False
    dv = np.zeros(ref.r)
    dv[free] = (g.get_q_state()[1] - qv)[free]
    dv[moved] = (u - q[moved]) / ref.h - qv[moved]
    w = FemIntegrator(v, t, (), matrix_precision=F64)
    w.set_q_state(q, qv)
    w.set_external_forces(fext)
    K, rhs0 = w.system()
    Keff = bsr_to_scipy(*w.pattern(), K)
    lam_dev = ((Keff @ dv) / ref.h - rhs0 / ref.h)[moved]
    _close(lam, lam_dev, 1e-12, "reactions from the rest records against the handle's own matrices")
    w.close(); g.close()
