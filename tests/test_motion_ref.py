"""tests/motionref.py (the rule of constrained motion in NumPy) pinned on the CPU: with targets 0 on the clamp it is the oracle's step,
and its reactions close the momentum balance."""
import numpy as np
import pytest

import fem_params as fp
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, truth_cube
from motionref import MotionRef, momentum_terms
from oracle.pyoracle import OrcFem


def _cube(n):
    v, t = truth_cube(n, n, n, 0.1)
    return v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))


def test_zero_targets_on_the_clamp_are_the_oracles_step():
    """Three steps under the reference load with the whole clamp in the set at target 0: q within 2e-5 of max|q| of OrcFem.step(),
    qvel within ten times that -- the fp64 bound of test_three_steps_reference_load (a direct solve against a PCG at 1e-6)."""
    v, t, fixed = _cube(6)
    o = OrcFem(v, t)
    o.integrator(fixed)
    ref = MotionRef(v, t)
    fext = np.zeros(o.r)
    fext[1::3] = -10000.0
    q, qv = np.zeros(o.r), np.zeros(o.r)
    for k in range(3):
        o.set_external_forces(fext)
        o.step()
        out = ref.step(q, qv, fext, fixed, fixed, np.zeros(len(fixed)))
        q, qv = out["q"], out["qvel"]
        qo, vo = o.get_state()
        assert np.abs(q - qo).max() <= 2e-5 * np.abs(qo).max(), k
        assert np.abs(qv - vo).max() <= 2e-4 * np.abs(vo).max(), k
        assert not q[fixed].any() and not qv[fixed].any()
        # ... and an empty set is the same rule
        assert np.array_equal(ref.step(q, qv, fext, fixed)["q"][fixed], np.zeros(len(fixed)))


@pytest.mark.parametrize("name", fp.NAMES)
def test_zero_targets_on_the_clamp_are_the_oracles_step_at_every_parameter_set(name):
    """One step from fem_params.live_state under fem_params.load with the whole clamp in the set at target 0, at every parameter set:
    the bounds of the pin above against OrcFem.step() solved to 1e-12 (at the oracle's default 1e-6 the two differ by up to 1e-4 at
    near_incomp, which is where that PCG stops and not the rule)."""
    v, t, fixed = _cube(5)
    o = OrcFem(v, t, **fp.material(name))
    o.integrator(fixed, **fp.integrator(name))
    ref = MotionRef(v, t, **fp.material(name), **fp.integrator(name))
    q, qv = fp.live_state(o.r, fixed)
    fext = fp.load(name, o.r)
    o.set_state(q, qv)
    o.set_external_forces(fext)
    o.step(cg_eps=1e-12, cg_maxiter=20000)
    out = ref.step(q, qv, fext, fixed, fixed, np.zeros(len(fixed)))
    qo, vo = o.get_state()
    eq, ev = np.abs(out["q"] - qo).max() / np.abs(qo).max(), np.abs(out["qvel"] - vo).max() / np.abs(vo).max()
    print("%s: q %.2e (bound 2e-5), qvel %.2e (bound 2e-4)" % (name, eq, ev))
    assert eq <= 2e-5 and ev <= 2e-4
    assert not out["q"][fixed].any() and not out["qvel"][fixed].any()


def _moved_case(v, fixed, r, seed=11):
    """the far plane moved by random targets, the clamp at 0, a random state and load: (every constrained DOF, targets, q, qvel, fext)"""
    rng = np.random.default_rng(seed)
    x = np.asarray(v).reshape(-1, 3)[:, 0]
    far = np.flatnonzero(np.isclose(x, x.max()))
    moved = np.sort(np.concatenate([3 * far, 3 * far + 1, 3 * far + 2]))
    allc = np.sort(np.concatenate([fixed, moved]))
    u = np.zeros(len(allc))
    u[np.isin(allc, moved)] = rng.normal(size=len(moved)) * 0.004
    q, qv = rng.normal(size=r) * 0.003, rng.normal(size=r) * 0.05
    q[fixed] = 0
    qv[fixed] = 0
    return allc, u, q, qv, rng.normal(size=r) * 5.0


@pytest.mark.parametrize("name", fp.NAMES)
def test_reactions_close_the_momentum_balance_at_every_parameter_set(name):
    """cM != 0 too: sum(lambda) + sum(fext) - ((1 + h cM) / h) sum_b m_b dv_b - cM sum_b m_b qvel_b = -(1/h) sum_f r_f by axis, to 1e-10
    of the largest term (measured: 3e-11 at the worst set); where cM > 0 the new term is not small change"""
    v, t, fixed = _cube(4)
    ref = MotionRef(v, t, **fp.material(name), **fp.integrator(name))
    allc, u, q, qv, fext = _moved_case(v, fixed, ref.r)
    fext *= fp.PARAMS[name]["E"] / 1e7
    out = ref.step(q, qv, fext, allc, allc, u)
    terms = momentum_terms(ref, q, qv, fext, allc, out["dv"], out["residual"], lam=out["lam"])
    gap, big = np.abs(terms.sum(axis=1)).max(), np.abs(terms).max()
    print("%s: gap %.2e of %.2e (%.1e relative, bound 1e-10)" % (name, gap, big, gap / big))
    assert terms.shape == (3, 5) and gap <= 1e-10 * big, terms
    assert np.abs(terms[:, 0]).max() > 1e-3 * big
    if ref.cM > 0:
        assert np.abs(terms[:, 3]).max() > 100 * 1e-10 * big       # the c_M qvel term: a balance without it misses the bound a hundredfold
    else:
        assert not terms[:, 3].any()


def test_orphan_nodes_constrained():
    """Two nodes that no element uses (what FB_DETACH_REMOVE leaves): with orphans_constrained the step is the step of the mesh without
    them, bit for bit, an orphan DOF of the set ends at its target with lambda = -fext, and the others end at 0"""
    v, t, fixed = _cube(4)
    ref = MotionRef(v, t)
    allc, u, q, qv, fext = _moved_case(v, fixed, ref.r)
    out = ref.step(q, qv, fext, allc, allc, u)
    v2 = np.concatenate([np.asarray(v, np.float64).reshape(-1, 3), [[9.0, 9.0, 9.0], [9.5, 9.0, 9.0]]])
    ref2 = MotionRef(v2, t)
    r = ref.r
    assert np.array_equal(ref2.orphan_dofs, np.arange(r, r + 6)) and len(ref.orphan_dofs) == 0
    rng = np.random.default_rng(5)
    pad = lambda x: np.concatenate([x, rng.normal(size=6)])
    q2, qv2, fext2 = pad(q), pad(qv), pad(fext)
    held = np.array([r + 1, r + 3])                                  # one DOF of each orphan is held and moved
    allc2, u2 = np.concatenate([allc, held]), np.concatenate([u, [0.01, -0.02]])
    out2 = ref2.step(q2, qv2, fext2, allc2, allc2, u2, orphans_constrained=True)
    for k in ("q", "qvel", "dv", "rhs"):
        assert np.array_equal(out2[k][:r], out[k]), k
    assert np.array_equal(out2["lam"][:len(allc)], out["lam"])
    assert np.array_equal(out2["q"][held], [0.01, -0.02]) and np.array_equal(out2["lam"][len(allc):], -fext2[held])
    rest = np.setdiff1d(ref2.orphan_dofs, held)
    assert not out2["q"][rest].any() and not out2["qvel"][rest].any() and not out2["rhs"][rest].any()


@pytest.mark.parametrize("warp", [0, 1])
def test_reactions_close_the_momentum_balance(warp):
    """cM = 0: sum(lambda) + sum(fext) - (1/h) sum_b m_b dv_b = -(1/h) sum_f r_f by axis, to 1e-10 of the largest term (lambda over
    every constrained DOF: the clamp at target 0 and the moved plane are both in the set)."""
    n = 4
    v, t, fixed = _cube(n)
    ref = MotionRef(v, t, warp=warp, cM=0.0, cK=0.01)
    rng = np.random.default_rng(11)
    far = np.flatnonzero(np.isclose(np.asarray(v).reshape(-1, 3)[:, 0], np.asarray(v).reshape(-1, 3)[:, 0].max()))
    moved = np.sort(np.concatenate([3 * far, 3 * far + 1, 3 * far + 2]))
    allc = np.sort(np.concatenate([fixed, moved]))
    u = np.zeros(len(allc))
    u[np.isin(allc, moved)] = rng.normal(size=len(moved)) * 0.004
    q, qv = rng.normal(size=ref.r) * 0.003, rng.normal(size=ref.r) * 0.05
    q[fixed] = 0
    qv[fixed] = 0
    fext = rng.normal(size=ref.r) * 5.0
    out = ref.step(q, qv, fext, allc, allc, u)
    assert np.array_equal(out["q"][allc], u)
    terms = momentum_terms(ref, q, qv, fext, allc, out["dv"], out["residual"], lam=out["lam"])
    assert np.abs(terms.sum(axis=1)).max() <= 1e-10 * np.abs(terms).max(), terms
    # the reactions are not small change: they carry the balance
    assert np.abs(terms[:, 0]).max() > 1e-3 * np.abs(terms).max()
    assert np.allclose(out["lam_sum"], terms[:, 0], rtol=1e-12, atol=0)
