"""tests/motionref.py (the rule of constrained motion in NumPy) pinned on the CPU: with targets 0 on the clamp it is the oracle's step,
and its reactions close the momentum balance."""
import numpy as np
import pytest

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
