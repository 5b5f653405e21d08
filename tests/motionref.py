"""TEST INFRASTRUCTURE ONLY -- the rule of constrained motion ("Constrained motion" in include/fembrain_hip.h) in
NumPy / SciPy, on the oracle's matrices.

A motion set is a subset of the constrained DOFs with target displacements u_c.  One step from (q, qvel, fext):

    f, K   = OrcFem.assemble(q)            (on the oracle's CSR pattern; warp 0 / 1 / 2 through its setters)
    M      = OrcFem.mass_on_pattern()
    Keff   = h (h + cK) K + (1 + h cM) M                    (unmasked)
    rhs    = -h ((h K + D) qvel + f - fext),  D = cK K + cM M
    v*_c   = (u_c - q_c) / h,   dv_c = v*_c - qvel_c        (DOFs of the set; every other constrained DOF has dv = 0)
    Keff_ff dv_f = rhs_f - Keff_fc dv_c                     (scipy.sparse.linalg.spsolve)
    qvel_f += dv_f, q_f += h qvel_f;   q_c = u_c, qvel_c = v*_c;   other constrained DOFs: q = qvel = 0
    lambda_c = (1/h) [Keff dv]_c + [(h K + D) qvel + f - fext]_c      (dv: all DOFs, the moved ones included; qvel before the step)

Per-element materials go through tests/matref.py (sums of uniform oracles per element), whose f, K and M have the same layout.
tests/test_motion_ref.py pins this file against OrcFem.step() (targets 0 on the clamp) and by the momentum identity.

Orphan nodes (no element: what FB_DETACH_REMOVE leaves behind) have empty rows here and identity rows on the device; with
``orphans_constrained`` step() treats their DOFs as constrained (the free block would be singular otherwise), ``orphan_dofs`` lists them
and comparisons skip those that are neither in the caller's constrained list nor in the set.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle.pyoracle import OrcFem


class MotionRef:
    def __init__(self, verts, tets, E=1e7, nu=0.46, rho=1000.0, warp=1, timestep=0.0333, cM=0.0, cK=0.01, materials=None, ids=None):
        """materials / ids: [(E, nu, rho)] and one id per element (MatRef); else the uniform oracle of (E, nu, rho)"""
        self.h, self.cM, self.cK = float(timestep), float(cM), float(cK)
        self.mat = None
        used = np.zeros(len(np.asarray(verts).reshape(-1, 3)), bool)
        used[np.asarray(tets, np.int64).reshape(-1)] = True
        lone = np.flatnonzero(~used)
        self.orphan_dofs = (3 * lone[:, None] + np.arange(3)[None]).reshape(-1)   # DOFs of nodes that no element uses, ascending
        if materials is not None:
            from matref import MatRef
            self.mat = MatRef(verts, tets, materials, ids, warp=warp)
            self.r = self.mat.r
            self.ia, self.ja = self.mat.ia, self.mat.ja
            self.Mv = self.mat.mass_csr_values()
        else:
            self.orc = OrcFem(verts, tets, E=E, nu=nu, rho=rho)
            self.orc.set_warp(warp)
            self.r = self.orc.r
            self.ia, self.ja = self.orc.csr()
            self.Mv = self.orc.mass_on_pattern()
        self.M = self.csr(self.Mv)

    def csr(self, values):
        return sp.csr_matrix((np.asarray(values, np.float64), self.ja, self.ia), shape=(self.r, self.r))

    def assemble(self, q):
        """(f, K as a scipy CSR matrix) at displacement q"""
        q = np.ascontiguousarray(q, np.float64)
        if self.mat is not None:
            f, Kb = self.mat.assemble(q)
            return f, self.csr(self.mat.blocks_to_csr(Kb))
        f, Kv = self.orc.assemble(q)
        return f, self.csr(Kv)

    def system(self, q, qvel, fext):
        """(Keff, rhs before the correction, g = (hK + D) qvel + f - fext) on all DOFs"""
        h, cM, cK = self.h, self.cM, self.cK
        f, K = self.assemble(q)
        keff = (h * (h + cK)) * K + (1.0 + h * cM) * self.M
        g = ((h + cK) * K + cM * self.M) @ np.asarray(qvel, np.float64) + f - np.asarray(fext, np.float64)
        return keff.tocsr(), -h * g, g

    def step(self, q, qvel, fext, fixed, dofs=(), targets=(), orphans_constrained=False):
        """One step.  fixed: every constrained DOF; dofs / targets: the motion set (a subset of fixed).  Returns a dict: q, qvel (after),
        dv (all DOFs), rhs (the corrected right-hand side, 0 on constrained rows), lam (reactions in the set's order), lam_sum (3,),
        residual (r = Keff_ff dv_f - rhs_f on all DOFs, 0 on constrained ones), keff.  orphans_constrained: the DOFs of nodes without an
        element count as constrained too (q = qvel = 0 after the step unless they are in the set)"""
        h = self.h
        q = np.array(q, np.float64)
        qvel = np.array(qvel, np.float64)
        fixed = np.asarray(fixed, np.int64).reshape(-1)
        dofs = np.asarray(dofs, np.int64).reshape(-1)
        u = np.asarray(targets, np.float64).reshape(-1)
        assert len(dofs) == len(u) and np.isin(dofs, fixed).all()
        free = np.ones(self.r, bool)
        free[fixed] = False
        if orphans_constrained:
            free[self.orphan_dofs] = False
        keff, rhs0, g = self.system(q, qvel, fext)
        vstar = (u - q[dofs]) / h
        dv = np.zeros(self.r)
        dv[dofs] = vstar - qvel[dofs]
        rhs = np.zeros(self.r)
        rhs[free] = rhs0[free] - (keff @ dv)[free]
        A = keff[free][:, free].tocsc()
        dv[free] = spla.spsolve(A, rhs[free])
        residual = np.zeros(self.r)
        residual[free] = A @ dv[free] - rhs[free]
        lam = (keff @ dv)[dofs] / h + g[dofs]
        qn, vn = np.zeros(self.r), np.zeros(self.r)
        vn[free] = qvel[free] + dv[free]
        qn[free] = q[free] + h * vn[free]
        qn[dofs] = u
        vn[dofs] = vstar
        lam_sum = np.array([lam[dofs % 3 == a].sum() for a in range(3)])
        return dict(q=qn, qvel=vn, dv=dv, rhs=rhs, lam=lam, lam_sum=lam_sum, residual=residual, keff=keff)


def reactions_at(ref, q, qvel, fext, dofs, dv):
    """lambda of the rule at the DOFs ``dofs`` for a given dv on all DOFs (the device's own, say): (1/h) [Keff dv]_c + g_c"""
    keff, _, g = ref.system(q, qvel, fext)
    dofs = np.asarray(dofs, np.int64)
    return (keff @ np.asarray(dv, np.float64))[dofs] / ref.h + g[dofs]


def momentum_terms(ref, q, qvel, fext, fixed, dv, residual, lam=None):
    """The five terms of the momentum identity by axis, (3, 5): sum(lambda over ALL constrained DOFs; ``lam``, in the order of
    ``fixed``, where the caller has its own -- the device's -- else formed here from dv), sum(fext),
    -((1 + h cM) / h) sum_b m_b dv_b, -cM sum_b m_b qvel_b, (1/h) sum_f r_f.  They add up to zero for ANY dv whose free rows leave the
    residual r: the rows of K sum to zero over the nodes and so does f, so summing (1/h) Keff dv + (hK + D) qvel + f - fext over all
    rows of an axis leaves ((1 + h cM) / h) sum_b m_b dv_b + cM sum_b m_b qvel_b - sum fext (m_b: the column sums of M; D = cK K + cM M);
    the free rows contribute (1/h) r (r = Keff_ff dv_f - rhs_f: they solve the system up to r), the constrained rows lambda.  That is
    sum(lambda) + sum(fext) - ((1 + h cM) / h) sum_b m_b dv_b - cM sum_b m_b qvel_b = -(1/h) sum_f r_f."""
    h, cM = ref.h, ref.cM
    keff, _, g = ref.system(q, qvel, fext)
    fixed = np.asarray(fixed, np.int64)
    lam_all = (keff @ dv)[fixed] / h + g[fixed] if lam is None else np.asarray(lam, np.float64)
    mcol = np.asarray(ref.M.sum(axis=0)).reshape(-1)
    qvel = np.asarray(qvel, np.float64)
    out = np.zeros((3, 5))
    for a in range(3):
        out[a, 0] = lam_all[fixed % 3 == a].sum()
        out[a, 1] = np.asarray(fext, np.float64)[a::3].sum()
        out[a, 2] = -(1.0 + h * cM) * (mcol[a::3] * dv[a::3]).sum() / h
        out[a, 3] = -cM * (mcol[a::3] * qvel[a::3]).sum()
        out[a, 4] = residual[a::3].sum() / h
    return out
