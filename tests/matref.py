"""TEST INFRASTRUCTURE ONLY -- the heterogeneous FEM system restated from uniform oracles.

f, K and M are sums over elements, and an element's terms depend on its own material only.  So the answer for a mesh whose elements
have different materials is a sum of uniform answers: every element's (f_e, K_e) comes from ``OrcFem.element(e, u)`` of the
full-mesh uniform oracle of ITS material and is scattered as ``orc_fem_assemble`` scatters (oracle/fem_oracle.c:298-311); the mass
is ``rho_e V_e / 20 (1 + delta_ij)`` per block (tetMesh.cpp:171, generateMassMatrix.cpp), inflated to the three DOFs of a node.
On top of them, as ``orc_build_system`` / ``orc_step`` write them:

    Keff = h (h + c_K) K + (1 + h c_M) M
    rhs  = -h ((h K + D) qdot + f_int - f_ext),   D = c_K K + c_M M
    Keff[free, free] dv = rhs[free]               (sparse direct solve)
    qdot += dv;  q += h qdot;  clamped DOFs zero

tests/test_materials_ref.py pins this file against the uniform oracle (all ids equal) and against sums of the reference's own
sub-mesh assemblies (tests/golden/fem_cube5_materials.npz).
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle.pyoracle import OrcFem, orc_pcg


def region_ids(verts, tets, mean=None):
    """The three-region function of the tests: ids = min(2, [cx > mean] + 2 [cy > mean and cz > mean]) over element centroids
    (mean: of the vertices, unless given -- the planes of a mesh BEFORE a cut, for the pieces after it)"""
    c = np.asarray(verts, np.float64).reshape(-1, 3)[np.asarray(tets).reshape(-1, 4)].mean(axis=1)
    m = np.asarray(verts, np.float64).reshape(-1, 3).mean(axis=0) if mean is None else np.asarray(mean, np.float64)
    return np.minimum(2, (c[:, 0] > m[0]).astype(np.int64) + 2 * ((c[:, 1] > m[1]) & (c[:, 2] > m[2]))).astype(np.uint8)


def three_materials():
    """default / soft_damped of tests/fem_params.py / (5e7, 0.2, 800): [(E, nu, rho)] * 3"""
    import fem_params as fp
    d, s = fp.PARAMS["default"], fp.PARAMS["soft_damped"]
    return [(d["E"], d["nu"], d["rho"]), (s["E"], s["nu"], s["rho"]), (5e7, 0.2, 800.0)]


class MatRef:
    def __init__(self, verts, tets, materials, ids, warp=1):
        self.v = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
        self.t = np.ascontiguousarray(tets, np.int32).reshape(-1, 4)
        self.materials = [tuple(float(x) for x in m) for m in materials]
        self.ids = np.asarray(ids, np.int64).reshape(-1)
        assert len(self.ids) == len(self.t) and (self.ids >= 0).all() and (self.ids < len(self.materials)).all()
        self.nv, self.nt, self.r = len(self.v), len(self.t), 3 * len(self.v)
        self.orc = {}
        for m in np.unique(self.ids):
            E, nu, rho = self.materials[m]
            o = OrcFem(self.v, self.t, E=E, nu=nu, rho=rho)
            o.set_warp(warp)
            self.orc[int(m)] = o
        o = next(iter(self.orc.values()))
        self.ia, self.ja = o.csr()
        self.bptr, self.bcol = o.blocks()
        self.nblk = len(self.bcol)
        # the block of (row node t[e, i], column node t[e, j])
        self.elblk = np.empty((self.nt, 4, 4), np.int64)
        for e in range(self.nt):
            for i in range(4):
                a = self.t[e, i]
                row = self.bcol[self.bptr[a]:self.bptr[a + 1]]
                self.elblk[e, i] = self.bptr[a] + np.searchsorted(row, self.t[e])
        assert np.array_equal(self.bcol[self.elblk], np.broadcast_to(self.t[:, None, :], self.elblk.shape))

    # ---- layouts ----
    def blocks_to_csr(self, Kb):
        """[nblk, 3, 3] in block order -> values on the oracle's scalar CSR pattern"""
        Kb = np.asarray(Kb).reshape(self.nblk, 3, 3)
        out = np.empty(len(self.ja))
        for a in range(self.nv):
            seg = Kb[self.bptr[a]:self.bptr[a + 1]]
            for k in range(3):
                out[self.ia[3 * a + k]:self.ia[3 * a + k + 1]] = seg[:, k, :].reshape(-1)
        return out

    def csr(self, values):
        return sp.csr_matrix((np.asarray(values, np.float64), self.ja, self.ia), shape=(self.r, self.r))

    # ---- element sums ----
    def assemble(self, u):
        """(f, K blocks [nblk, 3, 3]) at displacement u: the per-element scatter from the uniform oracles"""
        u = np.ascontiguousarray(u, np.float64)
        f, Kb = np.zeros(self.r), np.zeros((self.nblk, 3, 3))
        for e in range(self.nt):
            _, Ke, fe = self.orc[int(self.ids[e])].element(e, u)
            for j in range(4):
                f[3 * self.t[e, j]:3 * self.t[e, j] + 3] += fe[3 * j:3 * j + 3]
            for i in range(4):
                for j in range(4):
                    Kb[self.elblk[e, i, j]] += Ke[3 * i:3 * i + 3, 3 * j:3 * j + 3]
        return f, Kb

    def volumes(self):
        p = self.v[self.t]
        return np.abs(np.einsum("ij,ij->i", p[:, 0] - p[:, 3], np.cross(p[:, 1] - p[:, 3], p[:, 2] - p[:, 3]))) / 6.0

    def mass_blocks(self):
        """m_ab = sum_e rho_e V_e / 20 (1 + delta_ij), one value per block"""
        rho = np.array([m[2] for m in self.materials])[self.ids]
        w = rho * self.volumes() / 20.0
        mb = np.zeros(self.nblk)
        for e in range(self.nt):
            for i in range(4):
                for j in range(4):
                    mb[self.elblk[e, i, j]] += w[e] * (2.0 if i == j else 1.0)
        return mb

    def mass_csr_values(self):
        """the mass inflated x3 on the stiffness pattern (zero off the block diagonals), as orc_fem_mass_on_pattern lays it out"""
        mb = self.mass_blocks()
        return self.blocks_to_csr(mb[:, None, None] * np.eye(3)[None])

    # ---- the step ----
    def system(self, q, qvel, fext, h, cM, cK):
        """(Keff CSR values, rhs, f_int) on all DOFs, as orc_build_system forms them"""
        f, Kb = self.assemble(q)
        K = self.blocks_to_csr(Kb)
        M = self.mass_csr_values()
        D = cK * K + cM * M
        keff = h * (h + cK) * K + (1.0 + h * cM) * M
        rhs = -h * (self.csr(h * K + D) @ np.asarray(qvel, np.float64) + f - np.asarray(fext, np.float64))
        return keff, rhs, f

    def free(self, fixed):
        fr = np.ones(self.r, bool)
        fr[np.asarray(fixed, np.int64)] = False
        return fr

    def solve(self, keff, rhs, fixed):
        """dv by a sparse direct solve on the free DOFs (zero on the clamped ones)"""
        fr = self.free(fixed)
        A = self.csr(keff)[fr][:, fr].tocsc()
        dv = np.zeros(self.r)
        dv[fr] = spla.spsolve(A, rhs[fr])
        return dv

    def pcg_iterations(self, keff, rhs, fixed, eps=1e-6, maxit=10000):
        """(orc_pcg's return value, its dv) on the same free-DOF system: Jacobi PCG as the reference runs it (oracle/fem_oracle.c:318)"""
        fr = self.free(fixed)
        A = self.csr(keff)[fr][:, fr].tocsr()
        A.sort_indices()
        info, x = orc_pcg(A.indptr, A.indices, A.data, rhs[fr], eps=eps, maxit=maxit)
        dv = np.zeros(self.r)
        dv[fr] = x
        return info, dv

    def step(self, q, qvel, fext, fixed, h, cM, cK, pcg_eps=None):
        """One semi-implicit step: (q, qvel, dv, PCG info or None).  pcg_eps: solve with orc_pcg at that tolerance (what a handle
        stepping with the same cg_eps is compared against); None: the direct solve."""
        keff, rhs, _ = self.system(q, qvel, fext, h, cM, cK)
        info = None
        if pcg_eps is None:
            dv = self.solve(keff, rhs, fixed)
        else:
            info, dv = self.pcg_iterations(keff, rhs, fixed, eps=pcg_eps)
        qvel = np.asarray(qvel, np.float64) + dv
        q = np.asarray(q, np.float64) + h * qvel
        q[np.asarray(fixed, np.int64)] = 0.0
        qvel[np.asarray(fixed, np.int64)] = 0.0
        return q, qvel, dv, info
