"""Golden data for the per-element material tests, made with the reference's own translation units (oracle/_ref, RefFem).

  fem_cube5_materials.npz   the 5^3 truth cube (384 tets) with three materials by region (tests/matref.py: region_ids,
                            three_materials): f and K at the seeded displacement of make_fem_golden.py's cube5 (rng 12345, 0.01), and
                            the mass matrix, each as the SUM of what RefFem gives on the sub-mesh of one material's elements over the
                            full node list (nodes a sub-mesh does not reference are harmless to it) -- an element's terms depend on
                            its own material only.  Values are stored on the full mesh's scalar CSR pattern (ia, ja of RefFem(v, t)).

Run where the reference build exists:  python tests/golden/make_materials_golden.py
"""
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
from fembrain_amd.meshgen import truth_cube
from oracle.pyoracle import RefFem
from matref import region_ids, three_materials


def on_pattern(A, ia, ja):
    """values of the sparse matrix A at the entries of the CSR pattern (ia, ja); everything of A must lie on the pattern"""
    A = sp.csr_matrix(A)
    r = len(ia) - 1
    rows = np.repeat(np.arange(r), np.diff(ia))
    out = np.asarray(A[rows, ja]).reshape(-1)
    assert abs(sp.csr_matrix((out, ja, ia), shape=A.shape) - A).max() == 0
    return out


def cube5_materials():
    n = 5
    v, t = truth_cube(n, n, n, 0.1)
    mats, ids = three_materials(), region_ids(v, t)
    full = RefFem(v, t)
    ia, ja = full.csr()
    r = full.r
    u = np.random.default_rng(12345).normal(size=r) * 0.01
    f, K, M = np.zeros(r), sp.csr_matrix((r, r)), sp.csr_matrix((r, r))
    for m, (E, nu, rho) in enumerate(mats):
        sub = RefFem(v, t[ids == m], E=E, nu=nu, rho=rho)
        sia, sja = sub.csr()
        fm, Km = sub.assemble(u)
        f += fm
        K = K + sp.csr_matrix((Km, sja, sia), shape=(r, r))
        mia, mja, ma = sub.mass_csr()
        M = M + sp.csr_matrix((ma, mja, mia), shape=(r, r))
    np.savez_compressed(os.path.join(HERE, "fem_cube5_materials.npz"), n=n, materials=np.array(mats), ids=ids, u=u, ia=ia, ja=ja, f=f,
                        K=on_pattern(K, ia, ja), M=on_pattern(M, ia, ja))
    print("cube5 materials: elements per material", np.bincount(ids), "nnz", len(ja))


if __name__ == "__main__":
    cube5_materials()
