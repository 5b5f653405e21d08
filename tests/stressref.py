"""Numpy restatement of the element stress and strain of include/fembrain_hip.h ("Element stress and strain"): what
tests/test_stress_gpu.py compares the device against, pinned to the oracle's force model by tests/test_stress_ref.py.

A loop per element in fp64.  The rotation is the oracle's (``OrcFem.element``: flipped where the determinant is negative, I in the
linear mode), the shape-function gradients are the first three columns of the oracle's ``Minv``."""
import numpy as np

SIX = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (2, 0))  # xx yy zz xy yz zx: the row order of the reference's B


def lame(E, nu):
    """(lambda, mu) as corotationalLinearFEM.cpp:55-66 forms them"""
    return (nu * E) / ((1 + nu) * (1 - 2 * nu)), E / (2 * (1 + nu))


def six(T):
    return np.array([T[i, j] for i, j in SIX])


def full(s):
    """the symmetric 3 x 3 tensor of a six-vector"""
    T = np.zeros((3, 3))
    for k, (i, j) in enumerate(SIX):
        T[i, j] = T[j, i] = s[k]
    return T


def von_mises(s):
    """of six-vectors (..., 6)"""
    s = np.asarray(s)
    return np.sqrt(0.5 * ((s[..., 0] - s[..., 1]) ** 2 + (s[..., 1] - s[..., 2]) ** 2 + (s[..., 2] - s[..., 0]) ** 2)
                   + 3.0 * (s[..., 3] ** 2 + s[..., 4] ** 2 + s[..., 5] ** 2))


def rest_volume(X):
    """tetMesh.cpp:184-188 on the four rest positions"""
    return abs(np.dot(X[0] - X[3], np.cross(X[1] - X[3], X[2] - X[3]))) / 6.0


def det3(F):
    """the plain cofactor expansion along the first row"""
    return F[0, 0] * (F[1, 1] * F[2, 2] - F[1, 2] * F[2, 1]) - F[0, 1] * (F[1, 0] * F[2, 2] - F[1, 2] * F[2, 0]) + F[0, 2] * (F[1, 0] * F[2, 1] - F[1, 1] * F[2, 0])


def element(o, e, u, lam, mu, world=False):
    """Stress and strain of element e of the oracle handle ``o`` under the displacement ``u`` (3 n,) with the Lame parameters given.
    dict of strain, stress (6,), von_mises, energy_density, J, V and what they were made of: R (3, 3), b (4, 3)."""
    t = o.tets[e]
    X = o.verts[t]
    P = X + np.asarray(u, np.float64).reshape(-1, 3)[t]
    b = o.Minv(e)[:, :3]
    R = o.element(e, u)[0]
    # the sums in the order the definitions write them (k = 0 .. 3, one product and one addition at a time): on a sliver, where |b| is
    # thousands, another order moves F by more than J's bound
    F = np.zeros((3, 3))              # sum_k P_k b_k^T
    for i in range(3):
        for j in range(3):
            F[i, j] = P[0, i] * b[0, j] + P[1, i] * b[1, j] + P[2, i] * b[2, j] + P[3, i] * b[3, j]
    # H = sum_j (R^T P_j - X_j) b_j^T as (R^T - I) + R^T D with the displacement gradient D = sum_j u_j b_j^T (sum_j X_j b_j^T = I):
    # summed node by node, a flat element would multiply the rounding of X + u (5.5e-17) by |b| of thousands
    U = np.asarray(u, np.float64).reshape(-1, 3)[t]
    D = np.zeros((3, 3))
    for j in range(4):
        D += np.outer(U[j], b[j])
    H = (R.T - np.eye(3)) + R.T @ D
    eps = 0.5 * (H + H.T)
    sig = lam * np.trace(H) * np.eye(3) + mu * (H + H.T)
    s6, e6 = six(sig), six(eps)
    out = dict(von_mises=float(von_mises(s6)), energy_density=0.5 * float(np.sum(sig * eps)), J=float(det3(F)), V=rest_volume(X), R=R, b=b)
    if world:
        s6, e6 = six(R @ sig @ R.T), six(R @ eps @ R.T)
    out["stress"], out["strain"] = s6, e6
    return out


def stress(o, u, lam, mu, world=False, elements=None):
    """``element`` over the elements given (default: all) as arrays; lam / mu scalars or one value per element of the mesh"""
    ids = np.arange(o.nt) if elements is None else np.asarray(elements, np.int64)
    lam, mu = np.broadcast_to(np.asarray(lam, np.float64), (o.nt,)), np.broadcast_to(np.asarray(mu, np.float64), (o.nt,))
    rows = [element(o, int(e), u, lam[e], mu[e], world) for e in ids]
    return {k: np.array([r[k] for r in rows]) for k in ("strain", "stress", "von_mises", "energy_density", "J", "V", "R", "b")}


def element_forces(sig6, R, b, V, world=False):
    """V R sigma b_i stacked over i (n, 12) from stresses in the rest frame, or with ``world`` (R sigma R^T) R b_i from world ones"""
    out = np.zeros((len(sig6), 12))
    for e in range(len(sig6)):
        S = full(sig6[e])
        M = S @ R[e] if world else R[e] @ S
        out[e] = (V[e] * (b[e] @ M.T)).reshape(-1)
    return out


def surface_mean(vm, faces, vertex_ids, face_tets):
    """per surface vertex the mean of vm over the elements behind its faces: an fp64 sum in ascending face order over the face count"""
    out = np.zeros(len(vertex_ids))
    for k, v in enumerate(vertex_ids):
        fs = np.nonzero((np.asarray(faces) == v).any(axis=1))[0]
        s = 0.0
        for f in fs:
            s += float(vm[face_tets[f]])
        out[k] = s / len(fs)
    return out


def invert_element(v, t, u, e=3, factor=2.2):
    """``u`` with node 0 of element e pushed through its opposite face: moved towards the face's centroid by ``factor`` times its
    distance to it (in the displaced configuration)"""
    u = np.array(u, np.float64).reshape(-1, 3)
    p = np.asarray(v, np.float64).reshape(-1, 3) + u
    n = t[e]
    c = p[n[1:]].mean(axis=0)
    u[n[0]] += factor * (c - p[n[0]])
    return u.reshape(-1)
