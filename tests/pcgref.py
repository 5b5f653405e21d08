"""Host reference of the PCG products and iterations (numpy / scipy only, no library call): the arithmetic the SpMV and PCG
kernels are to be held against (tests/test_product_inputs.py checks it against itself).

The operator is what the handle multiplies: ``FemIntegrator.system()`` hands out the STORED values (fp32 widened, the diagonal block as
hi + lo) in ``pattern()`` order; ``operator()`` makes a CSR matrix with ``np.longdouble`` data of them.  ``pcg`` follows the reference's
CGSolver.cpp:129-190 (Jacobi-preconditioned CG, the exact residual every 30th iteration) as tools/pipelined_pcg_numerics.py restates it,
in its literal form and as the Ghysels-Vanroose pipelined recurrences with the full refresh that k_pcg_pipe runs; the ``longdouble``
literal run is the reference, the two ``float64`` forms calibrate what rounding alone does (``calibrate``)."""
import numpy as np

REFRESH = 30


class Csr:
    """CSR with data of any numpy float type; the product is np.add.reduceat(data * x[indices], indptr[:-1])."""

    def __init__(self, indptr, indices, data):
        self.indptr, self.indices, self.data = np.asarray(indptr, np.int64), np.asarray(indices, np.int64), data
        self.n = len(self.indptr) - 1
        assert (np.diff(self.indptr) > 0).all(), "every row holds its diagonal"

    def astype(self, dtype):
        return Csr(self.indptr, self.indices, self.data.astype(dtype))

    def dot(self, x):
        return np.add.reduceat(self.data * x[self.indices], self.indptr[:-1])

    def abs_dot(self, x):
        return np.add.reduceat(np.abs(self.data) * np.abs(x[self.indices]), self.indptr[:-1])

    def diagonal(self):
        rows = np.repeat(np.arange(self.n), np.diff(self.indptr))
        d = np.zeros(self.n, self.data.dtype)
        at = rows == self.indices
        d[rows[at]] = self.data[at]
        return d

    def row_nnz(self):
        return np.diff(self.indptr)


def operator(bptr, bcol, blocks):
    """The 3x3-block CSR of fb_fem_pattern / fb_fem_system as a scalar CSR with np.longdouble data (explicit zeros kept: they are
    terms of the kernels' sums as well)."""
    bptr, bcol = np.asarray(bptr, np.int64), np.asarray(bcol, np.int64)
    blocks = np.asarray(blocks, np.float64).reshape(-1, 3, 3)
    nb_row = np.diff(bptr)
    indptr = np.zeros(3 * len(nb_row) + 1, np.int64)
    indptr[1:] = np.cumsum(np.repeat(3 * nb_row, 3))
    # scalar row 3a + i: its blocks in order, three columns each
    data = np.empty(9 * len(bcol), np.longdouble)
    indices = np.empty(9 * len(bcol), np.int64)
    blk_row = np.repeat(np.arange(len(nb_row)), nb_row)
    within = np.arange(len(bcol)) - bptr[blk_row]
    for i in range(3):
        base = indptr[3 * blk_row + i] + 3 * within
        for j in range(3):
            data[base + j] = blocks[:, i, j]
            indices[base + j] = 3 * bcol + j
    return Csr(indptr, indices, data)


def inv_diag(A):
    """1 / (stored diagonal entry), formed in fp64 as the assembly kernels do (fem_device.hip.h: invdiag = 1.0 / (hi + lo))"""
    return 1.0 / A.diagonal().astype(np.float64)


def row_bound(A, x):
    """(nnz_row + 2) * 2^-52 * sum_j |a_ij| |x_j|: the rounding bound of an fp64 sum of that many products in any order"""
    return (A.row_nnz() + 2) * 2.0 ** -52 * A.abs_dot(np.asarray(x, np.longdouble)).astype(np.float64)


def pcg_iterates(A, b, inv_diag, caps, dtype=np.float64, form="literal", eps=1e-8):
    """{cap: x after `cap` iterations from x = 0} for every cap asked for -- one run up to the largest: the iterate after k iterations
    does not depend on the cap.  Every vector and scalar in `dtype`.  A run that converges (to eps) before a cap has no entry for it."""
    A = A.astype(dtype)
    b, iv = np.asarray(b).astype(dtype), np.asarray(inv_diag).astype(dtype)
    eps2 = dtype(eps) * dtype(eps)
    caps = sorted(set(int(c) for c in caps))
    out = {}
    x = np.zeros_like(b)
    it = 1
    if form == "literal":
        r = b - A.dot(x)
        d = iv * r
        rn = np.sum(r * r * iv)
        rn0 = rn
        while rn > eps2 * rn0 and it <= caps[-1]:
            q = A.dot(d)
            a = rn / np.sum(d * q)
            x = x + a * d
            r = b - A.dot(x) if it % REFRESH == 0 else r - a * q
            rn_new = np.sum(r * r * iv)
            d = iv * r + (rn_new / rn) * d
            rn = rn_new
            if it in caps:
                out[it] = x.copy()
            it += 1
        return out
    assert form == "pipelined", form
    r = b - A.dot(x)
    w = A.dot(iv * r)
    z, s, p = np.zeros_like(b), np.zeros_like(b), np.zeros_like(b)
    gam_old = alpha_old = dtype(1)
    gam0 = None
    while it <= caps[-1]:
        u = iv * r
        gam, delta = np.sum(r * u), np.sum(w * u)
        if gam0 is None:
            gam0 = gam
        if not gam > eps2 * gam0:
            break
        nvec = A.dot(iv * w)
        if it > 1:
            beta = gam / gam_old
            alpha = gam / (delta - beta * gam / alpha_old)
        else:
            beta, alpha = dtype(0), gam / delta
        z, s, p = nvec + beta * z, w + beta * s, u + beta * p
        x = x + alpha * p
        if it % REFRESH == 0:
            r = b - A.dot(x)
            w = A.dot(iv * r)
            s = A.dot(p)
            z = A.dot(iv * s)
        else:
            r, w = r - alpha * s, w - alpha * z
        gam_old, alpha_old = gam, alpha
        if it in caps:
            out[it] = x.copy()
        it += 1
    return out


def pcg(A, b, inv_diag, cap, dtype=np.float64, form="literal", eps=1e-8):
    """x after `cap` iterations (the solve must not converge before)"""
    return pcg_iterates(A, b, inv_diag, (cap,), dtype, form, eps)[cap]


def deviation(x, x_ref):
    """max |x - x_ref| / max |x_ref|, in long double"""
    x_ref = np.asarray(x_ref, np.longdouble)
    return float(np.abs(np.asarray(x, np.longdouble) - x_ref).max() / np.abs(x_ref).max())


FLOOR = 1e-14
MARGIN = 64.0


def calibrate(A, b, iv, caps):
    """{cap: (x_ref, tol, calibration)}: the longdouble literal iterate; tol = max(64 x the larger deviation of the two fp64 forms from
    it on the same matrix, right-hand side and cap, 1e-14).  The margin covers what the host forms do not reproduce: a row's blocks
    added in slot order, the sums added in workgroup order, helpers' partial sums."""
    ref = pcg_iterates(A, b, iv, caps, np.longdouble, "literal")
    f64 = [pcg_iterates(A, b, iv, caps, np.float64, form) for form in ("literal", "pipelined")]
    out = {}
    for cap in caps:
        cal = max(deviation(f[cap], ref[cap]) for f in f64)
        out[cap] = (ref[cap], max(MARGIN * cal, FLOOR), cal)
    return out
