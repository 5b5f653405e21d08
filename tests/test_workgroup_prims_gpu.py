"""The in-workgroup primitives of the mesh-side kernels (fembrain_amd/csrc/workgroup.hip.h) and k_run_bounds (mesh_device.hip.h), directly:
fb_test_workgroup runs each through the two-launch pattern its users have (per-workgroup partials, a single-workgroup final) and every
comparison here is exact.  The sizes are the edges of a wavefront (64) and of a workgroup (256); 65,537 items leave 257 partials, the
fewest at which the final's strided fold takes a second turn."""
import ctypes as C

import numpy as np
import pytest

from fembrain_amd import lib as fl

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 513, 65537]
SUM, BEST_LOW_INT, BEST_HIGH_INT, BEST_LOW_LL, BEST_HIGH_LL, RANKS, BOX_FLOAT, BOX_DOUBLE, RUN_BOUNDS = range(9)
GUARD = 8  # FB_TEST_WG_GUARD
SEED = 20304  # (chosen on the host: at every size but 1 the sum's tree gives another double than np.sum and than the plain left-to-right sum)
_llp = C.POINTER(C.c_longlong)


def _call(what, n, m=0, values=None, keys=None, flags=None, n_d=0, n_i=0):
    out_d, out_i = np.full(n_d, np.nan), np.full(n_i, -7, np.int64)
    hold = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((values, np.float64), (keys, np.int64), (flags, np.uint8))]
    ptr = [None if a is None else a.ctypes.data_as(t) for a, t in zip(hold, (fl._dp, _llp, fl._bp))]
    code = fl.lib().fb_test_workgroup(what, n, m, ptr[0], ptr[1], ptr[2], out_d.ctypes.data_as(fl._dp) if n_d else None, out_i.ctypes.data_as(_llp) if n_i else None)
    return code, out_d, out_i


def _run(*a, **k):
    code, out_d, out_i = _call(*a, **k)
    fl.check(code)
    return out_d, out_i


# ---- sum ----

def _tree(rows):
    """rows[:, 256] -> the workgroup tree of each row: every wavefront of 64 folds its upper half onto its lower (32, 16, .. 1), then
    (w0 + w1) + (w2 + w3)"""
    w = rows.reshape(-1, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w[:, :, :o] + w[:, :, o:2 * o]
    w = w[:, :, 0]
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def _pad256(x):
    return np.concatenate([x, np.zeros(-len(x) % 256)]).reshape(-1, 256)  # (idle threads carry 0.0)


def _emulated_sum(x):
    part = _pad256(_tree(_pad256(x)))  # thread t of the final takes the partials t, t + 256, ... in that order, from 0.0
    acc = np.zeros(256)
    for row in part:
        acc = acc + row
    return _tree(acc[None, :])[0]


def _sum_values(n):
    rng = np.random.default_rng(SEED + n)
    return rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-15, 16, n) * rng.choice([-1.0, 1.0], n)  # some thirty binades, mixed signs


def _bits(x):
    return np.float64(x).tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_sum_is_the_documented_tree(gpu, n):
    x = _sum_values(n)
    want = _emulated_sum(x)
    if n >= 3:  # (an implementation that adds in another order must not pass by luck)
        plain = 0.0
        for v in x:
            plain = plain + v
        assert _bits(want) != _bits(np.sum(x)) and _bits(want) != _bits(plain), "the data do not tell the tree from numpy's or the plain sum"
    out_d, _ = _run(SUM, n, values=x, n_d=1)
    print("n = %d: device %r, tree %r, np.sum %r" % (n, out_d[0], want, np.sum(x)))
    assert _bits(out_d[0]) == _bits(want)


# ---- best ----

FIVE = np.array([-2.0, -0.5, 0.0, 0.75, 3.0])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("what", [BEST_LOW_INT, BEST_HIGH_INT, BEST_LOW_LL, BEST_HIGH_LL])
def test_best_is_the_lexicographic_optimum(gpu, what, n):
    rng = np.random.default_rng(SEED + 7 * n + what)
    vals = FIVE[rng.integers(0, 5, n)]  # ties everywhere
    keys = rng.permutation(n).astype(np.int64)
    if what in (BEST_LOW_LL, BEST_HIGH_LL):
        keys += 2 ** 33
    high = what in (BEST_HIGH_INT, BEST_HIGH_LL)
    best = np.lexsort((keys, -vals if high else vals))[0]  # (of equal values the lowest key, both ways)
    out_d, out_i = _run(what, n, values=vals, keys=keys, n_d=1, n_i=1)
    assert (out_d[0], out_i[0]) == (vals[best], keys[best])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("what,sentinel", [(BEST_LOW_INT, 2 ** 31 - 1), (BEST_LOW_LL, 2 ** 63 - 1)])
def test_best_of_nothing_found_keeps_the_sentinel(gpu, what, sentinel, n):
    out_d, out_i = _run(what, n, values=np.full(n, np.inf), keys=np.full(n, sentinel, np.int64), n_d=1, n_i=1)
    assert out_d[0] == np.inf and out_i[0] == sentinel


# ---- count / rank / scan ----

def _flags(case, n):
    f = np.zeros(n, np.uint8)
    if case == "all":
        f[:] = 1
    elif case == "half":
        f[:] = np.random.default_rng(SEED + 3 * n).integers(0, 2, n)
    elif case == "last":
        f[-1] = 1
    return f


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", ["none", "all", "half", "last"])
def test_count_rank_and_scan(gpu, case, n):
    f = _flags(case, n)
    _, out_i = _run(RANKS, n, flags=f, n_i=n + 4)
    f = f.astype(np.int64)
    assert np.array_equal(out_i[:n], np.cumsum(f) - f)  # the exclusive rank of every item, over all workgroups
    per_workgroup = np.concatenate([f, np.zeros(-n % 256, np.int64)]).reshape(-1, 256).sum(1)
    assert list(out_i[n:]) == [f.sum(), n - f.sum(), f.sum(), per_workgroup.max()]


# ---- box ----

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("what,dtype", [(BOX_FLOAT, np.float32), (BOX_DOUBLE, np.float64)])
def test_box(gpu, what, dtype, n):
    rng = np.random.default_rng(SEED + 11 * n)
    xyz = rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-3, 4, (n, 1))
    out_d, _ = _run(what, n, values=xyz, n_d=6)
    p = xyz.astype(dtype)
    assert np.array_equal(out_d, np.concatenate([p.min(0), p.max(0)]).astype(np.float64))


# ---- run bounds ----

@pytest.mark.parametrize("n", SIZES)
def test_run_bounds(gpu, n):
    rng = np.random.default_rng(SEED + 13 * n)
    m = n // 3 + 5
    present = np.flatnonzero(rng.random(m) < 0.6)  # (the other keys are absent)
    if not len(present):
        present = np.array([m // 2])
    n_tail = min(n - 1, 5)
    keys = np.concatenate([np.sort(rng.choice(present, n - n_tail)), np.sort(rng.integers(m, m + GUARD, n_tail))]).astype(np.int64)
    _, out_i = _run(RUN_BOUNDS, n, m=m, keys=keys, n_i=2 * (m + GUARD))
    lo, hi = out_i[:m + GUARD], out_i[m + GUARD:]
    ids = np.arange(m)
    left, right = np.searchsorted(keys, ids, "left"), np.searchsorted(keys, ids, "right")
    there = right > left
    assert np.array_equal(lo[:m], np.where(there, left, 0)) and np.array_equal(hi[:m], np.where(there, right, 0))
    assert np.all(lo[m:] == -1) and np.all(hi[m:] == -1)  # nothing written for the tail


# ---- refusals ----

def test_refusals_launch_nothing(gpu):
    x, k, f = np.ones(4), np.arange(4, dtype=np.int64), np.ones(4, np.uint8)
    assert _call(SUM, 0, values=x, n_d=1)[0] == fl.FB_EINVAL
    assert _call(SUM, 4, n_d=1)[0] == fl.FB_EINVAL
    assert _call(SUM, 4, values=x)[0] == fl.FB_EINVAL
    assert _call(BEST_LOW_INT, 4, values=x, n_d=1, n_i=1)[0] == fl.FB_EINVAL
    assert _call(BEST_LOW_INT, 4, values=x, keys=k + 2 ** 33, n_d=1, n_i=1)[0] == fl.FB_EINVAL
    assert _call(RANKS, 4, n_i=8)[0] == fl.FB_EINVAL
    assert _call(BOX_FLOAT, 4, n_d=6)[0] == fl.FB_EINVAL
    assert _call(RUN_BOUNDS, 4, m=0, keys=k, n_i=16)[0] == fl.FB_EINVAL
    assert _call(RUN_BOUNDS, 4, m=2, keys=k[::-1], n_i=20)[0] == fl.FB_EINVAL
    assert _call(RUN_BOUNDS, 4, m=2, keys=k + 20, n_i=20)[0] == fl.FB_EINVAL
    assert _call(9, 4, values=x, keys=k, flags=f, n_d=8, n_i=8)[0] == fl.FB_EINVAL
    assert _call(-1, 4, values=x, keys=k, flags=f, n_d=8, n_i=8)[0] == fl.FB_EINVAL
