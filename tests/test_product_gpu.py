"""Product-level parity of every SpMV and persistent-PCG instantiation against arithmetic that does not come from this library
(tests/pcgref.py: the stored operator in np.longdouble), on slice shapes chosen on purpose (tests/product_inputs.py).

Every case: (a) builds the handle and checks what runs -- kernel name, the plan's pipe_* arrays against slice_off and persist_info(), after each solve the path asked for, no fall-back, never
FB_PCG_PATH_RESOLVED; (b) asserts the census classes it exists for (product_inputs.census over fb_fem_device_plan_get's pipe_* names): a
class that is not hit FAILS; (c) g.spmv(x) of two random x row by row within pcgref.row_bound; (d) capped solves, caps 1 / 2 / 3, against
the longdouble literal PCG with tol = 64 x the deviation of the two fp64 host forms from it (floor 1e-14), caps 30 and 31 (exact
residual, refresh) where that calibration is below 1e-11 -- on these inputs it is everywhere, also with the two Delaunay lattices of
`irregular` among the parts (5e-13 on the oracle's matrix; the 2.7e-3 of a whole jittered lattice after 37 iterations is not reached by
a mesh of which the lattices are a fifth).  Three iterations after a dropped 3x3 block x differs by 1e-3 and more; the tolerances are
twelve orders below.  Persistent cases run once more cut into launches of one iteration (FEMBRAIN_PERSIST_MAX_RUN=1): the uncut bits.

Widths 2 and 3 do not exist on a tet mesh (a referenced node has three neighbours and itself); the classes "below 4" are served by
width 1 (isolated nodes) and the narrowest real ones, 4 and 5.

Calibration (host, from the reference alone; oracle matrices of the inputs rounded to fp32, tests/test_product_inputs.py prints the
first three) and what every case prints next to its own deviation (`pytest -s`):
  input      cap 1     cap 2     cap 3     cap 30    cap 31     (tol = 64 x, floor 1e-14)
  regular    1.4e-16   1.9e-16   2.8e-16   6.0e-13   6.5e-13
  irregular  1.1e-16   4.2e-16   8.8e-16   5.2e-13   5.9e-13
  On the MI355X (each case's own stored operator; the larger of caps 30 and 31 for calibration and deviation, the largest deviation of caps 1-3,
  whose calibration is 0.9e-16 .. 2.2e-16 and tolerance the floor 1e-14 .. 1.4e-14):
    case                                    calibration   deviation   caps 1-3
    two-launch merged    f32 rows / split   9.2e-13       3.2e-13 / 4.0e-13   4.8e-16
    two-launch reference f32 rows / split   9.2e-13       2.4e-13 / 2.6e-13   1.3e-16
    two-launch merged    f64 rows / split   1.5e-12       1.0e-12 / 6.9e-13   2.9e-15
    two-launch reference f64 rows / split   1.5e-12       4.3e-13 / 3.2e-13   2.2e-16
    split in two, 65,601 nodes (caps 1-3)   2.1e-16       --                  2.1e-16
    8x8 c16 / c32                           6.9e-13       6.9e-13             2.5e-16
    5x16 c16 / c32                          6.9e-13       9.1e-13             2.5e-16
    12x7 window c16 / c32                   6.9e-13       8.3e-13             2.5e-16
    12x6 window c16 / c32                   1.3e-12       7.3e-13             1.0e-16
    12x window after cut + delta re-sync    1.3e-12       1.1e-12             1.3e-16
    12x6 task table, planes / node by node  9.2e-13       1.1e-12             3.1e-16
    two-row, planes / node by node          6.9e-13 / 9.2e-13   5.3e-13 / 8.8e-13   2.5e-16
  (16- and 32-bit columns and the temporal / non-temporal forms give the same bits.)  Products: the worst row at 0.10 .. 0.15 of its bound.
"""
import hashlib

import numpy as np
import pytest

import pcgref
import product_inputs as pi
from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator

pytestmark = pytest.mark.gpu

CAPS, LATE_CAPS, LATE_BELOW = (1, 2, 3), (30, 31), 1e-11
_refs = {}


class _Ref:
    """the reference of one operator: products of two random x with their row bounds, the capped iterates with their tolerances"""

    def __init__(self, name, g, K):
        bptr, bcol = g.pattern()
        self.A = pcgref.operator(bptr, bcol, K)
        rng = np.random.default_rng(len(name) + g.n_nodes)
        self.xs = [rng.normal(size=self.A.n), rng.normal(size=self.A.n) * np.exp(rng.uniform(-8, 8, size=self.A.n))]
        self.ys = [self.A.dot(x.astype(np.longdouble)) for x in self.xs]
        self.bounds = [pcgref.row_bound(self.A, x) for x in self.xs]
        self.iv = pcgref.inv_diag(self.A)
        self.rhs = rng.normal(size=self.A.n)
        self.cal = {}

    def caps(self, fixed, caps):
        if not self.cal:
            self.rhs[fixed] = 0.0
            self.cal = pcgref.calibrate(self.A, self.rhs, self.iv, CAPS + LATE_CAPS)
        late = all(self.cal[c][2] < LATE_BELOW for c in LATE_CAPS)
        return [c for c in caps if c in CAPS or late]


def _reference(name, g):
    K, _ = g.system()
    key = (name, g.n_nodes, hashlib.sha1(K.tobytes()).hexdigest())
    if key not in _refs:
        _refs[key] = _Ref(name, g, K)
    return _refs[key]


def _check_products(g, ref, what):
    worst = 0.0
    for x, y, bound in zip(ref.xs, ref.ys, ref.bounds):
        err = np.abs(g.spmv(x).astype(np.longdouble) - y).astype(np.float64)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        bad = np.nonzero(err > bound)[0]
        assert len(bad) == 0, "%s: %d rows of g.spmv leave the longdouble product by more than the row bound, first %d: %.3e > %.3e" % (
            what, len(bad), bad[0], err[bad[0]], bound[bad[0]])
    return worst


def _check_solves(g, ref, fixed, what, path, monkeypatch, cut=False, caps=CAPS + LATE_CAPS):
    """capped solves against the reference; cut: once more in launches of one iteration, bit for bit.  Returns (calibration, deviation)
    maxima over the caps run."""
    cal_max = dev_max = 0.0
    for cap in ref.caps(fixed, caps):
        x_ref, tol, cal = ref.cal[cap]
        it, x = g.pcg(ref.rhs, eps=1e-8, max_iter=cap)
        p = g.pcg_path()
        assert it == -cap and p["path"] == path and p["fallbacks"] == 0, (what, cap, it, p)
        dev = pcgref.deviation(x, x_ref)
        print("%s cap %d: calibration %.2e tol %.2e deviation %.2e" % (what, cap, cal, tol, dev))
        assert dev <= tol, (what, cap, dev, tol)
        assert not x[fixed].any()
        cal_max, dev_max = max(cal_max, cal), max(dev_max, dev)
        if cut:
            monkeypatch.setenv("FEMBRAIN_PERSIST_MAX_RUN", "1")
            itc, xc = g.pcg(ref.rhs, eps=1e-8, max_iter=cap)
            monkeypatch.delenv("FEMBRAIN_PERSIST_MAX_RUN")
            p = g.pcg_path()
            assert itc == -cap and p["path"] == path and p["fallbacks"] == 0 and np.array_equal(xc, x), (what, cap, "cut into launches of 1")
    return cal_max, dev_max


# ---- the two-launch solver: k_spmv / k_spmv_split ------------------------------------------------------------------------------------
def _index_bytes(g, f64):
    mt = 8 if f64 else 4
    n, nb = g.n_nodes, g.num_blocks()
    return (g.spmv_bytes() - (n + 1) * 4 - 6 * mt * n - 96 * n) / nb - 9 * mt


def _two_launch(monkeypatch, name, prec, spmv, variant, c16=None, nt=None):
    v, t, fixed = pi.mesh(name)
    monkeypatch.setenv("FEMBRAIN_PCG_PERSIST", "0")
    if c16 is not None:
        monkeypatch.setenv("FEMBRAIN_SPMV_C16", c16)
    if nt is not None:
        monkeypatch.setenv("FEMBRAIN_SPMV_NT", nt)
    g = FemIntegrator(v, t, fixed, matrix_precision=prec, spmv_kernel=spmv, pcg_variant=variant, renumber=fl.FB_RENUMBER_OFF)
    assert not g.persist_info()[0] and g.pcg_path()["kernel"] == "" and not g.renumbering()[0]
    assert g.matrix_precision() == prec
    return g, fixed


_ROWS = [(c16, nt) for c16 in ("0", "1") for nt in ("0", "1")]


@pytest.mark.parametrize("prec", [fl.FB_MATRIX_F32, fl.FB_MATRIX_F64], ids=["f32", "f64"])
@pytest.mark.parametrize("c16,nt", _ROWS + [(None, None)], ids=["rows-c%s-nt%s" % (("16" if c == "1" else "32"), n) for c, n in _ROWS] + ["split4"])
def test_two_launch_products(gpu, monkeypatch, prec, c16, nt):
    """k_spmv<MT, mode, column words, NT> (FB_SPMV_ROWS) and k_spmv_split with a slice's slots dealt to four wavefronts (FB_SPMV_SPLIT at
    <= 1,024 slices; widths below 4 leave wavefronts without a slot), fp32 and fp64 storage, under both two-launch variants, on `irregular`:
    widths 1, 4 and 5, odd, even, >= 25 and the hub's 71."""
    rows = c16 is not None
    cls = pi.width_classes(pi.widths(*pi.mesh("irregular")))
    assert all(cls.values()), cls
    for variant, vname in ((fl.FB_PCG_MERGED, "merged"), (fl.FB_PCG_REFERENCE, "reference")):
        g, fixed = _two_launch(monkeypatch, "irregular", prec, fl.FB_SPMV_ROWS if rows else fl.FB_SPMV_SPLIT, variant, c16, nt)
        what = "two-launch %s %s %s" % (vname, "f64" if prec == fl.FB_MATRIX_F64 else "f32", "rows c16=%s nt=%s" % (c16, nt) if rows else "split")
        if rows:
            assert _index_bytes(g, prec == fl.FB_MATRIX_F64) == (2.0 if c16 == "1" else 4.0), what
        else:
            assert len(pi.device_plan(g, "slice_off")) - 1 <= 1024
        ref = _reference("irregular", g)
        print("%s: worst product error / row bound %.3f" % (what, _check_products(g, ref, what)))
        _check_solves(g, ref, fixed, what, fl.FB_PCG_PATH_TWO_LAUNCH, monkeypatch)
        g.close()


def test_two_launch_split_in_two_on_the_large_input(gpu, monkeypatch):
    """k_spmv_split with two wavefronts per slice: FB_SPMV_SPLIT from 1,025 slices on (65,601 nodes = 1,026 slices, odd widths among them)"""
    wd = pi.widths(*pi.mesh("large"))
    assert len(wd) >= 1025 and ((wd % 2 == 1) & (wd > 1)).any()
    g, fixed = _two_launch(monkeypatch, "large", fl.FB_MATRIX_F32, fl.FB_SPMV_SPLIT, fl.FB_PCG_MERGED)
    ref = _reference("large", g)
    print("split in two: worst product error / row bound %.3f" % _check_products(g, ref, "split2"))
    _check_solves(g, ref, fixed, "two-launch merged f32 split in two", fl.FB_PCG_PATH_TWO_LAUNCH, monkeypatch, caps=CAPS)
    g.close()


# ---- the persistent solver: one case per non-timing, unsharded, Jacobi row of kPipeKernels ---------------------------------------------
_STREAM = ("0", "1", "2", "3", "even", "odd")


def _need(found, what):
    missing = [k for k, v in found.items() if not v]
    assert not missing, "%s: census classes not hit: %s" % (what, missing)


def _census_plain(c, what):
    """kernels without window and task table: the stream behind the resident slots"""
    _need(pi.count_classes(c["back"]), what + " streamed part")


def _census_window(c, what, twelve):
    parts = pi.count_classes(list(c["front"]) + list(c["back"]))
    _need(parts, what + " streamed part in front of or behind the window")
    run = c["mirror"] + c["plain"]
    _need({"front and back": bool(((c["front"] > 0) & (c["back"] > 0)).any()), "run 1": bool((run == 1).any()), "run 2": bool((run == 2).any()),
           "run 3": bool((run == 3).any()), "run 4": bool((run == 4).any()), "run >= 5": bool((run >= 5).any()),
           "run clipped by the width": bool(((c["front"] + run == c["width"]) & (c["plain"] < c["dealt"])).any()),
           "mirror layers": bool((c["mirror"] > 0).any()), "workgroup without mirrors": len(c["no_mirror_wgs"]) > 0}, what)
    groups = [n for n in c["groups"] if n > 0]
    assert 9 <= max(groups) <= 12, groups
    if twelve:
        _need({"workgroup with 12 slices": 12 in groups, "workgroup with a spare wavefront": min(groups) < 12}, what)


def _census_tasks(c, what):
    halves = [n for h in c["helpers"] for n in h]
    _need({"helper half of odd length": any(n % 2 == 1 for n in halves), "helper half of even length": any(n % 2 == 0 for n in halves)}, what)
    _need(pi.count_classes(list(c["back"]) + halves), what + " streamed part (owners and helpers)")


def _census_pipe2(c, what):
    _need(pi.count_classes(c["back"]), what + " streamed part")
    groups = [n for n in c["groups"] if n > 0]
    two_rows = False
    for b in set(c["wg"].tolist()):
        mine = np.nonzero(c["wg"] == b)[0]
        for w in set(c["wave"][mine].tolist()):
            wd = c["width"][mine[c["wave"][mine] == w]]
            two_rows = two_rows or (len(wd) == 2 and wd[0] != wd[1])
    _need({"workgroup with an odd number of slices": any(n % 2 == 1 for n in groups), "lane whose two rows lie in slices of different width": two_rows}, what)


_ONE_XCD = {"FEMBRAIN_CU_MASK": "0:32"}
_NO_TABLE = {"FEMBRAIN_PIPE_HELPERS": "0", "FEMBRAIN_PIPE_XYZ": "0"}
_TABLE = {"FEMBRAIN_PIPE_HELPERS": "1", "FEMBRAIN_PIPE_HELP_MINLEN": "4"}
# name: (input, knobs, kernel, 16-bit columns, task table, node-by-node vector, census check)
_PERSISTENT = {}
for _c16 in (True, False):
    _w = "c16" if _c16 else "c32"
    _PERSISTENT.update({
        "8x8-" + _w: ("regular", dict(_NO_TABLE), "k_pcg_pipe<float,%s,8,8>" % _w, _c16, False, False, _census_plain),
        "5x16-" + _w: ("regular", dict(_NO_TABLE, FEMBRAIN_PIPE_SMALL="1", FEMBRAIN_PIPE_BALANCE="0"), "k_pcg_pipe<float,%s,5,16>" % _w, _c16, False, False, _census_plain),
        "12x7-window-" + _w: ("regular", dict(_NO_TABLE, FEMBRAIN_PIPE_BALANCE="0", **_ONE_XCD), "k_pcg_pipe<float,%s,12,7>" % _w, _c16, False, False,
                             lambda c, what: _census_window(c, what, False)),
        "12x6-window-" + _w: ("regular12", dict(_NO_TABLE, FEMBRAIN_PIPE_BALANCE="0", **_ONE_XCD), "k_pcg_pipe<float,%s,12,6>" % _w, _c16, False, False,
                             lambda c, what: _census_window(c, what, True)),
        "12x6-tasks-" + _w: ("irregular", dict(_TABLE, FEMBRAIN_PIPE_XYZ="0", FEMBRAIN_PIPE_LDS_CAP="6"), "k_pcg_pipe<float,%s,12,6>" % _w, _c16, True, False, _census_tasks),
        "12x6-tasks-xyz-" + _w: ("irregular", dict(_TABLE, FEMBRAIN_PIPE_XYZ="1", FEMBRAIN_PIPE_LDS_CAP="12"), "k_pcg_pipe<float,%s,12,6>" % _w, _c16, True, True, _census_tasks),
        "pipe2-" + _w: ("regular", dict(_NO_TABLE, FEMBRAIN_PERSIST_ROWS="2", FEMBRAIN_PIPE_BALANCE="0", **_ONE_XCD), "k_pcg_pipe2<%s>" % _w, _c16, False, False, _census_pipe2),
        "pipe2-xyz-" + _w: ("irregular", dict(FEMBRAIN_PIPE_HELPERS="0", FEMBRAIN_PIPE_XYZ="1", FEMBRAIN_PERSIST_ROWS="2", FEMBRAIN_PIPE_BALANCE="0", **_ONE_XCD),
                           "k_pcg_pipe2<%s>" % _w, _c16, False, True, _census_pipe2),
    })


def _census_cut(c, what):
    """after synthetic_cut(stride=3) + resync_delta: widths the uncut input does not have, windows that differ from slice to slice"""
    before = set(pi.widths(*pi.mesh("regular")).tolist())
    _need({"widths the uncut input has not": bool(set(c["width"].tolist()) - before), "mirror layers": bool((c["mirror"] > 0).any()),
           "windows of several lengths": len(set(c["mirror"].tolist())) >= 3, "streamed in front and behind": bool(((c["front"] > 0) & (c["back"] > 0)).any())}, what)


_PERSISTENT["12x-window-cut-c16"] = ("regular", dict(_NO_TABLE, FEMBRAIN_PIPE_BALANCE="0", **_ONE_XCD), "k_pcg_pipe<float,c16,12,", True, False, False, _census_cut)


def make_persistent(monkeypatch, case):
    name, knobs, kernel, c16, table, xyz, _ = _PERSISTENT[case]
    v, t, fixed = pi.mesh(name)
    monkeypatch.setenv("FEMBRAIN_PERSIST_MIN_WAVES", "1")
    monkeypatch.setenv("FEMBRAIN_SPMV_C16", "1" if c16 else "0")
    for k, val in knobs.items():
        monkeypatch.setenv(k, val)
    g = FemIntegrator(v, t, fixed, pcg_variant=fl.FB_PCG_PERSISTENT, matrix_precision=fl.FB_MATRIX_F32, renumber=fl.FB_RENUMBER_OFF)
    if "cut" in case:
        g.resync_delta(pi.cut_delta(v, t)[2], fixed)     # (the knobs are read again for the new plan)
    for k in list(knobs) + ["FEMBRAIN_SPMV_C16", "FEMBRAIN_PERSIST_MIN_WAVES"]:
        monkeypatch.delenv(k)
    return g, fixed


def persistent_handle(monkeypatch, case):
    """the case's handle; what it must say about itself before anything runs"""
    name, knobs, kernel, c16, table, xyz, _ = _PERSISTENT[case]
    g, fixed = make_persistent(monkeypatch, case)
    assert g.persist_info()[0] and g.pcg_path()["kernel"].startswith(kernel), (case, g.pcg_path(), g.persist_info())
    assert "cut" in case or not g.renumbering()[0]
    assert (pi.device_plan(g, "pipe_tasks") is not None) == table and g.persist_gather()[0] == xyz, (case, g.persist_gather())
    assert (pi.device_plan(g, "pipe_windows") is not None) == ("window" in case), case
    return g, fixed


def _check_plan(g, c, case):
    """what fb_fem_device_plan_get's pipe_* names and the census say must agree with slice_off and persist_info()"""
    on, waves, nb, dealt = g.persist_info()
    so = pi.device_plan(g, "slice_off")
    ns = len(so) - 1
    groups = np.array(c["groups"])
    assert len(groups) == nb and groups.sum() == ns and groups.max() == waves and groups.min() >= 0, (case, groups, waves)
    wg_first = pi.device_plan(g, "pipe_wg_first")
    if wg_first is not None:
        assert len(wg_first) == 2 * nb + 2 and wg_first[nb] == ns
        first, count = wg_first[:nb], wg_first[nb + 1:2 * nb + 1]
        per = nb // 8
        for x in range(8):                      # ascending, contiguous runs inside every XCD's share
            f, n = first[x::8][:per], count[x::8][:per]
            assert (f[1:] == f[:-1] + n[:-1]).all(), (case, x)
    assert np.array_equal(np.sort(np.concatenate([np.arange(f, f + n) for f, n in pi.deal(wg_first, ns, nb) if n > 0])), np.arange(ns))
    helped = np.array([sum(h) for h in c["helpers"]])
    assert np.array_equal(c["front"] + c["mirror"] + c["plain"] + c["back"] + helped, c["width"]), case      # every slot of every slice exactly once
    assert (c["mirror"] <= 4).all() and (c["dealt"] >= 0).all() and (c["plain"] <= c["dealt"]).all(), case
    tasks = pi.device_plan(g, "pipe_tasks")
    if tasks is not None:
        assert len(tasks) == nb * pi.TASK_STRIDE * 4 and sum(len(h) for h in c["helpers"]) == fl.lib().fb_fem_persist_helpers(g.h)
    windows = pi.device_plan(g, "pipe_windows")
    if windows is not None:
        mon, layers, pool, plain = g.persist_mirror()
        assert len(windows) == 3 * ns and windows.reshape(ns, 3)[:, 1].sum() == layers and windows.reshape(ns, 3)[:, 2].min() == plain, (case, layers, plain)


@pytest.mark.parametrize("case", sorted(_PERSISTENT))
def test_persistent_products(gpu, monkeypatch, case):
    """k_pcg_pipe / k_pcg_pipe2 in every unsharded Jacobi instantiation, selected with the knobs the other suites use; the streamed parts
    (pcg_pipe_stream.hip.h: tails for 1, 2, 3, even and odd slot counts, per <C16, XYZ>) and the on-chip run (pcg_pipe_onchip.hip.h: fewer
    layers than its pipeline is deep) are asserted from what the live handle planned."""
    name = _PERSISTENT[case][0]
    g, fixed = persistent_handle(monkeypatch, case)
    c = pi.census(g)
    _check_plan(g, c, case)
    _PERSISTENT[case][6](c, case)
    ref = _reference(name + ("-cut" if "cut" in case else ""), g)
    print("%s: worst product error / row bound %.3f" % (case, _check_products(g, ref, case)))
    cal, dev = _check_solves(g, ref, fixed, case, fl.FB_PCG_PATH_PERSISTENT, monkeypatch, cut=True)
    print("%s: calibration %.2e deviation %.2e" % (case, cal, dev))
    g.close()
