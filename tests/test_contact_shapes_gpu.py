"""fb_fem_body_contact, fb_fem_self_contact and their friction calls on the inputs of tests/contact_shapes.py -- bodies turned against the
grid, reentrant edges and a reentrant vertex, faces of mixed and of graded size, a plate one cell thick, faces of zero area -- against
the same brute-force references as test_body_contact_gpu.py, test_self_contact_gpu.py and test_friction_gpu.py, with their helpers and
their rules: contact sets and integers exactly, the doubles BIT FOR BIT, at most 2 % of the candidates left out (none is, on any case:
test_contact_shapes_ref.py pins that on the CPU, with the census asserted here again on the device's own records).  No tolerance is
new: that device and reference are one sequence of fp64 operations is what is under test, now also through closest_on_triangle's
vertex and edge returns, weights that are exactly 0 and 1, a 0 / 0 that must not win, and a ring search whose R is many faces wide.

No handle makes a time step: the graded and the collapsed meshes are not for solving."""
import numpy as np
import pytest

import contact_shapes as cs
import frictionref as F
import selfcontactref as S
import test_body_contact_gpu as TB
import test_friction_gpu as TF
import test_self_contact_gpu as TS
from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator
from test_contact_shapes_ref import CENSUS, UNION, WIDE

pytestmark = pytest.mark.gpu

K, KW = TB.K, TB.KW


def _pair(name):
    """the two handles of a case at its current positions, which they hold to the bit"""
    ra, ta, ca, rb, tb, cb = cs.case(name)
    ga, gb = FemIntegrator(ra, ta, **KW), FemIntegrator(rb, tb, **KW)
    ga.set_q_state((ca - ra).reshape(-1))
    gb.set_q_state((cb - rb).reshape(-1))
    assert np.array_equal(TB._current(ga)[2], ca) and np.array_equal(TB._current(gb)[2], cb)   # so cs.reference(name) is the reference of this state
    return ga, gb


def _union():
    rest, t, cur, n_a, _ = cs.union("notch_vertex")
    g = FemIntegrator(rest, t, **KW)
    g.set_q_state((cur - rest).reshape(-1))
    assert np.array_equal(TS._current(g)[2], cur)
    return g


_SELF_REFS = {}


def _self_reference(mode):
    """the reference of the union at its current positions: computed once per mode, never changed"""
    if mode not in _SELF_REFS:
        rest, t, cur, _, _ = cs.union("notch_vertex")
        ref = S.self_contact(rest, t, cur, K, 0.0, TS.MODES[mode])
        ref["extent"] = float((cur.max(axis=0) - cur.min(axis=0)).max())
        _SELF_REFS[mode] = ref
    return _SELF_REFS[mode]


def _census_of(out):
    return tuple(cs.regions(d["bary"]) for d in out["dirs"])


@pytest.mark.parametrize("name", cs.CASES)
def test_cases_against_the_reference(name):
    ga, gb = _pair(name)
    out = TB._call(ga, gb, K)
    counts, split, _ = CENSUS[name]
    print("%s: device (candidates, contacts) %s, regions (interior, edge, vertex) per direction %s; reference %s, %s" % (
        name, tuple(zip(out["info"]["n_candidates"], out["info"]["n_contacts"])), _census_of(out), counts, split))
    assert TB._compare(out, cs.reference(name), 0.02, name) == 0
    assert tuple(zip(out["info"]["n_candidates"], out["info"]["n_contacts"])) == counts
    assert _census_of(out) == split          # the edge and the vertex returns were the answers compared
    if name == "collapsed":   # faces of zero area at the positions the handle holds, and contacts they win
        faces = gb.surface()["faces"]
        zero = cs.zero_area_faces(TB._current(gb)[2], faces)
        assert np.array_equal(faces, cs.reference(name)["faces_b"]) and len(zero) == 2
        won = np.isin(out["dirs"][0]["face"], zero)
        assert won.sum() == 23 and np.isfinite(out["dirs"][0]["depth"]).all() and (out["dirs"][0]["depth"][won] > 0).all()
    ga.close(); gb.close()


@pytest.mark.parametrize("name", cs.CASES)
def test_scan_ring_starved_ring_and_default_give_the_same_bits(name):
    ga, gb = _pair(name)
    n_faces = (len(gb.surface()["faces"]), len(ga.surface()["faces"]))
    with TB._Env(FEMBRAIN_BODY_CONTACT="ring", FEMBRAIN_BODY_CONTACT_BUDGET=None):
        ring = TB._call(ga, gb, K)
    with TB._Env(FEMBRAIN_BODY_CONTACT="scan", FEMBRAIN_BODY_CONTACT_BUDGET=None):
        scan = TB._call(ga, gb, K)
    with TB._Env(FEMBRAIN_BODY_CONTACT="ring", FEMBRAIN_BODY_CONTACT_BUDGET=1):
        starved = TB._call(ga, gb, K)
    with TB._Env(FEMBRAIN_BODY_CONTACT=None, FEMBRAIN_BODY_CONTACT_BUDGET=None):
        default = TB._call(ga, gb, K)
    assert ring["info"]["path"] == fl.FB_BODY_CONTACT_RING and starved["info"]["path"] == fl.FB_BODY_CONTACT_RING
    assert scan["info"]["path"] == fl.FB_BODY_CONTACT_SCAN and default["info"]["path"] == fl.FB_BODY_CONTACT_RING
    every = sum(n * f for n, f in zip(scan["info"]["n_contacts"], n_faces))
    assert scan["info"]["faces_tested"] == every and scan["info"]["n_face_grid_builds"] == 0
    assert ring["info"]["n_face_grid_builds"] == sum(1 for n in ring["info"]["n_contacts"] if n)
    assert 0 < ring["info"]["faces_tested"] and starved["info"]["faces_tested"] > every   # every point gave up and was scanned
    # (on the graded bodies, with an R of most of the grid, the ring may test as many faces as the scan: printed, not asserted)
    print("%s faces tested: ring %d, scan %d, starved ring %d" % (name, ring["info"]["faces_tested"], every, starved["info"]["faces_tested"]))
    for other in (scan, starved, default):
        TB._same_bits(ring, other)
    assert default["info"]["faces_tested"] == ring["info"]["faces_tested"]
    assert TB._compare(scan, cs.reference(name), 0.02, name + " scan") == 0
    ga.close(); gb.close()


@pytest.mark.parametrize("name", ["notch_vertex", "jittered"])
def test_permuted_ids_and_forced_renumbering(name):
    handles = []
    for (rest, t, cur), seed in zip((cs.case(name)[:3], cs.case(name)[3:]), (3, 4)):
        p = np.random.default_rng(seed).permutation(len(rest))   # new id of old node i
        rest2, cur2 = np.empty_like(rest), np.empty_like(cur)
        rest2[p], cur2[p] = rest, cur
        g = FemIntegrator(rest2, p[t].astype(np.int32), renumber=fl.FB_RENUMBER_ON, **KW)
        g.set_q_state((cur2 - rest2).reshape(-1))
        assert g.renumbering()[0] and np.array_equal(TB._current(g)[2], cur2)
        handles.append(g)
    ga, gb = handles
    out = TB._call(ga, gb, K)
    counts, split, _ = CENSUS[name]
    assert out["info"]["n_contacts"] == tuple(c[1] for c in counts)
    assert TB._compare(out, TB._reference(ga, gb, K), 0.02, name + " permuted") == 0
    # (the faces and their corners come in another order, and with them which weight of an edge winner is the constant zero: a vertex
    # winner is one under any order)
    assert _census_of(out)[0][2] == split[0][2] and sum(_census_of(out)[0]) == sum(split[0])
    # the caller's numbering: every contact node is a surface vertex of its own body, element and face index the other body's arrays
    assert set(out["dirs"][0]["node"]) <= set(ga.surface()["vertex_ids"]) and out["dirs"][0]["face"].max() < len(gb.surface()["faces"])
    ga.close(); gb.close()


def test_union_through_the_self_call_other_parts():
    g = _union()
    out = TS._call(g, "other_parts")
    ref = _self_reference("other_parts")
    assert (len(ref["vids"]), len(ref["node"]), ref["n_dropped"]) == (UNION["vids"], UNION["contacts"], 0)
    assert TS._compare(out, ref, 0.0, "union of notch_vertex, other_parts") == 0
    print("union other_parts: device regions", cs.regions(out["contacts"]["bary"]))
    assert out["info"]["n_contacts"] == UNION["contacts"] and cs.regions(out["contacts"]["bary"]) == UNION[S.OTHER_PARTS]
    g.close()


def test_union_under_any_every_bit():
    """Under ANY a vertex of b next to the notch meets faces that share its closest point: the least gap to a different closest point is 0
    and bodycontactref.generic would leave those contacts out.  The rule is defined there -- equal d, the lowest face -- containment is
    clear of rounding (least margin 2.3e-3), and device and reference are the same operations: nothing is left out and every integer,
    every double, the vector and the sums are compared exactly, as in test_many_onto_one_under_any_every_bit."""
    g = _union()
    out = TS._call(g, "any")
    ref = _self_reference("any")
    assert (len(ref["vids"]), len(ref["node"]), ref["n_dropped"]) == (UNION["vids"], UNION["contacts"], 0) and ref["contain_margin"].min() > 1e-3
    info, dev = out["info"], out["contacts"]
    print("union any: device %d contacts, faces that differ %d, max |f - ref| %.3g, regions %s, faces tested %d" % (
        info["n_contacts"], int((dev["face"] != ref["face"]).sum()) if len(dev["face"]) == len(ref["face"]) else -1, np.abs(out["f"] - ref["f"]).max(),
        cs.regions(dev["bary"]), info["faces_tested"]))
    assert info["n_contacts"] == UNION["contacts"] and info["n_degenerate"] == 0 and info["n_points"] == UNION["vids"]
    for key in ("node", "element", "face", "closest", "bary", "depth"):
        assert np.array_equal(dev[key], ref[key]), key
    assert np.array_equal(out["f"], ref["f"]) and info["max_depth"] == ref["max_depth"]
    assert np.array_equal(info["force_on_points"], ref["force_on_points"]) and np.array_equal(info["force_on_faces"], ref["force_on_faces"])
    assert cs.regions(dev["bary"]) == UNION[S.ANY]
    g.close()


@pytest.mark.parametrize("mode", ["any", "other_parts"])
def test_union_scan_ring_and_a_starved_ring_give_the_same_bits(mode):
    g = _union()
    nf = len(g.surface()["faces"])
    with TB._Env(FEMBRAIN_SELF_CONTACT="ring", FEMBRAIN_SELF_CONTACT_BUDGET=None):
        ring = TS._call(g, mode)
    with TB._Env(FEMBRAIN_SELF_CONTACT="scan", FEMBRAIN_SELF_CONTACT_BUDGET=None):
        scan = TS._call(g, mode)
    with TB._Env(FEMBRAIN_SELF_CONTACT="ring", FEMBRAIN_SELF_CONTACT_BUDGET=3):
        starved = TS._call(g, mode)
    with TB._Env(FEMBRAIN_SELF_CONTACT=None, FEMBRAIN_SELF_CONTACT_BUDGET=None):
        default = TS._call(g, mode)
    assert ring["info"]["path"] == fl.FB_BODY_CONTACT_RING and scan["info"]["path"] == fl.FB_BODY_CONTACT_SCAN and default["info"]["path"] == fl.FB_BODY_CONTACT_RING
    every = scan["info"]["n_contacts"] * nf
    assert scan["info"]["faces_tested"] == every and scan["info"]["n_face_grid_builds"] == 0 and ring["info"]["n_face_grid_builds"] == 1
    assert 0 < ring["info"]["faces_tested"] and starved["info"]["faces_tested"] > every   # every point gave up and was scanned
    print("union %s faces tested: ring %d, scan %d" % (mode, ring["info"]["faces_tested"], every))
    for other in (scan, starved, default):
        TS._same_bits(ring, other)
    assert np.array_equal(scan["contacts"]["face"], _self_reference(mode)["face"])
    g.close()


@pytest.mark.parametrize("damping", [0.0, 400.0])
def test_friction_on_notch_vertex(damping):
    """the corner velocities of a vertex or edge winner are interpolated with weights that are exactly 0 or 1"""
    ga, gb = _pair("notch_vertex")
    TF._move_pair(ga, gb)
    out = TF._call(ga, gb, damping=damping)
    ref = TF._reference(ga, gb, damping=damping)
    assert TF._compare(out, ref, 0.0, "notch_vertex damping %g" % damping) == 0
    assert out["info"]["n_contacts"] == tuple(c[1] for c in CENSUS["notch_vertex"][0]) and _census_of(out) == CENSUS["notch_vertex"][1]
    bary = out["dirs"][0]["bary"]
    assert (bary == 1.0).any() and (bary == 0.0).any()
    fi = out["friction"]
    assert sum(fi["n_sticking"]) + sum(fi["n_sliding"]) + sum(fi["n_separating"]) == sum(out["info"]["n_contacts"])
    if damping:
        assert fi["n_separating"][0] > 0 and fi["n_sliding"][0] > 0
    ga.close(); gb.close()


def test_friction_on_the_union_other_parts():
    rest, t, cur, n_a, _ = cs.union("notch_vertex")
    g = FemIntegrator(rest, t, **KW)
    g.set_q_state((cur - rest).reshape(-1), F.union_fields(cur, n_a).reshape(-1))
    for damping in (0.0, 400.0):
        out = TF._self_call(g, "other_parts", damping=damping)
        ref = TF._self_reference(g, "other_parts", damping=damping)
        assert len(ref["node"]) == UNION["contacts"]
        assert TF._self_compare(out, ref, 0.0, "union of notch_vertex damping %g" % damping) == 0
        assert cs.regions(out["contacts"]["bary"]) == UNION[S.OTHER_PARTS]
    g.close()


@pytest.mark.parametrize("name", ["graded_near", "graded_far"])
def test_graded_contacts_inside_elements_of_the_overflow_list(name):
    """The containment grid of a into b lies over the overlap of the two boxes, a cell per element that meets it.  In the dense corner
    (graded_near) 345 elements meet that overlap, their volumes five orders apart (1e-9 to 1.3e-4): 28 of them cover more than
    kEmbedWideCells = 64 cells (the widest 216) and go to the overflow list, and for 27 of the 49 contacts such an element is the LOWEST
    containing one -- a device that skipped the list or walked it wrongly would report other elements or lose contacts.  Against the
    sparse far corner (graded_far) 16 large elements meet the overlap, the grid has as few cells, and none spans more than 27: the graded
    body gives no overflow there, which is stated (WIDE) and not stretched into one."""
    ga, gb = _pair(name)
    ref = cs.reference(name)
    span = cs.overlap_cells_spanned(TB._current(ga)[2], ref["vids_a"], TB._current(gb)[2], gb.read_mesh()[1])
    in_wide = span[ref["dirs"][0]["element"]] > 64
    print("%s: %d elements over more than 64 cells (the widest %d), %d of %d contacts lie in one" % (name, (span > 64).sum(), span.max(), in_wide.sum(), len(in_wide)))
    assert (int((span > 64).sum()), int(in_wide.sum())) == WIDE[name]
    if name == "graded_near":
        assert in_wide.sum() >= 1 and (~in_wide).sum() >= 1      # both walks decide contacts of this call
    out = TB._call(ga, gb, K)
    assert TB._compare(out, ref, 0.02, name + " overflow") == 0
    assert np.array_equal(out["dirs"][0]["element"], ref["dirs"][0]["element"])
    ga.close(); gb.close()
