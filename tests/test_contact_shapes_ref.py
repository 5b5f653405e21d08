"""tests/contact_shapes.py on the CPU (no GPU): the census of every case under tests/bodycontactref.py and tests/selfcontactref.py pinned as
literals, and the conditions tests/test_contact_shapes_gpu.py relies on -- edge and vertex winners where the notches promise them, a
winner that is a face of zero area, an R of many face sizes, elements on the overflow list, at most 2 % of the candidates left out by
bodycontactref.generic (a condition on the INPUTS: a case above it gets another seed, not another cap), friction classes away from
their boundaries, and the float64 reference agreeing with itself in np.longdouble on every contact set and face, so that no decision
of these inputs sits on a rounding."""
import numpy as np
import pytest

import bodycontactref as B
import contact_shapes as cs
import frictionref as F
import selfcontactref as S

K, MU, SLIP = 1000.0, 0.5, 0.15

# per case: (candidates, contacts) a into b, b into a; (interior, edge, vertex) winners a into b, b into a; R max, R median of b's faces
CENSUS = {
    "rotated":      (((20, 20), (24, 9)), ((20, 0, 0), (9, 0, 0)), (0.0745, 0.0745)),
    "notch_vertex": (((56, 54), (1, 1)), ((18, 24, 12), (1, 0, 0)), (0.0745, 0.0745)),
    "notch_edge":   (((56, 49), (2, 2)), ((26, 23, 0), (2, 0, 0)), (0.0745, 0.0745)),
    "jittered":     (((22, 22), (8, 1)), ((22, 0, 0), (1, 0, 0)), (0.4262, 0.2490)),
    "graded_near":  (((49, 49), (36, 0)), ((49, 0, 0), (0, 0, 0)), (0.7454, 0.0787)),
    "graded_far":   (((56, 56), (0, 0)), ((56, 0, 0), (0, 0, 0)), (0.7454, 0.0787)),
    "plate":        (((12, 12), (8, 3)), ((12, 0, 0), (3, 0, 0)), (0.0373, 0.0373)),
    "collapsed":    (((56, 55), (0, 0)), ((20, 30, 5), (0, 0, 0)), (0.0943, 0.0745)),
}
LEFT_OUT = {name: 0 for name in CENSUS}     # of the candidates of both directions
SIZES = {"rotated": (162, 750, 300), "notch_vertex": (162, 1134, 432), "notch_edge": (162, 972, 396), "jittered": (643, 2040, 94), "graded_near": (162, 2816, 376),
         "graded_far": (162, 2816, 376), "plate": (48, 864, 672), "collapsed": (162, 1134, 432)}   # elements of a, of b, faces of b
# the union of notch_vertex: surface vertices, contacts, and per mode the winners' regions
UNION = {"vids": 274, "contacts": 55, S.OTHER_PARTS: (19, 24, 12), S.ANY: (7, 48, 0)}
WIDE = {"graded_near": (28, 27), "graded_far": (0, 0)}    # elements over more than 64 cells of the containment grid, contacts whose element is one


def test_the_cases_are_built_once_and_read_only():
    assert set(CENSUS) == set(cs.CASES)
    for name in cs.CASES:
        c = cs.case(name)
        assert c is cs.case(name) and all(not x.flags.writeable for x in c)
        ra, ta, ca, rb, tb, cb = c
        assert ra.shape == ca.shape and rb.shape == cb.shape and ta.max() < len(ra) and tb.max() < len(rb)
        assert len(np.unique(ta)) == len(ra) and len(np.unique(tb)) == len(rb)          # no node without an element
        for rest, t in ((ra, ta), (rb, tb)):                                             # one orientation per mesh at rest, no flat element
            v = rest[t]
            vol = np.einsum("ij,ij->i", v[:, 1] - v[:, 0], np.cross(v[:, 2] - v[:, 0], v[:, 3] - v[:, 0]))
            assert (vol > 0).all() or (vol < 0).all()
    u = cs.union("notch_vertex")
    assert u is cs.union("notch_vertex") and not u[0].flags.writeable and u[3] == 64 and u[4] == 162


@pytest.mark.parametrize("name", cs.CASES)
def test_census(name):
    ra, ta, ca, rb, tb, cb = cs.case(name)
    ref = cs.reference(name)
    counts, split, (r_max, r_median) = CENSUS[name]
    assert (len(ta), len(tb), len(ref["faces_b"])) == SIZES[name]
    radii = cs.face_radii(cb, ref["faces_b"])
    left = [cs.left_out(d, ref["extent"][k]) for k, d in enumerate(ref["dirs"])]
    got = tuple((len(d["candidates"]), len(d["node"])) for d in ref["dirs"])
    print("%s: (candidates, contacts) %s, regions %s, left out %s, R max / median %.4f / %.4f, least margins %s" % (
        name, got, [cs.regions(d["bary"]) for d in ref["dirs"]], left, radii.max(), np.median(radii),
        [(float(d["contain_margin"].min()) if len(d["candidates"]) else None, float(d["gap"].min()) if len(d["node"]) else None) for d in ref["dirs"]]))
    assert got == counts
    assert tuple(cs.regions(d["bary"]) for d in ref["dirs"]) == split
    assert (round(float(radii.max()), 4), round(float(np.median(radii)), 4)) == (r_max, r_median)
    assert sum(left) == LEFT_OUT[name]
    assert sum(left) <= 0.02 * sum(len(d["candidates"]) for d in ref["dirs"])          # the cap test_body_contact_gpu.py states
    assert not any(d["degenerate"].any() for d in ref["dirs"])


def test_what_the_gpu_tests_rely_on():
    split = {name: CENSUS[name][1][0] for name in CENSUS}
    assert split["notch_vertex"][1] >= 10 and split["notch_vertex"][2] >= 5
    assert split["notch_edge"][1] >= 10
    for name in ("graded_near", "graded_far"):
        assert CENSUS[name][2][0] >= 5 * CENSUS[name][2][1]
    # the tail of launch_waves (four contacts a workgroup): a direction with one contact, and counts that are no multiple of four
    counts = [c[1] for name in CENSUS for c in CENSUS[name][0]]
    assert 1 in counts and any(c % 4 for c in counts if c > 4)
    # the plate is one cell thick, and a sits half-way through it
    _, _, ca, _, _, cb = cs.case("plate")
    assert len(np.unique(cb[:, 2])) == 2 and ca[:, 2].min() < cb[:, 2].min() < cb[:, 2].max() < ca[:, 2].max()


def test_how_much_of_R_the_winners_need():
    """The ring search visits the cells within D = best_d + R of the point.  (|g - p| - d) / R of a winner with centroid g says how much
    of that R its contact needs: a search that kept less of it would not visit the winner's cell (but for the one cell it adds on every
    side).  The lattice pairs need up to 0.73 of an R that is one face; graded_far needs 0.87 of an R nine median faces wide, for most
    of its contacts -- its winners are the two faces of a side of the unit cube, met near a corner."""
    need = {}
    for name in cs.CASES:
        _, _, ca, _, _, cb = cs.case(name)
        ref = cs.reference(name)
        need[name] = cs.share_of_R_needed(ca, ref["dirs"][0], cb, ref["faces_b"])
        print("%s: share of R needed, max %.3f median %.3f" % (name, need[name].max(), np.median(need[name])))
    assert need["graded_far"].max() > 0.85 and np.median(need["graded_far"]) > 0.7
    assert need["rotated"].max() > 0.7 and need["plate"].max() > 0.6 and need["jittered"].max() > 0.4


def test_collapsed_has_faces_of_zero_area_and_one_wins():
    ra, ta, ca, rb, tb, cb = cs.case("collapsed")
    ref = cs.reference("collapsed")
    assert (cb != rb).any(axis=1).sum() == 1                                            # one node moved, in the current positions only
    zero = cs.zero_area_faces(cb, ref["faces_b"])
    v = cb[tb]
    flat = np.einsum("ij,ij->i", v[:, 1] - v[:, 0], np.cross(v[:, 2] - v[:, 0], v[:, 3] - v[:, 0])) == 0
    d = ref["dirs"][0]
    wins = int(np.isin(d["face"], zero).sum())
    print("collapsed: %d faces of zero area, %d elements of zero volume, %d of %d contacts won by a face of zero area" % (len(zero), flat.sum(), wins, len(d["node"])))
    assert len(zero) == 2 and flat.sum() > 0 and len(cs.zero_area_faces(rb, ref["faces_b"])) == 0
    assert wins == 23
    # such a winner came out of a vertex return (an edge return of a collapsed triangle divides 0 by 0 and never wins)
    assert np.isfinite(d["depth"]).all() and ((d["bary"][np.isin(d["face"], zero)] == 0).sum(axis=1) >= 1).all()
    assert not np.isin(d["element"], np.nonzero(flat)[0]).any()                         # an element of zero volume contains nothing


@pytest.mark.parametrize("name", cs.CASES)
def test_float64_and_longdouble_decide_alike(name):
    r64, rld = cs.reference(name), cs.reference(name, longdouble=True)
    worst = B.spread(r64, rld)                                                          # asserts equal contact sets and faces
    for a, b in zip(r64["dirs"], rld["dirs"]):
        assert np.array_equal(a["candidates"], b["candidates"]) and np.array_equal(a["element"], b["element"])
    scale = K * r64["max_depth"]
    print("%s: float64 against longdouble, largest force difference %.3g of stiffness * max_depth" % (name, worst / scale))
    # The sets and faces agreeing is the point; the forces then differ by roundings only.  A contribution is below `scale` and a dozen
    # roundings from its inputs; a node receives at most one record per contact, n in all (graded_far: a corner of the unit cube is a
    # corner of nearly every winner), and summing n of them rounds n times at a size below n * scale: (n^2 / 2 + 12 n) half-units.
    n = sum(len(d["node"]) for d in r64["dirs"])
    assert worst <= (n * n / 2 + 12 * n) * 2.0 ** -53 * scale


def test_union_census():
    rest, t, cur, n_a, _ = cs.union("notch_vertex")
    ext = float((cur.max(axis=0) - cur.min(axis=0)).max())
    for mode in (S.OTHER_PARTS, S.ANY):
        r = S.self_contact(rest, t, cur, K, mode=mode)
        cand_ok, contact_ok = B.generic(r, ext)
        print("union mode %d: %d surface vertices, %d contacts, dropped %d, least margin %.3g, least gap %.3g, regions %s" % (
            mode, len(r["vids"]), len(r["node"]), r["n_dropped"], r["contain_margin"].min(), r["gap"].min(), cs.regions(r["bary"])))
        assert (len(r["vids"]), len(r["node"]), r["n_dropped"]) == (UNION["vids"], UNION["contacts"], 0)
        assert cs.regions(r["bary"]) == UNION[mode] and not r["degenerate"].any()
        assert r["contain_margin"].min() > 1e-3                                         # containment is clear of rounding under both modes
        if mode == S.OTHER_PARTS:
            assert cand_ok.all() and contact_ok.all() and r["gap"].min() > 1e-7
            rld = S.self_contact(rest, t, cur, K, mode=mode, dtype=np.longdouble)
            assert np.array_equal(r["node"], rld["node"]) and np.array_equal(r["face"], rld["face"]) and np.array_equal(r["element"], rld["element"])
        else:   # ties at shared closest points: the rule's "equal d, lowest face" decides, and the filter would leave those out
            assert r["gap"].min() == 0.0
    # OTHER_PARTS holds the contacts of both directions of the pair
    assert UNION["contacts"] == sum(c[1] for c in CENSUS["notch_vertex"][0])


def test_friction_classes_of_notch_vertex_are_clear_of_their_boundaries():
    """N_raw = sd - damping vn and s are a handful of roundings each: their relative error is below 1e-14.  A class changes only where
    |s - slip_speed| / slip_speed or |N_raw| / sd falls under that; 1e-6 is eight orders above it."""
    ra, ta, ca, rb, tb, cb = cs.case("notch_vertex")
    va, vb = F.fields(ca, cb)
    rest, t, cur, n_a, _ = cs.union("notch_vertex")
    for damping in (0.0, 400.0):
        pair = F.body_contact(ra, ta, ca, va, rb, tb, cb, vb, K, mu=MU, slip_speed=SLIP, damping=damping)
        one = F.self_contact(rest, t, cur, F.union_fields(cur, n_a), K, mode=S.OTHER_PARTS, mu=MU, slip_speed=SLIP, damping=damping)
        for d in pair["dirs"] + (one,):
            slip, normal = F.class_margins(d, SLIP)
            assert slip >= 1e-6 and normal >= 1e-6, (damping, slip, normal)
        fi = pair["friction"]
        print("notch_vertex damping %g: sticking %s sliding %s separating %s" % (damping, fi["n_sticking"], fi["n_sliding"], fi["n_separating"]))
        assert sum(fi["n_sticking"]) + sum(fi["n_sliding"]) + sum(fi["n_separating"]) == 55
        assert sum(one["friction"][key][0] for key in ("n_sticking", "n_sliding", "n_separating")) == 55
    assert sum(fi["n_separating"]) > 0 and sum(fi["n_sliding"]) > 0                    # with the damper both classes occur


@pytest.mark.parametrize("name", ["graded_near", "graded_far"])
def test_graded_elements_on_the_overflow_list(name):
    _, _, ca, _, tb, cb = cs.case(name)
    ref = cs.reference(name)
    span = cs.overlap_cells_spanned(ca, ref["vids_a"], cb, tb)
    in_wide = span[ref["dirs"][0]["element"]] > 64
    print("%s: %d elements over more than 64 cells (the widest %d), %d of %d contacts lie in one" % (name, (span > 64).sum(), span.max(), in_wide.sum(), len(in_wide)))
    assert (int((span > 64).sum()), int(in_wide.sum())) == WIDE[name]
    for nudge in (-1e-6, 1e-6):   # (the grid rule in numpy need not round as the library's: no element is within 1e-6 of a cell of changing sides)
        assert np.array_equal(cs.overlap_cells_spanned(ca, ref["vids_a"], cb, tb, nudge) > 64, span > 64)
