"""The census of tests/adversarial_inputs.py: every property of these meshes that tests/test_mesh_side_adversarial_gpu.py relies on, pinned
from the host references alone, so that a change to an input cannot quietly make a device test vacuous.  No GPU.

Every assertion here fails on a cube of similar size: a cube is one part, has no unused and no shared node, no node in more than 24
elements or with more than 14 neighbours, no aligned run of 64 nodes without an element, and another node count."""
import numpy as np
import pytest

import adversarial_inputs as ai
import contactref as cr
import embedref as er
import partsref as pr
import surfref as sr
from fembrain_amd.fem import ProbeContact

MIN_SUM = 1e-3       # tests/test_fem_surface_gpu.py: below it a vertex would be left out of the normals' comparison
MARGIN = 1e-9        # tests/test_embed_gpu.py: how far a generic point's binding is from depending on rounding
SIGMA_MAX_COUNT = 1023   # kSigmaMaxCount of fembrain_amd/csrc/renumber.hip


@pytest.mark.parametrize("name", list(ai.INPUTS))
def test_node_counts_and_indices(name):
    v, t, fixed = ai.mesh(name)
    assert len(v) == ai.NODES[name] and v.shape == (len(v), 3) and t.dtype == np.int32 and t.min() >= 0 and t.max() < len(v)
    assert len(fixed) and np.all(np.diff(fixed) > 0) and fixed.max() < 3 * len(v)
    assert np.abs(sr.determinants(v, t)).min() / 6 > 1e-9, "no flat element"
    v2, t2, f2 = ai.mesh(name, True)
    perm = np.random.default_rng(3).permutation(len(v))
    assert np.array_equal(v2[perm], v) and np.array_equal(t2, perm[t]) and not np.array_equal(perm, np.arange(len(v)))


def test_the_exact_node_counts_of_the_edge_meshes():
    assert [len(ai.mesh(n)[0]) for n in ("edges255", "edges256", "edges257", "edges64k")] == [255, 256, 257, 256 * 256 + 1]
    assert len(ai.mesh("crumbs")[0]) % 64 == 1
    for n in ("edges255", "edges256", "edges257", "edges64k"):
        v, t, _ = ai.mesh(n)
        used = np.zeros(len(v), bool)
        used[t.reshape(-1)] = True
        assert len(t) > 100 and not used[-1] and 0 < used.sum() < len(v), "elements to move, and the last node is one no element uses"


@pytest.mark.parametrize("name", ["edges255", "edges256", "edges257", "edges64k"])
def test_three_exact_pick_ties_among_the_last_nodes(name):
    import hapticref as hr
    v, _, _ = ai.mesh(name)
    ties = ai.tie_pairs(name)
    assert len(ties) == 3 and all(a < b and b >= len(v) - 40 for a, b, _ in ties)
    assert not np.isin([n for a, b, _ in ties for n in (a, b)], ai.mesh(name)[1]).any(), "the tied nodes are nodes no element uses"
    if len(v) < 1000:           # (the reference's own loop: the first of the two wins)
        assert [hr.pick_vertex(v, w)[0] for _, _, w in ties] == [a for a, _, _ in ties]


def test_parts_census():
    v, t, _ = ai.mesh("crumbs")
    p = pr.parts(v, t)
    assert (p["n_parts"], p["n_unused_nodes"], p["n_shared_nodes"], int((p["elements"] == 1).sum()), int((p["elements"] == 2).sum())) == (143, 177, 0, 96, 40)
    assert p["largest_part"] == 138 and p["elements"].max() == 594          # the rod; the cube has 384
    unused = np.nonzero(p["node_part"] < 0)[0]
    assert len(np.unique(unused // 64)) >= 4, "unused nodes spread through the numbering"
    v, t, _ = ai.mesh("bowtie")
    p = pr.parts(v, t)
    assert (p["n_parts"], p["n_unused_nodes"], p["n_shared_nodes"], int((p["elements"] == 1).sum())) == (3, 0, 3, 0)
    assert p["elements"].tolist() == [384, 384, 384] and p["largest_part"] == 0, "a three-way tie for the largest part: the lowest"
    uses = np.bincount(np.unique(np.stack([np.repeat(p["element_part"], 4), t.reshape(-1)], 1), axis=0)[:, 1], minlength=len(v))
    assert tuple(np.nonzero(uses > 1)[0]) == ai.BOWTIE_SHARED
    # node adjacency is one component although the parts are three
    bptr, bcol = cr.pattern_of(t, len(v))
    assert len(cr.ball(bptr, bcol, 124, 40)) == len(v) - 1
    for name, want in (("bighub", (2, 0)), ("far", (2, 3)), ("edges256", (13, 124))):
        v, t, _ = ai.mesh(name)
        p = pr.parts(v, t)
        assert (p["n_parts"], p["n_unused_nodes"]) == want, name


def test_crumbs_has_an_aligned_run_of_64_nodes_without_an_element():
    v, t, _ = ai.mesh("crumbs")
    used = np.zeros(len(v) // 64 * 64, bool)
    tt = t.reshape(-1)
    used[tt[tt < len(used)]] = True
    empty = np.nonzero(~used.reshape(-1, 64).any(axis=1))[0]
    assert 0 in empty
    faces, _ = sr.vectorised(v, t)
    on_surface = np.zeros(len(v), bool)
    on_surface[sr.vertex_ids(faces)] = True
    assert not on_surface[:64].any(), "a bitmap word of the surface's vertex set with no bit in it"


def test_bighub_exceeds_the_walk_table_and_the_count_clip():
    v, t, _ = ai.mesh("bighub")
    bptr, bcol = cr.pattern_of(t, len(v))
    degree = np.diff(bptr) - 1
    assert degree.max() == degree[0] == ai.BIGHUB > cr.BALL_MAX
    count = np.bincount(t.reshape(-1), minlength=len(v))
    assert count.max() == count[0] == 2196 > SIGMA_MAX_COUNT
    assert len(cr.ball(bptr, bcol, 0, 2)) == ai.BIGHUB, "the ball overflows in ring 1"
    v8, t8, _ = ai.mesh("bighub8k")
    count = np.bincount(t8.reshape(-1), minlength=len(v8))
    assert np.array_equal(t8, t) and len(v8) == 8193 > 8192 and count.max() > SIGMA_MAX_COUNT and (count == 0).sum() == 8193 - len(v)
    # (8,192 = kRenumberMinNodes of fembrain_amd/csrc/renumber.h: below it the order has no second stage and nothing is clipped)
    # very different incidence lists in one launch: 3 faces at a corner of a lone tet, hundreds of elements at a hub
    v, t, _ = ai.mesh("crumbs")
    faces, _ = sr.vectorised(v, t)
    per_vertex = np.bincount(faces.reshape(-1), minlength=len(v))
    assert per_vertex[per_vertex > 0].min() == 3 and per_vertex.max() >= 8
    assert np.bincount(t.reshape(-1)).max() == 136


def test_far_has_a_node_box_far_larger_than_its_elements():
    v, t, _ = ai.mesh("far")
    edge = np.linalg.norm(v[t[:, 0]] - v[t[:, 1]], axis=1).max()
    assert (v.max(0) - v.min(0)).min() >= 1e3 and edge < 0.2
    used = np.zeros(len(v), bool)
    used[t.reshape(-1)] = True
    assert tuple(np.nonzero(~used)[0]) == ai.FAR_LONE


@pytest.mark.parametrize("name", ["crumbs", "bowtie", "bighub", "far", "edges255", "edges256", "edges257", "edges64k"])
def test_no_surface_vertex_falls_below_the_normals_floor(name):
    """with the displacement the device tests set; at rest the shared corner of bowtie has a sum of exactly zero (the corners of two
    cubes, opposite each other), which is why the device test compares normals at the displaced state only"""
    v, t, _ = ai.mesh(name)
    faces, _ = sr.vectorised(v, t)
    assert sr.euler(faces) >= 4 or name == "bowtie", "the surfaces of several bodies"
    if name == "bowtie":
        assert 124 in sr.vertex_ids(faces) and sr.normals(v, faces, [124])[1][0] == 0.0
    for scale in (1.0, 0.5):
        _, length = sr.normals(v + scale * ai.displacement(v).reshape(-1, 3), faces)
        assert length.min() >= 5 * MIN_SUM, (name, scale, length.min())


@pytest.mark.parametrize("name", ["crumbs", "bowtie", "bighub", "far"])
def test_the_displacement_folds_no_element(name):
    v, t, _ = ai.mesh(name)
    rest = sr.determinants(v, t)
    now = sr.determinants(v + ai.displacement(v).reshape(-1, 3), t)
    assert np.abs(now / rest - 1).max() < 0.2 and np.abs(ai.displacement(v)).max() > 0.01
    assert pr.parts(v, t)["n_parts"] >= 2


def _contact_lists(case):
    """the host session's list after each move of the case"""
    name = ai.contact_mesh(case)
    v, t, _ = ai.mesh(name)
    probe, out = ProbeContact(), []
    for k, (lo, hi) in enumerate(ai.contact_boxes(case)):
        info = probe.move(v + ai.CONTACT_SCALES[k] * ai.displacement(v).reshape(-1, 3), lo, hi, cr.COEFF)
        out.append((info, probe.ids.copy(), probe.forces.copy()))
    return out, cr.pattern_of(t, len(v))


def test_contact_cases_take_the_paths_the_device_test_expects():
    assert (ai.RECORDS, ai.LEVELS) == (cr.RECORDS, cr.LEVELS) and set(ai.CONTACT_PATHS.values()) == {cr.RECORDS, cr.LEVELS}
    lists = {}
    for (case, size), path in ai.CONTACT_PATHS.items():
        if case not in lists:
            lists[case] = _contact_lists(case)
        moves, (bptr, bcol) = lists[case]
        info, ids, forces = moves[-1]
        assert info["status"] == cr.fl.FB_CONTACT_SET and info["n_pushing"] == len(ids) > 0, case
        want = cr.spread_by_records(bptr, bcol, ids, forces, size, np.zeros(3 * (len(bptr) - 1)))
        assert want["path"] == path, (case, size, want)
    # crumbs: sources without a neighbour (no record) beside sources with some, and the second move finds new nodes
    moves, (bptr, bcol) = lists["crumbs"]
    ids = moves[-1][1]
    degree = np.maximum(np.diff(bptr) - 1, 0)[ids]          # (pattern_of gives a node no element uses an empty row)
    assert (degree == 0).sum() >= 20 and (degree == 3).sum() >= 20 and (degree == 4).sum() >= 20 and moves[1][0]["n_new"] > 0 and len(moves[0][1]) > 0
    # bowtie: the list has nodes of two bodies and the shared corner
    moves, _ = lists["bowtie"]
    ids = moves[-1][1]
    assert 124 in ids and (ids < 124).any() and (ids > 124).any() and len(moves[0][1]) == 1
    # bighub: one source each, the hub and a node of its shell
    assert lists["bighub_hub"][0][-1][1].tolist() == [0] and lists["bighub_shell"][0][-1][1].tolist() == [17]
    for name in ("edges255", "edges256", "edges257"):
        (info, ids, _), = _contact_lists(name)[0]
        assert info["status"] == cr.fl.FB_CONTACT_SET and 20 < len(ids) < ai.NODES[name]


def test_cluster64k_fills_two_slots_of_the_walk_table_beyond_its_probes():
    v, t, _ = ai.mesh("cluster64k")
    shell = ai.cluster_shell()
    bptr, bcol = cr.pattern_of(t, len(v))
    ring = sorted(n for n, _ in cr.ball(bptr, bcol, ai.CLUSTER_HUB, 2))
    assert ring == shell.tolist() and len(ring) == ai.CLUSTER_DEGREE
    slots = {ai.table_slot(n) for n in ring}
    # 32 probes from slot s or s + 1 reach s .. s + 32: 33 slots for 40 nodes, whatever the order they arrive in
    assert slots == {ai.CLUSTER_SLOT, ai.CLUSTER_SLOT + 1} and len(ring) > 33
    assert ai.table_slot(0) == 0 and ai.table_slot(1) == 0x9E3779B1 >> 21 and ai.table_slot(65536) == (0x9E3779B1 << 16 & 0xFFFFFFFF) >> 21
    (info, ids, forces), = _contact_lists("cluster64k")[0]
    assert ids.tolist() == [ai.CLUSTER_HUB] and info["n_pushing"] == 1
    # the count alone predicts records: this is the case the restatement does not model
    for size, n_records in ((1, 0), (2, ai.CLUSTER_DEGREE)):
        want = cr.spread_by_records(bptr, bcol, ids, forces, size, np.zeros(3 * len(v)))
        assert (want["path"], want["n_records"]) == (cr.RECORDS, n_records)
    assert ai.CLUSTER_PATHS == {("cluster64k", 1): cr.RECORDS, ("cluster64k", 2): cr.LEVELS}


def test_haptic_sources_are_what_their_labels_say():
    v, t, _ = ai.mesh("crumbs")
    bptr, bcol = cr.pattern_of(t, len(v))
    degree = np.maximum(np.diff(bptr) - 1, 0)               # (pattern_of gives a node no element uses an empty row)
    s = ai.haptic_sources("crumbs")
    assert degree[s["isolated"][0]] == 0 and degree[s["lone_tet"][0]] == 3 and degree[s["hub"][0]] == 70
    assert [int(degree[i]) for i in s["mixed"]] == [0, 4, 5, 14], "an unused node, a node of a pair, of the hub's shell, inside the cube"
    v, t, _ = ai.mesh("bowtie")
    bptr, bcol = cr.pattern_of(t, len(v))
    ring1 = [n for n, _ in cr.ball(bptr, bcol, 124, 2)]
    assert any(n < 124 for n in ring1) and any(125 <= n < 249 for n in ring1), "the corner's first ring lies in both bodies"
    v, t, _ = ai.mesh("far")
    assert np.diff(cr.pattern_of(t, len(v))[0])[ai.haptic_sources("far")["isolated"][0]] == 0


@pytest.mark.parametrize("name", ["far", "crumbs", "bighub"])
def test_embedded_points_are_generic_and_of_both_kinds(name):
    v, t, _ = ai.mesh(name)
    pts = ai.embed_points(name)
    W = er.all_weights(v, t, pts)
    m = er.margin(v, t, pts, W)
    assert m.min() >= MARGIN, (name, m.min())
    ref = er.bind(v, t, pts, W=W)
    assert 30 <= ref["n_external"] <= len(pts) - 30, (name, ref["n_external"], len(pts))
    bound_parts = np.unique(pr.parts(v, t)["element_part"][ref["elements"][~ref["external"]]])
    assert len(bound_parts) >= (3 if name == "crumbs" else 2), "points inside elements of several bodies"
    if name == "bighub":
        at_hub = int((ref["vertices"][~ref["external"]] == 0).any(axis=1).sum())
        assert at_hub >= 200, "the hub's touch table is hundreds long"
    if name == "far":
        first, second = ref["elements"] < 384, ref["elements"] >= 384
        assert (first & ~ref["external"]).sum() > 20 and (second & ~ref["external"]).sum() > 5 and (second & ref["external"]).sum() > 5
        # cells of 0.1 over a box of 1e3 would be 1e12: the grid cannot resolve the elements, whatever its dimensions
        assert (v.max(0) - v.min(0)).max() / 0.1 > 1e4


def test_the_split_plane_of_crumbs_classifies_hundreds_of_parts():
    v, t, _ = ai.mesh("crumbs")
    ref = pr.split(v, ai.displacement(v), t, ai.crumbs_split_quad(), 0.05)
    assert ref["min_distance"] > 1e-3
    assert (ref["n_front_parts"], ref["n_back_parts"], ref["n_straddling_parts"]) == (94, 48, 1)
