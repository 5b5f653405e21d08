"""The mesh-side device pipelines (surface, stress, parts, detach, haptic, contact, embed, renumber) on the meshes of
tests/adversarial_inputs.py against their host references: unused nodes spread through the numbering, hundreds of parts of one element,
parts that meet in a node or an edge, a node of degree 1,100 in 2,196 elements, a node box 1e4 times an element, node counts of
255 / 256 / 257 and 65,537, and a hub whose neighbours crowd two slots of the contact walk's hash table.  What these inputs are is pinned
without a GPU by tests/test_adversarial_inputs.py.

No bound of its own: every comparison is made by the checker of the feature's own test file, imported from there, or is exact.  One handle
per (mesh, variant) for the whole module -- ``off`` keeps the caller's order, ``on`` works in the locality order, ``on_scrambled`` is
``on`` under permuted caller ids -- at the state ``adversarial_inputs.displacement``, set with set_q_state; the tests that change a mesh
make handles of their own."""
import ctypes as C
import functools

import numpy as np
import pytest

import adversarial_inputs as ai
import contactref as cr
import detachref as dr
import embedref as er
import hapticref as hr
import partsref as pr
import stressref as sr
import surfref
from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator, ProbeContact
from oracle.pyoracle import OrcFem
from test_embed_forces_gpu import host_add
from test_embed_gpu import _check_degenerate, _check_generic
from test_fem_surface_gpu import MIN_SUM, _topology, _update
from test_haptic_gpu import _check_box, _check_pick, _check_volume, _forces
from test_parts_gpu import _all, _check
from test_stress_gpu import LAM, MU, E, NU, _check_arrays, _check_info, _surface_check

pytestmark = pytest.mark.gpu

OFF, ON = fl.FB_RENUMBER_OFF, fl.FB_RENUMBER_ON
VARIANTS = ("off", "on", "on_scrambled")
BODIES = ("crumbs", "bowtie", "bighub", "far")
EDGES = ("edges255", "edges256", "edges257", "edges64k")
SIZES = (1, 2, 5)


def _new_handle(name, variant, **kw):
    v, t, fixed = ai.mesh(name, variant == "on_scrambled")
    g = FemIntegrator(v, t, fixed, E=E, nu=NU, renumber=OFF if variant == "off" else ON, **kw)
    assert g.renumbering()[0] == (variant != "off"), (name, variant)
    return g


def _displace(g, scale=1.0):
    u = scale * ai.displacement(g.verts)
    g.set_q_state(u, np.zeros_like(u))
    return u


@pytest.fixture(scope="module")
def handles(gpu):
    made = {}

    def get(name, variant):
        if (name, variant) not in made:
            made[name, variant] = _new_handle(name, variant)
        g = made[name, variant]
        _displace(g)
        g.contact_reset(keep_face=False)
        return g
    yield get
    for g in made.values():
        g.close()


def _ids(name, variant, ids):
    return [int(i) for i in ai.caller_ids(name, ids, variant == "on_scrambled")]


# ---- the node order --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BODIES + EDGES + ("cluster64k", "bighub8k"))
def test_device_order_is_the_host_restatement(handles, name):
    """renumber.hip against fb_plan_slab_order, as tests/test_renumber_gpu.py holds it on a blob and a brick: here with nodes of no
    element (an element count of 0) and, on bighub8k, a count above the 1,023 the second sort key clips to (the second stage runs from
    8,192 nodes on: on bighub8k and the meshes of 65,537 nodes)"""
    for variant in ("on", "on_scrambled"):
        g = handles(name, variant)
        v, t, _ = ai.mesh(name, variant == "on_scrambled")
        order = np.empty(len(v), np.int32)
        a, b = C.c_int(0), C.c_int(0)
        fl.check(fl.lib().fb_plan_slab_order(len(v), fl.dptr(np.ascontiguousarray(v)), len(t), fl.iptr(np.ascontiguousarray(t)), fl.iptr(order), C.byref(a), C.byref(b)))
        on, sc, si = g.renumbering()
        assert on and np.array_equal(g.owned_nodes(), order) and (sc, si) == (a.value, b.value)
        assert np.array_equal(np.sort(order), np.arange(len(v)))


# ---- surface ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", BODIES + EDGES + ("bighub8k",))
def test_surface(handles, name, variant):
    g = handles(name, variant)
    s, x0, t0 = _topology(g)
    assert s["n_builds"] == 1
    q = g.get_q_state()[0].reshape(-1, 3)
    assert surfref.normals(x0 + q, s["faces"], s["vertex_ids"])[1].min() >= MIN_SUM, "nothing is left out of the normals' comparison"
    xyz, nrm = _update(g, s, x0)
    again = g.surface_update()
    assert xyz.tobytes() == again[0].tobytes() and nrm.tobytes() == again[1].tobytes()
    if variant == "on":
        w, wx, wn, wb = (lambda h: (h.surface(),) + h.surface_update())(handles(name, "off"))
        assert all(np.array_equal(s[k], w[k]) for k in ("faces", "vertex_ids", "face_tets", "aabb")) and np.array_equal(xyz, wx)


# ---- stress ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stress_ref(name, scramble, scale=1.0):
    v, t, _ = ai.mesh(name, scramble)
    o = OrcFem(np.array(v), np.array(t), E, NU)
    u = scale * ai.displacement(v)
    return sr.stress(o, u, LAM, MU), sr.stress(o, u, LAM, MU, world=True)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", BODIES)
def test_stress(handles, name, variant):
    g = handles(name, variant)
    for world, ref in zip((False, True), _stress_ref(name, variant == "on_scrambled")):
        info = g.stress(world=world, tensors=True)
        arr = g.element_stress()
        _check_arrays(arr, ref, what="%s %s %s" % (name, variant, "world" if world else "rest frame"))
        _check_info(info, arr, ref["V"])
    s = _surface_check(g, "%s %s" % (name, variant))
    per_vertex = np.bincount(s["faces"].reshape(-1))
    if name == "crumbs":
        assert per_vertex[per_vertex > 0].min() == 3 and per_vertex.max() >= 8, "corners of lone tets beside the hubs' shells, in one launch"


# ---- parts -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", BODIES + EDGES + ("cluster64k", "bighub8k"))
def test_parts(handles, name, variant):
    g = handles(name, variant)
    got, ref, x, t = _check(g)
    if name == "crumbs":
        assert got["n_parts"] == 143 and got["n_unused_nodes"] == 177 and (got["elements"] == 1).sum() == 96
    if name == "bowtie":
        assert (got["n_parts"], got["n_shared_nodes"], got["largest_part"]) == (3, 3, 0)
    if variant == "on":        # caller-order outputs do not depend on the internal order: the same bits, volumes included
        off = _all(handles(name, "off"))
        for k in got:
            if k != "n_builds":
                assert np.asarray(got[k]).tobytes() == np.asarray(off[k]).tobytes(), k


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name,parts", [("crumbs", (0, 138, 142)), ("bowtie", (0, 1, 2))])
def test_read_part(handles, name, parts, variant):
    """a part of one element, the largest and the last of crumbs; the three bodies of bowtie, each of which has nodes of another"""
    g = handles(name, variant)
    x, t = g.read_mesh()
    ref = pr.parts(x, t)
    assert ref["elements"][parts[0]] == (1 if name == "crumbs" else 384) and parts[-1] == ref["n_parts"] - 1
    if name == "crumbs":
        assert parts[1] == ref["largest_part"]
    for k in parts:
        for a, b in zip(g.read_part(k), pr.extract(x, t, ref["element_part"], k)):
            assert np.array_equal(a, b), (name, k)
    if name == "bowtie":
        shared = _ids(name, variant, ai.BOWTIE_SHARED)
        assert all(np.isin(shared[:2], g.read_part(k)[1]).all() for k in (0, 2)) and all(shared[2] in g.read_part(k)[1] for k in (0, 1))


@pytest.mark.parametrize("variant", VARIANTS)
def test_split_parts_of_crumbs(gpu, variant):
    """the plane of adversarial_inputs.crumbs_split_quad: 94 parts in front, 48 behind, one straddling; as tests/test_parts_gpu.py holds a
    split of two parts against partsref.split"""
    g = _new_handle("crumbs", variant)
    try:
        q = _displace(g)
        x, t = g.read_mesh()
        quad = ai.crumbs_split_quad()
        ref = pr.split(x, q, t, quad, 0.05)
        assert (ref["n_front_parts"], ref["n_back_parts"], ref["n_straddling_parts"]) == (94, 48, 1) and ref["min_distance"] > 1e-6
        labels = _all(g)
        s = g.split_parts(quad, 0.05)
        for k in ("n_front_parts", "n_back_parts", "n_straddling_parts", "n_nodes_moved"):
            assert s[k] == ref[k], k
        assert np.all(np.abs(s["shift"] - ref["shift"]) <= 4 * np.spacing(np.abs(ref["shift"])))
        x1 = g.read_mesh()[0]
        assert np.array_equal(x1[ref["sign"] > 0], x[ref["sign"] > 0] + s["shift"]) and np.array_equal(x1[ref["sign"] < 0], x[ref["sign"] < 0] - s["shift"])
        assert np.array_equal(x1[ref["sign"] == 0], x[ref["sign"] == 0]) and np.array_equal(np.any(x1 != x, axis=1), ref["moved"])
        assert np.array_equal(g.get_q_state()[0], q)
        after = _all(g)
        assert after["n_builds"] == labels["n_builds"] and np.array_equal(after["element_part"], labels["element_part"])
        _check(g)
        _topology(g)
    finally:
        g.close()


@pytest.mark.parametrize("variant", ("off", "on"))
def test_split_parts_of_bowtie_keeps_the_shared_nodes(gpu, variant):
    """a plane through the shared corner, across the diagonal the two bodies lie along: the first and the third body behind it, the second
    in front, and the corner -- a node of a front part and of a back part -- stays"""
    g = _new_handle("bowtie", variant)
    try:
        q = _displace(g)
        x, t = g.read_mesh()
        n = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
        a, b = np.cross(n, [0.0, 1.0, 0.0]), np.cross(n, np.cross(n, [0.0, 1.0, 0.0]))
        c = x[124] + q.reshape(-1, 3)[124] + 0.013 * n
        quad = np.array([c - 5 * a - 5 * b, c + 5 * a - 5 * b, c - 5 * a + 5 * b, c + 5 * a + 5 * b])
        ref = pr.split(x, q, t, quad, 0.05)
        assert ref["min_distance"] > 1e-6 and ref["n_straddling_parts"] == 0 and {ref["n_front_parts"], ref["n_back_parts"]} == {1, 2}
        assert ref["sign"][124] == 0 and ref["n_nodes_moved"] == len(x) - 1
        s = g.split_parts(quad, 0.05)
        for k in ("n_front_parts", "n_back_parts", "n_straddling_parts", "n_nodes_moved"):
            assert s[k] == ref[k], k
        assert np.all(np.abs(s["shift"] - ref["shift"]) <= 4 * np.spacing(np.abs(ref["shift"])))
        x1 = g.read_mesh()[0]
        assert np.array_equal(x1[ref["sign"] > 0], x[ref["sign"] > 0] + s["shift"]) and np.array_equal(x1[ref["sign"] < 0], x[ref["sign"] < 0] - s["shift"])
        assert np.array_equal(x1[124], x[124]) and np.array_equal(np.any(x1 != x, axis=1), ref["moved"])
        _check(g)
        sf, x0, _ = _topology(g)
        _update(g, sf, x0)
    finally:
        g.close()


# ---- detach ----------------------------------------------------------------------------------------------------------------------------
def _contact_session(g, case):
    """the moves of adversarial_inputs.contact_boxes(case), each at its state, on the handle and on the host session side by side; after the
    last one every contact_apply of adversarial_inputs.CONTACT_PATHS for the case, on the path predicted"""
    probe, pattern = ProbeContact(), g.pattern()[:2]
    g.contact_reset(keep_face=False)
    boxes = ai.contact_boxes(case)
    for k, (lo, hi) in enumerate(boxes):
        _displace(g, ai.CONTACT_SCALES[k])
        dev, host = g.contact_move(lo, hi, cr.COEFF), probe.move(cr.positions(g), lo, hi, cr.COEFF)
        cr.assert_same_info(dev, host, "%s move %d" % (case, k))
        cr.assert_same_info(g.contact_info(), host, "%s info after move %d" % (case, k))
        cr.assert_same_list(g, probe, "%s move %d" % (case, k))
    assert dev["status"] == fl.FB_CONTACT_SET and dev["n_touched"] > 0
    pressed = probe.ids.copy()
    for (c, size), path in ai.CONTACT_PATHS.items():
        if c != case:
            continue
        info = cr.assert_apply(g, probe, pattern, size, "%s size %d" % (case, size), path=path)
        want = cr.spread_by_records(pattern[0], pattern[1], probe.ids, probe.forces, size, np.zeros(g.r))
        assert want["path"] == path
        if path == cr.RECORDS:
            assert (info["n_records"], info["n_targets"]) == (want["n_records"], want["n_targets"]), (case, size, info, want)
        else:
            assert (info["n_records"], info["n_targets"]) == (-1, -1), (case, size, info)
    # the session goes on after a reset that keeps the face
    g.contact_reset(keep_face=True)
    probe.reset(keep_face=True)
    cr.assert_same_info(g.contact_info(), probe.info(), "%s reset" % case)
    lo, hi = boxes[0]
    cr.assert_same_info(g.contact_move(lo, hi, cr.COEFF), probe.move(cr.positions(g), lo, hi, cr.COEFF), "%s after the reset" % case)
    cr.assert_same_list(g, probe, "%s after the reset" % case)
    _displace(g)
    return pressed


@pytest.mark.parametrize("variant", ("off", "on"))
@pytest.mark.parametrize("name,part", [("crumbs", 5), ("bowtie", 1), ("bowtie", 2)])
def test_detach_and_the_parent_afterwards(gpu, name, part, variant):
    """fb_fem_detach_part(remove) of a part of one element / of the body that shares the corner / of the body that shares the edge, whose
    two shared nodes are clamped: the piece is detachref.detach of read_part's arrays; the parent -- with fresh nodes no element uses and,
    on bowtie, nodes two bodies shared that one has now -- gives its parts, its surface and a contact session as any other mesh"""
    g = _new_handle(name, variant)
    try:
        _displace(g)
        fext = np.random.default_rng(5).normal(size=g.r) * 40.0
        g.set_external_forces(fext)
        fixed = g.constrained_dofs()
        assert np.array_equal(fixed, ai.mesh(name)[2])
        before = pr.parts(*g.read_mesh())
        assert before["elements"][part] == (1 if name == "crumbs" else 384)
        ids, nodes, xyz, tl = g.read_part(part)
        used_by_others = np.unique(g.read_mesh()[1][before["element_part"] != part])
        orphans = np.setdiff1d(nodes, used_by_others)
        assert len(orphans) == {("crumbs", 5): 4, ("bowtie", 1): 124, ("bowtie", 2): 123}[name, part]
        q, qv, qa = g.get_q_state()
        ref = dr.detach(ids, nodes, xyz, tl, fixed_dofs=fixed, vectors=dict(q=q, qvel=qv, qaccel=qa, fext=fext))
        piece, pids, pnodes = g.detach_part(part, remove=True)
        assert np.array_equal(pids, ids) and np.array_equal(pnodes, nodes)
        px, pt = piece.read_mesh()
        assert np.array_equal(px, ref["xyz"]) and np.array_equal(pt, ref["tets"]) and np.array_equal(piece.constrained_dofs(), ref["fixed"])
        for got, key in zip(piece.get_q_state(), ("q", "qvel", "qaccel")):
            assert np.array_equal(got, ref[key]), key
        assert np.array_equal(piece.external_forces(), ref["fext"])
        info = piece.detach_info
        assert (info["part"], info["n_elements"], info["n_nodes"], info["n_fixed_dofs"]) == (part, len(ids), len(nodes), len(ref["fixed"]))
        assert info["parent_elements_left"] == g.num_tets() == before["elements"].sum() - len(ids)
        piece.close()
        for a, b in zip(g.get_q_state(), (q, qv, qa)):
            assert np.array_equal(a, b)
        got, after, x, t = _check(g)
        assert after["n_parts"] == before["n_parts"] - 1
        assert after["n_unused_nodes"] == before["n_unused_nodes"] + len(orphans) and (after["node_part"][orphans] == -1).all()
        if name == "bowtie":
            assert after["n_shared_nodes"] == (2 if part == 1 else 1) and (after["node_part"][list(ai.BOWTIE_SHARED)] == 0).all()
            assert len(ref["fixed"]) == (0 if part == 1 else 6), "the clamped nodes of the shared edge are clamped in the piece"
        s, x0, _ = _topology(g)
        _update(g, s, x0)
        _check_volume(g)
        _contact_session(g, name)
    finally:
        g.close()


# ---- haptic ----------------------------------------------------------------------------------------------------------------------------
def _check_spread(g, ids, size, seed=3):
    """fb_fem_add_haptic_forces on top of gravity against hapticref.spread_by_levels on the mesh the handle holds: the same bits"""
    forces = _forces(len(ids), seed)
    g.set_uniform_force(1, cr.GRAVITY)
    g.add_haptic_forces(ids, forces, size)
    want = np.zeros(g.r)
    want[1::3] = cr.GRAVITY
    hr.spread_by_levels(g.n_nodes, g.read_mesh()[1], ids, forces, size, want)
    got = g.external_forces()
    assert np.array_equal(got, want), (ids, size, np.abs(got - want).max())
    return want.reshape(-1, 3)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", BODIES)
def test_haptic_spread(handles, name, variant):
    g = handles(name, variant)
    for label, src in ai.haptic_sources(name).items():
        ids = _ids(name, variant, src)
        for size in SIZES:
            f = _check_spread(g, ids, size)
            reached = np.nonzero(f[:, 0] != 0.0)[0]              # (x components come from the probe only)
            if label == "isolated":
                assert reached.tolist() == ids, "a source no element uses: its own force and nothing else"
            if (name, label) == ("bowtie", "corner") and size > 1:
                first, second = _ids(name, variant, np.arange(124)), _ids(name, variant, np.arange(125, 249))
                assert np.isin(reached, first).any() and np.isin(reached, second).any(), "forces arrive in both bodies"
            if (name, label) == ("bighub", "hub"):
                assert len(reached) == (1 if size == 1 else ai.BIGHUB + 1)
            if (name, label) == ("crumbs", "lone_tet"):
                assert len(reached) == (1 if size == 1 else 4)
    # more sources than a batch of the level arrays holds, nodes no element uses and a repeat among them
    many = np.random.default_rng(11).permutation(g.n_nodes)[:33].tolist()
    many[7] = many[2]
    bptr = g.pattern()[0]
    if name in ("crumbs", "far"):
        many[0], many[32] = _ids(name, variant, [ai.haptic_sources(name)["isolated"][0], ai.haptic_sources(name)["isolated"][0]])
        assert np.diff(bptr)[many[0]] == 1
    _check_spread(g, many, 5)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", EDGES)
def test_pick_box_and_volume_at_the_workgroup_edges(handles, name, variant):
    g = handles(name, variant)
    scr = variant == "on_scrambled"
    p = hr.positions(g.verts, g.get_q_state()[0])
    n = g.n_nodes
    last = int(ai.caller_ids(name, [n - 1], scr)[0]) if scr else n - 1
    # the winner is the node with the highest caller id -- and, scrambled or not, the last node of the unscrambled mesh
    for node in {n - 1, last}:
        assert _check_pick(g, tuple(p[node] + [3e-3, -2e-3, 1e-3])) == node
    # two nodes tie exactly and the lower caller id wins (at rest: adversarial_inputs.tie_pairs, three of them by the census)
    g.reset_to_rest()
    for a, b, w in ai.tie_pairs(name):
        a, b = _ids(name, variant, [a, b])
        assert _check_pick(g, w) == min(a, b)
    _displace(g)
    assert len(_check_box(g, p.min(0), p.max(0))) == n
    lo, hi = ai.contact_boxes(name)[0]
    assert 20 < len(_check_box(g, lo, hi)) < n
    assert len(_check_box(g, p[last], p[last])) == 1
    _check_volume(g)
    if variant == "on":
        ta, pa = g.volume(per_element=True)
        tb, pb = handles(name, "off").volume(per_element=True)
        assert np.array_equal(pa, pb) and ta == tb


# ---- contact ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", ["crumbs", "bowtie", "bighub_hub", "bighub_shell"])
def test_contact_sessions_and_spread_paths(handles, case, variant):
    """crumbs: sources without a neighbour reserve no record; bowtie: the walk crosses the shared corner; bighub: the hub's ball overflows
    the walk's table in ring 1 (size 2: the level arrays; size 1: no walk), a shell node's in ring 2"""
    g = handles(ai.contact_mesh(case), variant)
    pressed = _contact_session(g, case)
    if case == "crumbs":
        bptr, _ = g.pattern()[:2]
        assert (np.diff(bptr)[pressed] == 1).sum() >= 20, "sources with no neighbour in the list that was spread"


@pytest.mark.parametrize("variant", ("off", "on"))
def test_contact_fallback_by_record_budget_on_crumbs(handles, monkeypatch, variant):
    """tests/test_contact_gpu.py's budget fallback with sources that reserve no record in the list"""
    g = handles("crumbs", variant)
    probe, pattern = ProbeContact(), g.pattern()[:2]
    lo, hi = ai.contact_boxes("crumbs")[1]
    cr.assert_same_info(g.contact_move(lo, hi, cr.COEFF), probe.move(cr.positions(g), lo, hi, cr.COEFF))
    need = cr.assert_apply(g, probe, pattern, 5, path=cr.RECORDS)["n_records"]
    assert need == cr.spread_by_records(pattern[0], pattern[1], probe.ids, probe.forces, 5, np.zeros(g.r))["n_records"] > 0
    monkeypatch.setenv("FEMBRAIN_CONTACT_MAX_RECORDS", str(need - 1))
    info = cr.assert_apply(g, probe, pattern, 5, path=cr.LEVELS)
    assert info["n_records"] == need and info["n_targets"] == -1
    monkeypatch.setenv("FEMBRAIN_CONTACT_MAX_RECORDS", str(need))
    cr.assert_apply(g, probe, pattern, 5, path=cr.RECORDS)


def test_contact_walk_gives_up_by_clustering(handles):
    """cluster64k on a handle that keeps the caller's order: the 40 neighbours of the source have two home slots of the walk's table
    between them, and 32 probes reach 33 slots.  The walk must fall back to the level arrays with 41 nodes in its table of 1,024 --
    contactref.spread_by_records, which counts, predicts records here -- and the vector is the host's either way."""
    g = handles("cluster64k", "off")
    probe, pattern = ProbeContact(), g.pattern()[:2]
    (lo, hi), = ai.contact_boxes("cluster64k")
    cr.assert_same_info(g.contact_move(lo, hi, cr.COEFF), probe.move(cr.positions(g), lo, hi, cr.COEFF))
    cr.assert_same_list(g, probe)
    assert probe.ids.tolist() == [ai.CLUSTER_HUB]
    for (_, size), path in ai.CLUSTER_PATHS.items():
        info = cr.assert_apply(g, probe, pattern, size, "cluster64k size %d" % size, path=path)
        assert (info["n_records"], info["n_targets"]) == ((0, 0) if path == cr.RECORDS else (-1, -1)), info


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", EDGES)
def test_contact_move_at_the_workgroup_edges(handles, name, variant):
    g = handles(name, variant)
    probe = ProbeContact()
    (lo, hi), = ai.contact_boxes(name)
    dev, host = g.contact_move(lo, hi, cr.COEFF), probe.move(cr.positions(g), lo, hi, cr.COEFF)
    cr.assert_same_info(dev, host, name)
    cr.assert_same_list(g, probe, name)
    assert dev["status"] == fl.FB_CONTACT_SET and 20 < dev["n_touched"] < g.n_nodes
    cr.assert_apply(g, probe, g.pattern()[:2], 2, name, path=cr.RECORDS)


# ---- embed -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _embed_ref(name, scramble):
    v, t, _ = ai.mesh(name, scramble)
    gen = ai.embed_points(name)
    deg = er.degenerate_points(v, t)
    contained = np.array([len(c) > 0 for c in er.bind(v, t, deg, tol=1e-12)["containing"]])
    return gen, deg[contained]          # (a node no element uses is in no element: not a degenerate point of the rule)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["far", "crumbs", "bighub"])
def test_embed(handles, name, variant):
    g = handles(name, variant)
    v, t, _ = ai.mesh(name, variant == "on_scrambled")
    gen, deg = _embed_ref(name, variant == "on_scrambled")
    assert len(deg) >= 5
    n = len(gen)
    eid, info = g.embed(np.vstack([gen, deg]), info=True)
    e2 = None
    try:
        got = g.embedding(eid)
        head = {k: a[:n] for k, a in got.items()}
        ref = _check_generic(v, t, gen, head, None)
        assert 30 <= ref["n_external"] <= n - 30
        assert ref["n_external"] <= info["n_external"] <= ref["n_external"] + len(deg)   # (pinned on the generic points, as test_embed_gpu.py does)
        _check_degenerate(v, t, deg, {k: a[n:] for k, a in got.items()})
        e2, i2 = g.embed(gen, info=True)
        assert i2["n_external"] == ref["n_external"] and i2["n_points"] == n
        b = g.embedding(e2)
        # the update: one float rounding of the fp64 sum (test_embed_gpu.py's _check_update), at the displaced state
        want = np.float32(er.positions(*g.read_mesh()[:1], g.get_q_state()[0], b["vertices"], b["weights"]))
        xyz, _, uinfo = g.embed_update(e2)
        assert xyz.dtype == np.float32 and (np.abs(xyz.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
        assert np.array_equal(uinfo["aabb"], np.array([xyz.min(axis=0), xyz.max(axis=0)]))
        # the way back: the ordered scatter of test_embed_forces_gpu.py
        g.set_external_forces(np.random.default_rng(5).standard_normal(g.r) * 100.0)
        base = g.external_forces()
        f1 = np.random.default_rng(6).standard_normal((n, 3))
        g.embed_add_forces(e2, f1)
        out = g.external_forces()
        assert out.tobytes() == host_add(base, b, f1).tobytes(), "max difference %g" % np.abs(out - host_add(base, b, f1)).max()
        counts = np.bincount(b["vertices"].ravel(), minlength=len(v))
        fi = g.embed_forces_info(e2)
        assert fi == dict(n_table_builds=1, longest_run=int(counts.max()), n_nodes_touched=int((counts > 0).sum())), (fi, counts.max())
        if name == "bighub":
            hub = _ids(name, variant, [0])[0]
            assert counts.argmax() == hub and fi["longest_run"] >= 200, "the hub's run of the touch table is hundreds long"
        if name == "far":
            assert np.prod(info["grid"]) >= 1
    finally:
        g.embed_release(eid)
        if e2 is not None:
            g.embed_release(e2)


# ---- a host-built plan -----------------------------------------------------------------------------------------------------------------
def test_host_built_plan_on_crumbs(gpu, monkeypatch):
    monkeypatch.setenv("FEMBRAIN_PLAN_DEVICE", "0")
    g = _new_handle("crumbs", "off")
    try:
        assert g._L.fb_fem_plan_on_device(g.h) == 0
        _displace(g)
        _check(g)
        for label, src in ai.haptic_sources("crumbs").items():
            _check_spread(g, src, 5)
        _contact_session(g, "crumbs")          # (the pattern the walk reads is uploaded, not device-built)
    finally:
        g.close()


# ---- one step ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["crumbs", "bowtie", "bighub"])
def test_one_step_and_everything_that_reads_q_on_the_moved_state(gpu, name):
    """one do_timestep under a uniform load from rest on a handle of either numbering; between the two what tests/test_renumber_gpu.py
    asserts of a renumbered handle against one that keeps the caller's order (iteration counts within max(3, 2 %); q within 2e-5 of its
    largest where the matrix is stored in fp64, 2e-4 in fp32, qvel within five times that; nothing on a constrained DOF); then every check
    above that reads q, on the state the step left.

    bighub: the handle builds and solves with a row of 1,101 blocks (a slice 1,101 slots wide), and each numbering is held against the
    oracle's step as that file holds its handles (the same bounds).  The iteration counts of the two numberings are not compared there:
    the hub's 2,196 slivers make a system of 3,495 unknowns on which the oracle's CG takes 1,463 iterations, far into the regime where
    rounding decides when the residual crosses the tolerance -- measured with fp64 storage: 1,467 (caller's order) and 1,541 (locality
    order) for the merged solver, 1,542 and 1,464 for the reference variant, that is, two solvers in ONE order differ by as much as the
    two orders do, while every one of the four states agrees with the oracle's to 1.3e-9 of its largest."""
    a, b = _new_handle(name, "on"), _new_handle(name, "off")
    try:
        fixed = ai.mesh(name)[2]
        for g in (a, b):
            g.set_uniform_force(1, cr.GRAVITY)
        ia, ib = a.do_timestep(), b.do_timestep()
        assert a.last.converged == 1 and b.last.converged == 1
        (qa, wa, _), (qb, wb, _) = a.get_q_state(), b.get_q_state()
        print("%s: %d iterations in the locality order, %d in the caller's; q differs by %.3g of its largest" % (name, ia, ib, np.abs(qa - qb).max() / np.abs(qb).max()))
        assert a.matrix_precision() == b.matrix_precision()
        tol = 2e-5 if a.matrix_precision() == fl.FB_MATRIX_F64 else 2e-4
        assert np.abs(qb).max() > 0 and np.abs(qa - qb).max() <= tol * np.abs(qb).max() and np.abs(wa - wb).max() <= 5 * tol * np.abs(wb).max() and not qa[fixed].any()
        if name != "bighub":
            assert abs(ia - ib) <= max(3, 0.02 * ib), (ia, ib)
        else:
            v, t, _ = ai.mesh(name)
            o = OrcFem(np.array(v), np.array(t), E, NU)
            o.integrator(fixed)
            f = np.zeros(3 * len(v))
            f[1::3] = cr.GRAVITY
            o.set_external_forces(f)
            o.step()
            qo = o.get_state()[0]
            for q in (qa, qb):
                assert np.abs(q - qo).max() <= tol * np.abs(qo).max()
        for g, variant in ((a, "on"), (b, "off")):
            q = g.get_q_state()[0]
            s, x0, t0 = _topology(g)
            _update(g, s, x0)
            info = g.stress(tensors=True)
            arr = g.element_stress()
            o = OrcFem(np.array(g.verts), np.array(g.tets), E, NU)
            ref = sr.stress(o, q, LAM, MU)
            _check_arrays(arr, ref, what="%s %s after a step" % (name, variant))
            _check_info(info, arr, ref["V"])
            _surface_check(g, "%s %s after a step" % (name, variant))
            _check_volume(g)
            p = hr.positions(g.verts, q)
            _check_pick(g, tuple(p[g.n_nodes - 1] + 1e-3))
            assert len(_check_box(g, p.min(0), p.max(0))) == g.n_nodes
            lo, hi = ai.contact_boxes(name if name != "bighub" else "bighub_shell")[-1]
            probe = ProbeContact()
            cr.assert_same_info(g.contact_move(lo, hi, cr.COEFF), probe.move(cr.positions(g), lo, hi, cr.COEFF), name)
            cr.assert_same_list(g, probe, name)
            cr.assert_apply(g, probe, g.pattern()[:2], 2, name)
            if name == "crumbs":
                gen = ai.embed_points(name)
                eid = g.embed(gen)
                bnd = g.embedding(eid)
                want = np.float32(er.positions(x0, q, bnd["vertices"], bnd["weights"]))
                xyz = g.embed_update(eid)[0]
                assert (np.abs(xyz.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
                g.embed_release(eid)
    finally:
        a.close()
        b.close()
