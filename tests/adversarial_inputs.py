"""Meshes built to reach the branches, limits and index arithmetic of the mesh-side device pipelines (surface, stress, parts, detach, haptic,
contact, embed, renumber) that cubes, Delaunay lattices and the shipped blobs never reach; pinned without a GPU by
tests/test_adversarial_inputs.py, run on the device by tests/test_mesh_side_adversarial_gpu.py.  Built from the parts of product_inputs.py.

  crumbs     143 parts, most of one or two elements, 177 nodes no element uses spread through the numbering (a whole aligned 64-node run of
             them in front), a hub of degree 70, a cube, a rod; 64 * 22 + 1 nodes
  bowtie     three cube(5) blocks merged by index: the second shares one corner node with the first, the third one edge (two nodes) of
             the first -- three parts, three shared nodes, one component of the node adjacency
  bighub     hub(1100) and a cube(4): a node of degree 1,100 (above the contact walk's table of 1,024) in 2,196 elements (above the
             renumbering's count clip of 1,023)
  bighub8k   bighub and unused nodes up to 8,193 nodes, the size from which the renumbering sorts by element counts and that clip applies
  far        cube(5), a cube(3) 50 units away and three nodes no element uses at 1e3 along each axis: a node box four orders of
             magnitude larger than an element
  edges255 / edges256 / edges257   small joins of the same kinds padded to one below, exactly, and one above a workgroup of 256 threads
  edges64k   65,537 nodes, one more than 256 workgroups of 256 threads: a rod and two crumbs, the rest unused
  cluster64k edges64k with a hub of degree 40 on node ids that all hash to two neighbouring slots of the contact walk's table

Every mesh is (vertices, tets, fixed DOFs); ``scrambled`` permutes the caller's node ids.  The displacement the tests set, the contact
boxes, the haptic sources and the embedded points are defined here too, so that the census and the device tests speak of the same cases."""
import functools

import numpy as np

import cut_inputs as ci
import embedref as er
from fembrain_amd.meshgen import fixed_vertices_to_dofs
from product_inputs import cube, hub, hub_block, isolated, join, rod, tet_path


def scrambled(v, t, fixed, seed=3):
    """the same mesh with the caller's node ids permuted"""
    perm = np.random.default_rng(seed).permutation(len(v))          # new id of old node
    v2 = np.empty_like(v)
    v2[perm] = v
    t2 = np.ascontiguousarray(perm[t].astype(np.int32))
    node, comp = np.asarray(fixed, np.int64) // 3, np.asarray(fixed, np.int64) % 3
    return v2, t2, np.sort(3 * perm[node] + comp).astype(np.int32)


# ---- the meshes ---------------------------------------------------------------------------------------------------------------------
CRUMBS_NODES = 64 * 22 + 1
# node ranges of crumbs' parts (join places them in this order; the third is the pad to a multiple of 64)
CRUMBS_AT = dict(isolated=(0, 70), tet_path=(70, 654), pad=(654, 704), hub=(704, 775), cube=(775, 900), isolated3=(900, 903), rod=(903, 1303),
                 hub_block=(1303, 1355), tail=(1355, CRUMBS_NODES))


def crumbs():
    return join([isolated(70), tet_path(96, 40), 64, hub(70), cube(5), isolated(3), rod(2, 2, 100), hub_block(12)], n_nodes=CRUMBS_NODES)


BOWTIE_SHARED = (0, 1, 124)       # the edge (nodes 0 and 1 of the first block) and the corner (its last node)


def bowtie():
    """first block: nodes 0 .. 124; second: its node 0 IS node 124 of the first (the blocks lie corner to corner); third: its nodes 123
    and 124 ARE nodes 0 and 1 of the first (edge to edge, shifted along the edge so that no other two nodes coincide)"""
    v, t, f = cube(5)
    n = len(v)
    assert n == 125
    map_b = np.concatenate([[124], n + np.arange(n - 1)])                                  # old id of the second block -> merged id
    map_c = np.concatenate([2 * n - 1 + np.arange(n - 2), [0, 1]])
    vb, vc = v + (v[124] - v[0]), v + (v[0] - v[123])
    assert np.array_equal(vc[124], v[1]) or np.abs(vc[124] - v[1]).max() < 1e-15
    verts = np.concatenate([v, vb[1:], vc[:123]])
    tets = np.concatenate([t, map_b[t], map_c[t]]).astype(np.int32)
    return np.ascontiguousarray(verts), np.ascontiguousarray(tets), fixed_vertices_to_dofs(f)


BIGHUB = 1100


def bighub():
    return join([hub(BIGHUB), cube(4)])


def bighub8k():
    """bighub with nodes no element uses up to 8,193: from 8,192 nodes on the locality order has a second stage, a sort inside windows by
    the number of elements on a node, whose key clips that number to 1,023 -- the hub has 2,196, the unused nodes 0"""
    return join([hub(BIGHUB), cube(4)], n_nodes=8193)


def far():
    va, ta, fa = cube(5)
    vb, tb, _ = cube(3)
    lone = 1e3 * np.eye(3)
    verts = np.concatenate([va, lone, vb + [50.0, 0.0, 0.0]])
    tets = np.concatenate([ta, tb + len(va) + 3]).astype(np.int32)
    return np.ascontiguousarray(verts), np.ascontiguousarray(tets), fixed_vertices_to_dofs(fa)


FAR_LONE = (125, 126, 127)


def _edges(n_nodes):
    return join([isolated(5), tet_path(6, 4), hub(20), cube(3), isolated(3), rod(2, 2, 10)], n_nodes=n_nodes)


def edges64k():
    return join([isolated(70), rod(2, 2, 200), tet_path(4, 2)], n_nodes=256 * 256 + 1)


def table_slot(node):
    """the home slot of a node in the hash table of the contact walk (k_ct_walk of fembrain_amd/csrc/contact.hip: 2,048 slots, linear
    probing, at most 32 probes): the top 11 bits of node * 0x9E3779B1 in 32 bits"""
    return ((int(node) * 0x9E3779B1) & 0xFFFFFFFF) >> 21


CLUSTER_SLOT, CLUSTER_DEGREE, CLUSTER_HUB = 777, 40, 900


def cluster_shell():
    """the first CLUSTER_DEGREE node ids from 1,000 on whose home slot is CLUSTER_SLOT or the one after it"""
    ids = [i for i in range(1000, 256 * 256 + 1) if table_slot(i) in (CLUSTER_SLOT, CLUSTER_SLOT + 1)]
    return np.array(ids[:CLUSTER_DEGREE], np.int64)


def cluster64k():
    """edges64k with a hub(40) laid over 41 of its unused nodes: the centre on node 900, the shell on nodes whose ids all hash to two
    neighbouring slots of the walk's table.  On a handle that keeps the caller's order the walk from the centre wants 40 entries in the 33
    slots that 32 probes from those two reach: it must give up by clustering, with 41 nodes in a table of 1,024"""
    v, t, fixed = edges64k()
    hv, ht, _ = hub(CLUSTER_DEGREE)
    ids = np.concatenate([[CLUSTER_HUB], cluster_shell()])
    v = v.copy()
    v[ids] = hv + [0.0, 5.0, 0.0]
    return v, np.ascontiguousarray(np.concatenate([t, ids[ht]]).astype(np.int32)), fixed


INPUTS = {"cluster64k": cluster64k, "crumbs": crumbs, "bowtie": bowtie, "bighub": bighub, "bighub8k": bighub8k, "far": far, "edges255": lambda: _edges(255), "edges256": lambda: _edges(256),
          "edges257": lambda: _edges(257), "edges64k": edges64k}
NODES = {"crumbs": CRUMBS_NODES, "bowtie": 372, "bighub": BIGHUB + 1 + 64, "bighub8k": 8193, "far": 155, "edges255": 255, "edges256": 256, "edges257": 257, "edges64k": 65537, "cluster64k": 65537}


@functools.lru_cache(maxsize=None)
def mesh(name, scramble=False):
    """(vertices, tets, fixed DOFs) of INPUTS[name], computed once and never written to; scramble: under permuted caller ids"""
    out = INPUTS[name]()
    if scramble:
        out = scrambled(*out)
    for a in out:
        a.setflags(write=False)
    return out


# ---- the state the device tests set -------------------------------------------------------------------------------------------------
def displacement(v, scale=0.03):
    """ci.smooth_displacement at the scale the stress and haptic tests use, of sin(v) instead of v: those tests run it on bodies inside the
    unit box, where the field's gradient is a few per cent; its term ``cos(..) * x`` grows with the coordinates, and these meshes reach 50
    with elements and 1e3 with nodes, where it would shear an element by its own size.  sin keeps the argument in the unit box with a
    gradient of at most one, so the deformation gradient stays what it is there on every part, wherever it lies."""
    return ci.smooth_displacement(np.sin(np.asarray(v, np.float64).reshape(-1, 3)), scale).reshape(-1)


# ---- the haptic sources ---------------------------------------------------------------------------------------------------------------
def haptic_sources(name):
    """{label: [node ids]} of the spreads the device test runs on mesh ``name`` (caller ids of the unscrambled mesh)"""
    if name == "crumbs":
        a = CRUMBS_AT
        return {"isolated": [3], "lone_tet": [a["tet_path"][0] + 5], "hub": [a["hub"][0]], "mixed": [a["pad"][0], a["tet_path"][0] + 4 * 96 + 2, a["hub"][0] + 7, a["cube"][0] + 62]}
    if name == "bowtie":
        return {"corner": [124], "edge": [0, 1], "inside": [62]}
    if name == "bighub":
        return {"hub": [0], "shell": [17], "hub_and_cube": [0, BIGHUB + 1 + 21]}
    if name == "far":
        return {"isolated": [FAR_LONE[1]], "both": [62, 128 + 13]}
    raise KeyError(name)


# ---- the contact cases ------------------------------------------------------------------------------------------------------------------
def contact_boxes(name):
    """[(lo, hi)] of the tool box's moves on mesh ``name`` at the state ``displacement``: the second box contains the first"""
    v, _, _ = mesh(contact_mesh(name))
    p = v + displacement(v).reshape(-1, 3)
    if name == "crumbs":          # over the first isolated nodes (z = 0) and the first tet_path crumbs of both rows (z = 10)
        return [(np.array([-1.0, -2.0, -1.0]), np.array([1.55, 1.0, 11.0])), (np.array([-1.0, -2.0, -1.0]), np.array([3.05, 1.0, 11.0]))]
    if name == "bowtie":          # around the shared corner, then wider: nodes of the first and the second block
        c = p[124]
        return [(c - 0.05, c + 0.05), (c - 0.12, c + 0.12)]
    if name == "bighub_hub":      # the hub alone
        return [(p[0] - 0.02, p[0] + 0.02)]
    if name == "bighub_shell":    # one node of the shell alone
        r = 0.4 * np.sort(np.linalg.norm(p[1:BIGHUB + 1] - p[17], axis=1))[1]
        return [(p[17] - r, p[17] + r)]
    if name == "cluster64k":      # the centre of the hub alone
        return [(p[CLUSTER_HUB] - 0.02, p[CLUSTER_HUB] + 0.02)]
    if name.startswith("edges"):  # everything with x <= 0.25: isolated nodes, crumbs, a slice of the rod
        lo = p.min(0) - 1.0
        hi = p.max(0) + 1.0
        hi[0] = 0.25
        return [(lo, hi)]
    raise KeyError(name)


CONTACT_SCALES = (1.0, 0.5)       # move k is made at the state CONTACT_SCALES[k] * displacement: first-touch positions differ from current ones
RECORDS, LEVELS = 0, 1            # lib.FB_CONTACT_SPREAD_RECORDS / _LEVELS (the census holds them against the library's)
# (case, size) of every contact_apply the device test makes after the case's last move, and the path contactref.spread_by_records
# predicts for it (pinned by the census): the level arrays on bighub by overflow of the walk's table in ring 1 (the hub) and ring 2 (a
# node of its shell); on cluster64k by the 32 probes, where the count alone (41 nodes) predicts records -- CLUSTER_PATHS has what the device
# must do on a handle that keeps the caller's order
CLUSTER_PATHS = {("cluster64k", 1): RECORDS, ("cluster64k", 2): LEVELS}
CONTACT_PATHS = {("crumbs", 1): RECORDS, ("crumbs", 2): RECORDS, ("crumbs", 5): RECORDS, ("bowtie", 2): RECORDS, ("bowtie", 5): RECORDS,
                 ("bighub_hub", 1): RECORDS, ("bighub_hub", 2): LEVELS, ("bighub_shell", 2): RECORDS, ("bighub_shell", 3): LEVELS}


def contact_mesh(case):
    return case.split("_")[0]


def caller_ids(name, ids, scramble):
    """node ids of the unscrambled mesh ``name`` as the caller of ``mesh(name, scramble)`` numbers them"""
    ids = np.asarray(ids, np.int64)
    return ids if not scramble else np.random.default_rng(3).permutation(NODES[name])[ids]


# ---- pick ties --------------------------------------------------------------------------------------------------------------------------
def tie_pairs(name, most=3):
    """[(a, b, w)], a < b: points w at rest exactly as far from node a as from node b (the same bits of hapticref.pick_vertex's d) and
    farther from every other node -- midpoints of neighbours among the last 40 nodes, which no element uses and which lie 0.1 apart along
    x; found from the last node down"""
    v, _, _ = mesh(name)
    out = []
    for b in range(len(v) - 1, len(v) - 40, -1):
        a = b - 1
        w = (v[a] + v[b]) / 2.0
        dx = v - w
        d = (dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]) + dx[:, 2] * dx[:, 2]
        if d[a] == d[b] and np.count_nonzero(d <= d[a]) == 2:
            out.append((a, b, w))
        if len(out) == most:
            break
    return out


# ---- the embedded points ------------------------------------------------------------------------------------------------------------------
def embed_points(name):
    """generic points (embedref.generic_points: float32 values) for mesh ``name``: inside and around its bodies, and in the box of all nodes"""
    v, t, _ = mesh(name)
    if name == "far":
        return np.vstack([er.generic_points(v[:125], 200, 51), er.generic_points(v[128:], 100, 52), er.generic_points(v, 60, 53, grow=0.0)])
    if name == "crumbs":
        a = CRUMBS_AT
        return np.vstack([er.generic_points(v[a["cube"][0]:a["cube"][1]], 150, 54), er.generic_points(v[a["hub"][0]:a["hub"][1]], 80, 55),
                          er.generic_points(v[a["tet_path"][0]:a["tet_path"][0] + 40], 60, 56), er.generic_points(v, 40, 57, grow=0.0)])
    if name == "bighub":
        return np.vstack([er.generic_points(v[:BIGHUB + 1], 500, 58, grow=0.0), er.generic_points(v[BIGHUB + 1:], 60, 59)])
    raise KeyError(name)


# ---- the split plane of crumbs -------------------------------------------------------------------------------------------------------------
def crumbs_split_quad():
    """a plane x = const through the tet_path rows of crumbs (crumb i starts at x = 0.2 i and is 0.1 wide; the centroids of a pair's two
    elements lie 0.025 and 0.05 into it): the crumbs before it and the bodies around the origin lie behind, the ones after it in front,
    and pair 20 straddles -- at the state ``displacement``, which moves that row by 0.025 along x, its two centroids are at 4.0497 and
    4.0754, 0.0128 either side of the plane"""
    x = 0.2 * 20 + 0.0625
    return np.array([[x, -5.0, -5.0], [x, 5.0, -5.0], [x, -5.0, 120.0], [x, 5.0, 120.0]])
