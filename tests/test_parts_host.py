"""tests/partsref.py pinned on hand-made cases with literal answers: the checker of test_parts_gpu.py is itself checked where no GPU is."""
import numpy as np

import cutref as cr
import partsref as pr
from fembrain_amd.meshgen import truth_cube

X7 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [2, 0, 0], [0, 2, 0]], np.float64)


def test_one_tet():
    p = pr.parts(X7[:4], [[0, 1, 2, 3]])
    assert p["n_parts"] == 1 and p["largest_part"] == 0 and p["n_shared_nodes"] == 0 and p["n_unused_nodes"] == 0
    assert p["element_part"].tolist() == [0] and p["node_part"].tolist() == [0, 0, 0, 0]
    assert p["elements"].tolist() == [1] and p["nodes"].tolist() == [4] and p["first_element"].tolist() == [0]
    assert p["volume"].tolist() == [1.0 / 6.0]


def test_a_face_connects_an_edge_or_a_node_does_not():
    face = pr.parts(X7[:5], [[0, 1, 2, 3], [1, 2, 3, 4]])
    assert face["n_parts"] == 1 and face["element_part"].tolist() == [0, 0] and face["nodes"].tolist() == [5] and face["n_shared_nodes"] == 0
    edge = pr.parts(X7[:6], [[0, 1, 2, 3], [0, 1, 4, 5]])
    assert edge["n_parts"] == 2 and edge["element_part"].tolist() == [0, 1]
    assert edge["node_part"].tolist() == [0, 0, 0, 0, 1, 1] and edge["nodes"].tolist() == [4, 4] and edge["n_shared_nodes"] == 2
    node = pr.parts(X7, [[0, 1, 2, 3], [0, 4, 5, 6]])
    assert node["n_parts"] == 2 and node["node_part"].tolist() == [0, 0, 0, 0, 1, 1, 1] and node["n_shared_nodes"] == 1
    assert node["largest_part"] == 0  # (lowest index of equals)


def test_three_on_one_face_a_loose_tet_and_an_orphan_node():
    x = np.vstack([X7, [[5, 5, 5], [6, 5, 5], [5, 6, 5], [5, 5, 6], [9, 9, 9]]])
    t = [[7, 8, 9, 10], [0, 1, 2, 3], [0, 1, 2, 4], [0, 1, 2, 5]]   # the loose tet first: it is part 0
    p = pr.parts(x, t)
    assert p["n_parts"] == 2 and p["element_part"].tolist() == [0, 1, 1, 1] and p["first_element"].tolist() == [0, 1]
    assert p["largest_part"] == 1 and p["elements"].tolist() == [1, 3] and p["nodes"].tolist() == [4, 6]
    assert p["node_part"].tolist() == [1, 1, 1, 1, 1, 1, -1, 0, 0, 0, 0, -1] and p["n_unused_nodes"] == 2 and p["n_shared_nodes"] == 0


def test_parts_are_ordered_by_their_smallest_element():
    # elements 0, 2 | 1, 3 are the two face-connected pairs whatever their node ids are
    x = np.vstack([X7[:5], X7[:5] + 10.0])
    t = [[5, 6, 7, 8], [0, 1, 2, 3], [6, 7, 8, 9], [1, 2, 3, 4]]
    p = pr.parts(x, t)
    assert p["element_part"].tolist() == [0, 1, 0, 1] and p["first_element"].tolist() == [0, 1]
    assert p["node_part"].tolist() == [1] * 5 + [0] * 5


def test_a_long_chain_is_one_part_and_agrees_with_the_union_find():
    v, t = truth_cube(60, 2, 2, 0.1)
    assert len(np.unique(pr.roots(t))) == 1
    t2 = np.vstack([t[:100], t[130:]])   # a gap of five cells
    r, f = pr.roots(t2), cr.face_components(t2)
    assert len(np.unique(r)) == 2
    assert np.array_equal(r[:, None] == r[None, :], f[:, None] == f[None, :])
    assert np.array_equal(r, np.where(np.arange(len(t2)) < 100, 0, 100))


def test_split_moves_front_and_back_and_keeps_a_shared_node():
    # two tets that meet in node 0 only, on either side of the plane x = 0.5
    x = np.array([[0.5, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [2, 1, 0], [2, 0, 1], [3, 0, 0]], np.float64)
    t = [[0, 1, 2, 3], [0, 4, 5, 6]]
    quad = [[0.5, -5, -5], [0.5, 5, -5], [0.5, -5, 5], [0.5, 5, 5]]   # (q1 - q0) x (q2 - q0) = +x
    s = pr.split(x, np.zeros_like(x), t, quad, 0.25)
    assert s["shift"].tolist() == [0.25, 0.0, 0.0]
    assert (s["n_front_parts"], s["n_back_parts"], s["n_straddling_parts"]) == (1, 1, 0)
    assert s["sign"].tolist() == [0, -1, -1, -1, 1, 1, 1] and s["n_nodes_moved"] == 6
    assert np.array_equal(s["x0"][:, 0], [0.5, -0.25, -0.25, -1.25, 2.25, 2.25, 3.25]) and np.array_equal(s["x0"][:, 1:], x[:, 1:])
    # a plane through the first tet: it straddles and stays, the other is in front
    quad2 = [[-0.2, -5, -5], [-0.2, 5, -5], [-0.2, -5, 5], [-0.2, 5, 5]]
    s2 = pr.split(x, np.zeros_like(x), [[0, 1, 2, 3], [1, 2, 3, 0], [0, 4, 5, 6]], quad2, 1.0)
    assert (s2["n_front_parts"], s2["n_back_parts"], s2["n_straddling_parts"]) == (2, 0, 0)   # both centroids of part 0 lie at x = -0.125 > -0.2
    s3 = pr.split(x, np.zeros_like(x), [[0, 1, 2, 3], [4, 5, 6, 0]], [[1.0, -5, -5], [1.0, 5, -5], [1.0, -5, 5], [1.0, 5, 5]], 1.0)
    assert s3["sign"].tolist() == [0, -1, -1, -1, 1, 1, 1]
    # the displacement counts: with q the first tet is carried across the plane
    q = np.zeros_like(x)
    q[[1, 2, 3], 0] = 5.0
    s4 = pr.split(x, q, t, quad, 0.25)
    assert (s4["n_front_parts"], s4["n_back_parts"]) == (2, 0) and s4["sign"].tolist() == [1] * 7


def test_a_straddling_part_stays():
    v, t = truth_cube(4, 4, 4, 0.1)
    c = 0.5 * (v.min(0) + v.max(0)) + 0.003
    s = pr.split(v, np.zeros_like(v), t, cr.plane_strip(c, (1.0, 0.02, 0.013), half=5.0), 0.05)
    assert (s["n_front_parts"], s["n_back_parts"], s["n_straddling_parts"], s["n_nodes_moved"]) == (0, 0, 1, 0)
    assert np.array_equal(s["x0"], v)


def test_extract_numbers_nodes_by_first_use():
    x = np.arange(30, dtype=np.float64).reshape(10, 3)
    t = np.array([[9, 8, 7, 6], [3, 1, 2, 0], [6, 7, 8, 5], [1, 2, 0, 4]])
    part = pr.parts(x, t)["element_part"]
    assert part.tolist() == [0, 1, 0, 1]
    ids, nodes, xyz, tl = pr.extract(x, t, part, 1)
    assert ids.tolist() == [1, 3] and nodes.tolist() == [3, 1, 2, 0, 4]
    assert tl.tolist() == [[0, 1, 2, 3], [1, 2, 3, 4]] and np.array_equal(xyz, x[[3, 1, 2, 0, 4]])
    ids, nodes, _, tl = pr.extract(x, t, part, 0)
    assert ids.tolist() == [0, 2] and nodes.tolist() == [9, 8, 7, 6, 5] and tl.tolist() == [[0, 1, 2, 3], [3, 2, 1, 4]]
