"""tests/detachref.py pinned on hand-made cases with literal answers: the checker of test_detach_gpu.py is itself checked where no GPU is."""
import numpy as np

import detachref as dr
import partsref as pr

X7 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [2, 0.3, 1], [0.2, 2, 1.1]], np.float64)


def _pieces(x, t, **kw):
    p = pr.parts(x, t)
    return [dr.detach(*pr.extract(x, t, p["element_part"], k), **kw) for k in range(p["n_parts"])], p


def test_a_fixed_dof_on_a_shared_node_lands_in_both_pieces():
    # two tets with node 3 in common, which the second names first; its y is clamped, and so are node 1 (first piece) and node 6 z (second)
    t = [[0, 1, 2, 3], [3, 4, 5, 6]]
    q = np.arange(21, dtype=np.float64) * 0.5
    pieces, p = _pieces(X7, t, fixed_dofs=[3, 4, 5, 10, 20], vectors=dict(q=q))
    assert p["n_parts"] == 2 and p["n_shared_nodes"] == 1
    a, b = pieces
    assert a["tets"].tolist() == [[0, 1, 2, 3]] and b["tets"].tolist() == [[0, 1, 2, 3]]
    assert a["fixed"].tolist() == [3, 4, 5, 10] and a["fixed"].dtype == np.int32   # node 1 -> local 1, node 3 -> local 3
    assert b["fixed"].tolist() == [1, 11]                                          # node 3 -> local 0, node 6 -> local 3
    assert np.array_equal(a["xyz"], X7[[0, 1, 2, 3]]) and np.array_equal(b["xyz"], X7[[3, 4, 5, 6]])
    assert a["q"].tolist() == q[:12].tolist() and b["q"].tolist() == q[9:21].tolist()   # each piece has its own copy of node 3
    assert a["materials"] is None and b["materials"] is None


def test_an_orphan_node_lands_in_no_piece():
    # node 2 belongs to no element; its clamped DOFs go nowhere, and the nodes behind it keep their own values
    x = np.vstack([X7[:5], [[9, 9, 9]]])[[0, 1, 5, 2, 3, 4]]
    t = [[0, 1, 3, 4], [1, 3, 4, 5]]
    f = np.arange(18, dtype=np.float64)
    pieces, p = _pieces(x, t, fixed_dofs=[0, 6, 7, 8, 17], vectors=dict(fext=f), material_ids=[2, 1])
    assert p["n_parts"] == 1 and p["n_unused_nodes"] == 1
    (a,) = pieces
    assert len(a["xyz"]) == 5 and a["tets"].tolist() == [[0, 1, 2, 3], [1, 2, 3, 4]]
    assert a["fixed"].tolist() == [0, 14]                                          # node 0 x; node 5 z -> local 4
    assert a["fext"].tolist() == f.reshape(-1, 3)[[0, 1, 3, 4, 5]].reshape(-1).tolist()
    assert a["materials"].tolist() == [2, 1] and a["materials"].dtype == np.uint8


def test_the_fixed_list_comes_out_ascending_after_the_map():
    # the element names its nodes high to low: the order of first use reverses the caller's, and so would the mapped list without the sort
    x = X7[[3, 2, 1, 0]]
    t = [[3, 2, 1, 0]]
    pieces, _ = _pieces(x, t, fixed_dofs=[0, 1, 5, 9, 11])
    (a,) = pieces
    assert a["tets"].tolist() == [[0, 1, 2, 3]] and np.array_equal(a["xyz"], x[[3, 2, 1, 0]])
    # node 0 -> local 3, node 1 -> local 2, node 3 -> local 0
    assert a["fixed"].tolist() == [0, 2, 8, 9, 10]
    assert np.all(np.diff(a["fixed"]) > 0)
    assert dr.fixed_local([3, 2, 1, 0], []).tolist() == [] and dr.fixed_local([], [1]).tolist() == []
