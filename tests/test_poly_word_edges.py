"""CPU: the word-edge grid list of tests/poly_inputs.py is checked on the oracle alone, so that the list the device runs
(tests/test_poly_gpu.py::test_pipeline_on_word_edge_grids) cannot quietly stop exercising what it was chosen for."""
import numpy as np

import poly_inputs as pi


def _oracle(case):
    tree, dims, where = case
    blob, lower, cell, xyzf = pi.oracle_case(tree, dims, where)
    o = pi.oracle_on_grid(blob, lower, cell, dims, xyzf)
    return o, o.classify(), xyzf


def test_word_edge_shapes_sit_on_the_word_edges():
    """what the shapes were chosen for, from the shapes alone"""
    shapes = pi.WORD_EDGE_SHAPES
    assert len(shapes) == 26 and len(set(shapes)) == 26 and len(pi.WORD_EDGE_CASES) == 52 + 2 * len(pi.NESTED_SHAPES)
    assert len(pi.NESTED_SHAPES) == 8 and set(pi.NESTED_SHAPES) <= set(shapes) and {(64, 3, 3), (8, 8, 9), (65, 64, 64)} <= set(pi.NESTED_SHAPES)
    points = {s: s[0] * s[1] * s[2] for s in shapes}
    words = {(n + 63) // 64 for n in points.values()}
    assert min(points.values()) < 64                                           # a grid smaller than one word
    assert any(s[0] * s[1] < 64 for s in shapes) and any(s[0] * s[1] == 64 for s in shapes)   # z neighbours in the same word / one word on
    for edge in (16, 62, 256, 4096):                                           # k_tet_vertices, the tet prefetch run, k_ranks, the scan chunk
        assert edge in words and any(edge < w <= edge + edge // 16 + 1 for w in words), edge   # full, and just over
    assert any(n % 64 == 0 and s[0] % 64 for s, n in points.items())          # full words whose rows are not
    assert {s[0] for s in shapes if s[0] % 64 == 0} == {64, 128}               # k_classify<ROWS64> with one and with two words per row
    assert {s for s, _ in pi.SLAB_CASES} <= set(shapes)


def test_word_edge_cases_are_live():
    per_face = np.zeros(6, int)
    unclamped_differs = np.zeros(3, int)
    for case in pi.WORD_EDGE_CASES:
        tree, dims, where = case
        o, oc, xyzf = _oracle(case)
        assert oc["n_crossed_edges"] > 0 and oc["n_included_cells"] > 0, case
        assert (np.abs(xyzf[:, 3] - pi.ISO) > 1e-5).all(), case   # no sample the device's last ulp could classify the other way
        if not pi.sqrt_free(o.blob):
            # where the device's field may differ by an ulp the normals must exist: a flat field (0 / 0) would compare NaN with a number
            assert np.isfinite(o.surface()[1]).all(), case
            continue
        inside = xyzf[:, 3] >= pi.ISO
        g3 = inside.reshape(dims[2], dims[1], dims[0])
        faces = (g3[:, :, 0], g3[:, :, -1], g3[:, 0, :], g3[:, -1, :], g3[0], g3[-1])
        per_face += [bool(f.any() and not f.all()) for f in faces]
        # a classifier without the last-plane masks reads the next row / plane / nothing: the oracle's flags must tell
        unclamped_differs += [bool((u != ((o.edge_flags & bit) != 0)).any()) for u, bit in zip(pi.unclamped_flags(inside, dims), (4, 2, 1))]
    assert (per_face >= 20).all(), per_face
    assert (unclamped_differs >= 40).all(), unclamped_differs
