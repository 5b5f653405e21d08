"""The tools of test_tool_contact_ref.py and test_tool_contact_gpu.py on truth_cube(9, 9, 9): 729 nodes, 3,072 tets, 386 surface vertices
(two workgroups of 256 points, the second ragged).  Per case the shapes, and what tests/toolref.py gives at rest: contacts, contacts by
shape, degenerate contacts."""
import numpy as np

import surfref
from fembrain_amd.meshgen import truth_cube

N = 9
K = 1000.0


def rot():
    """R = Rz(0.3) @ Rx(0.2): its rows are the box's axes"""
    cz, sz, cx, sx = np.cos(0.3), np.sin(0.3), np.cos(0.2), np.sin(0.2)
    return np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])


def lattice(i, j, k):
    return (i * N + j) * N + k


_MESH = {}


def mesh():
    """(x, tets, surface vertex ids ascending) of the cube, computed once"""
    if not _MESH:
        x, t = truth_cube(N, N, N)
        faces, _ = surfref.vectorised(x, t)
        _MESH["m"] = (x, t, np.asarray(surfref.vertex_ids(faces), np.int32))
    return _MESH["m"]


def cases():
    x = mesh()[0]
    centre = x[lattice(4, 8, 4)]
    sphere = ("sphere", (-0.037, 0.85, -0.054), 0.25)
    capsule = ("capsule", (-0.3, 0.85, -0.2), (0.2, 0.9, 0.1), 0.18)
    box = ("box", (0.004, 0.83, -0.007), (0.22, 0.09, 0.15), rot())
    half = np.abs(x[lattice(5, 8, 5)] - centre) + np.array([0.0, 0.03, 0.0])
    # name: (shapes, contacts, contacts by shape, degenerate contacts)
    return {
        "sphere": ([sphere], 21, [21], 0),
        "capsule": ([capsule], 26, [26], 0),
        "box": ([box], 15, [15], 0),
        "all_three": ([sphere, capsule, box], 32, [14, 17, 1], 0),
        "twins": ([sphere, sphere], 21, [21, 0], 0),
        "on_a_node": ([("sphere", tuple(centre), 0.12)], 5, [5], 1),
        "flush_box": ([("box", tuple(centre), tuple(half), None)], 9, [9], 0),
        "corner": ([("sphere", (0.37, 0.82, 0.37), 0.2)], 7, [7], 0),
        "miss": ([("sphere", (0.0, 2.0, 0.0), 0.3)], 0, [0], 0),
    }
