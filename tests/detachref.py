"""What fb_fem_detach_part hands a piece, written down in numpy: from fb_fem_read_part's arrays (element_ids, node_ids in order of first
use, rest_xyz, tets_local) plus the parent's state vectors, constrained-DOF list and material ids, all in the parent caller's numbering.
The piece's mesh IS read_part's arrays; everything else is a gather through node_ids (vectors), a map of the constrained DOFs into the
local ids (sorted ascending: fb_fem_create wants them so, and the order of first use is not the caller's) or a gather through
element_ids (material bytes).  Pinned by test_detach_host.py on hand-written cases."""
import numpy as np


def fixed_local(node_ids, fixed_dofs):
    """the parent's constrained DOFs (caller ids) that sit on a node of the part, in the part's local ids, ascending (int32)"""
    node_ids = np.asarray(node_ids, np.int64).reshape(-1)
    fixed = np.asarray(fixed_dofs, np.int64).reshape(-1)
    if node_ids.size == 0 or fixed.size == 0:
        return np.zeros(0, np.int32)
    local_of = np.full(int(max(node_ids.max(), fixed.max() // 3)) + 1, -1, np.int64)
    local_of[node_ids] = np.arange(len(node_ids))
    loc = local_of[fixed // 3]
    keep = loc >= 0
    return np.sort(3 * loc[keep] + fixed[keep] % 3).astype(np.int32)


def gather_vector(node_ids, vec):
    """a per-DOF vector of the parent (3 n_nodes, caller order) on the part's nodes: (3 n_part_nodes,)"""
    node_ids = np.asarray(node_ids, np.int64).reshape(-1)
    return np.ascontiguousarray(np.asarray(vec, np.float64).reshape(-1, 3)[node_ids]).reshape(-1)


def detach(element_ids, node_ids, rest_xyz, tets_local, fixed_dofs=(), vectors=None, material_ids=None):
    """the piece: dict of xyz (n, 3), tets (m, 4) int32, fixed (ascending local DOFs, int32), one entry per name of `vectors`
    (a dict of parent vectors, each gathered) and materials (uint8 per element of the piece, None without a parent map)"""
    out = dict(xyz=np.asarray(rest_xyz, np.float64).reshape(-1, 3), tets=np.asarray(tets_local, np.int32).reshape(-1, 4),
               fixed=fixed_local(node_ids, fixed_dofs))
    for name, vec in (vectors or {}).items():
        out[name] = gather_vector(node_ids, vec)
    out["materials"] = None if material_ids is None else np.asarray(material_ids, np.uint8).reshape(-1)[np.asarray(element_ids, np.int64)]
    return out
