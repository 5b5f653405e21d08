"""Taking the tissue under a tool away, through the host: which elements of a tet mesh lie under a set of spheres, capsules and oriented
boxes (an aspirator, a cautery tip), optionally only of one material or at or above a von Mises limit (a tear), which nodes their removal
frees, their rest volume and mass -- and ``erode_host``, which takes them out of a ``FemIntegrator`` with state and forces carried.

This is the HOST route, written once: read_mesh + get_q_state, the selection below in numpy, fb_fem_resync_delta(removed = ...), then
set_q_state and set_external_forces again, because a re-sync zeroes the vectors.  The library has no device call for the selection yet;
the second half of one -- an ascending device list of elements taken out of a handle with state and forces carried -- is
remove_elements_device() in csrc/fem_build.hip.  The rule is fixed to the bit so that such a call can be compared with this module.

The rule, in IEEE fp64 with every sum written out in this order (no np.dot / einsum, which may fuse or reorder) and no square root:
  - a corner is at x0 (frame "rest") or x0 + q (frame "world"), one addition per component; the centroid of an element is
    ((p0 + p1) + (p2 + p3)) * 0.25 per component, the corners in the element's stored order (read_mesh's);
  - dot(u, v) = (ux*vx + uy*vy) + uz*vz, dist2(u) = dot(u, u);
  - sphere: inside iff dist2(p - a) <= radius*radius;
  - capsule: d = b - a, dd = dist2(d), t = dd > 0 ? min(max(dot(p - a, d) / dd, 0), 1) : 0, c = a + t*d (a multiply, then an add),
    inside iff dist2(p - c) <= radius*radius; with a == b it is the sphere;
  - box: u = p - a, l_i = dot(row i of R, u), inside iff |l_i| <= half_i for i = 0, 1, 2;
  - a point is inside the tool iff it is inside any shape; rule "centroid": the centroid is; "all_nodes": all four corners are (not
    necessarily in the same shape); "any_node": at least one corner is; without shapes every element passes and a filter must be active;
  - filters, ANDed: the element's material id equals `material`; von_mises[e] >= min_von_mises (a NaN never passes);
  - freed nodes: those the selected elements use and no surviving element uses.
A shape is a tuple:
  ("sphere", centre, radius)   ("capsule", a, b, radius)   ("box", centre, half, R)      R (3, 3): row i is axis i, None: identity
"""
import numpy as np

RULES = ("centroid", "all_nodes", "any_node")


def _dot(ux, uy, uz, vx, vy, vz):
    return (ux * vx + uy * vy) + uz * vz


def inside_shape(shape, P):
    """(n,) bool: the points P (n, 3) inside one shape"""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    px, py, pz = P[:, 0], P[:, 1], P[:, 2]
    kind = shape[0]
    a = np.asarray(shape[1], np.float64)
    ux, uy, uz = px - a[0], py - a[1], pz - a[2]
    if kind == "box":
        half = np.asarray(shape[2], np.float64)
        R = np.eye(3) if len(shape) < 4 or shape[3] is None else np.asarray(shape[3], np.float64).reshape(3, 3)
        ok = np.ones(len(P), bool)
        for i in range(3):
            ok &= np.abs(_dot(R[i, 0], R[i, 1], R[i, 2], ux, uy, uz)) <= half[i]
        return ok
    if kind == "sphere":
        r = np.float64(shape[2])
        return _dot(ux, uy, uz, ux, uy, uz) <= r * r
    if kind == "capsule":
        b, r = np.asarray(shape[2], np.float64), np.float64(shape[3])
        d = b - a
        dd = _dot(d[0], d[1], d[2], d[0], d[1], d[2])
        if dd > 0:
            t = np.minimum(np.maximum(_dot(ux, uy, uz, d[0], d[1], d[2]) / dd, 0.0), 1.0)
        else:
            t = np.zeros(len(P))
        cx, cy, cz = a[0] + t * d[0], a[1] + t * d[1], a[2] + t * d[2]
        wx, wy, wz = px - cx, py - cy, pz - cz
        return _dot(wx, wy, wz, wx, wy, wz) <= r * r
    raise ValueError("unknown shape %r" % (kind,))


def inside_tool(shapes, P):
    """inside any of the shapes"""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    ok = np.zeros(len(P), bool)
    for s in shapes:
        ok |= inside_shape(s, P)
    return ok


def positions(x0, q, frame):
    x0 = np.asarray(x0, np.float64).reshape(-1, 3)
    if frame == "rest":
        return x0
    assert frame == "world"
    return x0 + np.asarray(q, np.float64).reshape(-1, 3)


def select(x0, tets, q, shapes, rule="centroid", frame="world", material_ids=None, material=None, von_mises=None, min_von_mises=0.0):
    """The ascending ids (int32) of the elements the call selects.  x0 (n, 3), tets (m, 4) and q (3 n) in the caller's numbering
    (read_mesh, get_q_state); material_ids (m,) or None (id 0 everywhere); von_mises (m,) where min_von_mises > 0."""
    tets = np.asarray(tets, np.int64).reshape(-1, 4)
    m = len(tets)
    shapes = list(shapes or ())
    if not shapes and material is None and not min_von_mises > 0:
        raise ValueError("no shape and no filter")
    ok = np.ones(m, bool)
    if shapes:
        X = positions(x0, q, frame)
        c = [X[tets[:, k]] for k in range(4)]
        if rule == "centroid":
            ok = inside_tool(shapes, ((c[0] + c[1]) + (c[2] + c[3])) * 0.25)
        else:
            ins = [inside_tool(shapes, c[k]) for k in range(4)]
            if rule == "all_nodes":
                ok = ins[0] & ins[1] & ins[2] & ins[3]
            elif rule == "any_node":
                ok = ins[0] | ins[1] | ins[2] | ins[3]
            else:
                raise ValueError("unknown rule %r" % (rule,))
    if material is not None:
        ids = np.zeros(m, np.int64) if material_ids is None else np.asarray(material_ids, np.int64)
        ok = ok & (ids == int(material))
    if min_von_mises > 0:
        with np.errstate(invalid="ignore"):
            ok = ok & (np.asarray(von_mises, np.float64) >= min_von_mises)   # (a NaN never passes)
    return np.nonzero(ok)[0].astype(np.int32)


def freed_nodes(tets, selected):
    """The nodes the selected elements use and no surviving element uses, ascending (int32)"""
    tets = np.asarray(tets, np.int64).reshape(-1, 4)
    gone = np.zeros(len(tets), bool)
    gone[np.asarray(selected, np.int64)] = True
    return np.setdiff1d(np.unique(tets[gone]), np.unique(tets[~gone])).astype(np.int32)


def rest_volumes(x0, tets):
    """(m,) the rest volume of every element: |det(x1 - x0, x2 - x0, x3 - x0)| / 6"""
    x0 = np.asarray(x0, np.float64).reshape(-1, 3)
    tets = np.asarray(tets, np.int64).reshape(-1, 4)
    u, v, w = x0[tets[:, 1]] - x0[tets[:, 0]], x0[tets[:, 2]] - x0[tets[:, 0]], x0[tets[:, 3]] - x0[tets[:, 0]]
    det = (u[:, 0] * (v[:, 1] * w[:, 2] - v[:, 2] * w[:, 1]) + u[:, 1] * (v[:, 2] * w[:, 0] - v[:, 0] * w[:, 2])
           + u[:, 2] * (v[:, 0] * w[:, 1] - v[:, 1] * w[:, 0]))
    return np.abs(det) / 6.0


def volume_and_mass(x0, tets, selected, rho=1000.0, material_ids=None):
    """(volume, mass) of the selected elements: rho a number, or the table indexed by material_ids"""
    V = rest_volumes(x0, tets)[np.asarray(selected, np.int64)]
    if material_ids is None:
        r = np.full(len(V), float(np.asarray(rho, np.float64).reshape(-1)[0]))
    else:
        r = np.asarray(rho, np.float64)[np.asarray(material_ids, np.int64)[np.asarray(selected, np.int64)]]
    return float(V.sum()), float((r * V).sum())


def check_shapes(shapes):
    """ValueError for an unknown kind, a negative or non-finite radius or half extent, any other non-finite number"""
    for s in shapes:
        kind = s[0]
        if kind not in ("sphere", "capsule", "box"):
            raise ValueError("unknown shape %r" % (kind,))
        points = [np.asarray(s[1], np.float64).reshape(-1)]      # xyz triples
        R = None
        if kind == "sphere":
            size = np.asarray([s[2]], np.float64)
        elif kind == "capsule":
            points.append(np.asarray(s[2], np.float64).reshape(-1))
            size = np.asarray([s[3]], np.float64)
        else:
            size = np.asarray(s[2], np.float64).reshape(-1)
            points.append(size)
            if len(s) > 3 and s[3] is not None:
                R = np.asarray(s[3], np.float64).reshape(-1)
        if any(len(a) != 3 for a in points) or (R is not None and len(R) != 9):
            raise ValueError("%s: points and half extents are xyz triples, R is 3 x 3" % kind)
        nums = points + ([R] if R is not None else [])
        if not all(np.isfinite(a).all() for a in nums) or not np.isfinite(size).all() or (size < 0).any():
            raise ValueError("%s: a non-finite number, or a negative radius or half extent" % kind)


def erode_host(g, shapes, rule="centroid", frame="world", material=None, min_von_mises=0.0, max_elements=0, dry_run=False, track=True):
    """The elements under the tool taken out of the unsharded ``FemIntegrator`` ``g`` through the host route (module docstring).  Returns
    a dict: status, n_selected, n_removed, n_elements_left, n_nodes_freed, resync_path, volume and mass (rest volume and rho * rest volume
    of the SELECTED elements), element_ids (ascending, the numbering before the call) and freed_nodes (caller ids, ascending).
    status "none" (nothing selected), "all" (every element selected: refused, a handle cannot be left without elements), "over_cap"
    (n_selected > max_elements > 0: refused as a whole, never partial) and "dry" (dry_run) change nothing -- no re-sync, the same mesh
    generation.  "done": as ``g.resync_delta(dict(removed=element_ids))`` with q, qvel, qaccel and the external forces set again; the
    survivors keep their order, the node count does not change, the freed nodes stay as identity rows with the q they had; materials,
    embeddings and the motion set follow as they follow any delta re-sync.  ``min_von_mises`` > 0 runs ``g.stress()`` first (with the
    default flags) and reads its von Mises array.  ValueError before anything is read: an unknown rule, frame or shape kind, a bad
    number in a shape, material outside 0 .. 255, min_von_mises < 0 or not finite, max_elements < 0, no shape and no filter."""
    shapes = list(shapes or ())
    check_shapes(shapes)
    if rule not in RULES:
        raise ValueError("rule is 'centroid', 'all_nodes' or 'any_node', not %r" % (rule,))
    if frame not in ("world", "rest"):
        raise ValueError("frame is 'world' or 'rest', not %r" % (frame,))
    if material is not None and not 0 <= int(material) <= 255:
        raise ValueError("material ids are 0 .. 255")
    if not (min_von_mises >= 0 and np.isfinite(min_von_mises)):
        raise ValueError("min_von_mises is 0 or a positive number")
    if max_elements < 0:
        raise ValueError("max_elements < 0")
    if not shapes and material is None and not min_von_mises > 0:
        raise ValueError("no shape and no filter")
    x, t = g.read_mesh()
    state = g.get_q_state()
    mats = g.element_materials()
    vm = None
    if min_von_mises > 0:
        g.stress()
        vm = g.element_stress(tensors=False)["von_mises"]
    ids = select(x, t, state[0], shapes, rule=rule, frame=frame, material_ids=mats, material=material, von_mises=vm, min_von_mises=min_von_mises)
    freed = freed_nodes(t, ids)
    volume, mass = volume_and_mass(x, t, ids, rho=g.materials()[2], material_ids=mats)
    if len(ids) == 0:
        status = "none"
    elif len(ids) == len(t):
        status = "all"
    elif max_elements > 0 and len(ids) > max_elements:
        status = "over_cap"
    elif dry_run:
        status = "dry"
    else:
        status = "done"
        fext = g.external_forces()
        g.resync_delta(dict(removed=ids), fixed_dofs=g.constrained_dofs(), track=track)
        g.set_q_state(*state)
        g.set_external_forces(fext)
        g.n_tets_global = len(t) - len(ids)
    return dict(status=status, n_selected=len(ids), n_removed=len(ids) if status == "done" else 0, n_elements_left=int(g.num_tets()),
                n_nodes_freed=len(freed), resync_path=g.resync_path(), volume=volume, mass=mass, element_ids=ids, freed_nodes=freed)
