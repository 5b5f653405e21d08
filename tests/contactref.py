"""Host restatements for the probe's box contact (fb_fem_contact_move / fb_fem_contact_apply): the record formulation of the ring spread
as fembrain_amd/csrc/contact.hip runs it, the press sequence the tests walk a tool box through, and the comparisons of a device
session with ``fembrain_amd.fem.ProbeContact``."""
import numpy as np

from fembrain_amd import lib as fl
from fembrain_amd.fem import ProbeContact, spread_haptic_forces

RECORDS, LEVELS = fl.FB_CONTACT_SPREAD_RECORDS, fl.FB_CONTACT_SPREAD_LEVELS
BALL_MAX = 1024     # kContactBallMax of fembrain_amd/csrc/contact.h: nodes the walk's table holds for one source
BATCH = 32          # kHapticBatch of fembrain_amd/csrc/haptic.h
GRAVITY = -10.0     # (a thousandth of the driver's, and a coefficient to match: the clamped bodies move by far less than half a cell between the
COEFF = 213.4573    # moves, so the tool meets the node layers the sequence expects; no power of two: every product rounds)
INFO_FIELDS = ("status", "n_touched", "n_new", "face", "closest_node", "n_pushing", "list_size", "n_clears", "contact_dist")


def pattern_of(tets, n_nodes):
    """(bptr, bcol) of the stiffness pattern: per node the ascending nodes that share an element with it, itself included"""
    t = np.asarray(tets, np.int64).reshape(-1, 4)
    pairs = np.unique(np.concatenate([np.stack([t[:, a], t[:, b]], axis=1) for a in range(4) for b in range(4)]), axis=0)
    bptr = np.zeros(n_nodes + 1, np.int32)
    np.add.at(bptr, pairs[:, 0] + 1, 1)
    return np.cumsum(bptr).astype(np.int32), pairs[:, 1].astype(np.int32)


def ball(bptr, bcol, root, size):
    """[(node, ring)] of the nodes first reached in ring 1 .. size-1 of the breadth-first walk from root"""
    seen, last, out = {int(root)}, [int(root)], []
    for j in range(1, size):
        new = set()
        for u in last:
            for v in bcol[bptr[u]:bptr[u + 1]]:
                v = int(v)
                if v != u and v not in seen:
                    new.add(v)
        if not new:
            break
        seen |= new
        last = sorted(new)
        out += [(v, j) for v in last]
    return out


def spread_by_levels(bptr, bcol, ids, forces, size, ext):
    """The fallback: per batch of BATCH sources a ring per (source, node), then every node's additions over the batch's sources ascending"""
    n_nodes = len(bptr) - 1
    mag = [1.0] + [1.0 * (size - j) / float(size) for j in range(1, size)]
    for base in range(0, len(ids), BATCH):
        level = np.full((min(BATCH, len(ids) - base), n_nodes), 255, np.uint8)
        for s in range(level.shape[0]):
            for v, j in ball(bptr, bcol, ids[base + s], size):
                level[s, v] = j
        for node in range(n_nodes):
            for s in np.nonzero(level[:, node] != 255)[0]:
                ext[3 * node:3 * node + 3] += mag[level[s, node]] * forces[base + s]
    return ext


def spread_by_records(bptr, bcol, ids, forces, size, ext, ball_max=BALL_MAX, max_records=None):
    """``Deformable::applyHapticForces`` as contact.hip forms it: each force to its own node; then per source with a force the (target,
    source rank, ring) records of its ball, sorted by (target, rank), and every target's additions in that order.  A ball of more
    than ball_max nodes (the source included), or more than max_records records, sends the whole spread to the level arrays.
    Adds into ext; returns dict(path, n_records, n_targets)."""
    ids = [int(i) for i in ids]
    forces = np.asarray(forces, np.float64).reshape(-1, 3)
    pushing = [s for s in range(len(ids)) if (forces[s] != 0.0).any()]
    for s in pushing:
        ext[3 * ids[s]:3 * ids[s] + 3] += forces[s]
    if size <= 1 or not pushing:
        return dict(path=RECORDS, n_records=0, n_targets=0)
    records, overflow = [], False
    for s in pushing:
        b = ball(bptr, bcol, ids[s], size)
        overflow = overflow or len(b) + 1 > ball_max
        records += [(v, s, j) for v, j in b]
    if overflow or (max_records is not None and len(records) > max_records):
        spread_by_levels(bptr, bcol, ids, forces, size, ext)
        return dict(path=LEVELS, n_records=-1 if overflow else len(records), n_targets=-1)
    records.sort()
    for v, s, j in records:
        ext[3 * v:3 * v + 3] += (1.0 * (size - j) / float(size)) * forces[s]
    return dict(path=RECORDS, n_records=len(records), n_targets=len({r[0] for r in records}))


def host_vector(pattern, ids, forces, size, n_dofs, gravity=True):
    """The reference: gravity (or zero) plus ``spread_haptic_forces`` of the list"""
    f = np.zeros(n_dofs)
    if gravity:
        f[1::3] = GRAVITY
    return spread_haptic_forces(pattern[0], pattern[1], [int(i) for i in ids], [tuple(x) for x in np.asarray(forces, np.float64).reshape(-1, 3)], size, f)


def press_sequence(v, step):
    """The tool box's path over a mesh with vertices v and node spacing ``step``: a list of ("move", lo, hi) and ("reset", keep_face).
    miss, touch the top from above, deeper, retreat, reset keeping the face, touch from the +x side (the face stays), reset to a new
    probe, touch from that side again (the face changes)."""
    lo, hi = v.min(0), v.max(0)
    wide_lo, wide_hi = lo - 1.0, hi + 1.0

    def from_top(depth, lift=0.0):
        return ("move", np.array([wide_lo[0], hi[1] - depth + lift, wide_lo[2]]), np.array([wide_hi[0], hi[1] + 0.5 + lift, wide_hi[2]]))

    side = ("move", np.array([hi[0] - 0.5 * step, wide_lo[1], wide_lo[2]]), np.array([hi[0] + 0.5, wide_hi[1], wide_hi[2]]))
    # (the kept face is the far one of the side box, so its forces are large: walk_sequence steps under gravity alone after that move, lest
    # the body leave the box before the last one)
    return [from_top(0.0, lift=0.75), from_top(0.5 * step), from_top(1.5 * step), from_top(0.5 * step), ("reset", True), side + ("gravity only",), ("reset", False), side]


def assert_same_info(dev, host, where=""):
    for k in INFO_FIELDS:
        assert dev[k] == host[k], (where, k, dev[k], host[k])
    assert np.array_equal(dev["closest_point"], host["closest_point"]), (where, dev["closest_point"], host["closest_point"])


def assert_same_list(g, probe, where=""):
    """every array of fb_fem_read_contact against the host session's"""
    ids, first, forces = g.read_contact()
    h_ids, h_first, h_forces = probe.read()
    assert np.array_equal(ids, h_ids), (where, "ids")
    assert np.array_equal(first, h_first), (where, "first-touch positions")
    assert np.array_equal(forces, h_forces), (where, "forces")


def positions(g):
    return np.asarray(g.verts, np.float64).reshape(-1, 3) + g.get_q_state()[0].reshape(-1, 3)


def assert_apply(g, probe, pattern, size, where="", path=None):
    """gravity, then the device spread of the stored list: the vector equals the host walk's.  Returns the device's spread info."""
    g.set_uniform_force(1, GRAVITY)
    info = g.contact_apply(size)
    want = host_vector(pattern, probe.ids, probe.forces, size, g.r)
    assert np.array_equal(g.external_forces(), want), (where, size, info)
    assert info["n_sources"] == len(probe.ids) and info["n_pushing"] == int((probe.forces != 0.0).any(axis=1).sum()), (where, info)
    if path is not None:
        assert info["path"] == path, (where, info)
    return info


def walk_sequence(g, probe, sizes=(1, 2, 5), step=0.1, coeff=COEFF):
    """The press sequence on handle g and host session probe side by side, a real step after every move (so q != 0 and first-touch
    positions differ from current ones).  Returns the infos of the moves."""
    pattern = g.pattern()[:2]
    infos = []
    for k, op in enumerate(press_sequence(np.asarray(g.verts).reshape(-1, 3), step)):
        if op[0] == "reset":
            g.contact_reset(keep_face=op[1])
            probe.reset(keep_face=op[1])
            assert_same_info(g.contact_info(), probe.info(), "reset %d" % k)
            continue
        dev = g.contact_move(op[1], op[2], coeff)
        host = probe.move(positions(g), op[1], op[2], coeff)
        assert_same_info(dev, host, "move %d" % k)
        assert_same_info(g.contact_info(), host, "info after move %d" % k)
        assert_same_list(g, probe, "move %d" % k)
        for size in sizes:
            assert_apply(g, probe, pattern, size, "move %d" % k)
        if len(op) > 3:
            g.set_uniform_force(1, GRAVITY)
        g.do_timestep()
        infos.append(dev)
    return infos
