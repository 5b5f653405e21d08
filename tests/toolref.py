"""fb_fem_tool_contact's rule (include/fembrain_hip.h, "Contact with a rigid tool") in plain Python floats: one scalar loop per point,
every fp64 operation in the header's order, no np.dot / einsum (which may fuse or reorder).  Shapes are erosion.py's tuples:
("sphere", centre, radius)   ("capsule", a, b, radius)   ("box", centre, half, R)   R (3, 3): row i is axis i, None: identity."""
import math

import numpy as np

from fembrain_amd import erosion

SEPARATING, STICKING, SLIDING = 0, 1, 2
MAX_SHAPES = 16


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _f(v):
    return [float(x) for x in np.asarray(v, np.float64).reshape(-1)]


def _sphere(p, c, r):
    """None, or (depth, n, degenerate) of the sphere (c, r) at p"""
    u = [p[0] - c[0], p[1] - c[1], p[2] - c[2]]
    l2 = _dot(u, u)
    if not l2 <= r * r:
        return None
    l = math.sqrt(l2)
    if l == 0.0:
        return r, [0.0, 0.0, 0.0], True
    return r - l, [u[0] / l, u[1] / l, u[2] / l], False


def shape_at(shape, p):
    """None where the shape does not hold p, else (depth, outward normal, degenerate)"""
    kind, a = shape[0], _f(shape[1])
    if kind == "sphere":
        return _sphere(p, a, float(shape[2]))
    if kind == "capsule":
        b, r = _f(shape[2]), float(shape[3])
        d = [b[0] - a[0], b[1] - a[1], b[2] - a[2]]
        dd = _dot(d, d)
        u = [p[0] - a[0], p[1] - a[1], p[2] - a[2]]
        t = min(max(_dot(u, d) / dd, 0.0), 1.0) if dd > 0 else 0.0
        return _sphere(p, [a[0] + t * d[0], a[1] + t * d[1], a[2] + t * d[2]], r)
    if kind == "box":
        half = _f(shape[2])
        R = _f(np.eye(3) if len(shape) < 4 or shape[3] is None else shape[3])
        u = [p[0] - a[0], p[1] - a[1], p[2] - a[2]]
        l = [_dot(R[3 * i:3 * i + 3], u) for i in range(3)]
        if not all(abs(l[i]) <= half[i] for i in range(3)):
            return None
        axis, e = 0, half[0] - abs(l[0])
        for i in (1, 2):
            ei = half[i] - abs(l[i])
            if ei < e:
                axis, e = i, ei
        row = R[3 * axis:3 * axis + 3]
        return e, [-x for x in row] if l[axis] < 0 else list(row), False
    raise ValueError("unknown shape %r" % (kind,))


def check(shapes, stiffness, depth_cap, points, origin, velocity, omega, mu, slip_speed, damping):
    """ValueError for what the call refuses before it launches anything"""
    shapes = list(shapes)
    erosion.check_shapes(shapes)
    if not 1 <= len(shapes) <= MAX_SHAPES:
        raise ValueError("%d shapes" % len(shapes))
    for s in shapes:
        if s[0] == "box" and len(s) > 3 and s[3] is not None:
            R = _f(s[3])
            for i in range(3):
                for j in range(3):
                    if not abs(_dot(R[3 * i:3 * i + 3], R[3 * j:3 * j + 3]) - (1.0 if i == j else 0.0)) <= 1e-9:
                        raise ValueError("the rows of R are not orthonormal")
    if points not in ("surface", "all_nodes"):
        raise ValueError("points %r" % (points,))
    for name, v in (("stiffness", stiffness), ("depth_cap", depth_cap), ("mu", mu), ("slip_speed", slip_speed), ("damping", damping)):
        if not (math.isfinite(v) and v >= 0):
            raise ValueError("%s %r" % (name, v))
    if mu > 0 and slip_speed == 0:
        raise ValueError("friction needs a slip speed above zero")
    if not np.isfinite(np.asarray([origin, velocity, omega], np.float64)).all():
        raise ValueError("origin, velocity or omega is not finite")


def tool_contact(x0, q, point_ids, shapes, stiffness, depth_cap=0.0, origin=(0, 0, 0), velocity=(0, 0, 0), omega=(0, 0, 0), qvel=None, friction=None, f0=None,
                 points="surface"):
    """The call on the points ``point_ids`` (ascending caller ids: surface.vertex_ids, or every node) at x0 + q.  friction: None, or
    (mu, slip_speed, damping) with qvel the nodes' velocities.  f0: the force vector before the call (default zero).  Returns the
    records (node, shape, depth, normal, force, normal_force, slip, friction, cls, degenerate), the vector f after the call and the
    info fields.  ValueError as the call: a refusal of ``check``, a position -- with friction a velocity -- of a point that is not finite."""
    mu, slip_speed, damping = friction if friction is not None else (0.0, 0.0, 0.0)
    check(shapes, stiffness, depth_cap, points, origin, velocity, omega, mu, slip_speed, damping)
    shapes = list(shapes)
    x0 = np.asarray(x0, np.float64).reshape(-1, 3)
    q = np.asarray(q, np.float64).reshape(-1, 3)
    qv = None if qvel is None else np.asarray(qvel, np.float64).reshape(-1, 3)
    ids = [int(i) for i in point_ids]
    if not np.isfinite(x0[ids] + q[ids]).all():
        raise ValueError("a position of a point is not finite")
    if friction is not None and not np.isfinite(qv[ids]).all():
        raise ValueError("a velocity of a point is not finite")
    O, V, W = _f(origin), _f(velocity), _f(omega)
    stiffness, depth_cap = float(stiffness), float(depth_cap)
    f = np.zeros_like(x0) if f0 is None else np.array(f0, np.float64).reshape(-1, 3)
    rec = dict(node=[], shape=[], depth=[], normal=[], force=[], normal_force=[], slip=[], friction=[], cls=[], degenerate=[])
    by_shape = [0] * len(shapes)
    on_body, on_tool, torque = [0.0] * 3, [0.0] * 3, [0.0] * 3
    n_deg, n_class = 0, [0, 0, 0]
    max_depth = max_slip = max_N = max_rate = 0.0
    for i in ids:
        p = [float(x0[i, k]) + float(q[i, k]) for k in range(3)]
        best = None
        for s, shape in enumerate(shapes):
            got = shape_at(shape, p)
            if got is not None and (best is None or got[0] > best[1][0]):
                best = (s, got)
        if best is None:
            continue
        s, (depth, n, degenerate) = best
        by_shape[s] += 1
        F, N, t, mf, cls = [0.0] * 3, 0.0, [0.0] * 3, [0.0] * 3, -1
        if degenerate:
            n_deg += 1
        else:
            capped = min(depth, depth_cap) if depth_cap > 0 else depth
            sd = stiffness * capped
            r = [p[0] - O[0], p[1] - O[1], p[2] - O[2]]
            if friction is None:
                F = [sd * n[k] for k in range(3)]
            else:
                vt = [V[0] + (W[1] * r[2] - W[2] * r[1]), V[1] + (W[2] * r[0] - W[0] * r[2]), V[2] + (W[0] * r[1] - W[1] * r[0])]
                w = [float(qv[i, k]) - vt[k] for k in range(3)]
                vn = _dot(w, n)
                N = sd - damping * vn
                if not N > 0.0:
                    N = 0.0
                t = [w[k] - vn * n[k] for k in range(3)]
                sl = math.sqrt(_dot(t, t))
                den = max(sl, slip_speed)
                g = (mu * N) / den if den > 0 else 0.0
                fk = [g * t[k] for k in range(3)]
                F = [N * n[k] - fk[k] for k in range(3)]
                mf = [-x for x in fk]
                cls = SEPARATING if N == 0.0 else STICKING if sl < slip_speed else SLIDING
                n_class[cls] += 1
                max_slip, max_N = max(max_slip, sl), max(max_N, N)
                if slip_speed > 0:
                    max_rate = max(max_rate, mu * N / slip_speed)
            max_depth = max(max_depth, capped)
            m = [-F[0], -F[1], -F[2]]
            for k in range(3):
                f[i, k] += F[k]
                on_body[k] += F[k]
                on_tool[k] += m[k]
            torque[0] += r[1] * m[2] - r[2] * m[1]
            torque[1] += r[2] * m[0] - r[0] * m[2]
            torque[2] += r[0] * m[1] - r[1] * m[0]
        for key, v in (("node", i), ("shape", s), ("depth", depth), ("normal", n), ("force", F), ("normal_force", N), ("slip", t), ("friction", mf), ("cls", cls),
                       ("degenerate", degenerate)):
            rec[key].append(v)
    out = dict(node=np.array(rec["node"], np.int32), shape=np.array(rec["shape"], np.int32), depth=np.array(rec["depth"], np.float64),
               normal=np.array(rec["normal"], np.float64).reshape(-1, 3), force=np.array(rec["force"], np.float64).reshape(-1, 3),
               normal_force=np.array(rec["normal_force"], np.float64), slip=np.array(rec["slip"], np.float64).reshape(-1, 3),
               friction=np.array(rec["friction"], np.float64).reshape(-1, 3), cls=np.array(rec["cls"], np.int32), degenerate=np.array(rec["degenerate"], bool))
    out.update(f=f, n_points=len(ids), n_contacts=len(rec["node"]), n_degenerate=n_deg, contacts_by_shape=np.array(by_shape), n_separating=n_class[SEPARATING],
               n_sticking=n_class[STICKING], n_sliding=n_class[SLIDING], max_depth=max_depth, max_slip_speed=max_slip, max_normal_force=max_N, max_stick_rate=max_rate,
               force_on_body=np.array(on_body), force_on_tool=np.array(on_tool), torque_on_tool=np.array(torque))
    return out
