"""The rule of fb_fem_body_contact_friction / fb_fem_self_contact_friction (include/fembrain_hip.h, "Friction and damping of a contact")
restated in numpy on top of bodycontactref.direction and selfcontactref.self_contact, which already give node, face, closest point,
weights, depth and the degenerate flag of every contact.  Here: the force law in the header's operation order (elementwise float64
numpy does not fuse multiply and add, so the same expression gives the kernels' bits), the scatter in the rule's order, the classes
and the maxima, and the velocity field the tests share."""
import numpy as np

import bodycontactref as B
import selfcontactref as S

SEPARATING, STICKING, SLIDING = 0, 1, 2
LAW_KEYS = ("N", "s", "t", "mf", "n", "sd", "N_raw", "cls")


def law(p, c, bary, d, degenerate, vp, vt, stiffness, depth_cap, mu, slip_speed, damping):
    """The law for k contacts at once.  p, c (k, 3); bary (k, 3); d (k,); vp (k, 3) the points' velocities; vt (k, 3 corners, 3).
    Returns dict(F, N, s, t, mf = -f, n, sd, cls); every row of a degenerate contact is zero and its class is -1."""
    k = len(d)
    z3 = np.zeros((k, 3))
    if k == 0:
        return dict(F=z3, N=np.zeros(0), s=np.zeros(0), t=z3.copy(), mf=z3.copy(), n=z3.copy(), sd=np.zeros(0), N_raw=np.zeros(0), cls=np.zeros(0, np.int64))
    with np.errstate(divide="ignore", invalid="ignore"):
        n = (c - p) / d[:, None]
        depth = np.minimum(d, np.float64(depth_cap)) if depth_cap > 0 else d
        sd = np.float64(stiffness) * depth
        vf = (bary[:, 0:1] * vt[:, 0] + bary[:, 1:2] * vt[:, 1]) + bary[:, 2:3] * vt[:, 2]
        w = vp - vf
        vn = (w[:, 0] * n[:, 0] + w[:, 1] * n[:, 1]) + w[:, 2] * n[:, 2]
        N_raw = sd - np.float64(damping) * vn
        N = np.where(N_raw > 0, N_raw, 0.0)
        t = w - vn[:, None] * n
        s = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])
        den = np.maximum(s, np.float64(slip_speed))
        g = np.where(den > 0, (np.float64(mu) * N) / np.where(den > 0, den, 1.0), 0.0)
        f = g[:, None] * t
        F = N[:, None] * n - f
    cls = np.where(N == 0, SEPARATING, np.where(s < slip_speed, STICKING, SLIDING))
    dg = np.asarray(degenerate, bool)
    out = dict(F=F, N=N, s=s, t=t, mf=-f, n=n, sd=sd, N_raw=N_raw)
    for key, v in out.items():
        out[key] = np.where(dg[:, None] if v.ndim == 2 else dg, 0.0, v)
    out["cls"] = np.where(dg, -1, cls)
    return out


def _info():
    return dict(n_sticking=[0, 0], n_sliding=[0, 0], n_separating=[0, 0], max_slip_speed=0.0, max_normal_force=0.0, max_stick_rate=0.0,
                friction_on_points=np.zeros((2, 3)))


def _account(info, k, L, i, mu, slip_speed):
    """contact i of direction k into the friction info, in record order"""
    name = ("n_separating", "n_sticking", "n_sliding")[int(L["cls"][i])]
    info[name][k] += 1
    info["max_slip_speed"] = max(info["max_slip_speed"], float(L["s"][i]))
    info["max_normal_force"] = max(info["max_normal_force"], float(L["N"][i]))
    if slip_speed > 0:
        info["max_stick_rate"] = max(info["max_stick_rate"], float(np.float64(mu) * L["N"][i] / np.float64(slip_speed)))
    info["friction_on_points"][k] += L["mf"][i]


def body_contact(rest_a, tets_a, cur_a, vel_a, rest_b, tets_b, cur_b, vel_b, stiffness, depth_cap=0.0, directions=B.A_INTO_B | B.B_INTO_A, mu=0.0, slip_speed=0.0,
                 damping=0.0, fa0=None, fb0=None):
    """bodycontactref.body_contact with the friction law in the place of step 5: the same dict, each direction's dict extended by the
    law's arrays (force = F), and ``friction`` the fields of fb_fem_contact_friction_info."""
    cur_a, cur_b = np.asarray(cur_a, np.float64).reshape(-1, 3), np.asarray(cur_b, np.float64).reshape(-1, 3)
    vel_a, vel_b = np.asarray(vel_a, np.float64).reshape(-1, 3), np.asarray(vel_b, np.float64).reshape(-1, 3)
    faces_a, vids_a = B.surface_of(rest_a, tets_a)
    faces_b, vids_b = B.surface_of(rest_b, tets_b)
    fa = np.zeros_like(cur_a) if fa0 is None else np.array(fa0, np.float64).reshape(-1, 3)
    fb = np.zeros_like(cur_b) if fb0 is None else np.array(fb0, np.float64).reshape(-1, 3)
    on_a, on_b, max_depth = np.zeros(3), np.zeros(3), 0.0
    info, dirs = _info(), [None, None]
    for k, bit in enumerate((B.A_INTO_B, B.B_INTO_A)):
        if not directions & bit:
            continue
        (xp, vp, velp, fp, on_p), (xt, tt, velt, ft, fct, on_t) = ((cur_a, vids_a, vel_a, fa, on_a), (cur_b, tets_b, vel_b, fb, faces_b, on_b)) if k == 0 else \
                                                                  ((cur_b, vids_b, vel_b, fb, on_b), (cur_a, tets_a, vel_a, fa, faces_a, on_a))
        r = B.direction(xp, vp, xt, tt, fct, stiffness, depth_cap)
        L = law(xp[r["node"]], r["closest"], r["bary"], r["depth"], r["degenerate"], velp[r["node"]], velt[fct[r["face"]]] if len(r["node"]) else np.zeros((0, 3, 3)),
                stiffness, depth_cap, mu, slip_speed, damping)
        r = dict(r, force=L["F"], **{key: L[key] for key in LAW_KEYS})
        dirs[k] = r
        for i in range(len(r["node"])):  # ascending surface vertex; inside a contact the corners 0, 1, 2
            if r["degenerate"][i]:
                continue
            F = r["force"][i]
            fp[r["node"][i]] += F
            on_p += F
            for corner in range(3):
                contribution = (-F) * r["bary"][i, corner]
                ft[fct[r["face"][i], corner]] += contribution
                on_t += contribution
            dep = float(r["depth"][i])
            max_depth = max(max_depth, min(dep, depth_cap) if depth_cap > 0 else dep)
            _account(info, k, L, i, mu, slip_speed)
    return dict(dirs=tuple(dirs), fa=fa, fb=fb, force_on_a=on_a, force_on_b=on_b, max_depth=max_depth, faces_a=faces_a, faces_b=faces_b, vids_a=vids_a, vids_b=vids_b,
                friction=info)


def self_contact(rest, tets, cur, vel, stiffness, depth_cap=0.0, mode=S.ANY, mu=0.0, slip_speed=0.0, damping=0.0, f0=None):
    """selfcontactref.self_contact with the friction law in the place of step 5: the same dict with f, force, force_on_points,
    force_on_faces formed from F, the law's arrays, and ``friction``."""
    cur, vel = np.asarray(cur, np.float64).reshape(-1, 3), np.asarray(vel, np.float64).reshape(-1, 3)
    r = S.self_contact(rest, tets, cur, stiffness, depth_cap, mode)
    faces = r["faces"]
    L = law(cur[r["node"]], r["closest"], r["bary"], r["depth"], r["degenerate"], vel[r["node"]], vel[faces[r["face"]]] if len(r["node"]) else np.zeros((0, 3, 3)),
            stiffness, depth_cap, mu, slip_speed, damping)
    f = np.zeros_like(cur) if f0 is None else np.array(f0, np.float64).reshape(-1, 3)
    on_p, on_f, info = np.zeros(3), np.zeros(3), _info()
    for i in range(len(r["node"])):  # records 4 i + r in ascending order onto the one vector
        if r["degenerate"][i]:
            continue
        F = L["F"][i]
        f[r["node"][i]] += F
        on_p += F
        for corner in range(3):
            contribution = (-F) * r["bary"][i, corner]
            f[faces[r["face"][i], corner]] += contribution
            on_f += contribution
        _account(info, 0, L, i, mu, slip_speed)
    return dict(r, f=f, force=L["F"], force_on_points=on_p, force_on_faces=on_f, friction=info, **{key: L[key] for key in LAW_KEYS})


# ---- the velocity field the tests share ----

def field_a(x, centre):
    """(0.30, -0.20, 0.10) + cross((0, 2.0, 0.5), x - centre)"""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    return np.array([0.30, -0.20, 0.10])[None, :] + np.cross(np.array([0.0, 2.0, 0.5])[None, :], x - np.asarray(centre, np.float64)[None, :])


def field_b(x, centre):
    """(0.4 (y - cy), -0.1 (x - cx), 0.25 (z - cz) (x - cx))"""
    d = np.asarray(x, np.float64).reshape(-1, 3) - np.asarray(centre, np.float64)[None, :]
    return np.stack([0.4 * d[:, 1], -0.1 * d[:, 0], 0.25 * d[:, 2] * d[:, 0]], axis=1)


def fields(cur_a, cur_b):
    """(vel_a, vel_b) at the current positions, about the bodies' mean positions"""
    cur_a, cur_b = np.asarray(cur_a, np.float64).reshape(-1, 3), np.asarray(cur_b, np.float64).reshape(-1, 3)
    return field_a(cur_a, cur_a.mean(axis=0)), field_b(cur_b, cur_b.mean(axis=0))


def union_fields(cur, n_a):
    """the same two fields on the union mesh of selfcontactref.union (a's nodes first)"""
    cur = np.asarray(cur, np.float64).reshape(-1, 3)
    va, vb = fields(cur[:n_a], cur[n_a:])
    return np.concatenate([va, vb])


def class_margins(r, slip_speed):
    """How far the contacts that are not degenerate are from the two class boundaries: (the least |s - slip_speed| / slip_speed over the
    contacts with N > 0, the least |sd - damping vn| / sd over all of them); inf where there is none."""
    live = r["cls"] >= 0
    pushing = live & (r["N"] > 0)
    slip = float((np.abs(r["s"][pushing] - slip_speed) / slip_speed).min()) if pushing.any() and slip_speed > 0 else np.inf
    normal = float((np.abs(r["N_raw"][live]) / r["sd"][live]).min()) if live.any() else np.inf
    return slip, normal
