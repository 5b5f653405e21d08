"""fb_fem_body_contact_friction / fb_fem_self_contact_friction on the device against tests/frictionref.py, the law in numpy.

The comparison rules are test_body_contact_gpu.py's and test_self_contact_gpu.py's (their ``_compare`` runs here on the friction calls'
output): contact sets and integers of the points whose decision lies outside rounding exactly, and wherever nothing is left out the
doubles BIT FOR BIT -- the two force vectors, the sums, and here also N, t, -f per contact and the maxima -- with equal class counts.
test_friction_ref.py shows that no contact of the shared shapes is within 1 % of slip_speed or 60 % of sd of a class boundary, so no
class is a matter of rounding.  The calls go through the C entry points directly, so that mu = damping = 0 also reaches the new ones
(``FemIntegrator.body_contact`` sends all zeros to the frictionless call)."""
import ctypes as C

import numpy as np
import pytest

import bodycontactref as B
import frictionref as F
import selfcontactref as S
import test_body_contact_gpu as TB
import test_self_contact_gpu as TS
from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator

pytestmark = pytest.mark.gpu

K, MU, SLIP = 1000.0, 0.5, 0.15
KW = TB.KW
CLASSES = {"two_way": ((1, 15), (1, 8)), "many_onto_one": ((28, 364), (1, 3)), "deep": ((8, 18), (0, 0))}   # sticking / sliding per direction, damping 0
INFO_KEYS = ("n_sticking", "n_sliding", "n_separating", "max_slip_speed", "max_normal_force", "max_stick_rate", "friction_on_points")


def _state(g):
    """(rest, tets, current positions, velocities) as the handle holds them, caller ids"""
    x, t = g.read_mesh()
    q, qvel = g.get_q_state()[:2]
    return x, t, x + q.reshape(-1, 3), qvel.reshape(-1, 3)


def _move_pair(ga, gb):
    """the shared velocity field at the current positions of both bodies"""
    (_, _, ca, _), (_, _, cb, _) = _state(ga), _state(gb)
    va, vb = F.fields(ca, cb)
    ga.set_q_state(ga.get_q_state()[0], va.reshape(-1))
    gb.set_q_state(gb.get_q_state()[0], vb.reshape(-1))


def _friction(mu, slip, damping, reserved=0.0):
    fr = fl.ContactFrictionParams()
    fr.mu, fr.slip_speed, fr.damping, fr.reserved = mu, slip, damping, reserved
    return fr


def _read_body(ga, counts):
    """both directions of the last call through the two read calls (the wrappers size their arrays by the counts they were told)"""
    ga._body_contacts = ga._body_friction_contacts = tuple(counts)
    bits = (fl.FB_BODY_A_INTO_B, fl.FB_BODY_B_INTO_A)
    return tuple(ga.read_body_contact(b) for b in bits), tuple(ga.read_body_contact_friction(b) for b in bits)


def _call(ga, gb, mu=MU, slip=SLIP, damping=0.0, depth_cap=0.0, directions="both", fa0=None, fb0=None, stiffness=K):
    """sets the two force vectors (zero where none is given), calls fb_fem_body_contact_friction, returns everything that comes back"""
    for g, f in ((ga, fa0), (gb, fb0)):
        g.set_external_forces_to_zero() if f is None else g.set_external_forces(f)
    p, fr, info, fi = ga._body_params(stiffness, depth_cap, directions), _friction(mu, slip, damping), fl.BodyContactInfo(), fl.ContactFrictionInfo()
    fl.check(ga._L.fb_fem_body_contact_friction(ga.h, gb.h, C.byref(p), C.byref(fr), C.byref(info), C.byref(fi)))
    out = dict(n_candidates=tuple(info.n_candidates), n_contacts=tuple(info.n_contacts), n_degenerate=tuple(info.n_degenerate), path=int(info.path),
               n_tet_grid_builds=int(info.n_tet_grid_builds), n_face_grid_builds=int(info.n_face_grid_builds), faces_tested=int(info.faces_tested),
               max_depth=float(info.max_depth), force_on_a=np.array(info.force_on_a[:]), force_on_b=np.array(info.force_on_b[:]))
    dirs, fric = _read_body(ga, out["n_contacts"])
    return dict(info=out, friction=ga._friction_info(fi), dirs=dirs, fric=fric, fa=ga.external_forces().reshape(-1, 3), fb=gb.external_forces().reshape(-1, 3))


def _reference(ga, gb, mu=MU, slip=SLIP, damping=0.0, depth_cap=0.0, directions=3, fa0=None, fb0=None):
    (xa, ta, ca, va), (xb, tb, cb, vb) = _state(ga), _state(gb)
    ref = F.body_contact(xa, ta, ca, va, xb, tb, cb, vb, K, depth_cap, directions, mu, slip, damping, fa0, fb0)
    ref["extent"] = (float((cb.max(axis=0) - cb.min(axis=0)).max()), float((ca.max(axis=0) - ca.min(axis=0)).max()))
    return ref


def _law_rows(dev, fric, r, contact_ok, label):
    """N, t, -f of the contacts whose decision lies outside rounding, bit for bit"""
    where = {int(n): i for i, n in enumerate(dev["node"])}
    keep = np.nonzero(contact_ok)[0]
    rows = np.array([where[int(r["node"][i])] for i in keep], np.int64)
    for dkey, rkey in (("normal_force", "N"), ("slip", "t"), ("friction", "mf")):
        assert np.array_equal(fric[dkey][rows], r[rkey][keep]), (label, dkey, np.abs(fric[dkey][rows] - r[rkey][keep]).max())


def _compare(out, ref, max_left_out=0.0, label=""):
    left = TB._compare(out, ref, max_left_out, label)   # sets, integers, geometry, and where nothing is left out the vectors and sums
    nothing_left = True
    for k, (dev, fric, r) in enumerate(zip(out["dirs"], out["fric"], ref["dirs"])):
        if r is None:
            assert len(fric["normal_force"]) == 0
            continue
        cand_ok, contact_ok = B.generic(r, ref["extent"][k])
        nothing_left &= bool(cand_ok.all() and contact_ok.all())
        _law_rows(dev, fric, r, contact_ok, "%s direction %d" % (label, k))
    print(label, {key: out["friction"][key] for key in INFO_KEYS[:6]})
    if nothing_left:
        for key in INFO_KEYS:
            assert np.array_equal(out["friction"][key], ref["friction"][key]), (label, key, out["friction"][key], ref["friction"][key])
    return left


def _same_bits(x, y):
    TB._same_bits(x, y)
    for fx, fy in zip(x["fric"], y["fric"]):
        for key in fx:
            assert np.array_equal(fx[key], fy[key]), key
    for key in INFO_KEYS:
        assert np.array_equal(x["friction"][key], y["friction"][key]), key


def _moving_pair(name, **kw):
    ga, gb = TB._pair(name, **kw)
    _move_pair(ga, gb)
    return ga, gb


@pytest.mark.parametrize("name,damping,depth_cap", [(n, d, 0.0) for n in CLASSES for d in (0.0, 400.0)] + [("two_way", 400.0, 0.02), ("many_onto_one", 0.0, 0.02),
                                                                                                           ("deep", 400.0, 0.1)])
def test_shapes_against_the_reference(name, damping, depth_cap):
    ga, gb = _moving_pair(name)
    out = _call(ga, gb, damping=damping, depth_cap=depth_cap)
    assert out["info"]["n_contacts"] == TB.WANT[name]
    assert _compare(out, _reference(ga, gb, damping=damping, depth_cap=depth_cap), 0.0, "%s damping %g cap %g" % (name, damping, depth_cap)) == 0
    fi = out["friction"]
    if depth_cap:
        assert out["info"]["max_depth"] == depth_cap
    elif damping == 0.0:
        assert tuple(zip(fi["n_sticking"], fi["n_sliding"])) == CLASSES[name] and fi["n_separating"] == (0, 0)
    else:
        want = (0, 4) if name == "many_onto_one" else (0, 0)
        assert fi["n_separating"] == want and fi["n_sticking"][0] == CLASSES[name][0][0] and fi["n_sliding"][0] == CLASSES[name][0][1]
    assert fi["max_stick_rate"] == MU * fi["max_normal_force"] / SLIP
    ga.close(); gb.close()


@pytest.mark.parametrize("name", list(CLASSES))
def test_without_friction_the_bits_of_the_frictionless_call(name):
    ga, gb = _moving_pair(name)
    before = TB._call(ga, gb, K)
    new = _call(ga, gb, mu=0.0, slip=0.0, damping=0.0)
    TB._same_bits(before, new)
    assert before["info"]["faces_tested"] == new["info"]["faces_tested"]
    fi = new["friction"]
    assert fi["n_sticking"] == (0, 0) and fi["n_separating"] == (0, 0) and fi["n_sliding"] == tuple(c - d for c, d in zip(new["info"]["n_contacts"], new["info"]["n_degenerate"]))
    assert fi["max_stick_rate"] == 0.0 and not fi["friction_on_points"].any()
    # the frictionless call after a friction call: its old bits, against its own reference too
    _call(ga, gb, damping=400.0)
    after = TB._call(ga, gb, K)
    TB._same_bits(before, after)
    assert TB._compare(after, TB._reference(ga, gb, K), 0.0, name + " frictionless after friction") == 0
    ga.close(); gb.close()


def test_both_bodies_deformed_and_moving():
    va, ta, vb, tb = B.two_cubes(*B.SHAPES["two_way"])
    ga, gb = FemIntegrator(va, ta, **KW), FemIntegrator(vb, tb, **KW)
    rng = np.random.default_rng(11)
    for g in (ga, gb):
        g.set_q_state(rng.normal(size=3 * g.n_nodes) * 2e-3)
    _move_pair(ga, gb)
    out = _call(ga, gb, damping=400.0)
    assert sum(out["info"]["n_contacts"]) > 10
    _compare(out, _reference(ga, gb, damping=400.0), 0.02, "deformed and moving")
    ga.close(); gb.close()


def test_permuted_ids_and_forced_renumbering():
    va, ta, vb, tb = B.two_cubes(*B.SHAPES["many_onto_one"])
    meshes = []
    for v, t, seed in ((va, ta, 3), (vb, tb, 4)):
        p = np.random.default_rng(seed).permutation(len(v))   # new id of old node i
        v2 = np.empty_like(v)
        v2[p] = v
        meshes.append((v2, p[t].astype(np.int32)))
    with TB._Env(FEMBRAIN_RENUMBER=1):
        ga, gb = (FemIntegrator(v, t, **KW) for v, t in meshes)
    assert ga.renumbering()[0] and gb.renumbering()[0]
    _move_pair(ga, gb)
    out = _call(ga, gb)
    assert out["info"]["n_contacts"] == TB.WANT["many_onto_one"]
    assert _compare(out, _reference(ga, gb), 0.0, "permuted") == 0
    fi = out["friction"]
    assert tuple(zip(fi["n_sticking"], fi["n_sliding"])) == CLASSES["many_onto_one"]   # the field is one of positions: the classes are the unpermuted pair's
    ga.close(); gb.close()


def test_additivity_two_calls_and_direction_masks():
    ga, gb = _moving_pair("two_way")
    rng = np.random.default_rng(7)
    fa0, fb0 = rng.normal(size=3 * ga.n_nodes) * 5.0, rng.normal(size=3 * gb.n_nodes) * 5.0
    both = _call(ga, gb, damping=400.0, fa0=fa0, fb0=fb0)
    assert _compare(both, _reference(ga, gb, damping=400.0, fa0=fa0, fb0=fb0), 0.0, "onto a prior vector") == 0
    touched = np.concatenate([both["dirs"][0]["node"], ga.surface()["faces"][both["dirs"][1]["face"]].reshape(-1)])
    untouched = ~np.isin(np.arange(ga.n_nodes), touched)
    assert untouched.any() and np.array_equal(both["fa"][untouched], fa0.reshape(-1, 3)[untouched])
    again = _call(ga, gb, damping=400.0, fa0=fa0, fb0=fb0)
    _same_bits(both, again)
    assert both["info"]["faces_tested"] == again["info"]["faces_tested"]
    # one direction after the other on the same vectors is the call with both: a into b first
    one = _call(ga, gb, damping=400.0, directions="a_into_b", fa0=fa0, fb0=fb0)
    assert one["info"]["n_contacts"][1] == 0 and len(one["fric"][1]["normal_force"]) == 0 and one["friction"]["n_sliding"][1] == 0
    assert _compare(one, _reference(ga, gb, damping=400.0, directions=1, fa0=fa0, fb0=fb0), 0.0, "a into b") == 0
    two = _call(ga, gb, damping=400.0, directions="b_into_a", fa0=one["fa"].reshape(-1), fb0=one["fb"].reshape(-1))
    assert two["info"]["n_contacts"][0] == 0 and len(two["fric"][0]["normal_force"]) == 0
    assert np.array_equal(two["fa"], both["fa"]) and np.array_equal(two["fb"], both["fb"])
    for key in both["fric"][0]:
        assert np.array_equal(one["fric"][0][key], both["fric"][0][key]) and np.array_equal(two["fric"][1][key], both["fric"][1][key])
    for key in ("n_sticking", "n_sliding", "n_separating"):
        assert (one["friction"][key][0], two["friction"][key][1]) == both["friction"][key]
    ga.close(); gb.close()


@pytest.mark.parametrize("name", list(CLASSES))
def test_scan_and_ring_give_the_same_bits(name):
    ga, gb = _moving_pair(name)
    with TB._Env(FEMBRAIN_BODY_CONTACT="ring", FEMBRAIN_BODY_CONTACT_BUDGET=None):
        ring = _call(ga, gb, damping=400.0)
    with TB._Env(FEMBRAIN_BODY_CONTACT="scan", FEMBRAIN_BODY_CONTACT_BUDGET=None):
        scan = _call(ga, gb, damping=400.0)
    with TB._Env(FEMBRAIN_BODY_CONTACT="ring", FEMBRAIN_BODY_CONTACT_BUDGET=1):
        starved = _call(ga, gb, damping=400.0)
    assert ring["info"]["path"] == fl.FB_BODY_CONTACT_RING and scan["info"]["path"] == fl.FB_BODY_CONTACT_SCAN
    _same_bits(ring, scan)
    _same_bits(ring, starved)
    ga.close(); gb.close()


# ---- the self call ----

def _self_call(g, mode, mu=MU, slip=SLIP, damping=0.0, depth_cap=0.0, f0=None):
    g.set_external_forces_to_zero() if f0 is None else g.set_external_forces(f0)
    p, fr, info, fi = g._self_params(K, depth_cap, mode), _friction(mu, slip, damping), fl.SelfContactInfo(), fl.ContactFrictionInfo()
    fl.check(g._L.fb_fem_self_contact_friction(g.h, C.byref(p), C.byref(fr), C.byref(info), C.byref(fi)))
    out = {name: int(getattr(info, name)) for name in ("n_points", "n_contacts", "n_degenerate", "path", "n_point_grid_builds", "n_face_grid_builds", "n_parts_builds",
                                                        "faces_tested")}
    out.update(max_depth=float(info.max_depth), force_on_points=np.array(info.force_on_points[:]), force_on_faces=np.array(info.force_on_faces[:]))
    g._self_contacts = g._self_friction_contacts = out["n_contacts"]
    return dict(info=out, friction=g._friction_info(fi), contacts=g.read_self_contact(), fric=g.read_self_contact_friction(), f=g.external_forces().reshape(-1, 3))


def _self_reference(g, mode, mu=MU, slip=SLIP, damping=0.0, depth_cap=0.0, f0=None):
    x, t, cur, vel = _state(g)
    ref = F.self_contact(x, t, cur, vel, K, depth_cap, TS.MODES[mode], mu, slip, damping, f0)
    ref["extent"] = float((cur.max(axis=0) - cur.min(axis=0)).max())
    return ref


def _self_compare(out, ref, max_left_out=0.0, label=""):
    left = TS._compare(out, ref, max_left_out, label)
    cand_ok, contact_ok = B.generic(ref, ref["extent"])
    _law_rows(out["contacts"], out["fric"], ref, contact_ok, label)
    print(label, {key: out["friction"][key] for key in INFO_KEYS[:6]})
    if cand_ok.all() and contact_ok.all():
        for key in INFO_KEYS:
            got = out["friction"][key]
            assert np.array_equal(got, ref["friction"][key]), (label, key, got, ref["friction"][key])
        assert out["friction"]["n_sticking"][1] == 0 and out["friction"]["n_sliding"][1] == 0 and not out["friction"]["friction_on_points"][1].any()
    return left


def _moving_union(name):
    v, t, n_a, _ = S.union(name)
    g = FemIntegrator(v, t, **KW)
    g.set_q_state(np.zeros(3 * len(v)), F.union_fields(v, n_a).reshape(-1))
    return g


@pytest.mark.parametrize("name,mode", [("two_way", "any"), ("two_way", "other_parts"), ("many_onto_one", "other_parts")])
def test_unions_through_the_self_call(name, mode):
    g = _moving_union(name)
    plain = TS._call(g, mode)
    for damping in (0.0, 400.0):
        out = _self_call(g, mode, damping=damping)
        ref = _self_reference(g, mode, damping=damping)
        assert len(ref["node"]) == TS.WANT[name][1]
        assert _self_compare(out, ref, 0.0, "%s %s damping %g" % (name, mode, damping)) == 0
        if mode == "other_parts" and damping == 0.0:   # the contacts of both directions of the pair, in one list
            assert out["friction"]["n_sticking"][0] == sum(c[0] for c in CLASSES[name]) and out["friction"]["n_sliding"][0] == sum(c[1] for c in CLASSES[name])
    if name == "many_onto_one":
        assert ref["records_per_node"].max() == 177
    else:   # a node that is a point of one contact and a corner of others
        assert len(np.intersect1d(out["contacts"]["node"], g.surface()["faces"][out["contacts"]["face"]].reshape(-1))) == 24
    # without friction: the bits of fb_fem_self_contact, before and after
    zero = _self_call(g, mode, mu=0.0, slip=0.0, damping=0.0)
    TS._same_bits(plain, zero)
    TS._same_bits(plain, TS._call(g, mode))
    # two calls, and scan against ring
    with TB._Env(FEMBRAIN_SELF_CONTACT="scan", FEMBRAIN_SELF_CONTACT_BUDGET=None):
        scan = _self_call(g, mode, damping=400.0)
    assert scan["info"]["path"] == fl.FB_BODY_CONTACT_SCAN and out["info"]["path"] == fl.FB_BODY_CONTACT_RING
    for other in (scan, _self_call(g, mode, damping=400.0)):
        TS._same_bits(out, other)
        for key in out["fric"]:
            assert np.array_equal(out["fric"][key], other["fric"][key]), key
        for key in INFO_KEYS:
            assert np.array_equal(out["friction"][key], other["friction"][key]), key
    g.close()


def test_cut_beam_just_cut_then_pressed_with_part_one_moving():
    g, v, blade = TS._cut_beam()
    TS._cut(g, blade)
    n = g.r // 3
    x, t = g.read_mesh()
    _, node_part, n_parts = S.parts_of(t, len(x))
    assert n_parts == 2
    moving = np.where((node_part == 1)[:, None], F.field_a(x, x[node_part == 1].mean(axis=0)), 0.0)
    q = g.get_q_state()[0]
    g.set_q_state(q, moving.reshape(-1))
    # right after the cut every contact is at d == 0: nothing is pushed whatever the velocities, and the vector keeps its bits
    f0 = np.random.default_rng(9).normal(size=3 * n)
    for mode in ("any", "other_parts"):
        out = _self_call(g, mode, damping=400.0, f0=f0)
        assert out["info"]["n_degenerate"] == out["info"]["n_contacts"] and (out["contacts"]["depth"] == 0).all()
        assert np.array_equal(out["f"].reshape(-1), f0)
        fi = out["friction"]
        assert sum(fi["n_sticking"]) + sum(fi["n_sliding"]) + sum(fi["n_separating"]) == 0 and not out["fric"]["normal_force"].any() and not out["fric"]["friction"].any()
    # the far part pushed 0.31 of a cell into the near one, and moving
    g.set_q_state((q.reshape(-1, 3) + np.where((node_part == 1)[:, None], np.array(S.PRESS)[None, :], 0.0)).reshape(-1), moving.reshape(-1))
    out = _self_call(g, "other_parts", damping=400.0)
    ref = _self_reference(g, "other_parts", damping=400.0)
    assert (len(ref["vids"]), len(ref["node"])) == TS.WANT["cut_pressed"]
    assert _self_compare(out, ref, 0.02, "cut pressed, part 1 moving") == 1   # (one candidate on a boundary of an element, as in test_self_contact_gpu.py)
    assert out["friction"]["n_sliding"][0] > 0 and out["friction"]["max_slip_speed"] > SLIP
    g.close()


def test_self_additivity():
    g = _moving_union("two_way")
    f0 = np.random.default_rng(7).normal(size=3 * g.n_nodes) * 5.0
    once = _self_call(g, "any", damping=400.0, f0=f0)
    assert _self_compare(once, _self_reference(g, "any", damping=400.0, f0=f0), 0.0, "self, onto a prior vector") == 0
    c = once["contacts"]
    touched = np.concatenate([c["node"], g.surface()["faces"][c["face"]].reshape(-1)])
    untouched = ~np.isin(np.arange(g.n_nodes), touched)
    assert untouched.any() and np.array_equal(once["f"][untouched], f0.reshape(-1, 3)[untouched])
    g.close()


# ---- what is refused ----

BAD = [dict(mu=-0.1), dict(mu=np.nan), dict(mu=np.inf), dict(slip=-1.0), dict(slip=np.nan), dict(slip=np.inf), dict(damping=-1.0), dict(damping=np.nan),
       dict(damping=np.inf), dict(mu=0.5, slip=0.0), dict(reserved=1.0)]


def _raw_body(ga, gb, p, fr):
    info, fi = fl.BodyContactInfo(), fl.ContactFrictionInfo()
    return ga._L.fb_fem_body_contact_friction(ga.h, gb.h, C.byref(p) if p is not None else None, C.byref(fr) if fr is not None else None, C.byref(info), C.byref(fi))


def _raw_self(g, p, fr):
    info, fi = fl.SelfContactInfo(), fl.ContactFrictionInfo()
    return g._L.fb_fem_self_contact_friction(g.h, C.byref(p) if p is not None else None, C.byref(fr) if fr is not None else None, C.byref(info), C.byref(fi))


def test_invalid_arguments_leave_the_force_vectors_alone():
    ga, gb = _moving_pair("two_way")
    gs = _moving_union("two_way")
    rng = np.random.default_rng(13)
    f0 = {g: rng.normal(size=3 * g.n_nodes) for g in (ga, gb, gs)}
    for g, f in f0.items():
        g.set_external_forces(f)

    def untouched():
        for g, f in f0.items():
            assert np.array_equal(g.external_forces().reshape(-1), f)

    good_p, good_s = ga._body_params(K, 0.0, "both"), gs._self_params(K, 0.0, "any")
    for kw in BAD:
        fr = _friction(*[dict(dict(mu=MU, slip=SLIP, damping=0.0), **{k: v for k, v in kw.items() if k != "reserved"})[key] for key in ("mu", "slip", "damping")],
                       reserved=kw.get("reserved", 0.0))
        assert _raw_body(ga, gb, good_p, fr) == fl.FB_EINVAL, kw
        assert _raw_self(gs, good_s, fr) == fl.FB_EINVAL, kw
        untouched()
    good = _friction(MU, SLIP, 400.0)
    assert _raw_body(ga, gb, good_p, None) == fl.FB_EINVAL and _raw_self(gs, good_s, None) == fl.FB_EINVAL
    # everything the frictionless calls refuse
    assert _raw_body(ga, ga, good_p, good) == fl.FB_EINVAL and _raw_body(ga, gb, None, good) == fl.FB_EINVAL and _raw_self(gs, None, good) == fl.FB_EINVAL
    for bad_p in (ga._body_params(-1.0, 0.0, "both"), ga._body_params(np.inf, 0.0, "both"), ga._body_params(K, -0.1, "both"), ga._body_params(K, np.nan, "both"),
                  ga._body_params(K, 0.0, 0)):
        assert _raw_body(ga, gb, bad_p, good) == fl.FB_EINVAL
    for bad_s in (gs._self_params(-1.0, 0.0, "any"), gs._self_params(K, np.nan, "any"), gs._self_params(K, 0.0, 7)):
        assert _raw_self(gs, bad_s, good) == fl.FB_EINVAL
    untouched()
    # a velocity that is not finite, in either body
    for g, other, value in ((ga, gb, np.nan), (gb, ga, np.inf), (gs, None, np.nan)):
        q, qvel = g.get_q_state()[:2]
        broken = qvel.copy()
        broken[3 * (g.n_nodes // 2) + 1] = value
        g.set_q_state(q, broken)
        assert (_raw_self(gs, good_s, good) if other is None else _raw_body(ga, gb, good_p, good)) == fl.FB_EINVAL
        untouched()
        g.set_q_state(q, qvel)
    # and all of them still work
    assert _raw_body(ga, gb, good_p, good) == fl.FB_OK and _raw_self(gs, good_s, good) == fl.FB_OK
    for g in (ga, gb, gs):
        assert not np.array_equal(g.external_forces().reshape(-1), f0[g])
        g.set_uniform_force(1, -5.0)
        g.do_timestep()
        assert g.last.converged == 1
        g.close()


def test_the_wrappers_route_by_the_three_values():
    """``FemIntegrator.body_contact`` / ``self_contact``: all zero is the frictionless entry point and its dict, anything else the new one"""
    ga, gb = _moving_pair("two_way")
    ga.set_external_forces_to_zero(); gb.set_external_forces_to_zero()
    plain = ga.body_contact(gb, K)
    assert "n_sticking" not in plain
    ga.set_external_forces_to_zero(); gb.set_external_forces_to_zero()
    info = ga.body_contact(gb, K, mu=MU, slip_speed=SLIP, damping=400.0)
    want = _call(ga, gb, damping=400.0)
    for key in INFO_KEYS:
        assert np.array_equal(info[key], want["friction"][key]), key
    assert np.array_equal(ga.read_body_contact_friction("a_into_b")["normal_force"], want["fric"][0]["normal_force"])
    gs = _moving_union("two_way")
    gs.set_external_forces_to_zero()
    info = gs.self_contact(K, mode="any", mu=MU, slip_speed=SLIP)
    assert info["n_sticking"][0] + info["n_sliding"][0] == info["n_contacts"] and len(gs.read_self_contact_friction()["normal_force"]) == info["n_contacts"]
    assert "n_sticking" not in gs.self_contact(K, mode="any")
    for g in (ga, gb, gs):
        g.close()
