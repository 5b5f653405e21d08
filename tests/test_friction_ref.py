"""tests/frictionref.py against itself: the numpy restatement of the friction law (include/fembrain_hip.h, "Friction and damping of a
contact") has the properties a Coulomb law must have, reduces to the frictionless references bit for bit, and classes the contacts of
the shared shapes as the GPU tests expect -- far enough from the class boundaries that a rounding cannot move one."""
import functools
import math

import numpy as np
import pytest

import bodycontactref as B
import frictionref as F
import selfcontactref as S

K, MU, SLIP = 1000.0, 0.5, 0.15
EPS = np.finfo(np.float64).eps
NAMES = ["two_way", "many_onto_one", "deep"]
# sticking / sliding per direction with damping 0
CLASSES = {"two_way": ((1, 15), (1, 8)), "many_onto_one": ((28, 364), (1, 3)), "deep": ((8, 18), (0, 0))}


def _contributions_cancel(force, bary, live, records_per_contact):
    """Action and reaction: F and the three (-F) b_k of every contact that pushes sum to zero.  The sum is formed exactly (math.fsum), so
    what is left is the rounding of the contributions themselves -- b0 = (1 - b1) - b2 and three products per contact, under 3 eps |F|
    a contact -- and not that of a summation order: within n_records eps max|F|."""
    F, b = force[live], bary[live]
    if not len(F):
        return
    parts = np.concatenate([F[:, None, :], (-F)[:, None, :] * b[:, :, None]], axis=1).reshape(-1, 3)
    total = np.array([math.fsum(parts[:, k]) for k in range(3)])
    bound = records_per_contact * len(F) * EPS * np.abs(F).max()
    assert (np.abs(total) <= bound).all(), (total, bound)


@functools.lru_cache(maxsize=None)
def _pair(name):
    va, ta, vb, tb = B.two_cubes(*B.SHAPES[name])
    vela, velb = F.fields(va, vb)
    return va, ta, vb, tb, vela, velb


@functools.lru_cache(maxsize=None)
def _body(name, mu=MU, slip=SLIP, damping=0.0):
    va, ta, vb, tb, vela, velb = _pair(name)
    return F.body_contact(va, ta, va, vela, vb, tb, vb, velb, K, mu=mu, slip_speed=slip, damping=damping)


@pytest.mark.parametrize("name", NAMES)
def test_without_friction_it_is_the_frictionless_reference(name):
    va, ta, vb, tb, vela, velb = _pair(name)
    got, want = _body(name, 0.0, 0.0, 0.0), B.body_contact(va, ta, va, vb, tb, vb, K)
    for key in ("fa", "fb", "force_on_a", "force_on_b"):
        assert np.array_equal(got[key], want[key]), key
    assert got["max_depth"] == want["max_depth"]
    for g, w in zip(got["dirs"], want["dirs"]):
        assert np.array_equal(g["force"], w["force"]) and np.array_equal(g["node"], w["node"])
    # and with a slip speed but no friction coefficient
    again = F.body_contact(va, ta, va, vela, vb, tb, vb, velb, K, mu=0.0, slip_speed=SLIP)
    assert np.array_equal(again["fa"], want["fa"]) and np.array_equal(again["fb"], want["fb"])


@pytest.mark.parametrize("name,mode", [("two_way", S.ANY), ("two_way", S.OTHER_PARTS), ("many_onto_one", S.OTHER_PARTS)])
def test_unions_without_friction(name, mode):
    v, t, n_a, _ = S.union(name)
    vel = F.union_fields(v, n_a)
    got, want = F.self_contact(v, t, v, vel, K, mode=mode), S.self_contact(v, t, v, K, mode=mode)
    assert len(want["node"]) > 0
    for key in ("f", "force", "force_on_points", "force_on_faces"):
        assert np.array_equal(got[key], want[key]), key


@pytest.mark.parametrize("damping", [0.0, 400.0])
@pytest.mark.parametrize("name", NAMES)
def test_the_law_is_a_coulomb_law(name, damping):
    r = _body(name, damping=damping)
    for d in r["dirs"]:
        live = d["cls"] >= 0
        f, n, t, N, s = -d["mf"][live], d["n"][live], d["t"][live], d["N"][live], d["s"][live]
        if not len(N):
            continue
        size = np.sqrt((f * f).sum(axis=1))
        # friction lies in the tangent plane: f = g t and t = w - (w . n) n, so |f . n| is a few roundings of |f|
        assert (np.abs((f * n).sum(axis=1)) <= 16 * EPS * np.maximum(size, 1e-300)).all()
        assert (size <= MU * N * (1 + 4 * EPS)).all()
        sliding = d["cls"][live] == F.SLIDING
        assert np.allclose(size[sliding], MU * N[sliding], rtol=4 * EPS, atol=0.0)
        assert ((f * t).sum(axis=1) >= 0).all()   # it opposes the slip: -f . t <= 0
        assert (N >= 0).all() and (d["force"][d["cls"] == F.SEPARATING] == 0).all()   # no adhesion; a separating contact gets nothing
        _contributions_cancel(d["force"], d["bary"], live, 3)   # (a direction makes three records per contact)


@pytest.mark.parametrize("name", NAMES)
def test_classes_and_their_margins(name):
    r0, r400 = _body(name), _body(name, damping=400.0)
    for k in range(2):
        assert (r0["friction"]["n_sticking"][k], r0["friction"]["n_sliding"][k]) == CLASSES[name][k]
        assert r0["friction"]["n_separating"][k] == 0
    want = {key: list(r0["friction"][key]) for key in ("n_sticking", "n_sliding", "n_separating")}
    if name == "many_onto_one":   # the four points of b in a leave fast enough that the damper would pull: they separate
        want["n_sticking"][1], want["n_sliding"][1], want["n_separating"][1] = 0, 0, 4
    for key, v in want.items():
        assert list(r400["friction"][key]) == v, key
    for r in (r0, r400):
        for d in r["dirs"]:
            slip, normal = F.class_margins(d, SLIP)
            assert slip >= 0.01 and normal >= 0.6, (name, slip, normal)
    # the maxima belong to a contact
    fi = r0["friction"]
    every_N = np.concatenate([d["N"] for d in r0["dirs"]])
    assert fi["max_normal_force"] == every_N.max() and fi["max_stick_rate"] == MU * every_N.max() / SLIP
    assert fi["max_slip_speed"] == np.concatenate([d["s"] for d in r0["dirs"]]).max()


def test_unions_class_like_the_pairs():
    """the union of the two cubes under OTHER_PARTS has the contacts of both directions of the pair, in one list"""
    for name in ("two_way", "many_onto_one"):
        v, t, n_a, _ = S.union(name)
        r = F.self_contact(v, t, v, F.union_fields(v, n_a), K, mode=S.OTHER_PARTS, mu=MU, slip_speed=SLIP)
        pair = _body(name)["friction"]
        assert r["friction"]["n_sticking"][0] == sum(pair["n_sticking"]) and r["friction"]["n_sliding"][0] == sum(pair["n_sliding"])
        _contributions_cancel(r["force"], r["bary"], r["cls"] >= 0, 4)
