"""The rule of fb_fem_tool_contact as tests/toolref.py states it, pinned without a device: the counts of tests/tool_cases.py on
truth_cube(9, 9, 9) at rest, the shapes against erosion.py's inside tests, the choice among shapes, the refusals, the law at
mu = damping = 0 against the frictionless force, and the torque of a frictionless sphere about its own centre."""
import numpy as np
import pytest

import tool_cases as TC
import toolref as T
from fembrain_amd import erosion

CASES = TC.cases()


def _at_rest(shapes, **kw):
    x, _, vids = TC.mesh()
    return T.tool_contact(x, np.zeros_like(x), vids, shapes, TC.K, **kw)


def test_the_cube_has_two_ragged_workgroups_of_surface_vertices():
    x, t, vids = TC.mesh()
    assert (len(x), len(t), len(vids)) == (729, 3072, 386)
    R = TC.rot()
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15


@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_of_every_case(name):
    shapes, n, by_shape, n_deg = CASES[name]
    r = _at_rest(shapes)
    print(name, r["n_contacts"], r["contacts_by_shape"], r["n_degenerate"])
    assert r["n_contacts"] == n == len(r["node"]) and list(r["contacts_by_shape"]) == by_shape and r["n_degenerate"] == n_deg
    assert np.all(np.diff(r["node"]) > 0) and r["n_points"] == 386
    # the contacts are the points erosion.py's test holds, whichever shape wins
    x, _, vids = TC.mesh()
    assert np.array_equal(r["node"], vids[erosion.inside_tool(shapes, x[vids])])
    # every normal that exists has unit length to rounding, and the force is sd * n
    live = ~r["degenerate"]
    assert np.abs(np.linalg.norm(r["normal"][live], axis=1) - 1.0).max(initial=0.0) < 1e-15 * 4
    assert np.array_equal(r["force"][live], (TC.K * r["depth"][live])[:, None] * r["normal"][live])
    assert not r["force"][~live].any() and not r["normal"][~live].any()
    assert np.array_equal(r["force_on_tool"], -r["force_on_body"])


def test_the_sphere_on_a_node_is_degenerate_there_and_pushes_its_neighbours():
    r = _at_rest(CASES["on_a_node"][0])
    at = int(np.nonzero(r["degenerate"])[0][0])
    assert r["node"][at] == 400 and r["depth"][at] == 0.12
    assert np.all(r["depth"][~r["degenerate"]] > 0) and r["max_depth"] == r["depth"][~r["degenerate"]].max()


def test_the_flush_box_holds_eight_nodes_at_depth_zero_with_zero_force():
    r = _at_rest(CASES["flush_box"][0])
    assert int((r["depth"] == 0.0).sum()) == 8 and not r["force"][r["depth"] == 0.0].any()
    assert r["node"][r["depth"] > 0].tolist() == [400] and r["n_degenerate"] == 0


def test_twins_give_the_single_sphere_and_the_deepest_shape_wins():
    one, two = _at_rest(CASES["sphere"][0]), _at_rest(CASES["twins"][0])
    for key in ("node", "depth", "normal", "force", "f"):
        assert np.array_equal(one[key], two[key]), key
    shapes = CASES["all_three"][0]
    r = _at_rest(shapes)
    x = TC.mesh()[0]
    for node, s, depth in zip(r["node"], r["shape"], r["depth"]):
        held = [T.shape_at(sh, [float(v) for v in x[node]]) for sh in shapes]
        depths = [h[0] if h is not None else -1.0 for h in held]
        assert depth == max(depths) and s == depths.index(max(depths))


def test_depth_cap_caps_the_force_and_max_depth_but_not_the_record():
    free, capped = _at_rest(CASES["sphere"][0]), _at_rest(CASES["sphere"][0], depth_cap=0.05)
    assert np.array_equal(free["depth"], capped["depth"]) and capped["max_depth"] == 0.05 < free["max_depth"]
    assert np.array_equal(capped["force"], (TC.K * np.minimum(free["depth"], 0.05))[:, None] * free["normal"])


def test_the_vector_is_before_plus_scatter():
    x, _, _ = TC.mesh()
    f0 = np.random.default_rng(5).standard_normal(x.shape)
    r = _at_rest(CASES["all_three"][0], f0=f0)
    want = f0.copy()
    want[r["node"]] += r["force"]
    assert np.array_equal(r["f"], want)


BAD = [
    dict(shapes=[]),
    dict(shapes=[("sphere", (0, 0, 0), 0.1)] * 17),
    dict(shapes=[("disc", (0, 0, 0), 0.1)]),
    dict(shapes=[("sphere", (0, 0, 0), -0.1)]),
    dict(shapes=[("sphere", (0, np.nan, 0), 0.1)]),
    dict(shapes=[("capsule", (0, 0, 0), (0, np.inf, 0), 0.1)]),
    dict(shapes=[("box", (0, 0, 0), (0.1, -0.1, 0.1), None)]),
    dict(shapes=[("box", (0, 0, 0), (0.1, 0.1, 0.1), 1.001 * np.eye(3))]),
    dict(shapes=[("box", (0, 0, 0), (0.1, 0.1, 0.1), [[1, 1e-8, 0], [0, 1, 0], [0, 0, 1]])]),
    dict(stiffness=-1.0),
    dict(stiffness=np.nan),
    dict(depth_cap=-0.1),
    dict(points="faces"),
    dict(origin=(0, np.nan, 0)),
    dict(velocity=(np.inf, 0, 0)),
    dict(omega=(0, 0, np.nan)),
    dict(friction=(-0.1, 0.1, 0.0)),
    dict(friction=(0.5, 0.0, 0.0)),
    dict(friction=(0.5, 0.1, np.nan)),
]


@pytest.mark.parametrize("i", range(len(BAD)))
def test_refusals_raise(i):
    x, _, vids = TC.mesh()
    kw = dict(shapes=CASES["sphere"][0], stiffness=TC.K, qvel=np.zeros_like(x))
    kw.update(BAD[i])
    shapes, stiffness = kw.pop("shapes"), kw.pop("stiffness")
    with pytest.raises(ValueError):
        T.tool_contact(x, np.zeros_like(x), vids, shapes, stiffness, **kw)


def test_a_position_or_velocity_that_is_not_finite_raises():
    x, _, vids = TC.mesh()
    q = np.zeros_like(x)
    q[vids[7], 1] = np.nan
    with pytest.raises(ValueError):
        T.tool_contact(x, q, vids, CASES["sphere"][0], TC.K)
    v = np.zeros_like(x)
    v[vids[7], 2] = np.inf
    with pytest.raises(ValueError):
        T.tool_contact(x, np.zeros_like(x), vids, CASES["sphere"][0], TC.K, qvel=v, friction=(0.3, 0.1, 1.0))
    T.tool_contact(x, np.zeros_like(x), vids, CASES["sphere"][0], TC.K, qvel=v)   # (without friction no velocity is read)
    interior = np.setdiff1d(np.arange(len(x)), vids)[0]
    q = np.zeros_like(x)
    q[interior, 0] = np.nan
    T.tool_contact(x, q, vids, CASES["sphere"][0], TC.K)                          # (not a point of the call)
    with pytest.raises(ValueError):
        T.tool_contact(x, q, np.arange(len(x)), CASES["sphere"][0], TC.K, points="all_nodes")


def _moving(seed):
    x, _, vids = TC.mesh()
    rng = np.random.default_rng(seed)
    return x, 0.01 * rng.standard_normal(x.shape), 0.3 * rng.standard_normal(x.shape), vids, rng.standard_normal(x.shape)


def test_the_law_without_friction_and_damping_gives_the_frictionless_force():
    x, q, qv, vids, f0 = _moving(11)
    tool = dict(origin=(0.1, 0.9, -0.2), velocity=(0.3, -0.2, 0.1), omega=(0.5, 1.0, -0.7))
    for name in ("all_three", "flush_box", "on_a_node"):
        plain = T.tool_contact(x, q, vids, CASES[name][0], TC.K, f0=f0, **tool)
        law = T.tool_contact(x, q, vids, CASES[name][0], TC.K, f0=f0, qvel=qv, friction=(0.0, 0.05, 0.0), **tool)
        assert plain["n_contacts"] == law["n_contacts"] > 0
        # the vector bit for bit; the records as numbers: N * n_k - 0 * t_k gives +0 where sd * n_k is -0
        assert np.array_equal(plain["f"].view(np.uint64), law["f"].view(np.uint64))
        assert np.array_equal(plain["force"], law["force"]) and np.array_equal(law["normal_force"][~law["degenerate"]], TC.K * law["depth"][~law["degenerate"]])
        assert law["n_separating"] + law["n_sticking"] + law["n_sliding"] == law["n_contacts"] - law["n_degenerate"]


def test_friction_populates_every_class_and_opposes_the_slip():
    x, q, qv, vids, _ = _moving(11)
    r = T.tool_contact(x, q, vids, CASES["all_three"][0], TC.K, qvel=qv, friction=(0.4, 0.3, 40.0), velocity=(0.05, 0.0, 0.0), omega=(0.0, 0.4, 0.0), origin=(0.0, 0.9, 0.0))
    print(r["n_separating"], r["n_sticking"], r["n_sliding"])
    assert min(r["n_separating"], r["n_sticking"], r["n_sliding"]) > 0
    live = r["cls"] >= 0
    assert np.all((r["friction"][live] * r["slip"][live]).sum(axis=1) <= 0)
    assert np.abs((r["slip"][live] * r["normal"][live]).sum(axis=1)).max() < 1e-15 * 8
    assert np.all(np.linalg.norm(r["friction"][live], axis=1) <= 0.4 * r["normal_force"][live] * (1 + 1e-15 * 4))
    assert not r["force"][r["cls"] == T.SEPARATING].any()


def test_a_frictionless_sphere_returns_no_torque_about_its_centre():
    """F is along r = p - centre, so r x F is rounding only: each of the two products of a component is within 2^-53 relative of |r||F|
    after the roundings of n and F, and their difference within 4 * 2^-52 * sum |r||F| over the contacts"""
    x, _, vids = TC.mesh()
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(200):
        c = np.array([-0.037, 0.85, -0.054]) + 0.05 * rng.standard_normal(3)
        q = 0.01 * rng.standard_normal(x.shape)
        r = T.tool_contact(x, q, vids, [("sphere", tuple(c), 0.25)], TC.K, origin=tuple(c))
        assert r["n_contacts"] > 0
        arm = np.linalg.norm((x + q)[r["node"]] - c, axis=1)
        unit = 2.0 ** -52 * float((arm * np.linalg.norm(r["force"], axis=1)).sum())
        worst = max(worst, float(np.abs(r["torque_on_tool"]).max()) / unit)
        assert np.abs(r["torque_on_tool"]).max() <= 4 * unit
    print("largest |torque| in units of 2^-52 sum |r||F|: %.3f" % worst)
