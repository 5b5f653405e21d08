"""fb_fem_tool_contact on the device against tests/toolref.py, the rule in plain Python floats.

The device functions and the reference are the same sequence of fp64 operations without contraction, and no decision of the rule has a
threshold beside the inside tests themselves, which both evaluate in the same bits: every output is compared BIT FOR BIT -- the
records, the external force vector (before + scatter, `before` a random vector) and the sums the host forms."""
import ctypes as C
import os

import numpy as np
import pytest

import tool_cases as TC
import toolref as T
from fembrain_amd import erosion
from fembrain_amd import lib as fl
from fembrain_amd.fem import FemIntegrator
from fembrain_amd.meshgen import fixed_vertices_to_dofs, truth_cube

pytestmark = pytest.mark.gpu

K = TC.K
KW = dict(E=1e6, timestep=0.01)
CASES = TC.cases()
FRAME = dict(origin=(0.1, 0.9, -0.2), velocity=(0.3, -0.2, 0.1), omega=(0.5, 1.0, -0.7))
INFO_KEYS = ("n_points", "n_contacts", "n_degenerate", "contacts_by_shape", "n_sticking", "n_sliding", "n_separating", "max_depth", "max_slip_speed",
             "max_normal_force", "max_stick_rate", "force_on_body", "force_on_tool", "torque_on_tool")
REC_KEYS = ("node", "shape", "depth", "normal", "force", "normal_force", "slip", "friction")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b.astype(a.dtype) if a.dtype != np.float64 else np.asarray(b, np.float64)))


def _cube(clamped=True, **kw):
    x, t, _ = TC.mesh()
    fixed = fixed_vertices_to_dofs(np.nonzero(x[:, 1] == 0.0)[0]) if clamped else ()
    return FemIntegrator(x, t, fixed, **dict(KW, **kw))


def _before(g, seed=5):
    return np.random.default_rng(seed).standard_normal(3 * int(g._L.fb_fem_num_nodes(g.h)))


def _call(g, shapes, f0=None, **kw):
    """sets the force vector (zero where none is given), calls, returns everything that comes back"""
    g.set_external_forces_to_zero() if f0 is None else g.set_external_forces(f0)
    info = g.tool_contact(shapes, K, **kw)
    return dict(info=info, contacts=g.read_tool_contact(), f=g.external_forces().reshape(-1, 3))


def _reference(g, shapes, f0=None, points="surface", depth_cap=0.0, mu=0.0, slip_speed=0.0, damping=0.0, **frame):
    x = g.read_mesh()[0]
    state = g.get_q_state()
    ids = g.surface()["vertex_ids"] if points == "surface" else np.arange(len(x))
    friction = None if mu == 0.0 and slip_speed == 0.0 and damping == 0.0 else (mu, slip_speed, damping)
    return T.tool_contact(x, state[0], ids, shapes, K, depth_cap, qvel=state[1], friction=friction, f0=f0, points=points, **frame)


def _compare(out, ref, label=""):
    info, dev = out["info"], out["contacts"]
    print("%s: %d points, %d contacts (reference %d), by shape %s, degenerate %d, classes %d / %d / %d" % (
        label, info["n_points"], info["n_contacts"], ref["n_contacts"], list(info["contacts_by_shape"]), info["n_degenerate"], info["n_separating"],
        info["n_sticking"], info["n_sliding"]))
    for key in REC_KEYS:
        assert _same(dev[key], ref[key]), (label, key)
    assert _same(out["f"], ref["f"]), (label, np.abs(out["f"] - ref["f"]).max())
    for key in INFO_KEYS:
        assert _same(info[key], ref[key]), (label, key, info[key], ref[key])
    assert np.array_equal(info["force_on_tool"], -info["force_on_body"])


def _both(g, shapes, label="", seed=5, **kw):
    f0 = _before(g, seed)
    out = _call(g, shapes, f0=f0, **kw)
    ref = _reference(g, shapes, f0=f0, **kw)
    _compare(out, ref, label)
    return out, ref


@pytest.fixture(scope="module")
def rest():
    g = _cube()
    yield g
    g.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_at_rest(rest, name):
    shapes, n, by_shape, n_deg = CASES[name]
    out, ref = _both(rest, shapes, name)
    info = out["info"]
    assert info["n_points"] == 386 and info["n_contacts"] == n and list(info["contacts_by_shape"]) == by_shape and info["n_degenerate"] == n_deg
    # before + scatter, written out
    want = _before(rest).reshape(-1, 3)
    want[out["contacts"]["node"]] += out["contacts"]["force"]
    assert _same(out["f"], want)
    if name == "flush_box":
        zero = out["contacts"]["depth"] == 0.0
        assert int(zero.sum()) == 8 and not out["contacts"]["force"][zero].any()


def test_the_miss_writes_nothing_and_reports_zeros(rest):
    f0 = _before(rest, 8)
    out = _call(rest, CASES["miss"][0], f0=f0)
    assert _same(out["f"].reshape(-1), f0) and len(out["contacts"]["node"]) == 0
    for key in INFO_KEYS[1:]:
        assert not np.any(out["info"][key]), key


def test_depth_cap(rest):
    out, ref = _both(rest, CASES["all_three"][0], "capped", depth_cap=0.04)
    assert out["info"]["max_depth"] == 0.04 < out["contacts"]["depth"].max()


@pytest.mark.parametrize("integrator", [fl.FB_INTEGRATOR_VOLUME_CONSERVING, fl.FB_INTEGRATOR_NEWMARK])
def test_loaded_handle(integrator):
    g = _cube(integrator=integrator)
    for _ in range(3):
        g.set_uniform_force(0, 40.0)
        g.do_timestep()
    q, qvel = g.get_q_state()[:2]
    assert np.abs(q).max() > 1e-4 and np.abs(qvel).max() > 1e-3
    out, _ = _both(g, CASES["all_three"][0], "loaded")
    print("loaded handle, integrator %d: %d contacts" % (integrator, out["info"]["n_contacts"]))
    assert out["info"]["n_contacts"] > 0
    out, ref = _both(g, CASES["all_three"][0], "loaded, friction", mu=0.4, slip_speed=0.3, damping=40.0, **FRAME)
    assert out["info"]["n_contacts"] > 0
    g.close()


def _moving(g, seed=11):
    """a state that is not zero, the same on every handle of the same mesh: set in the caller's order"""
    n = int(g._L.fb_fem_num_nodes(g.h))
    rng = np.random.default_rng(seed)
    q, qvel = 0.01 * rng.standard_normal((n, 3)), 0.3 * rng.standard_normal((n, 3))
    x = g.read_mesh()[0]
    q[x[:, 1] == 0.0] = 0.0
    qvel[x[:, 1] == 0.0] = 0.0
    g.set_q_state(q.reshape(-1), qvel.reshape(-1))


def test_friction_classes_records_and_maxima():
    g = _cube()
    _moving(g)
    kw = dict(mu=0.4, slip_speed=0.3, damping=40.0, velocity=(0.05, 0.0, 0.0), omega=(0.0, 0.4, 0.0), origin=(0.0, 0.9, 0.0))
    ref = _reference(g, CASES["all_three"][0], **kw)
    assert min(ref["n_separating"], ref["n_sticking"], ref["n_sliding"]) > 0   # every class, in the reference first
    out, _ = _both(g, CASES["all_three"][0], "friction", **kw)
    assert out["info"]["max_stick_rate"] > 0 and out["info"]["max_slip_speed"] > 0.3
    # the law without friction and damping, through the friction entry (slip_speed alone is not zero): the frictionless vector
    f0 = _before(g, 6)
    plain = _call(g, CASES["all_three"][0], f0=f0, **FRAME)
    law = _call(g, CASES["all_three"][0], f0=f0, slip_speed=0.05, **FRAME)
    assert plain["info"]["n_contacts"] == law["info"]["n_contacts"] > 0 and law["info"]["n_sliding"] + law["info"]["n_sticking"] > 0
    assert _same(plain["f"], law["f"]) and np.array_equal(plain["contacts"]["force"], law["contacts"]["force"])
    g.close()


def test_all_nodes_takes_interior_nodes_in_caller_order():
    g = _cube()
    _moving(g)
    shapes = [("sphere", (-0.037, 0.7, -0.054), 0.25), CASES["capsule"][0][0]]
    out, ref = _both(g, shapes, "all nodes", points="all_nodes", mu=0.2, slip_speed=0.1, damping=5.0, **FRAME)
    vids = g.surface()["vertex_ids"]
    node = out["contacts"]["node"]
    assert out["info"]["n_points"] == 729 and np.all(np.diff(node) > 0) and len(np.setdiff1d(node, vids)) > 0
    surf, _ = _both(g, shapes, "surface of the same", points="surface")
    assert set(surf["contacts"]["node"]) == set(node) & set(vids.tolist())
    g.close()


def _permuted():
    x, t, _ = TC.mesh()
    p = np.random.default_rng(3).permutation(len(x))   # new id of old node i
    x2 = np.empty_like(x)
    x2[p] = x
    return x2, p[t].astype(np.int32)


def test_renumbered_handle_gives_its_plain_twin_in_caller_ids():
    x, t = _permuted()
    fixed = fixed_vertices_to_dofs(np.nonzero(x[:, 1] == 0.0)[0])
    outs = []
    for renumber in (fl.FB_RENUMBER_ON, fl.FB_RENUMBER_OFF):
        g = FemIntegrator(x, t, fixed, renumber=renumber, **KW)
        assert bool(g.renumbering()[0]) == (renumber == fl.FB_RENUMBER_ON)
        _moving(g)
        for points in ("surface", "all_nodes"):
            out, _ = _both(g, CASES["all_three"][0], "renumber %d %s" % (renumber, points), points=points, mu=0.4, slip_speed=0.3, damping=40.0, **FRAME)
            assert out["info"]["n_contacts"] > 0
            outs.append(out)
        g.close()
    for a, b in ((outs[0], outs[2]), (outs[1], outs[3])):
        for key in REC_KEYS:
            assert _same(a["contacts"][key], b["contacts"][key]), key
        assert _same(a["f"], b["f"])
        for key in INFO_KEYS:
            assert _same(a["info"][key], b["info"][key]), key


def _blade(x):
    """a tilted plane through the middle of the body, under the tools"""
    nrm = np.array([1.0, 0.02, 0.013])
    nrm /= np.linalg.norm(nrm)
    a = np.cross(nrm, [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(nrm, a)
    p = x.min(0) + (x.max(0) - x.min(0)) * np.array([0.51, 0.5, 0.5])
    return np.array([p - 5 * a - 5 * b, p - 5 * a + 5 * b, p + 5 * a - 5 * b, p + 5 * a + 5 * b])


def test_after_a_cut_and_after_elements_are_removed():
    g = _cube(expect_cuts=True)
    for _ in range(2):
        g.set_uniform_force(0, 40.0)
        g.do_timestep()
    before, _ = _both(g, CASES["all_three"][0], "before the cut")
    info, _ = g.cut(_blade(g.read_mesh()[0]), mode="carry")
    assert info["status"] == fl.FB_CUT_DONE and info["n_new_nodes"] > 0
    after, _ = _both(g, CASES["all_three"][0], "after the cut", mu=0.4, slip_speed=0.3, damping=40.0, **FRAME)
    assert after["info"]["n_points"] > before["info"]["n_points"] and after["contacts"]["node"].max() >= 729
    _both(g, CASES["all_three"][0], "after the cut, all nodes", points="all_nodes")
    # a delta re-sync that takes the elements under a smaller sphere away: the tool now reaches nodes that were inside
    x, t = g.read_mesh()
    state = g.get_q_state()
    gone = erosion.select(x, t, state[0], [("sphere", (-0.037, 0.85, -0.054), 0.17)])
    assert 0 < len(gone) < len(t)
    g.resync_delta(dict(removed=gone), fixed_dofs=g.constrained_dofs())
    g.set_q_state(*state)
    n_surface = len(g.surface()["vertex_ids"])
    out, _ = _both(g, CASES["all_three"][0], "after the removal")
    assert out["info"]["n_points"] == n_surface != after["info"]["n_points"] and out["info"]["n_contacts"] > 0
    g.close()


def test_two_calls_from_one_state_give_the_same_bits():
    g = _cube()
    _moving(g)
    f0 = _before(g, 4)
    kw = dict(mu=0.4, slip_speed=0.3, damping=40.0, **FRAME)
    a, b = _call(g, CASES["all_three"][0], f0=f0, **kw), _call(g, CASES["all_three"][0], f0=f0, **kw)
    for key in REC_KEYS:
        assert _same(a["contacts"][key], b["contacts"][key]), key
    for key in INFO_KEYS:
        assert _same(a["info"][key], b["info"][key]), key
    assert _same(a["f"], b["f"]) and a["info"]["n_contacts"] > 0
    g.close()


def _raw(g, tool, params, fr=None, info=True):
    """the C ABI itself: the return code"""
    out = fl.ToolContactInfo()
    return g._L.fb_fem_tool_contact(g.h, None if tool is None else C.byref(tool), None if params is None else C.byref(params), None if fr is None else C.byref(fr),
                                    C.byref(out) if info else None)


def _edited(g, shapes, edit):
    tool = g._tool(shapes, (0, 0, 0), (0, 0, 0), (0, 0, 0))
    params = g._tool_params(K, 0.0, "surface")
    fr = g._friction_params(0.3, 0.1, 1.0)
    got = edit(tool, params, fr)
    return tool, params, (fr if got == "friction" else None)


def _set(path, value):
    """an edit that stores value at path: ("tool" | "params" | "fr", field or index, ...)"""
    def edit(tool, params, fr):
        obj = dict(tool=tool, params=params, fr=fr)[path[0]]
        for name in path[1:-1]:
            obj = obj[name] if isinstance(name, int) else getattr(obj, name)
        if isinstance(path[-1], int):
            obj[path[-1]] = value
        else:
            setattr(obj, path[-1], value)
        return "friction" if path[0] == "fr" else None
    return edit


def _skewed(tool, params, fr):
    """the box's R the identity but for one entry: |dot(R_0, R_1)| = 1e-8 > 1e-9"""
    tool.shapes[2].R[:] = [1.0, 1e-8, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def _nudged(tool, params, fr):
    """the box's R off by 5e-10 in one entry: every |dot(R_i, R_j) - delta_ij| stays below 1e-9"""
    tool.shapes[2].R[1] += 5e-10


EDITS = {
    "no shapes": _set(("tool", "n_shapes"), 0),
    "seventeen shapes": _set(("tool", "n_shapes"), 17),
    "unknown kind": _set(("tool", "shapes", 1, "kind"), 3),
    "tool reserved": _set(("tool", "reserved"), 1),
    "shape reserved": _set(("tool", "shapes", 0, "reserved"), 1),
    "params reserved": _set(("params", "reserved"), 1),
    "negative radius": _set(("tool", "shapes", 0, "size", 0), -0.1),
    "radius not finite": _set(("tool", "shapes", 1, "size", 0), float("inf")),
    "negative half extent": _set(("tool", "shapes", 2, "size", 1), -0.1),
    "centre not finite": _set(("tool", "shapes", 0, "a", 1), float("nan")),
    "capsule end not finite": _set(("tool", "shapes", 1, "b", 2), float("inf")),
    "R not finite": _set(("tool", "shapes", 2, "R", 4), float("nan")),
    "R not orthonormal": _set(("tool", "shapes", 2, "R", 1), 0.5),
    "R off by 1e-8": _skewed,
    "origin not finite": _set(("tool", "origin", 0), float("nan")),
    "velocity not finite": _set(("tool", "velocity", 1), float("inf")),
    "omega not finite": _set(("tool", "omega", 2), float("nan")),
    "unknown points": _set(("params", "points"), 2),
    "negative stiffness": _set(("params", "stiffness"), -1.0),
    "stiffness not finite": _set(("params", "stiffness"), float("nan")),
    "negative depth cap": _set(("params", "depth_cap"), -0.01),
    "negative mu": _set(("fr", "mu"), -0.1),
    "mu without slip speed": _set(("fr", "slip_speed"), 0.0),
    "damping not finite": _set(("fr", "damping"), float("nan")),
    "friction reserved": _set(("fr", "reserved"), 1.0),
}


@pytest.mark.parametrize("what", sorted(EDITS))
def test_refusals_leave_the_force_vector_and_the_records_as_they_were(rest, what):
    f0 = _before(rest, 7)
    kept = _call(rest, CASES["sphere"][0], f0=f0)
    assert _raw(rest, *_edited(rest, CASES["all_three"][0], lambda *a: None)) == fl.FB_OK   # (the unedited call is accepted,
    assert _raw(rest, *_edited(rest, CASES["all_three"][0], lambda *a: "friction")) == fl.FB_OK  # with friction too,
    assert _raw(rest, *_edited(rest, CASES["all_three"][0], _nudged)) == fl.FB_OK  # and an R within 1e-9)
    rest.set_external_forces(kept["f"].reshape(-1))
    tool, params, fr = _edited(rest, CASES["all_three"][0], EDITS[what])
    assert _raw(rest, tool, params, fr) == fl.FB_EINVAL, what
    assert _same(rest.external_forces(), kept["f"].reshape(-1))


def test_null_arguments_are_refused(rest):
    f0 = _before(rest, 7)
    rest.set_external_forces(f0)
    tool, params, _ = _edited(rest, CASES["sphere"][0], lambda *a: None)
    assert _raw(rest, None, params) == fl.FB_EINVAL and _raw(rest, tool, None) == fl.FB_EINVAL
    assert _same(rest.external_forces(), f0)
    assert _raw(rest, tool, params, info=False) == fl.FB_OK   # (out may be NULL: the forces are added all the same)
    assert not _same(rest.external_forces(), f0)


def test_a_state_that_is_not_finite_is_refused_with_the_vector_untouched():
    g = _cube(clamped=False)
    vids = g.surface()["vertex_ids"]
    interior = np.setdiff1d(np.arange(729), vids)
    f0 = _before(g, 9)
    kw = dict(mu=0.3, slip_speed=0.1, damping=1.0)

    def refused(**k):
        g.set_external_forces(f0)
        with pytest.raises(fl.FbError) as e:
            g.tool_contact(CASES["sphere"][0], K, **k)
        assert e.value.code == fl.FB_EINVAL and _same(g.external_forces(), f0)

    q, qvel = np.zeros((729, 3)), np.zeros((729, 3))
    q[vids[300], 1] = np.nan                     # a surface node of the second workgroup, far from the tool
    g.set_q_state(q.reshape(-1), qvel.reshape(-1))
    refused()
    refused(points="all_nodes")
    q[:] = 0.0
    q[interior[5], 0] = np.inf                   # not a point of the surface call
    g.set_q_state(q.reshape(-1), qvel.reshape(-1))
    assert g.tool_contact(CASES["sphere"][0], K)["n_contacts"] == 21
    refused(points="all_nodes")
    q[:] = 0.0
    qvel[vids[10], 2] = np.nan
    g.set_q_state(q.reshape(-1), qvel.reshape(-1))
    assert g.tool_contact(CASES["sphere"][0], K)["n_contacts"] == 21   # (the frictionless call reads no velocity)
    refused(**kw)
    refused(points="all_nodes", **kw)
    g.close()


def test_python_arguments_are_checked_before_the_library(rest):
    with pytest.raises(ValueError):
        rest.tool_contact([("sphere", (0, 0, 0), -1.0)], K)
    with pytest.raises(ValueError):
        rest.tool_contact([], K)
    with pytest.raises(KeyError):
        rest.tool_contact(CASES["sphere"][0], K, points="faces")


def _sharded_worker(rank, world, shm_name, q):
    try:
        L = fl.lib()
        comm = C.c_void_p()
        fl.check(L.fb_comm_create_local(C.byref(comm), rank, world, shm_name.encode(), 8 << 20, 0))
        v, t = truth_cube(6, 4, 4, 0.1)
        g = FemIntegrator(v, t, np.arange(3 * 16, dtype=np.int32), shard=(world, rank, np.array([0, 48, 96], np.int32), comm))
        tool = [("sphere", (0.0, 0.35, 0.0), 0.2)]
        codes = []
        for call in (lambda: g.tool_contact(tool, K), lambda: g.tool_contact(tool, K, points="all_nodes", mu=0.3, slip_speed=0.1), lambda: g.time_tool_contact(tool, K)):
            try:
                call()
                codes.append(0)
            except fl.FbError as e:
                codes.append(e.code)
        g.set_uniform_force(1, -50.0)   # it still steps
        g.do_timestep()
        codes.append(g.last.converged)
        q.put((rank, codes))
        g.close()
        L.fb_comm_destroy(comm)
    except Exception as e:  # surface the failure instead of hanging the peer
        q.put((rank, repr(e)))
        q.close()
        q.join_thread()
        os._exit(1)


def test_a_sharded_handle_is_refused():
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sharded_worker, args=(r, 2, "/fembrain_test_tc_%d" % os.getpid(), q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=120) for _ in procs]
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for rank, codes in res:
        assert codes == [fl.FB_EINVAL, fl.FB_EINVAL, fl.FB_EINVAL, 1], (rank, codes)


def test_time_tool_contact_adds_no_force_and_keeps_the_records(rest):
    f0 = _before(rest, 12)
    kept = _call(rest, CASES["sphere"][0], f0=f0)
    for kw in (dict(), dict(mu=0.3, slip_speed=0.1, damping=1.0, points="all_nodes")):
        sec = rest.time_tool_contact(CASES["all_three"][0], K, reps=2, **kw)
        print("stages, seconds:", sec)
        assert sec.shape == (3,) and np.isfinite(sec).all() and (sec >= 0).all()
    assert _same(rest.external_forces(), kept["f"].reshape(-1))
    again = rest.read_tool_contact()
    for key in REC_KEYS:
        assert _same(again[key], kept["contacts"][key]), key


def test_a_lowered_sphere_is_held_out_by_the_tissue():
    """The cube clamped at its bottom plane, a sphere lowered into the top face above node 400 by 0.3 of a cell per step for ten steps
    (its radius, 0.4, is above that travel of 0.3: the deepest point stays the one under its centre).  Stiffness under the explicit rule of the friction section: the penalty spring is explicit like the dampers there, k dt^2 stays below
    the mass a contact pushes.  A node of the top face carries rho h^3 / 2 = 0.5 kg; k = 2000 N/m and dt = 0.01 s give k dt^2 = 0.2 kg."""
    x, _, _ = TC.mesh()
    radius, cell, stiffness = 0.4, 0.1, 2000.0
    top = x[TC.lattice(4, 8, 4)]
    g = _cube(E=1e4, timestep=0.01)
    info = None
    for step in range(1, 11):
        travel = 0.3 * cell * step
        shapes = [("sphere", (top[0], top[1] + radius - travel, top[2]), radius)]
        g.set_external_forces_to_zero()
        info = g.tool_contact(shapes, stiffness, velocity=(0.0, -0.3 * cell / 0.01, 0.0))
        g.do_timestep()
    info = g.tool_contact(shapes, stiffness)
    print("travel %.3f, max_depth with the call %.5f, force on the tool %s" % (travel, info["max_depth"], info["force_on_tool"]))
    assert info["max_depth"] < 0.5 * travel and info["force_on_tool"][1] > 0
    g.close()
    # without the call the body stays where it is, and the rule sees the whole travel
    vids = TC.mesh()[2]
    ref = T.tool_contact(x, np.zeros_like(x), vids, shapes, stiffness)
    print("without the call: penetration %.5f" % ref["max_depth"])
    assert abs(ref["max_depth"] - travel) < 1e-12
