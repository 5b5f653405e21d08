"""Contact of a C++ Deformable with a rigid tool (include/fembrain/Deformable.h: collideTool, setTool / clearTool, toolForce / toolTorque,
HipIntegrator::ToolContact) goes through fb_fem_tool_contact, and a host program over the class prints what the Python driver computes
through the same sequence."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "tool_contact_classes")


def _build():
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "tool_contact_classes.cpp"),
           "-o", EXE, "-L", os.path.join(ROOT, "fembrain_amd"), "-lfembrain_hip", "-Wl,-rpath," + os.path.join(ROOT, "fembrain_amd")]
    subprocess.check_call(cmd)


def _weighted(x):
    s = 0.0
    for i, v in enumerate(np.asarray(x).reshape(-1)):
        s += float(v) * float(i % 7 + 1)
    return s


def _tool(drop):
    """tool_at(drop) of the program: the shapes and the origin"""
    shapes = [("capsule", (-0.3, 0.85 - drop, -0.2), (0.2, 0.9 - drop, 0.1), 0.18), ("sphere", (-0.037, 0.85 - drop, -0.054), 0.25),
              ("box", (0.21, 0.83 - drop, 0.19), (0.12, 0.09, 0.15), None)]
    return shapes, (0.1, 0.9 - drop, -0.2)


def _floats(text):
    return [float(x) for x in text.split(",")]


def _check_info(kv, tag, info):
    assert int(kv["N_" + tag]) == info["n_contacts"] and int(kv["POINTS_" + tag]) == info["n_points"]
    assert [int(x) for x in kv["BY_SHAPE_" + tag].split(",")] == list(info["contacts_by_shape"])
    assert [int(x) for x in kv["CLASSES_" + tag].split(",")] == [info["n_separating"], info["n_sticking"], info["n_sliding"]]
    # the same library, inputs and call sequence: the same bits (%.17g round-trips a double)
    assert float(kv["MAXDEPTH_" + tag]) == info["max_depth"]
    assert _floats(kv["ON_TOOL_" + tag]) == list(info["force_on_tool"]) and _floats(kv["TORQUE_" + tag]) == list(info["torque_on_tool"])


def test_cpp_tool_contact_program_compiles_and_links_with_gxx():
    _build()  # (fails to link on a library without the entry points)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_body_matches_the_python_driver(gpu):
    import tool_cases as TC
    from fembrain_amd.fem import Deformable
    _build()
    out = subprocess.check_output([EXE], text=True)
    kv = dict(line.split("=", 1) for line in out.strip().splitlines())
    x, t, _ = TC.mesh()
    D = Deformable(x, t, np.nonzero(x[:, 1] == 0.0)[0], gravity=False, expect_cuts=True)   # (the C++ class makes its handles for cuttable bodies)
    try:
        shapes, origin = _tool(0.0)
        D.integrator.set_external_forces_to_zero()
        info = D.collide_tool(shapes, 1000.0, origin=origin)
        assert info["n_contacts"] > 20 and min(info["contacts_by_shape"]) > 0 and info["n_points"] == 386
        _check_info(kv, "PLAIN", info)
        c = D.integrator.read_tool_contact()
        assert int(kv["IDSUM"]) == sum((int(c["node"][i]) + 3 * int(c["shape"][i])) * (i + 1) for i in range(len(c["node"])))
        assert float(kv["DEPTHSUM"]) == _weighted(c["depth"]) and float(kv["FORCESUM"]) == _weighted(c["force"])
        assert float(kv["FEXT_PLAIN"]) == _weighted(D.integrator.external_forces())
        assert _floats(kv["WRENCH"]) == [D.tool_force()[1], D.tool_torque()[2]] and D.tool_force()[1] > 0

        friction = dict(mu=0.4, slip_speed=0.3, damping=40.0)
        D.integrator.set_external_forces_to_zero()
        info = D.collide_tool(shapes, 1000.0, depth_cap=0.04, points="all_nodes", origin=origin, velocity=(0.3, -0.2, 0.1), omega=(0.5, 1.0, -0.7), **friction)
        assert info["n_points"] == 729 and info["max_depth"] == 0.04 and info["n_sliding"] > 0
        _check_info(kv, "FRICTION", info)
        c = D.integrator.read_tool_contact()
        assert float(kv["NSUM"]) == _weighted(c["normal_force"]) and float(kv["SLIPSUM"]) == _weighted(c["slip"]) and float(kv["FRICTIONSUM"]) == _weighted(c["friction"])
        assert float(kv["FEXT_FRICTION"]) == _weighted(D.integrator.external_forces())

        for r in (1, 2, 3):
            shapes, origin = _tool(0.01 * r)
            D.set_tool(shapes, 1000.0, origin=origin, velocity=(0.0, -0.01 / 0.0333, 0.0), **friction)
            D.timestep()
        q = D.integrator.get_q_state()[0]
        iters = D.integrator.last.cg_iterations
        _check_info(kv, "STEPPED", D.last_tool_contact)
        D.clear_tool()
    finally:
        D.integrator.close()
    assert np.abs(q).max() > 1e-6   # the tool pushed the tissue
    assert float(kv["QSUM"]) == _weighted(q) and int(kv["ITERS"]) == iters
    assert int(kv["OFF"]) == 1
