"""The grip of a C++ Deformable (include/fembrain/Deformable.h: grip, moveGrip, releaseGrip, gripForce; HipIntegrator::Grasp / GraspMove /
ReadReactions / MotionInfo) goes through fb_fem_grasp and fb_fem_read_reactions, and a host program over the class prints what the Python
driver computes through the same sequence."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "motion_classes")


def _build():
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "motion_classes.cpp"),
           "-o", EXE, "-L", os.path.join(ROOT, "fembrain_amd"), "-lfembrain_hip", "-Wl,-rpath," + os.path.join(ROOT, "fembrain_amd")]
    subprocess.check_call(cmd)


def _weighted(x):
    s = 0.0
    for i, v in enumerate(np.asarray(x).reshape(-1)):
        s += float(v) * float(i % 7 + 1)
    return s


def test_cpp_motion_program_compiles_and_links_with_gxx():
    _build()  # (fails to link on a library without the entry points)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_grip_matches_the_python_driver(gpu):
    from fembrain_amd.fem import Deformable
    from fembrain_amd.meshgen import truth_cube
    _build()
    out = subprocess.check_output([EXE], text=True)
    kv = dict(line.split("=", 1) for line in out.strip().splitlines())
    nx, ny, nz = 6, 3, 3
    v, t = truth_cube(nx, ny, nz, 0.1)
    n = nx * ny * nz
    held = np.arange(n - ny * nz, n, dtype=np.int32)
    D = Deformable(v, t, fixed_vertices=np.arange(ny * nz, dtype=np.int32), gravity=False, expect_cuts=True)   # (the C++ class makes its handles for cuttable bodies)
    try:
        info = D.grip(held)
        assert info["n_dofs"] == 3 * len(held) == int(kv["GRIP_DOFS"]) and info["n_grasp_nodes"] == len(held) == int(kv["GRIP_NODES"])
        pivot = np.asarray(v, np.float64).reshape(-1, 3)[held[4]]
        for r in range(3):
            m = 60.0 / float(r + 1)
            c, s = (m * m - 1.0) / (m * m + 1.0), 2.0 * m / (m * m + 1.0)
            D.move_grip([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]], (0.002 * float(r + 1), 0.0, 0.0), pivot)
            D.timestep()
            # the same library, inputs and call sequence: the same bits (%.17g round-trips a double)
            assert [float(x) for x in kv["FORCE_%d" % r].split(",")] == list(D.grip_force()), r
            assert int(kv["ITERS_%d" % r]) == D.integrator.last.cg_iterations
        mi = D.integrator.motion_info()
        assert (mi["n_listed_elements"], mi["n_touched_nodes"], mi["longest_run"], mi["table_builds"]) == tuple(int(kv[k]) for k in ("LISTED", "TOUCHED", "LONGEST", "BUILDS"))
        assert mi["table_builds"] == 1 and mi["n_listed_elements"] > 0
        q = D.integrator.get_q_state()[0]
        assert float(kv["QSUM_HELD"]) == _weighted(q) and float(kv["REACT"]) == _weighted(D.integrator.reactions()[0])
        assert np.abs(D.grip_force()).max() > 0.0   # the tissue pulls back on the tool
        D.release_grip()
        assert int(kv["FIXED_AFTER"]) == len(D.integrator.constrained_dofs()) == 3 * ny * nz and int(kv["SET_AFTER"]) == D.integrator.motion_info()["n_dofs"] == 0
        D.timestep()
        q2 = D.integrator.get_q_state()[0]
        assert float(kv["QSUM_FREE"]) == _weighted(q2) and int(kv["ITERS_FREE"]) == D.integrator.last.cg_iterations
    finally:
        D.integrator.close()
    # let go, the end springs back: the held face moves towards its rest position
    assert np.abs(q2.reshape(-1, 3)[held]).max() < np.abs(q.reshape(-1, 3)[held]).max()
