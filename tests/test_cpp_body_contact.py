"""Contact between two C++ Deformable bodies (include/fembrain/Deformable.h: collideWith, setCollisionBody, HipIntegrator::BodyContact) goes
through fb_fem_body_contact, and a host program over the class prints what the Python driver computes through the same sequence."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "body_contact_classes")


def _build():
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "body_contact_classes.cpp"),
           "-o", EXE, "-L", os.path.join(ROOT, "fembrain_amd"), "-lfembrain_hip", "-Wl,-rpath," + os.path.join(ROOT, "fembrain_amd")]
    subprocess.check_call(cmd)


def _weighted(x):
    s = 0.0
    for i, v in enumerate(np.asarray(x).reshape(-1)):
        s += float(v) * float(i % 7 + 1)
    return s


def test_cpp_body_contact_program_compiles_and_links_with_gxx():
    _build()  # (fails to link on a library without the entry points)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_bodies_match_the_python_driver(gpu):
    import bodycontactref as R
    from fembrain_amd.fem import Deformable
    from fembrain_amd.meshgen import cube_fixed_plane_i0
    _build()
    out = subprocess.check_output([EXE], text=True)
    kv = dict(line.split("=", 1) for line in out.strip().splitlines())
    va, ta, vb, tb = R.two_cubes((3, 3, 3, 0.1), (5, 5, 5, 0.1), (0.1291, 0.3637, 0.0559))
    A = Deformable(va, ta, gravity=False, expect_cuts=True)   # (the C++ class makes its handles for cuttable bodies)
    B = Deformable(vb, tb, fixed_vertices=cube_fixed_plane_i0(5, 5), gravity=False, expect_cuts=True)
    try:
        A.integrator.set_external_forces_to_zero()
        B.integrator.set_external_forces_to_zero()
        info = A.collide_with(B, 200.0)
        assert info["n_contacts"][0] > 0 and info["n_contacts"][1] > 0
        assert (int(kv["N_AB"]), int(kv["N_BA"])) == info["n_contacts"] and (int(kv["CAND_AB"]), int(kv["CAND_BA"])) == info["n_candidates"]
        # the same library, inputs and call sequence: the same bits (%.17g round-trips a double)
        assert float(kv["MAXDEPTH"]) == info["max_depth"]
        assert [float(x) for x in kv["ON_A"].split(",")] == list(info["force_on_a"]) and [float(x) for x in kv["ON_B"].split(",")] == list(info["force_on_b"])
        c = A.integrator.read_body_contact("a_into_b")
        assert int(kv["IDSUM"]) == sum((int(c["node"][i]) + 3 * int(c["element"][i]) + 7 * int(c["face"][i])) * (i + 1) for i in range(len(c["node"])))
        assert float(kv["DEPTHSUM"]) == _weighted(c["depth"])
        assert float(kv["FEXT_A"]) == _weighted(A.integrator.external_forces()) and float(kv["FEXT_B"]) == _weighted(B.integrator.external_forces())
        assert float(kv["CAPPED"]) == A.collide_with(B, 200.0, 0.01)["max_depth"] == 0.01
        A.set_collision_body(B, 200.0)
        B.set_collision_body(A, 200.0)
        for _ in range(3):
            A.timestep()
            B.timestep()
        qa, qb = A.integrator.get_q_state()[0], B.integrator.get_q_state()[0]
        iters = (A.integrator.last.cg_iterations, B.integrator.last.cg_iterations)
    finally:
        A.integrator.close()
        B.integrator.close()
    assert qa.reshape(-1, 3)[:, 1].mean() > 1e-5 and np.abs(qb).max() > 1e-6   # the small cube is pushed up, the large one dented
    assert float(kv["QSUM_A"]) == _weighted(qa) and float(kv["QSUM_B"]) == _weighted(qb) and (int(kv["ITERS_A"]), int(kv["ITERS_B"])) == iters
    assert int(kv["OFF"]) == 1
