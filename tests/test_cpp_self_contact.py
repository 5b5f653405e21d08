"""Contact of a C++ Deformable with itself (include/fembrain/Deformable.h: selfCollide, setSelfCollision, HipIntegrator::SelfContact) goes
through fb_fem_self_contact, and a host program over the class prints what the Python driver computes through the same sequence."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "self_contact_classes")


def _build():
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "self_contact_classes.cpp"),
           "-o", EXE, "-L", os.path.join(ROOT, "fembrain_amd"), "-lfembrain_hip", "-Wl,-rpath," + os.path.join(ROOT, "fembrain_amd")]
    subprocess.check_call(cmd)


def _weighted(x):
    s = 0.0
    for i, v in enumerate(np.asarray(x).reshape(-1)):
        s += float(v) * float(i % 7 + 1)
    return s


def test_cpp_self_contact_program_compiles_and_links_with_gxx():
    _build()  # (fails to link on a library without the entry points)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_body_matches_the_python_driver(gpu):
    import selfcontactref as S
    from fembrain_amd.fem import Deformable
    _build()
    out = subprocess.check_output([EXE], text=True)
    kv = dict(line.split("=", 1) for line in out.strip().splitlines())
    v, t, _, _ = S.union("two_way")
    D = Deformable(v, t, gravity=False, expect_cuts=True)   # (the C++ class makes its handles for cuttable bodies)
    try:
        for m, mode in enumerate(("any", "other_parts")):
            D.integrator.set_external_forces_to_zero()
            info = D.self_collide(200.0, 0.0, mode)
            assert info["n_contacts"] == 25 == int(kv["N_%d" % m]) and info["n_points"] == 148 == int(kv["POINTS_%d" % m])
            assert info["n_parts_builds"] == int(kv["PARTS_BUILDS_%d" % m]) == m
            # the same library, inputs and call sequence: the same bits (%.17g round-trips a double)
            assert float(kv["MAXDEPTH_%d" % m]) == info["max_depth"]
            assert [float(x) for x in kv["ON_POINTS_%d" % m].split(",")] == list(info["force_on_points"])
            assert [float(x) for x in kv["ON_FACES_%d" % m].split(",")] == list(info["force_on_faces"])
            c = D.integrator.read_self_contact()
            assert int(kv["IDSUM_%d" % m]) == sum((int(c["node"][i]) + 3 * int(c["element"][i]) + 7 * int(c["face"][i])) * (i + 1) for i in range(len(c["node"])))
            assert float(kv["DEPTHSUM_%d" % m]) == _weighted(c["depth"]) and float(kv["FEXT_%d" % m]) == _weighted(D.integrator.external_forces())
        assert float(kv["CAPPED"]) == D.self_collide(200.0, 0.01)["max_depth"] == 0.01
        D.set_self_collision(200.0)
        for _ in range(3):
            D.timestep()
        q = D.integrator.get_q_state()[0]
        iters = D.integrator.last.cg_iterations
    finally:
        D.integrator.close()
    assert np.abs(q).max() > 1e-6   # the two cubes push each other apart
    assert float(kv["QSUM"]) == _weighted(q) and int(kv["ITERS"]) == iters
    assert int(kv["OFF"]) == 1
