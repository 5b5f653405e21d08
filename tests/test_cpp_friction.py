"""Friction and contact damping through the C++ classes (include/fembrain/Deformable.h: setContactFriction for collideWith, selfCollide and
the timestep() opt-ins, HipIntegrator::SetContactFriction / LastContactFriction / ReadBodyContactFriction) go through
fb_fem_body_contact_friction and fb_fem_self_contact_friction, and a host program over the classes prints what the Python driver
computes through the same sequence."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "friction_classes")
K, MU, SLIP, DAMPING = 200.0, 0.5, 0.15, 5.0


def _build():
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "friction_classes.cpp"),
           "-o", EXE, "-L", os.path.join(ROOT, "fembrain_amd"), "-lfembrain_hip", "-Wl,-rpath," + os.path.join(ROOT, "fembrain_amd")]
    subprocess.check_call(cmd)


def _weighted(x):
    s = 0.0
    for i, v in enumerate(np.asarray(x).reshape(-1)):
        s += float(v) * float(i % 7 + 1)
    return s


def _floats(text):
    return [float(x) for x in text.split(",")]


def test_cpp_friction_program_compiles_and_links_with_gxx():
    _build()  # (fails to link on a library without the friction entry points)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_friction_matches_the_python_driver(gpu):
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
        A.set_collision_body(B, K)
        B.set_collision_body(A, K)
        for _ in range(2):
            A.timestep()
            B.timestep()
        assert np.abs(A.integrator.get_q_state()[1]).max() > 1e-4   # moving
        A.integrator.set_external_forces_to_zero()
        B.integrator.set_external_forces_to_zero()
        info = A.collide_with(B, K, mu=MU, slip_speed=SLIP, damping=DAMPING)
        assert min(info["n_contacts"]) > 0 and sum(info["n_sliding"]) + sum(info["n_sticking"]) > 0 and info["max_slip_speed"] > 0
        # the same library, inputs and call sequence: the same bits (%.17g round-trips a double)
        assert (int(kv["N_AB"]), int(kv["N_BA"])) == info["n_contacts"]
        assert _floats(kv["ON_A"]) == list(info["force_on_a"]) and _floats(kv["ON_B"]) == list(info["force_on_b"])
        assert [int(x) for x in kv["CLASSES"].split(",")] == [info[key][k] for key in ("n_sticking", "n_sliding", "n_separating") for k in range(2)]
        assert _floats(kv["MAXIMA"]) == [info["max_slip_speed"], info["max_normal_force"], info["max_stick_rate"]]
        assert _floats(kv["FRICTION_AB"]) == list(info["friction_on_points"][0]) and _floats(kv["FRICTION_BA"]) == list(info["friction_on_points"][1])
        c = A.integrator.read_body_contact_friction("a_into_b")
        assert float(kv["NSUM"]) == _weighted(c["normal_force"]) and float(kv["SLIPSUM"]) == _weighted(c["slip"]) and float(kv["FRICSUM"]) == _weighted(c["friction"])
        assert float(kv["FEXT_A"]) == _weighted(A.integrator.external_forces()) and float(kv["FEXT_B"]) == _weighted(B.integrator.external_forces())
        A.set_collision_body(B, K, MU, SLIP, DAMPING)
        B.set_collision_body(A, K, MU, SLIP, DAMPING)
        for _ in range(3):
            A.timestep()
            B.timestep()
        qa, qb = A.integrator.get_q_state()[0], B.integrator.get_q_state()[0]
        iters = (A.integrator.last.cg_iterations, B.integrator.last.cg_iterations)
        self_info = A.self_collide(K, 0.0, "any", mu=MU, slip_speed=SLIP, damping=DAMPING)
        A.integrator.set_external_forces_to_zero()
        B.integrator.set_external_forces_to_zero()
        plain = A.collide_with(B, K)
    finally:
        A.integrator.close()
        B.integrator.close()
    assert float(kv["QSUM_A"]) == _weighted(qa) and float(kv["QSUM_B"]) == _weighted(qb) and (int(kv["ITERS_A"]), int(kv["ITERS_B"])) == iters
    assert [int(x) for x in kv["SELF"].split(",")] == [self_info["n_points"], self_info["n_contacts"]] and "n_sticking" in self_info
    assert _floats(kv["PLAIN_ON_A"]) == list(plain["force_on_a"]) and "n_sticking" not in plain
