"""The C++ AvatarProbe (include/fembrain/AvatarProbe.h) over the C++ Deformable: the probe's contact session and its spread go through
fb_fem_contact_move / fb_fem_contact_apply, and a host program over the two classes prints what the Python driver computes through the
same sequence."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "contact_classes")


def _build():
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "contact_classes.cpp"),
           "-o", EXE, "-L", os.path.join(ROOT, "fembrain_amd"), "-lfembrain_hip", "-Wl,-rpath," + os.path.join(ROOT, "fembrain_amd")]
    subprocess.check_call(cmd)


def test_cpp_contact_program_compiles_and_links_with_gxx():
    _build()  # (fails to link on a library without the five entry points)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_probe_matches_the_python_driver(gpu):
    from fembrain_amd import lib as fl
    from fembrain_amd.fem import Deformable
    from fembrain_amd.meshgen import cube_fixed_plane_i0, truth_cube
    _build()
    out = subprocess.check_output([EXE], text=True)
    kv = dict(line.split("=", 1) for line in out.strip().splitlines())
    n = 5
    v, t = truth_cube(n, n, n, 0.1)
    d = Deformable(v, t, fixed_vertices=cube_fixed_plane_i0(n, n), expect_cuts=True)   # (the C++ class makes its handle for a cuttable body)
    try:
        d.set_haptic_force_radius(3)
        assert (int(kv["IDLE"]), int(kv["IDLE_TOUCHED"])) == (fl.FB_CONTACT_MISS, 0)
        d.probe_start()
        top = 0.0 * 0.1 + 4.0 * 0.1
        for k, depth in enumerate((0.02, 0.06, 0.12)):
            c = d.probe_move((-1.25, top - depth, -1.25), (1.15, top + 1.0, 1.15), 21345.73)
            assert c["status"] == fl.FB_CONTACT_SET and c["n_touched"] > 0
            for key, name in (("STATUS", "status"), ("TOUCHED", "n_touched"), ("NEW", "n_new"), ("FACE", "face"), ("CLOSEST", "closest_node"), ("PUSHING", "n_pushing")):
                assert int(kv["%s%d" % (key, k)]) == c[name], (key, k)
            assert kv["FACENAME%d" % k] == "BOTTOM"
            # the same library, inputs and call sequence: the same bits (%.17g round-trips a double)
            assert float(kv["DIST%d" % k]) == c["contact_dist"]
            assert [float(x) for x in kv["POINT%d" % k].split(",")] == list(c["closest_point"])
            d.timestep()
        ids, _, forces = d.integrator.read_contact()
        fsum = 0.0
        for i in range(len(ids)):
            fsum += float(forces[i, 1]) * float(i % 5 + 1)
        assert int(kv["LIST"]) == len(ids) and int(kv["LIST_IDSUM"]) == sum(int(a) * (i + 1) for i, a in enumerate(ids)) and float(kv["LIST_FSUM"]) == fsum
        d.probe_end()
        d.timestep()
        after = d.integrator.contact_info()
        q = d.integrator.get_q_state()[0]
        iters = d.integrator.last.cg_iterations
    finally:
        d.integrator.close()
    qsum = 0.0
    for i, x in enumerate(q):
        qsum += float(x) * float(i % 7 + 1)
    assert (int(kv["END_LIST"]), int(kv["END_FACE"]), int(kv["IN_PROGRESS"])) == (after["list_size"], after["face"], 0) == (0, 2, 0)
    assert np.abs(q).max() > 1e-4 and float(kv["QSUM"]) == qsum and int(kv["ITERS"]) == iters
