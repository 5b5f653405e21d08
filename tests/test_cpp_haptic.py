"""The C++ Deformable (include/fembrain/Deformable.h) with a probe on: its pick, pulled steps, box pick and volume go through the device
entry points of the haptic probe, and a host program over it prints what the Python driver computes through the same sequence."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "haptic_classes")


def _build():
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "haptic_classes.cpp"),
           "-o", EXE, "-L", os.path.join(ROOT, "fembrain_amd"), "-lfembrain_hip", "-Wl,-rpath," + os.path.join(ROOT, "fembrain_amd")]
    subprocess.check_call(cmd)


def test_cpp_haptic_program_compiles_and_links_with_gxx():
    _build()  # (fails to link on a library without the four entry points)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_deformable_probe_matches_the_python_driver(gpu):
    from fembrain_amd.fem import Deformable
    from fembrain_amd.meshgen import cube_fixed_plane_i0, truth_cube
    _build()
    out = subprocess.check_output([EXE], text=True)
    kv = dict(line.split("=", 1) for line in out.strip().splitlines())
    n = 5
    v, t = truth_cube(n, n, n, 0.1)
    d = Deformable(v, t, fixed_vertices=cube_fixed_plane_i0(n, n), expect_cuts=True)   # (the C++ class makes its handle for a cuttable body)
    try:
        far = (10.0, 0.23, 10.0)
        clamped = d.haptic_start_at((-10.0, 0.23, 10.0))
        d.haptic_end()
        started = d.haptic_start_at(far)
        picked, _ = d.pick_vertex(far)
        d.haptic_set_current_forces([picked, picked - 1], [(0.0, 2500.0, 300.0), (-200.0, 900.0, 0.0)])
        vol0 = d.compute_volume()
        d.timestep()
        d.timestep()
        again, hit = d.pick_vertex(far)
        found, ids = d.pick_vertices(hit - 0.15, hit + 0.15)     # around where the pulled corner has got to
        vol, per = d.integrator.volume(per_element=True)
        q = d.integrator.get_q_state()[0]
        iters = d.integrator.last.cg_iterations
    finally:
        d.integrator.close()
    persum = 0.0
    for x in per:
        persum += float(x)
    qsum = 0.0
    for i, x in enumerate(q):
        qsum += float(x) * float(i % 7 + 1)
    assert picked == (n - 1) * n * n + 2 * n + (n - 1) and np.abs(q).max() > 1e-4 and again in ids
    assert (int(kv["CLAMPED_START"]), int(kv["STARTED"])) == (int(clamped), int(started)) == (0, 1)
    assert int(kv["PICKED"]) == picked and int(kv["PICKED_AGAIN"]) == again
    assert [float(x) for x in kv["PICK_XYZ"].split(",")] == list(hit)
    assert int(kv["BOX"]) == len(ids) and int(kv["BOX_IDSUM"]) == sum(int(a) * (k + 1) for k, a in enumerate(ids))
    assert [float(x) for x in kv["BOX_LAST"].split(",")] == list(found[-1])
    # the same library, inputs and call sequence: the same bits (%.17g round-trips a double)
    assert float(kv["VOL0"]) == vol0 and float(kv["VOL"]) == vol and float(kv["VOL_PERSUM"]) == persum
    assert float(kv["QSUM"]) == qsum and int(kv["ITERS"]) == iters
    assert int(kv["VOL_CHANGED"]) == int(abs(vol - vol0) > 0.0001)
