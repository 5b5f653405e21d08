"""CPU tests of the per-element material restatement (tests/matref.py) and of the .veg material readers.

matref.MatRef is what tests/test_materials_gpu.py compares the device against, so it is pinned here two ways: with all ids equal it
must reproduce the uniform oracle (OrcFem.assemble, mass_on_pattern, step(want=True)), and with the three-material cube it must match
sums of the REFERENCE's own sub-mesh assemblies (tests/golden/fem_cube5_materials.npz, made by tests/golden/make_materials_golden.py).
Bounds: 1e-12 of the largest entry -- both sides are fp64 sums of the same few dozen element terms per entry in a different order
(measured when the golden was made: 2.8e-15 in f, 7e-16 in K); dv: the oracle's PCG stops at a 1e-12 relative residual, the direct
solve at rounding, bound 1e-8 of max|dv| as tests/test_fem_gpu.py bounds a tight PCG against the oracle's."""
import os
import subprocess

import numpy as np
import pytest

import fem_params as fp
from fembrain_amd.meshgen import cube_fixed_plane_i0, fixed_vertices_to_dofs, read_veg, read_veg_materials, truth_cube
from matref import MatRef, region_ids, three_materials
from oracle.pyoracle import OrcFem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
VEG = os.path.join(GOLD, "cube3_materials.veg")


def _cube(n):
    v, t = truth_cube(n, n, n, 0.1)
    return v, t, fixed_vertices_to_dofs(cube_fixed_plane_i0(n, n))


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()


@pytest.mark.parametrize("name", ["default", "soft_damped"])
@pytest.mark.parametrize("warp", [0, 1, 2])
def test_equal_ids_reproduce_the_uniform_oracle(name, warp):
    v, t, fixed = _cube(5)
    mat = tuple(fp.material(name)[k] for k in ("E", "nu", "rho"))
    # two table entries, every element names the second: the lookup by id is live
    ref = MatRef(v, t, [(1.0, 0.0, 1.0), mat], np.ones(len(t), np.uint8), warp=warp)
    o = OrcFem(v, t, **fp.material(name))
    o.set_warp(warp)
    u = np.random.default_rng(12345).normal(size=o.r) * 0.01
    fo, Ko = o.assemble(u)
    f, Kb = ref.assemble(u)
    assert _rel(f, fo) <= 1e-12 and _rel(ref.blocks_to_csr(Kb), Ko) <= 1e-12
    assert _rel(ref.mass_csr_values(), o.mass_on_pattern()) <= 1e-12
    if warp == 2:
        return  # (the oracle's step is FemBrain's: warp 0 / 1)
    ig = fp.integrator(name)
    o.integrator(fixed, **ig)
    q0, v0 = fp.live_state(o.r, fixed)
    fext = fp.load(name, o.r)
    o.set_state(q0, v0)
    o.set_external_forces(fext)
    info, keff, rhs, dv = o.step(cg_eps=1e-12, cg_maxiter=20000, want=True)
    assert info > 0
    keff_r, rhs_r, _ = ref.system(q0, v0, fext, ig["timestep"], ig["cM"], ig["cK"])
    assert _rel(keff_r, keff) <= 1e-12 and _rel(rhs_r, rhs) <= 1e-12
    q1, v1, dv_r, _ = ref.step(q0, v0, fext, fixed, ig["timestep"], ig["cM"], ig["cK"])
    assert _rel(dv_r, dv) <= 1e-8
    qo, vo = o.get_state()
    assert _rel(q1, qo) <= 1e-8 and _rel(v1, vo) <= 1e-8 and not q1[fixed].any() and not v1[fixed].any()
    # ... and the same system through the oracle's PCG: the iteration count of the oracle's own step
    info_r, dv_p = ref.pcg_iterations(keff_r, rhs_r, fixed, eps=1e-12, maxit=20000)
    assert abs(info_r - info) <= 1 and _rel(dv_p, dv) <= 1e-8


def test_three_materials_match_the_reference_sub_mesh_sums():
    g = np.load(os.path.join(GOLD, "fem_cube5_materials.npz"))
    v, t, _ = _cube(int(g["n"]))
    mats, ids = three_materials(), region_ids(v, t)
    assert np.array_equal(np.asarray(mats), g["materials"]) and np.array_equal(ids, g["ids"])
    assert np.bincount(ids).tolist() == [144, 144, 96]
    ref = MatRef(v, t, mats, ids)
    assert np.array_equal(ref.ia, g["ia"]) and np.array_equal(ref.ja, g["ja"])
    f, Kb = ref.assemble(g["u"])
    err = (_rel(f, g["f"]), _rel(ref.blocks_to_csr(Kb), g["K"]), _rel(ref.mass_csr_values(), g["M"]))
    print("restatement vs reference sub-mesh sums: f %.2e K %.2e M %.2e" % err)
    assert max(err) <= 1e-12, err
    # the split of a uniform mesh is the whole: the same element sums, whatever the ids say, when the materials are equal
    uni = MatRef(v, t, [mats[0]] * 3, ids)
    whole = OrcFem(v, t, E=mats[0][0], nu=mats[0][1], rho=mats[0][2])
    fo, Ko = whole.assemble(g["u"])
    fu, Ku = uni.assemble(g["u"])
    assert _rel(fu, fo) <= 1e-12 and _rel(uni.blocks_to_csr(Ku), Ko) <= 1e-12


# ---- readers ----
def _expected_fixture():
    v, t = truth_cube(3, 3, 3, 0.1)
    ids = np.zeros(len(t), np.uint8)
    ids[:12] = 1       # *SET lower -> tumour
    ids[8:47] = 0      # *SET upper -> tissue, the later region: elements 9..12 change hands
    ids[47] = 2        # in no region: the file's last material
    return v, t, [(1e7, 0.46, 1000.0), (5e7, 0.2, 800.0), (2.5e5, 0.3, 1200.0)], ids


def test_veg_material_reader_on_the_fixture():
    v, t, mats, ids = _expected_fixture()
    rv, rt, rm, rid = read_veg_materials(VEG)
    assert np.array_equal(rt, t) and np.abs(rv - v).max() == 0 and rm == mats and rid.dtype == np.uint8 and np.array_equal(rid, ids)
    pv, pt = read_veg(VEG)  # read_veg stays what it was: the mesh alone
    assert np.array_equal(pt, t) and np.array_equal(pv, rv)


def _write(tmp_path, name, tail, n=2):
    from fembrain_amd.poly import write_veg
    v, t = truth_cube(n, n, n, 0.1)
    p = str(tmp_path / name)
    write_veg(p, v, t)
    mesh = open(p).read()
    with open(p, "w") as f:   # (write_veg ends with a material and a region of its own: the mesh alone, then this case's tail)
        f.write(mesh[:mesh.index("*MATERIAL")] + tail)
    return p, len(t)


def test_veg_material_reader_sets_regions_and_defaults(tmp_path):
    p, ne = _write(tmp_path, "all.veg", "*MATERIAL a\nENU, 900, 2e6, 0.4\n*MATERIAL b\nENU, 1100, 3e6, 0.1\n*REGION\nallElements, b\n*SET s\n 1,\n 2 , 3\n*REGION\n s , a\n")
    _, _, m, ids = read_veg_materials(p)
    assert m == [(2e6, 0.4, 900.0), (3e6, 0.1, 1100.0)] and ids.tolist() == [0, 0, 0] + [1] * (ne - 3)
    p, ne = _write(tmp_path, "none.veg", "")
    _, _, m, ids = read_veg_materials(p)   # no material at all: VolumetricMesh's defaults (volumetricMesh.cpp:40-42), as intended there
    assert m == [(1e9, 0.45, 1000.0)] and not ids.any() and len(ids) == ne
    p, ne = _write(tmp_path, "last.veg", "*MATERIAL a\nENU, 900, 2e6, 0.4\n*MATERIAL b\nENU, 1100, 3e6, 0.1\n*SET s\n1\n*REGION\ns, a\n")
    _, _, m, ids = read_veg_materials(p)   # unassigned elements: the region of material numMaterials - 1
    assert ids.tolist() == [0] + [1] * (ne - 1)


BAD = {
    "mooney": "*MATERIAL m\nMOONEYRIVLIN, 1000, 1, 2, 3\n",
    "nu": "*MATERIAL m\nENU, 1000, 1e6, 0.5\n",
    "E": "*MATERIAL m\nENU, 1000, -1, 0.3\n",
    "rho": "*MATERIAL m\nENU, 0, 1e6, 0.3\n",
    "short": "*MATERIAL m\nENU, 1000, 1e6\n",
    "set_before": "*MATERIAL m\nENU, 1000, 1e6, 0.3\n*REGION\ns, m\n*SET s\n1\n",
    "material_before": "*SET s\n1\n*REGION\ns, m\n*MATERIAL m\nENU, 1000, 1e6, 0.3\n",
    "element_range": "*MATERIAL m\nENU, 1000, 1e6, 0.3\n*SET s\n1, 7\n*REGION\ns, m\n",
    "element_zero": "*MATERIAL m\nENU, 1000, 1e6, 0.3\n*SET s\n0\n*REGION\ns, m\n",
    "not_a_number": "*MATERIAL m\nENU, 1000, 1e6, 0.3\n*SET s\n1, x\n*REGION\ns, m\n",
    "region_shape": "*MATERIAL m\nENU, 1000, 1e6, 0.3\n*REGION\nallElements\n",
    "too_many": "".join("*MATERIAL m%d\nENU, 1000, 1e6, 0.3\n" % k for k in range(257)),
}


def _cpp_exe():
    exe = os.path.join(ROOT, "tests", "cpp", "materials_host")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "materials_host.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "fembrain_amd"), "-lfembrain_hip", "-Wl,-rpath," + os.path.join(ROOT, "fembrain_amd")])
    return exe


def _cpp_read(exe, path):
    r = subprocess.run([exe, "veg", path], capture_output=True, text=True)
    if r.returncode != 0:
        return None
    kv = dict(line.split("=", 1) for line in r.stdout.strip().splitlines())
    mats = []
    for k in range(int(kv["MATERIALS"])):
        _, E, nu, rho = kv["MATERIAL%d" % k].split()
        mats.append((float(E), float(nu), float(rho)))
    return mats, np.array(kv["IDS"].split(","), np.int64).astype(np.uint8)


def test_malformed_files_are_refused_by_both_readers_and_good_ones_agree(tmp_path):
    exe = _cpp_exe()
    for name, tail in BAD.items():
        p, _ = _write(tmp_path, name + ".veg", tail)   # a 2^3 cube: 6 elements
        with pytest.raises(ValueError):
            read_veg_materials(p)
        assert _cpp_read(exe, p) is None, name
    good = [VEG]
    good.append(_write(tmp_path, "g1.veg", "*MATERIAL a\nENU, 900, 2e6, 0.4\n*MATERIAL b\nENU, 1100, 3e6, 0.1\n*REGION\nallElements, b\n*SET s\n 1,\n 2 , 3\n*REGION\n s , a\n")[0])
    good.append(_write(tmp_path, "g2.veg", "")[0])
    good.append(_write(tmp_path, "g3.veg", "*MATERIAL a\nENU, 900, 2e6, 0.4\n*MATERIAL b\nENU, 1100, 3e6, 0.1\n*SET s\n1\n*REGION\ns, a\n")[0])
    for p in good:
        _, _, m, ids = read_veg_materials(p)
        cm, cids = _cpp_read(exe, p)
        assert cm == m and np.array_equal(cids, ids), p
