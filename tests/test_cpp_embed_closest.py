"""PS::FEM::EmbeddedMesh::searchInfo (include/fembrain/EmbeddedMesh.h): the header compiles with a plain C++11 compiler (no GPU), and on the
GPU a C++ host program (tests/cpp/embed_closest_host.cpp) binds an enclosing surface through the centre grid and reports what the
search did."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "embed_closest_host")


def test_search_info_compiles_with_a_plain_compiler(tmp_path):
    src = tmp_path / "search_info.cpp"
    src.write_text('#include "fembrain/EmbeddedMesh.h"\n'
                   "long long tested(const PS::FEM::EmbeddedMesh& m) {\n"
                   "  const fb_fem_embed_search_info si = m.searchInfo();\n"
                   "  return si.path == FB_EMBED_CLOSEST_RING ? si.centres_tested : (long long)si.n_outside + si.n_far + si.centre_grid_builds + si.max_centres_one_point;\n"
                   "}\n"
                   "int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


@pytest.mark.gpu
def test_an_enclosing_surface_from_cpp(gpu):
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "embed_closest_host.cpp"),
           "-o", EXE, "-L", os.path.join(ROOT, "fembrain_amd"), "-lfembrain_hip", "-Wl,-rpath," + os.path.join(ROOT, "fembrain_amd")]
    subprocess.check_call(cmd)
    out = subprocess.check_output([EXE], text=True, timeout=300)  # (the program asks for the ring and a budget no point reaches)
    kv = dict(line.split(" =", 1) for line in out.strip().splitlines() if " =" in line)
    assert kv.get("embed_closest_host", "").strip() == "ok", out[-2000:]
    n_tets, n_points = int(kv["n_tets"]), int(kv["n_points"])
    path, n_outside, n_far, builds, most, tested = (int(x) for x in kv["search"].split())
    assert n_points == int(kv["n_external"]) == n_outside == 24 * 16 and builds == 1
    assert path == 2 and n_far == 0 and 0 < most and tested < n_outside * n_tets // 4, "a small part of what a scan tests"
