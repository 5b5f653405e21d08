"""The on-chip run of the persistent one-row kernels with an LDS window (fembrain_amd/csrc/pcg_pipe_onchip.hip.h: mirror layers, then the
plain LDS layers of a wavefront, hand-scheduled with the gathers four slots ahead) against bits RECORDED from the C++ loops it replaced
(tests/golden/pipe_onchip_bits.json, written by tests/golden/make_pipe_onchip_bits.py at the commit before).  The schedule changes, the order
of the additions does not: kernel name, window statistics, iteration counts and the SHA-256 of every solution are the recorded ones.

Every handle is confined to one XCD (FEMBRAIN_CU_MASK=0:32): 32 workgroups, so ~20k nodes are 9..12 slices per workgroup -- the
12-wavefront kernels at a size that solves in a second.  What the cases cover (host model fb_plan_mirror_model, 32 workgroups):
  cube28_c16  (12, 6), 10 and 11 slices per workgroup (service wavefront), 2.38 mirror layers per slice; launches cut into 1 / 7 / 30
              iterations; three reference-load steps
  cube28_c32  32-bit columns: the 384-byte mirror table, 1.89 layers per slice
  cube26_c16  (12, 7), 9 per workgroup; one workgroup keeps no mirrors (plain and mirror layouts in one launch)
  cube29_c16 / cube29_c32  12 per workgroup (no spare wavefront), slices of width 8 (the window clipped by the slice: runs shorter than the
              pipeline); c32: only some workgroups keep mirrors
  cut_c16     a cube after synthetic_cut(stride=3) + resync_delta: ragged widths, windows that differ from slice to slice, padding lanes
"""
import importlib.util
import json
import os

import pytest

from fembrain_amd import lib as fl

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_pipe_onchip_bits", os.path.join(_GOLDEN, "make_pipe_onchip_bits.py"))
_maker = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_maker)
with open(os.path.join(_GOLDEN, "pipe_onchip_bits.json")) as _f:
    _BITS = json.load(_f)

_CASES = {name: (n, c16, runs, steps) for name, n, c16, runs, steps in _maker.CASES}
_KERNELS = {"cube28_c16": "k_pcg_pipe<float,c16,12,6>", "cube28_c32": "k_pcg_pipe<float,c32,12,6>", "cube26_c16": "k_pcg_pipe<float,c16,12,7>",
            "cube29_c16": "k_pcg_pipe<float,c16,12,6>", "cube29_c32": "k_pcg_pipe<float,c32,12,6>"}


def test_the_recorded_cases_are_the_issue_s():
    """(no GPU needed, but the file is read by the GPU cases only) what the recording itself must show: the kernels, slices per workgroup
    and a window with mirror layers in every case, and cuts of the launches that agree with the uncut solve at the recorded commit"""
    assert set(_BITS) == set(_CASES) | {"cut_c16"}
    waves = {"cube28_c16": 11, "cube28_c32": 11, "cube26_c16": 9, "cube29_c16": 12, "cube29_c32": 12}
    for name, kernel in _KERNELS.items():
        rec = _BITS[name]
        assert rec["kernel"] == kernel and rec["path"] == fl.FB_PCG_PATH_PERSISTENT and rec["fallbacks"] == 0, name
        assert rec["persist_info"][:3] == [True, waves[name], 32] and rec["persist_mirror"][0] and rec["persist_mirror"][1] > 0, name
        assert rec["iterations"] > 100, name
    first = _BITS["cube28_c16"]
    assert sorted(first["runs"]) == ["1", "30", "7"] and len(first["steps"]) == 3
    for run in first["runs"].values():
        assert run == dict(iterations=first["iterations"], x_sha256=first["x_sha256"])
    cut = _BITS["cut_c16"]
    assert cut["kernel"].startswith("k_pcg_pipe<float,c16,12,") and cut["cut"] is not None and cut["persist_mirror"][0]


@pytest.mark.parametrize("name", sorted(_CASES) + ["cut_c16"])
def test_on_chip_run_gives_the_recorded_bits(gpu, monkeypatch, name):
    want = _BITS[name]
    if name == "cut_c16":
        n, c16, runs, steps = want["n"], want["c16"], (), 0
    else:
        n, c16, runs, steps = _CASES[name]
        assert (n, c16) == (want["n"], want["c16"])
    for knob in ("FEMBRAIN_CU_MASK", "FEMBRAIN_SPMV_C16", "FEMBRAIN_PERSIST_MAX_RUN", "FEMBRAIN_PIPE_MIRROR"):
        monkeypatch.delenv(knob, raising=False)
    got = _maker.run_case(n, c16, runs, steps, cut=want["cut"])
    assert got["kernel"] == want["kernel"] and got["kernel"].startswith("k_pcg_pipe<float,%s,12," % ("c16" if c16 else "c32"))
    assert got["path"] == fl.FB_PCG_PATH_PERSISTENT and got["fallbacks"] == 0
    assert got["persist_info"] == want["persist_info"] and got["persist_mirror"] == want["persist_mirror"]
    assert got["iterations"] == want["iterations"] and got["x_sha256"] == want["x_sha256"]
    assert got["runs"] == want["runs"] and got["steps"] == want["steps"]
