"""The run-ahead launch form of the persistent one-row kernel (fembrain_amd/csrc/pcg_pipe.hip.h: with a service wavefront, the totals are
handed over through LDS and every wavefront goes on to its recurrences and publish stores alone, without a barrier behind the sums)
against bits RECORDED from the form with that barrier.  The waits change, no addition does: kernel names, plan
statistics, iteration counts and the SHA-256 of every solution are the recorded ones.

A race between the wavefronts of a workgroup would show as an occasional mismatch, so the cases of tests/golden/pipe_onchip_bits.json that
take the new form are repeated in one process; the instantiations that file has no bits for -- (8, 8) and block-Jacobi -- have theirs
in tests/golden/pipe_runahead_bits.json (tests/golden/make_pipe_runahead_bits.py at the commit before), uncut and with the launches cut
into 1 and 7 iterations; and the 12-slice case, which keeps its barriers, runs once more here: both forms live in one library.

Every handle is confined to one XCD (FEMBRAIN_CU_MASK=0:32), as in tests/test_pipe_onchip_gpu.py.
"""
import importlib.util
import json
import os

import pytest

from fembrain_amd import lib as fl

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_GOLDEN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_onchip = _load("make_pipe_onchip_bits")
_maker = _load("make_pipe_runahead_bits")
with open(os.path.join(_GOLDEN, "pipe_onchip_bits.json")) as _f:
    _ONCHIP_BITS = json.load(_f)
with open(os.path.join(_GOLDEN, "pipe_runahead_bits.json")) as _f:
    _BITS = json.load(_f)

_KNOBS = ("FEMBRAIN_CU_MASK", "FEMBRAIN_SPMV_C16", "FEMBRAIN_PERSIST_MAX_RUN", "FEMBRAIN_PIPE_MIRROR")
# (case of pipe_onchip_bits.json, its kernel, slices of the fullest workgroup, wavefronts the kernel is built for)
_REPEATED = [("cube28_c16", "k_pcg_pipe<float,c16,12,6>", 11), ("cube26_c16", "k_pcg_pipe<float,c16,12,7>", 9)]


def _onchip_case(name):
    n, c16 = next((n, c16) for nm, n, c16, _, _ in _onchip.CASES if nm == name)
    want = _ONCHIP_BITS[name]
    assert (n, c16) == (want["n"], want["c16"])
    return n, c16, want


def test_the_recorded_cases_are_the_issue_s():
    """(no GPU needed, but the file is read by the GPU cases only) the recording shows the two instantiations with a wavefront to spare,
    and cuts of the launches that agree with the uncut solve at the recorded commit"""
    assert sorted(_BITS) == ["cube14_c16", "cube28_bj"]
    small, bj = _BITS["cube14_c16"], _BITS["cube28_bj"]
    assert small["kernel"] == _maker.KERNEL88 and small["persist_info"][:3] == [True, 2, 32] and small["persist_info"][1] < 8
    assert bj["kernel"] == _maker.KERNEL_BJ and bj["persist_info"][:3] == [True, 11, 32] and bj["persist_info"][1] < 12
    for rec in (small, bj):
        assert rec["path"] == fl.FB_PCG_PATH_PERSISTENT and rec["fallbacks"] == 0 and rec["iterations"] > 100
        assert sorted(rec["runs"]) == ["1", "7"]
        for run in rec["runs"].values():
            assert run == dict(iterations=rec["iterations"], x_sha256=rec["x_sha256"])
    for name, kernel, waves in _REPEATED:  # fewer slices than the 12 wavefronts: the service wavefront, so the run-ahead form
        assert _ONCHIP_BITS[name]["kernel"] == kernel and _ONCHIP_BITS[name]["persist_info"][:3] == [True, waves, 32]
    assert _ONCHIP_BITS["cube29_c16"]["persist_info"][:3] == [True, 12, 32]


@pytest.mark.parametrize("name", [r[0] for r in _REPEATED])
def test_run_ahead_repeats_the_recorded_bits(gpu, monkeypatch, name):
    """three solves on three handles in one process: every one the recorded iteration count and solution"""
    n, c16, want = _onchip_case(name)
    for knob in _KNOBS:
        monkeypatch.delenv(knob, raising=False)
    for rep in range(3):
        got = _onchip.run_case(n, c16, (), 0)
        assert got["kernel"] == want["kernel"] and got["path"] == fl.FB_PCG_PATH_PERSISTENT and got["fallbacks"] == 0, rep
        assert got["persist_info"] == want["persist_info"] and got["persist_mirror"] == want["persist_mirror"], rep
        assert (got["iterations"], got["x_sha256"]) == (want["iterations"], want["x_sha256"]), rep


@pytest.mark.parametrize("name", ["cube14_c16", "cube28_bj"])
def test_run_ahead_in_the_other_instantiations(gpu, monkeypatch, name):
    """(8, 8) and block-Jacobi: kernel, plan and bits as recorded, uncut and with launches of 1 and 7 iterations"""
    want = _BITS[name]
    for knob in _KNOBS:
        monkeypatch.delenv(knob, raising=False)
    got = _maker.run_case(want["n"], want["bj"])
    assert got["kernel"] == want["kernel"] == (_maker.KERNEL_BJ if want["bj"] else _maker.KERNEL88)
    assert got["path"] == fl.FB_PCG_PATH_PERSISTENT and got["fallbacks"] == 0
    assert got["persist_info"] == want["persist_info"]
    assert (got["iterations"], got["x_sha256"]) == (want["iterations"], want["x_sha256"])
    assert got["runs"] == want["runs"] and sorted(got["runs"]) == ["1", "7"]


def test_the_form_with_barriers_keeps_its_bits(gpu, monkeypatch):
    """12 slices per workgroup, no spare wavefront: the same library's other launch form"""
    n, c16, want = _onchip_case("cube29_c16")
    for knob in _KNOBS:
        monkeypatch.delenv(knob, raising=False)
    got = _onchip.run_case(n, c16, (), 0)
    assert got["kernel"] == want["kernel"] == "k_pcg_pipe<float,c16,12,6>" and got["path"] == fl.FB_PCG_PATH_PERSISTENT and got["fallbacks"] == 0
    assert got["persist_info"] == want["persist_info"] and got["persist_mirror"] == want["persist_mirror"]
    assert (got["iterations"], got["x_sha256"]) == (want["iterations"], want["x_sha256"])
