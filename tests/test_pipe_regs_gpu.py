"""Register slots of the persistent run-ahead LDS-window kernels (fembrain_amd/csrc/pcg_pipe_regs.hip.h: up to three streamed slots of a slice,
those next to its LDS window, keep their values in registers for a launch) against the bits ALREADY recorded in
tests/golden/pipe_onchip_bits.json: where a slot's values come from changes, the order of the additions does not, so under
FEMBRAIN_PIPE_REGS = 0, 2 and 3 alike the kernel name, iteration counts and the SHA-256 of every solution are the recorded ones.

One XCD (FEMBRAIN_CU_MASK=0:32), a fresh handle per case and setting:
  cube28_c16  (12, 6), 10 and 11 slices per workgroup; three steps with re-assembly (registers filled from a stale matrix would show), and
              launches cut into 1 and 7 iterations (the registers are filled again by every launch)
  cube28_c32  32-bit columns
  cube26_c16  (12, 7)
  cut_c16     ragged widths: slices that stream fewer slots than the setting, register slots on both sides of the window
  cube29_c16  12 slices per workgroup: no service wavefront, so the kernel with its barriers and no register slots -- whatever the knob says
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

_KNOBS = ("FEMBRAIN_CU_MASK", "FEMBRAIN_SPMV_C16", "FEMBRAIN_PERSIST_MAX_RUN", "FEMBRAIN_PIPE_MIRROR", "FEMBRAIN_PIPE_REGS")


def _run(want, regs, runs=(), steps=0):
    """The recorded case on a fresh handle made under FEMBRAIN_PIPE_REGS=regs (None: not set): what run_case records, and persist_regs()"""
    env = os.environ
    if regs is not None:
        env["FEMBRAIN_PIPE_REGS"] = str(regs)
    try:
        g = _maker.make_handle(want["n"], want["c16"], want["cut"], env)
    finally:
        env.pop("FEMBRAIN_PIPE_REGS", None)
    try:
        g.set_uniform_force(1, -10000.0)
        _, rhs = g.system()
        it, x = g.pcg(rhs, eps=1e-6, max_iter=20000)
        path = g.pcg_path()
        got = dict(kernel=path["kernel"], path=path["path"], iterations=it, x_sha256=_maker._sha(x), persist_info=list(g.persist_info()),
                   persist_mirror=list(g.persist_mirror()), persist_regs=g.persist_regs(), runs={}, steps=[])
        for run in runs:
            env["FEMBRAIN_PERSIST_MAX_RUN"] = str(run)
            try:
                itc, xc = g.pcg(rhs, eps=1e-6, max_iter=20000)
            finally:
                env.pop("FEMBRAIN_PERSIST_MAX_RUN", None)
            got["runs"][str(run)] = dict(iterations=itc, x_sha256=_maker._sha(xc))
        for _ in range(steps):
            its = g.do_timestep()
            got["steps"].append(dict(iterations=its, q_sha256=_maker._sha(g.get_q_state()[0])))
        got["fallbacks"] = g.pcg_path()["fallbacks"]
    finally:
        g.close()
    return got


def _same_bits(got, want):
    assert got["kernel"] == want["kernel"] and got["path"] == fl.FB_PCG_PATH_PERSISTENT and got["fallbacks"] == 0
    assert got["persist_info"] == want["persist_info"] and got["persist_mirror"] == want["persist_mirror"]  # (reported as before)
    assert got["iterations"] == want["iterations"] and got["x_sha256"] == want["x_sha256"]


@pytest.mark.parametrize("regs", [0, 2, 3])
@pytest.mark.parametrize("name", ["cube28_c16", "cube28_c32", "cube26_c16", "cut_c16"])
def test_register_slots_keep_the_recorded_bits(gpu, monkeypatch, name, regs):
    want = _BITS[name]
    for knob in _KNOBS:
        monkeypatch.delenv(knob, raising=False)
    first = name == "cube28_c16"
    got = _run(want, regs, runs=(1, 7) if first else (), steps=3 if first else 0)
    _same_bits(got, want)
    per_slice, total = got["persist_regs"]
    assert per_slice == regs and (total > 0) == (regs > 0)
    if regs > 0:
        slices = -(-(want["n"] + 1) ** 3 // 64) if want["cut"] is None else None
        assert slices is None or regs * slices // 2 < total <= regs * slices  # most slices stream that many slots
    if first:
        assert got["runs"] == {k: want["runs"][k] for k in ("1", "7")} and got["steps"] == want["steps"]


def test_default_is_three_register_slots(gpu, monkeypatch):
    for knob in _KNOBS:
        monkeypatch.delenv(knob, raising=False)
    want = _BITS["cube26_c16"]
    got = _run(want, None)
    _same_bits(got, want)
    assert got["persist_regs"][0] == 3 and got["persist_regs"][1] > 0


def test_no_service_wavefront_no_register_slots(gpu, monkeypatch):
    """12 slices per workgroup: the launch has no service wavefront, its kernel keeps its barriers and holds nothing in registers; slices of
    width 8 have nothing left to stream"""
    for knob in _KNOBS:
        monkeypatch.delenv(knob, raising=False)
    want = _BITS["cube29_c16"]
    got = _run(want, None)
    _same_bits(got, want)
    assert got["persist_regs"] == (0, 0)
