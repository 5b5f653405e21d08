"""Wavefront priority through the product of the persistent register-slot kernels (fembrain_amd/csrc/pcg_pipe.hip.h, "Priority 0 before every
wait"; FEMBRAIN_PIPE_PRIO = 0 off, 1 by progress, 2 static, 3 by progress + the service wavefront) against the bits ALREADY recorded in
tests/golden/pipe_onchip_bits.json: a priority changes when an instruction is issued and never what it computes, so under every value of the
knob, and without it, the kernel name, the iteration counts and the SHA-256 of every solution are the recorded ones.

One XCD (FEMBRAIN_CU_MASK=0:32), a fresh handle per case and setting:
  cube28_c16  (12, 6), 10 and 11 slices per workgroup; three steps with re-assembly, and launches cut into 1 and 7 iterations (every launch
              begins and ends at priority 0: a cut launch takes the exits)
  cube28_c32  32-bit columns
  cube26_c16  (12, 7)
  cut_c16     ragged widths: slices without a streamed front part or without register layers behind the window -- the steps fall through
              empty regions
  cube29_c16  12 slices per workgroup: no service wavefront, the kernel with its barriers has no priority form -- whatever the knob says
and a solve that the iteration cap ends (the early exit), against what the kernel without priorities leaves.
"""
import functools
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

_KNOBS = ("FEMBRAIN_CU_MASK", "FEMBRAIN_SPMV_C16", "FEMBRAIN_PERSIST_MAX_RUN", "FEMBRAIN_PIPE_MIRROR", "FEMBRAIN_PIPE_REGS", "FEMBRAIN_PIPE_PRIO",
          "FEMBRAIN_PERSIST_TIMING")
_DEFAULT_FORM = 1  # what profiles/r10_prio_ab_cube56.txt decided
_SETTINGS = [None, 0, 1, 2, 3]


def _clear(monkeypatch):
    for knob in _KNOBS:
        monkeypatch.delenv(knob, raising=False)


def _handle(want, prio, regs=None):
    """A fresh handle of the recorded case made under FEMBRAIN_PIPE_PRIO=prio and FEMBRAIN_PIPE_REGS=regs (None: not set)"""
    env = os.environ
    if prio is not None:
        env["FEMBRAIN_PIPE_PRIO"] = str(prio)
    if regs is not None:
        env["FEMBRAIN_PIPE_REGS"] = str(regs)
    try:
        return _maker.make_handle(want["n"], want["c16"], want["cut"], env)
    finally:
        env.pop("FEMBRAIN_PIPE_PRIO", None)
        env.pop("FEMBRAIN_PIPE_REGS", None)


def _run(want, prio, runs=(), steps=0):
    """What run_case records, and persist_prio()"""
    env = os.environ
    g = _handle(want, prio)
    try:
        g.set_uniform_force(1, -10000.0)
        _, rhs = g.system()
        it, x = g.pcg(rhs, eps=1e-6, max_iter=20000)
        path = g.pcg_path()
        got = dict(kernel=path["kernel"], path=path["path"], iterations=it, x_sha256=_maker._sha(x), persist_info=list(g.persist_info()),
                   persist_mirror=list(g.persist_mirror()), persist_regs=g.persist_regs(), persist_prio=g.persist_prio(), runs={}, steps=[])
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
    print("kernel %s prio %d iterations %d (recorded %d) x %s" % (got["kernel"], got["persist_prio"], got["iterations"], want["iterations"], got["x_sha256"][:16]))
    assert got["kernel"] == want["kernel"] and got["path"] == fl.FB_PCG_PATH_PERSISTENT and got["fallbacks"] == 0
    assert got["persist_info"] == want["persist_info"] and got["persist_mirror"] == want["persist_mirror"]
    assert got["iterations"] == want["iterations"] and got["x_sha256"] == want["x_sha256"]


@pytest.mark.parametrize("prio", _SETTINGS)
@pytest.mark.parametrize("name", ["cube28_c16", "cube28_c32", "cube26_c16", "cut_c16"])
def test_priority_forms_keep_the_recorded_bits(gpu, monkeypatch, name, prio):
    _clear(monkeypatch)
    want = _BITS[name]
    first = name == "cube28_c16"
    got = _run(want, prio, runs=(1, 7) if first else (), steps=3 if first else 0)
    _same_bits(got, want)
    assert got["persist_regs"][0] == 3  # the kernels that have the form
    assert got["persist_prio"] == (_DEFAULT_FORM if prio is None else prio)
    if first:
        assert got["runs"] == {k: want["runs"][k] for k in ("1", "7")} and got["steps"] == want["steps"]


@pytest.mark.parametrize("prio", _SETTINGS)
def test_no_service_wavefront_no_priority_form(gpu, monkeypatch, prio):
    """12 slices per workgroup: the kernel with its barriers, the parent's code -- persist_prio() is 0 whatever the knob says"""
    _clear(monkeypatch)
    want = _BITS["cube29_c16"]
    got = _run(want, prio)
    _same_bits(got, want)
    assert got["persist_prio"] == 0 and got["persist_regs"] == (0, 0)


def test_default_form(gpu, monkeypatch):
    """FEMBRAIN_PIPE_PRIO not set: the form the measurement chose; without register slots (FEMBRAIN_PIPE_REGS=0) the kernel has none"""
    _clear(monkeypatch)
    g = _handle(_BITS["cube26_c16"], None)
    try:
        assert g.persist_prio() == _DEFAULT_FORM and g.persist_regs()[0] == 3
    finally:
        g.close()
    g = _handle(_BITS["cube26_c16"], 1, regs=0)
    try:
        assert g.persist_prio() == 0 and g.persist_regs() == (0, 0)
    finally:
        g.close()


_CAP = 100  # iterations: far below the 992 the solve needs


@functools.lru_cache(maxsize=None)
def _capped(prio):
    """A solve the iteration cap ends, then a full one on the same handle: (iterations, solution, fallbacks) of each"""
    want = _BITS["cube26_c16"]
    g = _handle(want, prio)
    try:
        form = g.persist_prio()
        g.set_uniform_force(1, -10000.0)
        _, rhs = g.system()
        it, x = g.pcg(rhs, eps=1e-6, max_iter=_CAP)
        cut = (it, _maker._sha(x), g.pcg_path()["fallbacks"])
        it2, x2 = g.pcg(rhs, eps=1e-6, max_iter=20000)
        full = (it2, _maker._sha(x2), g.pcg_path()["fallbacks"])
    finally:
        g.close()
    return form, cut, full


@pytest.mark.parametrize("prio", [1, 2, 3])
def test_iteration_cap_leaves_what_the_kernel_without_priorities_leaves(gpu, monkeypatch, prio):
    """cg_maxiter below convergence: the launch leaves its loop from inside an iteration; it returns, reports what the unprioritised kernel
    reports, and the next solve on the handle has the recorded bits"""
    _clear(monkeypatch)
    want = _BITS["cube26_c16"]
    form0, cut0, full0 = _capped(0)
    form, cut, full = _capped(prio)
    print("cap %d: prio 0 -> %s, prio %d -> %s; next solve %s" % (_CAP, cut0, prio, cut, full))
    assert form0 == 0 and form == prio
    assert cut == cut0
    assert full == full0 and full[0] == want["iterations"] and full[1] == want["x_sha256"]
