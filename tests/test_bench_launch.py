"""`python bench.py --gpus N` without a launcher: the script starts its own ranks as CHILD processes -- the parent
never touches torch or HIP -- relays rank 0's ONE JSON line and leaves with the launcher's exit code."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lines(text):
    return [json.loads(x) for x in text.splitlines() if x.lstrip().startswith("{") and '"metric"' in x]


def test_self_launch_without_a_gpu_still_prints_one_line_and_fails():
    """no device in this container: every rank leaves at once ("needs an MI355X"); the parent must come back non-zero with ONE parsable
    line that says so -- and must not have imported torch itself (FEMBRAIN_BENCH_PARENT_TRACE lists the parent's modules at exit)"""
    try:
        from fembrain_amd import lib
        if lib.lib().fb_device_count() > 0:
            pytest.skip("a HIP device is visible: the GPU variant of this test runs instead")
    except Exception:
        pass
    env = dict(os.environ, FEMBRAIN_BENCH_PARENT_TRACE="1")
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], capture_output=True, text=True,
                         timeout=300, env=env, cwd=ROOT)
    assert out.returncode != 0
    recs = _lines(out.stdout)
    assert len(recs) == 1 and recs[0]["value"] is None and recs[0]["n_gpus"] == 2 and "error" in recs[0], out.stdout[-2000:]
    assert "torch.distributed.run" in recs[0]["launched"] and "--nproc-per-node 2" in recs[0]["launched"]
    assert "parent modules: torch=False" in out.stderr, out.stderr[-2000:]


@pytest.mark.gpu
def test_bench_gpus_2_runs_from_a_plain_python_command_on_the_one_gpu_box(gpu):
    """the command form the driver uses for N = 1, with --gpus 2 and --full: both ranks on device 0 through the host-staged communicator
    (FEMBRAIN_BENCH_LOCAL_COMM=1; RCCL refuses two ranks on one device).  One JSON line, rc 0, the sharded self-check passed, the
    collective-library leg and the 8M-tet `scaling_8m` block present.  Timings of this mode are meaningless; the control flow is the point."""
    env = dict(os.environ, FEMBRAIN_BENCH_LOCAL_COMM="1", FEMBRAIN_BENCH_8M_STEPS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full"], capture_output=True,
                         text=True, timeout=900, env=env, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    recs = _lines(out.stdout)
    assert len(recs) == 1, out.stdout[-3000:]
    d = recs[0]
    assert d["n_gpus"] == 2 and d["value"] > 0 and d.get("error") is None
    assert d["config"]["sharded_self_check"]["ok"]
    assert d["config"]["communicator"]["ranks"] == 2 and d["config"]["rccl_ranks"] == 0      # (the rehearsal's transport is not RCCL, and says so)
    leg = d["config"]["collective_library_leg"]
    assert leg["collective"]["cg_iterations"] == leg["as_timed"]["cg_iterations"] > 0
    assert "collective" in d["config"]["exchange_trials_ms_per_step"]
    s8 = d["scaling_8m"]
    assert s8["n_gpus"] == 2 and s8["steps_per_s"] > 0 and len(s8["us_per_cg_iteration_per_rank"]) == 2 and s8["n1_steps_per_s_committed"] > 0


def test_dump_outputs_writes_float64_and_samples_long_vectors_the_same_way(tmp_path):
    """bench.py --dump-outputs: short arrays whole; arrays above the cap replaced by ONE seeded sample of positions (the same for
    every array and every run, written beside them), so that a dump stays below 64 MB at every workload"""
    import bench
    n = bench.DUMP_MAX_VALUES + 12345
    q = np.arange(n, dtype=np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"q": q, "qvel": -q, "cg_iterations": [17]})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["cg_iterations.npy", "q.npy", "qvel.npy", "sample_index.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    qa, qv = np.load(tmp_path / "a" / "q.npy"), np.load(tmp_path / "a" / "qvel.npy")
    assert qa.dtype == qv.dtype == idx.dtype == np.float64 and len(qa) == len(idx) == bench.DUMP_MAX_VALUES
    assert np.array_equal(qa, idx) and np.array_equal(qv, -idx) and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "cg_iterations.npy"), [17.0])
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    bench.dump_outputs(str(tmp_path / "c"), {"q": q[:1000]})
    assert os.listdir(tmp_path / "c") == ["q.npy"] and np.array_equal(np.load(tmp_path / "c" / "q.npy"), q[:1000])


@pytest.mark.gpu
def test_plain_bench_times_exactly_the_steps_asked_for_and_dumps_the_last_state(gpu, tmp_path):
    """the plain one-GPU form: the headline keys, --steps timed steps and nothing measured beside them (no --full); --dump-outputs
    leaves the state of the last timed step, whole at 1M tets"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs",
                          str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    recs = _lines(out.stdout)
    assert len(recs) == 1, out.stdout[-3000:]
    d = recs[0]
    assert d["metric"] == "FEM steps/sec (assemble+PCG) at 1M tets" and d["unit"] == "steps/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64 arithmetic / f32 stored matrix" and d.get("error") is None
    assert d["steps"] == 3 and len(d["cg_iterations"]) == 3 and abs(d["ms_per_step"] * d["value"] - 1e3) < 1e-6 * 1e3
    for key in ("roofline", "value_at_fixed_state", "cpu_baseline", "field_mvoxels_per_s", "cube27", "cube111"):
        assert key not in d, key
    r = 3 * d["config"]["nodes"]
    for name in ("q", "qvel", "qaccel"):
        a = np.load(tmp_path / (name + ".npy"))
        assert a.dtype == np.float64 and a.shape == (r,) and np.all(np.isfinite(a)), name
    q = np.load(tmp_path / "q.npy")
    assert q[1::3].min() < 0 and np.abs(q).max() > 0          # loaded in -y
    assert np.array_equal(np.load(tmp_path / "cg_iterations.npy"), [float(d["cg_iterations"][-1])])
    assert not os.path.exists(tmp_path / "sample_index.npy")
