"""bench.py contract: JSON output shape, and the torchrun multi-rank flow
(2 CPU ranks over gloo exercising the same allgather/reduce path the driver's
multi-GPU scale run uses)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse_json_line(stdout: str) -> dict:
    for line in reversed(stdout.strip().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError(f"no JSON line in output:\n{stdout[-2000:]}")


REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
            "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"]


@pytest.mark.timeout(600)
def test_bench_cpu_single():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu",
                        "--steps", "2", "--warmup", "1", "--pop-per-gpu", "4",
                        "--max-steps", "20", "--env", "Hopper-v3", "--layers", "8",
                        "--tbl-size", "200000"],
                       capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    out = _parse_json_line(r.stdout)
    for k in REQUIRED:
        assert k in out, k
    assert out["value"] > 0 and out["scaling"] == "weak"
    assert out["config"]["global_batch"] == 4
    # encoding transparency: the perturbation format is always reported
    assert out["config"]["eps_encoding"] in ("bf16", "e4m3")


@pytest.mark.timeout(600)
def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's arrays as fp32/fp64 .npy,
    and two runs with the same arguments see identical inputs (fresh
    processes, so a per-process-salted seed anywhere would show up here)."""
    import numpy as np
    dumps = []
    for name in ("a", "b"):
        d = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu",
                            "--steps", "2", "--warmup", "1", "--pop-per-gpu", "4",
                            "--max-steps", "20", "--env", "Hopper-v3", "--layers", "8",
                            "--tbl-size", "200000", "--full",
                            "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, PYTHONPATH=ROOT))
        assert r.returncode == 0, r.stderr[-2000:]
        out = _parse_json_line(r.stdout)
        assert out["steps"] == 2 and out["ms_per_step"] > 0
        assert "last_step_timings" in out["config"]  # --full extra
        dumps.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = dumps
    assert {"fits_pos", "fits_neg", "noise_inds", "ranked_fits",
            "flat_params"} <= set(a) and set(a) == set(b)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), (k, a[k].dtype)
        assert np.isfinite(a[k]).all(), k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["fits_pos"].shape == (2, 1) and a["flat_params"].ndim == 1


@pytest.mark.timeout(600)
def test_bench_torchrun_world2_cpu():
    """The exact launcher shape the driver uses, world_size=2 on CPU/gloo."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", "2", "--standalone", "--local-addr", "127.0.0.1",
           os.path.join(ROOT, "bench.py"), "--cpu",
           "--gpus", "2", "--steps", "2", "--warmup", "1", "--pop-per-gpu", "4",
           "--max-steps", "20", "--env", "Hopper-v3", "--layers", "8",
           "--tbl-size", "200000"]
    # gloo named explicitly: on a machine with a visible GPU the default
    # transport is RCCL, which rejects two ranks sharing one device
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420,
                       env=dict(os.environ, PYTHONPATH=ROOT, ES_COMM_BACKEND="gloo"))
    assert r.returncode == 0, r.stderr[-3000:]
    out = _parse_json_line(r.stdout)
    assert out["n_gpus"] == 2
    assert out["config"]["global_batch"] == 8  # weak scaling: 4 per rank
    # whole-job env steps: 2 ranks x (8+1 noiseless... counted: 8 members) x 20 x 2 gens
    assert out["value"] > 0
