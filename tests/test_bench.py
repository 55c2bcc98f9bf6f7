"""bench.py's --dump-outputs: what the timed path returned in its last step, as float64 .npy files of bounded size,
and a plain run (no --full) that prints the result line without the CPU baseline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from oracle import gp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP_LIMIT = 64 * 10 ** 6   # bytes, all files together
FIT_NAMES = ["L_sample", "alpha", "info", "jitter", "logdet", "mll", "quad"]


def _fake_step(T, N, D, with_grad):
    o = dict(L=torch.randn(T, N, N, dtype=torch.float64), alpha=torch.randn(T, N, dtype=torch.float64),
             info=torch.zeros(T, dtype=torch.int32), Linv_diag=torch.randn(T, (N + 15) // 16, 16, 16, dtype=torch.float64) if with_grad else None,
             **{k: torch.randn(T, dtype=torch.float64) for k in ("quad", "logdet", "mll", "jitter")})
    return o, (torch.randn(T, D + 2, dtype=torch.float64) if with_grad else None)


@pytest.mark.parametrize("with_grad", [False, True], ids=["fit", "fit+grad"])
def test_dump_outputs_format_and_size(tmp_path, with_grad):
    T, N, D = bench.T_PER_GPU, bench.N_POINTS, bench.DIM
    o, g = _fake_step(T, N, D, with_grad)
    bench.dump_outputs(str(tmp_path), o, g)
    names = FIT_NAMES + (["Linv_diag_sample", "grad"] if with_grad else [])
    assert sorted(p[:-4] for p in os.listdir(tmp_path)) == sorted(names)
    assert sum(os.path.getsize(tmp_path / p) for p in os.listdir(tmp_path)) <= DUMP_LIMIT
    idx = bench.dump_tasks(T)
    np.testing.assert_array_equal(idx, bench.dump_tasks(T))   # fixed sample
    assert len(set(idx.tolist())) == bench.DUMP_L_TASKS and list(idx) == sorted(idx)
    arrays = {n: np.load(tmp_path / (n + ".npy")) for n in names}
    assert all(a.dtype == np.float64 for a in arrays.values())
    np.testing.assert_array_equal(arrays["L_sample"], o["L"][idx].numpy())
    np.testing.assert_array_equal(arrays["info"], o["info"].numpy().astype(np.float64))
    for k in ("alpha", "mll", "quad", "logdet", "jitter"):
        np.testing.assert_array_equal(arrays[k], o[k].numpy())
    if with_grad:
        np.testing.assert_array_equal(arrays["Linv_diag_sample"], o["Linv_diag"][idx].numpy())
        np.testing.assert_array_equal(arrays["grad"], g.numpy())


@pytest.mark.gpu
def test_plain_bench_run_dumps_last_step(device, tmp_path):
    """A plain run times exactly --steps steps, leaves the CPU baseline out and dumps the last step's fit, which matches
    the oracle on the sampled tasks (north-star tolerances) and sums to the MLL the timed region reduced."""
    dump = tmp_path / "out"
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.join(ROOT, "bench.py"),
           "--gpus", "1", "--steps", "3", "--warmup", "1", "--prewarm", "10", "--dump-outputs", str(dump)]
    res = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and "cpu_baseline" not in line
    assert sorted(p[:-4] for p in os.listdir(dump)) == sorted(FIT_NAMES)
    assert sum(os.path.getsize(dump / p) for p in os.listdir(dump)) <= DUMP_LIMIT
    got = {n: torch.from_numpy(np.load(dump / (n + ".npy"))) for n in FIT_NAMES}
    assert not got["info"].any()
    np.testing.assert_allclose(float(got["mll"].sum()), line["config"]["reduced_mll_sum_last_step"], rtol=1e-12)
    (X, y, th), _ = bench.make_inputs(0, torch.device("cpu"))
    idx = torch.from_numpy(bench.dump_tasks(X.shape[0]))[:4]
    ref_g = O.gp_fit_stack_loop(X[idx], y[idx], th[idx], O.KIND_MATERN52, dist="gpytorch")   # the reference's formulation
    ref_d = O.gp_fit_stack_loop(X[idx], y[idx], th[idx], O.KIND_MATERN52, dist="direct")     # the kernel's formulation
    assert _rel(got["mll"][idx], ref_g["mll"]) < 1e-3
    assert _rel(got["alpha"][idx], ref_g["alpha"]) < 1e-4
    assert _rel(got["L_sample"][:4], ref_d["L"]) < 1e-9


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
