"""bench.py's command line: --steps, the result line, --dump-outputs, --full.

The benchmark runs on the CPU here (GPUs hidden from the child processes)
at batch size 2 (batch norm needs more than one example): the checks are
about what the run writes and prints, not about speed.
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STEPS = 2
WARMUP = 1
BATCH = 2


def _launch(dump_dir, *extra):
  env = dict(os.environ)
  env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
  env["HIP_VISIBLE_DEVICES"] = ""
  env["CUDA_VISIBLE_DEVICES"] = ""
  # Two runs share the machine: keep each one's thread pool small.
  env["OMP_NUM_THREADS"] = "4"
  cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(STEPS),
         "--warmup", str(WARMUP), "--batch-size", str(BATCH),
         "--dump-outputs", str(dump_dir)] + list(extra)
  return subprocess.Popen(cmd, cwd=REPO, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True)


def _finish(proc):
  stdout, stderr = proc.communicate(timeout=600)
  assert proc.returncode == 0, stderr[-4000:]
  lines = [l for l in stdout.splitlines() if l.startswith("{")]
  assert len(lines) == 1, stdout
  return json.loads(lines[0])


@pytest.fixture(scope="module")
def two_runs(tmp_path_factory):
  """Two runs with the same arguments (the second also with --full),
  side by side: (result, dump dir) of each."""
  root = tmp_path_factory.mktemp("bench_dump")
  procs = [_launch(root / "a"), _launch(root / "b", "--full")]
  results = [_finish(p) for p in procs]
  return (results[0], root / "a"), (results[1], root / "b")


@pytest.mark.slow
def test_result_line_reports_steps_and_ms_per_step(two_runs):
  for result, _ in two_runs:
    assert result["steps"] == STEPS
    assert result["warmup"] == WARMUP
    assert result["unit"] == "images/sec"
    assert result["higher_is_better"] is True
    assert result["dtype"] == "float32"
    assert result["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region.
    assert result["value"] == pytest.approx(
        BATCH * 1000.0 / result["ms_per_step"], rel=1e-2)


@pytest.mark.slow
def test_dump_outputs_written_as_float_npy(two_runs):
  (_, dump), _ = two_runs
  names = sorted(p.name for p in dump.iterdir())
  assert names == ["inference_outputs.logit.npy",
                   "inference_outputs.q_predicted.npy", "loss.npy"]
  total = 0
  for name in names:
    a = np.load(dump / name)
    assert a.dtype in (np.float32, np.float64), name
    assert np.isfinite(a).all(), name
    total += a.nbytes
  assert total <= 64 * 1000 * 1000
  loss = np.load(dump / "loss.npy")
  assert loss.shape == (1,)
  logit = np.load(dump / "inference_outputs.logit.npy").astype(np.float64)
  q = np.load(dump / "inference_outputs.q_predicted.npy")
  assert q.shape == (BATCH,)
  np.testing.assert_allclose(q, 1.0 / (1.0 + np.exp(-logit)), rtol=1e-5)
  # The dump belongs to the LAST step: its loss is the sigmoid log loss of
  # the dumped logits against the labels of the batch that step consumed
  # (the pool is seeded and cycled in order).
  import bench
  pool = bench.make_synthetic_pool(BATCH, "cpu", seed=1234)
  _, labels = pool[(WARMUP + STEPS - 1) % len(pool)]
  target = labels["grasp_success"].numpy().reshape(-1).astype(np.float64)
  expected = np.mean(np.logaddexp(0.0, logit) - target * logit)
  np.testing.assert_allclose(loss[0], expected, rtol=1e-5)


@pytest.mark.slow
def test_same_arguments_same_outputs(two_runs):
  """Seeded inputs: two runs agree array for array (bit-exact on CPU), and
  --full does not change what the timed path computes."""
  (_, a), (_, b) = two_runs
  names = sorted(p.name for p in a.iterdir())
  assert names == sorted(p.name for p in b.iterdir())
  for name in names:
    np.testing.assert_array_equal(np.load(a / name), np.load(b / name),
                                  err_msg=name)


def test_dump_outputs_samples_down_to_budget(tmp_path, monkeypatch):
  import torch

  import bench
  monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
  tensors = {
      "big": torch.arange(10000, dtype=torch.float32).reshape(100, 100),
      "small/x": torch.ones(3, dtype=torch.bfloat16),
      "double": torch.zeros(2, dtype=torch.float64),
  }
  bench.dump_outputs(str(tmp_path / "one"), tensors)
  bench.dump_outputs(str(tmp_path / "two"), tensors)
  big = np.load(tmp_path / "one" / "big.npy")
  assert big.dtype == np.float32 and 0 < big.size < 10000
  # A sample of the original values, in index order, same on every call.
  assert np.all(np.diff(big) > 0) and big.max() < 10000
  np.testing.assert_array_equal(big, np.load(tmp_path / "two" / "big.npy"))
  small = np.load(tmp_path / "one" / "small.x.npy")
  assert small.dtype == np.float32 and small.tolist() == [1.0, 1.0, 1.0]
  assert np.load(tmp_path / "one" / "double.npy").dtype == np.float64
  total = sum(np.load(p).nbytes for p in (tmp_path / "one").iterdir())
  assert total <= 4000
