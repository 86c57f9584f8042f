"""bench.py's launch contract, on the CPU: --gpus N must
run exactly N ranks -- started by bench.py itself when torchrun's env is
absent -- and a world / GPU-count mismatch must fail non-zero instead of
printing a line for fewer GPUs than asked."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, **env):
    e = {k: v for k, v in os.environ.items()
         if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    e.update(env)
    return subprocess.run([sys.executable, BENCH] + args, env=e, capture_output=True, text=True,
                          timeout=120)


def test_world_mismatch_fails():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], WORLD_SIZE="1")
    assert r.returncode != 0
    assert "--gpus 2 but the process group has 1 rank" in r.stderr


def test_self_launch_starts_n_ranks_and_checks_gpus():
    """No torchrun env: bench.py starts 2 ranks (they rendezvous over gloo on
    this GPU-less host) and each refuses to run with fewer GPUs than ranks."""
    import torch
    if torch.cuda.device_count() >= 2:  # (a multi-GPU host would run the bench)
        return
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert r.stderr.count("--gpus 2 needs 2 visible GPUs") == 2, r.stderr
    assert "rank exit codes" in r.stderr


def test_gpus_must_be_positive():
    r = _run(["--gpus", "0"])
    assert r.returncode != 0


def test_full_and_dump_outputs_are_options():
    r = _run(["--help"])
    assert r.returncode == 0
    assert "--full" in r.stdout and "--dump-outputs DIR" in r.stdout


@pytest.mark.gpu
def test_plain_run_times_the_steps_only_and_dumps_its_outputs(tmp_path):
    """A plain run (no --full) on a 2 % products graph: the line carries the
    headline fields and none of the secondary measurements, and
    --dump-outputs leaves the last timed step's loss, seed-row logits and
    post-step parameters as float32 .npy files -- the same values from two
    runs with the same arguments (started side by side)."""
    import numpy as np
    outs = [tmp_path / "dump0", tmp_path / "dump1"]
    # (3,932 train seeds: three full batches of 1024 and a short one, not reached)
    args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--scale", "0.02", "--dump-outputs"]
    procs = [subprocess.Popen([sys.executable, BENCH] + args + [str(o)], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for o in outs]
    res = [p.communicate(timeout=120) for p in procs]
    for p, (_, err) in zip(procs, res):
        assert p.returncode == 0, err[-2000:]
    line = json.loads(res[0][0].strip().splitlines()[-1])
    assert line["steps"] == 2 and line["full"] is False
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "edges/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    for k in ("epoch_time_s", "eager_drop_in", "roofline", "cpu_baseline", "allreduce"):
        assert line[k] is None, k
    got, again = ({f[:-4]: np.load(o / f) for f in os.listdir(o)} for o in outs)
    shapes = {"loss": (), "logits": (1024, 47),
              "param.convs.0.lin_l.weight": (256, 100), "param.convs.0.lin_l.bias": (256,),
              "param.convs.0.lin_r.weight": (256, 100), "param.convs.1.lin_l.weight": (47, 256),
              "param.convs.1.lin_l.bias": (47,), "param.convs.1.lin_r.weight": (47, 256)}
    assert {k: v.shape for k, v in got.items()} == shapes
    for k, v in got.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k
    # one step from the seeded initial weights: the loss of a 47-class head is
    # near ln 47 and the logits are not constant
    assert 0.0 < float(got["loss"]) < 2 * np.log(47)
    assert float(got["logits"].std()) > 0
    # run to run: the forward and the loss sum in a fixed order (a few ulp of
    # values below 4 allowed: 1e-6).  The weight gradients carry the rounding
    # of the head's atomic scatter, |dg| <~ 2^-24 x 1e-3 = 6e-11; the first
    # Adam step, lr g / (|g| + eps), turns that into at most lr |dg| / eps =
    # 6e-6 for an element with |g| <~ eps = 1e-8 (far less elsewhere): 2e-5
    for k in shapes:
        tol = 1e-6 if k in ("loss", "logits") else 2e-5
        assert float(np.abs(got[k].astype(np.float64) - again[k]).max()) <= tol, k
