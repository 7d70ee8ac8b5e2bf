"""bench.py's launch logic (CPU): `--gpus N` must really put N GPUs to work or fail loudly — a SCALE run that silently
measured one GPU and printed "n_gpus": 1 was the defect of round 2."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (importing bench does not import torch or touch a GPU)


def plan(gpus, **env):
    return bench.launch_plan(types.SimpleNamespace(gpus=gpus), env)


def test_launch_plan():
    assert "torch" not in bench.__dict__                       # nothing GPU-related is imported at module level
    assert plan(1) == "rank"
    assert plan(8) == "ranks"                                  # python bench.py --gpus 8: this process only launches the ranks
    assert plan(8, WORLD_SIZE="8", RANK="3", LOCAL_RANK="3") == "rank"   # the driver's torch.distributed.run form
    assert plan(1, WORLD_SIZE="1") == "rank"
    with pytest.raises(SystemExit) as e:
        plan(8, WORLD_SIZE="2")                                # launcher and flag disagree: refuse
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        plan(1, WORLD_SIZE="4")
    assert plan(4, RC_BENCH_SINGLE_PROCESS="1") == "single"
    assert plan(4, RC_BENCH_SINGLE_PROCESS="0") == "ranks"
    with pytest.raises(SystemExit):
        plan(4, RC_BENCH_SINGLE_PROCESS="1", WORLD_SIZE="4")
    with pytest.raises(SystemExit):
        plan(0)


def test_gpus_2_without_two_gpus_fails_loudly():
    """No GPU in this container (one on the pool's boxes): `bench.py --gpus 2` starts two ranks in a fresh child, they
    cannot get two GPUs, and the run exits non-zero WITHOUT printing a result line — instead of measuring one GPU."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RC_BENCH_SINGLE_PROCESS")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode != 0
    assert b'"metric"' not in r.stdout
    assert b"2-rank child exited" in r.stderr
    # the single-process form refuses too
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2"],
                       env=dict(env, RC_BENCH_SINGLE_PROCESS="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode != 0 and b'"metric"' not in r.stdout


def test_median_and_windows_helpers():
    assert bench.median([3.0, 1.0, 2.0]) == 2.0 and bench.median([4.0, 1.0, 2.0, 3.0]) == 2.5

    class Fake:
        def __init__(self): self.calls = 0; self.syncs = 0
        def gibbs_sweep(self, r, p, seed, sweep, blocking=True): self.calls += 1
        def synchronize(self): self.syncs += 1
    f, bars = Fake(), []
    times, nxt = bench.timed_windows(f, 1, 1.0, 0.5, steps=7, warmup=3, windows=5, sync_all=lambda: bars.append(1), sweep0=10)
    assert len(times) == 5 and f.calls == 3 + 5 * 7 and nxt == 10 + 3 + 35 and len(bars) == 10   # exactly K steps per window, a barrier on both sides


def test_plain_and_full_options():
    a = bench.parse_args(["--steps", "30", "--warmup", "4"])
    assert a.steps == 30 and a.warmup == 4 and not a.full and a.dump_outputs is None   # a plain run: the headline alone
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_dump_outputs_files(tmp_path):
    clusts, sizes = np.array([2, 1, 2, 3], np.int64), np.array([1, 2, 1, 0], np.int64)
    bench.dump_outputs(str(tmp_path / "d"), (clusts, sizes, 3))
    got = {f: np.load(tmp_path / "d" / f"{f}.npy") for f in ("labels", "cluster_sizes", "num_clusters")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["labels"], clusts) and np.array_equal(got["cluster_sizes"], sizes) and got["num_clusters"].tolist() == [3.0]


@pytest.mark.gpu
def test_dump_is_the_state_after_the_timed_steps(tmp_path):
    """A plain run's --dump-outputs holds the state a caller gets after the last timed step: warm-up and timed sweeps 0..W+K-1 of a
    chain from the generating labels, whatever the clock-dependent settle phase ran before them — replayed here on a fresh context."""
    import json
    import redclust_amd as rc
    n, K, steps, warmup = 2000, 20, 6, 3
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RC_BENCH_SINGLE_PROCESS")}
    env.update(RC_BENCH_N=str(n), RC_BENCH_K=str(K))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(tmp_path)], env=env, stdout=subprocess.PIPE, timeout=600)
    assert r.returncode == 0
    line = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert "roofline" not in line and "cpu_baseline" not in line                  # figures of --full only
    data = rc.generatemixture(n, K, seed=1)
    D, truth = data["distancematrix"], data["clusts"]
    ctx = rc.Context(D)
    ctx.set_params(**rc.likelihood_hyperparams(D, truth))
    ctx.set_state(truth)
    for t in range(warmup + steps):
        ctx.gibbs_sweep(1.0, 0.5, 1, t)
    clusts, sizes, Kf = ctx.get_state()
    ctx.close()
    assert np.array_equal(np.load(tmp_path / "labels.npy"), clusts)
    assert np.array_equal(np.load(tmp_path / "cluster_sizes.npy"), sizes)
    assert np.load(tmp_path / "num_clusters.npy").tolist() == [Kf] == [line["K_final"]]
