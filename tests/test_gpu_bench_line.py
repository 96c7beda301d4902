"""bench.py --gpus 1 on the GPU ("a -m gpu test runs
--gpus 1 unchanged"): one rank, no launcher, the product engine (libnarde.so,
k_rollout_pc), and the line carries the world size, the env counts, the
roofline object and the episode totals the last timed launch reduced on the
device -- equal to the CPU oracle playing the same env ids for the same plies.
With --full the checker leg replays the timed region; a plain run runs the
headline alone and --dump-outputs writes its last ply.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUIET = ["--ramp-launches", "0", "--ramp-ms", "0", "--api-steps", "0", "--fused-launches", "0",
         "--other-launches", "0", "--dqn-steps", "0", "--no-cpu-baseline"]


def _bench(args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "NARDE_BENCH_TEST_ENGINE"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=100)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_bench_gpus1_line_and_totals():
    envs, ppl, warmup, steps = 4096, 50, 100, 200
    # --full with every leg but the checker switched off (QUIET): the C
    # oracle replays the timed region (parity_check)
    line = _bench(["--gpus", "1", "--envs", str(envs), "--plies-per-launch", str(ppl), "--warmup", str(warmup),
                   "--steps", str(steps), "--full", *QUIET])
    assert line["full"] is True and line["parity_check"]["mismatches"] == 0
    assert "engine" not in line  # the product engine, not the host rehearsal
    assert line["n_gpus"] == 1 and line["steps"] == steps and line["warmup"] == warmup
    cfg = line["config"]
    assert cfg["envs_per_gpu"] == envs and cfg["global_envs"] == envs
    assert cfg["collective"]["world_size"] == 1
    assert line["roofline"]["bound"] == "hbm" and 0 < line["roofline"]["frac"] < 1.5
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # the untimed launch-path warm-up (3 x the first and the last launch of
    # the region) + --warmup + --steps plies, from a fresh reset at seed 0
    plies = 3 * 2 * ppl + warmup + steps
    sp = O.SelfPlay(envs, seed=0, env0=0)
    sp.reset(0)
    sp.run(plies, record=False)
    want = sp.stats.astype(np.int64).sum(0, keepdims=True)
    assert np.array_equal(np.array(cfg["rank_totals"], np.int64), want)


def test_bench_plain_run_dumps_last_timed_ply(tmp_path):
    """A plain run (no --full) runs no leg beside the headline, and
    --dump-outputs writes the last timed ply's outputs: what the CPU oracle
    records for that ply after the same number of plies from a fresh reset at
    seed 0 -- whatever number of clock-dependent ramp launches (--ramp-ms) ran
    on their own env.  300 envs: two workgroups, the second one partial; 45
    timed plies as launches of 20, 20 and 5."""
    envs, ppl, warmup, steps, ramp = 300, 20, 7, 45, 10
    line = _bench(["--gpus", "1", "--envs", str(envs), "--plies-per-launch", str(ppl), "--warmup", str(warmup),
                   "--steps", str(steps), "--ramp-launches", str(ramp), "--ramp-ms", "60",
                   "--dump-outputs", str(tmp_path)])
    assert line["full"] is False and line["steps"] == steps and line["ms_per_step"] > 0
    for leg in ("cpu_baseline", "parity_check", "api_step", "other_rules", "config4_dqn", "selfplay_stats_only"):
        assert line[leg] is None, leg
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert sorted(got) == sorted(line["dumped_outputs"]) == [
        "actions", "legal_hi", "legal_lo", "obs", "reward", "terminated", "totals_rows", "truncated"]
    # ramp (1,000-ply launches) + 3 x the first and the last timed launch + --warmup + --steps
    plies = ramp * 1000 + 3 * (ppl + steps % ppl) + warmup + steps
    sp = O.SelfPlay(envs, seed=0, env0=0)
    sp.reset(0)
    sp.run(plies - 1, record=False)
    rec = sp.run(1)
    for name, key in (("obs", "obs"), ("reward", "reward"), ("terminated", "terminated"),
                      ("truncated", "truncated"), ("actions", "action")):
        assert got[name].dtype == np.float32
        assert np.array_equal(got[name], rec[key][0].astype(np.float32)), name
    legal = got["legal_lo"].astype(np.uint64) | (got["legal_hi"].astype(np.uint64) << np.uint64(32))
    assert got["legal_lo"].dtype == np.float64 and np.array_equal(legal, rec["legal"][0])
    rows = np.zeros((2 * 256, 3), np.int64)
    rows[:envs] = sp.stats
    assert np.array_equal(got["totals_rows"], rows.reshape(2, 256, 3).sum(1).astype(np.float64))
