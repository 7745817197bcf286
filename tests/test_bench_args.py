"""bench.py started as the driver starts it for N > 1 but WITHOUT a launcher: the command it re-executes itself
with (torch.distributed.run, one rank per GPU, rendezvous on 127.0.0.1) and the device-sharing fallback; a plain run and
what --dump-outputs writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench


def test_self_launch_command_one_rank_per_gpu():
    cmd, env = bench.self_launch_command(["--gpus", "8", "--steps", "20", "--warmup", "5"], 8, 8, port=29555)
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29555"
    assert cmd[-6:] == ["--gpus", "8", "--steps", "20", "--warmup", "5"] and cmd[-7].endswith("bench.py")
    assert env["MASTER_ADDR"] == "127.0.0.1" and "IDTO_BENCH_VISIBLE_GPUS" not in env


def test_self_launch_shares_devices_when_fewer_are_visible():
    cmd, env = bench.self_launch_command(["--gpus", "2"], 2, 1, port=1)
    assert "--nproc-per-node=2" in cmd and env["IDTO_BENCH_VISIBLE_GPUS"] == "1"
    _, env0 = bench.self_launch_command(["--gpus", "2"], 2, 0, port=1)   # no device at all: still one "slot"
    assert env0["IDTO_BENCH_VISIBLE_GPUS"] == "1"


def test_free_port_is_chosen():
    cmd, _ = bench.self_launch_command(["--gpus", "2"], 2, 2)
    assert 1024 < int(cmd[cmd.index("--master-port") + 1]) < 65536


def test_dump_outputs_writes_every_array_as_fp64(tmp_path):
    class Dev:
        def get(self, name):
            return np.arange(6, dtype=np.float64).reshape(2, 3) + len(name)
    bench.dump_outputs(Dev(), str(tmp_path / "out"))
    for name in bench.DUMP_ARRAYS:
        a = np.load(tmp_path / "out" / (name + ".npy"))
        assert a.dtype == np.float64 and np.array_equal(a, Dev().get(name))


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_timed_step(tmp_path):
    """A plain run prints the headline only, times exactly --steps steps, and --dump-outputs holds what a fresh context
    computes from the same input, bit for bit."""
    from idto_amd import hip
    from idto_amd.model import load_model
    from idto_amd.problem import load_config, make_problem, synthetic_trajectory
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], cwd=root, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == 7 and line["ms_per_step"] > 0 and line["value"] > 0
    assert {"metric", "unit", "higher_is_better", "dtype"} <= set(line) and line["dtype"] == "f64"
    assert not {"roofline", "cpu_baseline", "step_latency_ms", "batch_mode", "full_iteration"} & set(line)
    cfg, model = load_config("mini_cheetah"), load_model("mini_cheetah")
    prob, sp, _ = make_problem(cfg, model, num_steps=40)
    sp.scaling = sp.equality_constraints = False
    dev = hip.HipPath(model, prob, sp)
    dev.set_q(synthetic_trajectory(cfg, model, 40, seed=0, lower=0.01))
    dev.gn_step()
    for name in bench.DUMP_ARRAYS:
        assert np.array_equal(np.load(tmp_path / (name + ".npy")), dev.get(name)), name
    dev.close()
