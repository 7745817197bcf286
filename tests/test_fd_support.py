"""Which paths a column of q touches - what fd_kernel's lane map without the redundant path lanes rests on (DESIGN.md 3.1,
host/model_tables.cc BuildFdDedup) - on the CPU.

A column of q (or a mass column) that belongs to a joint of leg l changes nothing in the common body or in the other
legs, so in that evaluation the other legs' lanes repeat the baseline.  Two checks of that premise:
  - the oracle's partials of mini_cheetah (N = 3: the records k = 0, 1, 2 with their rules) have EXACT zeros in every
    (leg column, other leg's row) entry of all three blocks, and entries of the column's own leg that are not zero;
  - the path sets the host derives (tests/cpp/fd_dedup_check.cc prints them) are that pattern.
The stand-alone program also holds the lane words to the path sets - every evaluation on exactly the paths it touches,
whole evaluations on four aligned lanes, the helpers' pair records - and the refusal for a model whose pairs come in
another order; it is built with the address and undefined-behaviour sanitizers.
"""
import os
import subprocess

import numpy as np
import pytest

from idto_amd.model import load_model
from idto_amd.problem import load_config, make_problem, synthetic_trajectory
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "idto_amd", "csrc")
N = 3
MODELS = [os.path.join(ROOT, "idto_amd", "models", "mini_cheetah.model"),
          os.path.join(ROOT, "idto_amd", "models", "hopper.model"),
          os.path.join(ROOT, "idto_amd", "models", "allegro_hand.model"),
          os.path.join(ROOT, "tests", "golden", "examples", "dual_jaco.model"),
          os.path.join(ROOT, "tests", "golden", "examples", "punyo.model")]


def _leg_of(model):
    """path of every column of q and of every row / mass column of v: -1 for the common body's"""
    qleg, vleg = np.full(model.nq, -1), np.full(model.nv, -1)
    for b in range(model.nbodies):
        if b == model.common_body:
            continue
        qs, vs = int(model.qstart[b]), int(model.vstart[b])
        qleg[qs] = vleg[vs] = int(model.body_path[b])   # (one revolute joint a body)
    return qleg, vleg


@pytest.fixture(scope="module")
def host_paths(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fd_dedup") / "fd_dedup_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "fd_dedup_check.cc"),
                    os.path.join(CSRC, "host", "model_tables.cc"), "-o", exe], check=True)
    run = subprocess.run([exe] + MODELS, capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok: %d models" % len(MODELS)), run.stdout[-4000:] + run.stderr[-4000:]
    out = {}
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0] == "paths":
            iq, iv = w.index("q"), w.index("v")
            out[w[1]] = (int(w[2]), [int(x) for x in w[iq + 1:iv]], [int(x) for x in w[iv + 1:]])
        elif w[0] == "lanes":
            out["lanes " + w[1]] = {w[i]: int(w[i + 1]) for i in range(2, len(w), 2)}
    return out


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_oracle_partials_are_zero_outside_the_columns_leg(seed):
    cfg, model = load_config("mini_cheetah"), load_model("mini_cheetah")
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    q = synthetic_trajectory(cfg, model, N, seed=seed, lower=0.01)
    d = Oracle(model, prob, sp).eval_partials(q)
    qleg, vleg = _leg_of(model)
    other = (qleg[None, :] >= 0) & (vleg[:, None] >= 0) & (qleg[None, :] != vleg[:, None])   # [row, col]
    own = (qleg[None, :] >= 0) & (qleg[None, :] == vleg[:, None])
    assert other.sum() == 12 * 9 and own.sum() == 12 * 3
    # (dtau_t/dq_{t+1} for every t; dtau_t/dq_t from t = 1, dtau_t/dq_{t-1} from t = 2: q_0 is fixed, TO.cc:534, :556)
    for key, t0 in (("dtau_dqp", 0), ("dtau_dqt", 1), ("dtau_dqm", 2)):
        blk = d[key][t0:]
        assert np.all(np.isfinite(blk)), key
        assert np.all(blk[:, other] == 0.0), (key, int(np.count_nonzero(blk[:, other])))
        assert np.count_nonzero(blk[:, own]) > 0.5 * blk[:, own].size, key


def test_host_path_sets_are_that_pattern(host_paths):
    model = load_model("mini_cheetah")
    on, qp, vp = host_paths[model.name]
    assert on == 1
    qleg, vleg = _leg_of(model)
    everyone = (1 << model.npaths) - 1
    assert qp == [everyone if l < 0 else 1 << l for l in qleg]
    assert vp == [everyone if l < 0 else 1 << l for l in vleg]
    # 120 lane-evaluations: 15 whole evaluations with contact and 6 mass columns on four lanes, 24 + 12 on one
    nq, nv = model.nq, model.nv
    whole_q, whole_v = sum(p == everyone for p in qp), sum(p == everyone for p in vp)
    lanes = host_paths["lanes " + model.name]
    assert lanes["main"] == 4 * (1 + 2 * whole_q + whole_v) + 2 * (nq - whole_q) + (nv - whole_v) == 120
    assert lanes["foot"] == 4 * (1 + 2 * whole_q) + 2 * (nq - whole_q) == 84 and lanes["body"] == 1 + 2 * whole_q == 15


def test_other_models_keep_every_evaluation_on_all_paths(host_paths):
    for name, (on, qp, vp) in ((k, v) for k, v in host_paths.items() if not k.startswith("lanes ")):
        if name != load_model("mini_cheetah").name:
            assert on == 0, name
