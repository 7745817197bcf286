"""Shared pairs: contact pairs between the chains of two paths (include/idto_model.h), and the dual_jaco fixture.

The CPU oracle adds every pair's force onto both of its bodies in ascending pair order, whichever paths they are on, so
it needs no change.  What the tests below pin down is the model contract (Model.validate, the .model file) and that the
states the GPU tests use really make the shared pairs act: with the oracle, dropping the shared pairs changes tau there.
A test that reused the jaco trajectories would pass without the feature doing anything - the arms' hands are apart."""
import copy
import os

import numpy as np
import pytest

from idto_amd.model import load_model
from idto_amd.problem import load_config, make_problem
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = os.path.join(ROOT, "tests", "golden", "examples")
ARMS = 14          # dual_jaco: left arm bodies / joints 0-6, right arm 7-13, the box is body 14
MIN_CHANGE = 1e-3  # a state counts as "hands touching" when the shared pairs change tau by more than this


def dual_jaco():
    return (load_model(os.path.join(EXAMPLES, "dual_jaco.model")),
            load_config(os.path.join(EXAMPLES, "dual_jaco.yaml")))


def chain_paths(model, k):
    bodies = (int(model.geom_body[int(model.pair_a[k])]), int(model.geom_body[int(model.pair_b[k])]))
    return {int(model.body_path[b]) for b in bodies if b != -1 and b != model.common_body}


def shared_pairs(model):
    return [k for k in range(model.npairs) if len(chain_paths(model, k)) == 2]


def drop_pairs(model, drop):
    m = copy.deepcopy(model)
    keep = [k for k in range(m.npairs) if k not in set(drop)]
    m.pair_a, m.pair_b, m.pair_path = m.pair_a[keep], m.pair_b[keep], m.pair_path[keep]
    return m.normalize()


def touching_trajectory(model, cfg, N, seed, smoothing_factor=None, tries=2000):
    """A trajectory of N + 1 configurations whose shared pairs act at most time steps: both arms' joints at one random
    offset of up to +-1.2 rad from q_init (a fixed-seed scan: kept is the first offset where the shared pairs change the
    oracle's tau by more than MIN_CHANGE at N / 2 time steps or more), drifting by up to 0.02 rad over the horizon."""
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    if smoothing_factor is not None:
        sp.smoothing_factor = smoothing_factor
    full, cut = Oracle(model, prob, sp), Oracle(drop_pairs(model, shared_pairs(model)), prob, sp)
    q_init = np.asarray(cfg["q_init"], dtype=float)
    rng = np.random.default_rng(seed)
    ramp = np.linspace(0.0, 1.0, N + 1)[:, None]
    for _ in range(tries):
        d, drift = np.zeros(model.nq), np.zeros(model.nq)
        d[:ARMS] = rng.uniform(-1.2, 1.2, ARMS)
        drift[:ARMS] = rng.uniform(-0.02, 0.02, ARMS)
        q = q_init + d + ramp * drift
        change = np.abs(full.eval_traj(q)[2] - cut.eval_traj(q)[2]).max(axis=1)
        if np.count_nonzero(change > MIN_CHANGE) >= N // 2:
            return q
    raise AssertionError("no touching state found")


def test_dual_jaco_fixture():
    model, cfg = dual_jaco()
    assert (model.nbodies, model.nq, model.nv) == (15, 21, 20)
    arm = [f"j2s7s300_link_{i}" for i in range(1, 8)]
    assert model.body_names == [f"jaco_left::{n}" for n in arm] + [f"jaco_right::{n}" for n in arm] + ["box"]
    assert list(model.parent) == [-1, 0, 1, 2, 3, 4, 5, -1, 7, 8, 9, 10, 11, 12, -1]
    assert list(model.jtype) == [0] * 14 + [3]
    assert list(model.gravity_enabled) == [0] * 14 + [1]
    assert model.common_body == 14 and model.npaths == 2
    assert list(model.body_path) == [0] * 7 + [1] * 7 + [-1]
    assert model.ngeoms == 16 and model.npairs == 78
    sh = shared_pairs(model)
    assert len(sh) == 9
    assert sorted((int(model.pair_a[k]), int(model.pair_b[k])) for k in sh) == [(a, b) for a in (0, 1, 2) for b in (3, 4, 5)]
    # the converter names the path of geometry A's body
    for k in sh:
        assert int(model.pair_path[k]) == int(model.body_path[int(model.geom_body[int(model.pair_a[k])])]) == 0
    assert cfg["num_steps"] == 20 and cfg["time_step"] == 0.05 and cfg["max_iters"] == 50
    assert cfg["equality_constraints"] is False and cfg["gradients_method"] == "forward_differences"
    prob, sp, _ = make_problem(cfg, model)
    assert prob.num_steps == 20 and prob.time_step == 0.05 and not sp.equality_constraints


def test_validate_accepts_either_path_of_a_shared_pair():
    model, _ = dual_jaco()
    k = shared_pairs(model)[0]
    for p in (0, 1):
        m = copy.deepcopy(model)
        m.pair_path[k] = p
        m.validate()


def test_validate_refuses_a_third_path():
    model, _ = dual_jaco()
    m = copy.deepcopy(model)
    m.npaths = 4   # (two empty paths: a power of two)
    m.pair_path[shared_pairs(model)[0]] = 2
    with pytest.raises(AssertionError, match="outside path 2"):
        m.validate()
    # an ordinary pair of one arm still belongs to that arm's path only
    m = copy.deepcopy(model)
    k = next(k for k in range(model.npairs) if chain_paths(model, k) == {0})
    m.pair_path[k] = 1
    with pytest.raises(AssertionError, match="outside path 1"):
        m.validate()


def test_model_file_round_trip(tmp_path):
    src = os.path.join(EXAMPLES, "dual_jaco.model")
    model = load_model(src)
    out = tmp_path / "dual_jaco.model"
    model.save(str(out))
    assert out.read_bytes() == open(src, "rb").read()


@pytest.mark.parametrize("seed", [0, 1])
def test_touching_states_make_the_shared_pairs_act(seed):
    """At the example's contact parameters (sigma = 0.005: the force reaches ~0.15 m) the shared pairs act only where
    the hands touch; the scan finds such states, and there they change tau by more than MIN_CHANGE."""
    model, cfg = dual_jaco()
    N = 20
    q = touching_trajectory(model, cfg, N, seed)
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    assert sp.smoothing_factor == 0.005
    tau = Oracle(model, prob, sp).eval_traj(q)[2]
    tau_cut = Oracle(drop_pairs(model, shared_pairs(model)), prob, sp).eval_traj(q)[2]
    change = np.abs(tau - tau_cut).max(axis=1)
    assert np.count_nonzero(change > MIN_CHANGE) >= N // 2
    # the box's rows see no shared pair: its force from them is exactly zero
    assert np.array_equal(tau[:, ARMS:], tau_cut[:, ARMS:])


def test_a_larger_smoothing_factor_makes_every_shared_pair_act():
    """sigma = 0.05 (force reach ~1.6 m): every shared pair acts at ordinary poses - the YAML's own guess."""
    model, cfg = dual_jaco()
    N = 20
    prob, sp, q_guess = make_problem(cfg, model, num_steps=N)
    sp.smoothing_factor = 0.05
    tau = Oracle(model, prob, sp).eval_traj(q_guess)[2]
    for k in shared_pairs(model):
        tau_cut = Oracle(drop_pairs(model, [k]), prob, sp).eval_traj(q_guess)[2]
        assert np.abs(tau - tau_cut)[1:].max() > MIN_CHANGE, k
