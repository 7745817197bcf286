"""The device on the directed contact states of tests/golden/contact/regions_*.json (tests/test_contact_regions.py says what
they are and holds the CPU oracle to them): every state as a one-step trajectory whose (v_1, a_0) are the state's (v, a), in
the stored role order and with pair_a and pair_b exchanged, through id_fast.h (fd_fast 1, the shape asserted) and through
the generic id_eval.h (fd_fast 0).

Per state: tau against the independent generator's at the fixture's 1e-7, and v, a, tau, cost, the three partials, the
gradient and the Hessian bands bit for bit against the oracle on that trajectory (same() of tests/test_gpu_parity.py, its
NaN conventions included).  One context per test: the states go through idto_hip_set_problem, which carries q_init and
v_init, and idto_hip_set_q."""
import copy

import numpy as np
import pytest

from idto_amd import hip
from oracle_lib import Oracle
from test_contact_regions import MODELS, ROLES, setup
from test_golden import _qdot
from test_gpu_parity import same

pytestmark = pytest.mark.gpu

FAST_SHAPE = {"hopper": 2, "mini_cheetah": 3, "allegro_hand": 4}
PARTIALS = ("dtau_dqp", "dtau_dqt", "dtau_dqm")
BANDS = ("H_A", "H_B", "H_C")


def one_step(model, prob, st):
    """(problem, q[2]) of the trajectory with tau_0 = ID(q, v, a): q_0 = q - dt N(q) v, v_init = v - dt a"""
    q, v, a = (np.array(st[k]) for k in ("q", "v", "a"))
    q0 = q - prob.time_step * _qdot(model, q, v)
    p = copy.deepcopy(prob)
    p.q_init, p.v_init = q0.copy(), v - prob.time_step * a
    return p, np.stack([q0, q])


def run_states(name, role, fd_fast, method="forward_differences"):
    fix, model, prob, sp = setup(name, role)
    sp = copy.deepcopy(sp)
    sp.gradients_method = method
    p0, _ = one_step(model, prob, fix["states"][0])
    dev = hip.HipPath(model, p0, sp)
    orc = Oracle(model, p0, sp)
    dev.set_option("fd_fast", fd_fast)
    if fd_fast:   # (the exchanged roles and the hopper's small rotated ground keep the shape)
        assert dev.get_option("fast_shape") == FAST_SHAPE[name]
    worst = 0.0
    for i, st in enumerate(fix["states"]):
        what = (name, role, fd_fast, i, st["aim"])
        p, q = one_step(model, prob, st)
        dev.set_problem(p)
        orc.reset_initial_conditions(p.q_init, p.v_init)
        dev.set_q(q)
        dev.gn_step()
        got = {k: dev.get(k) for k in ("v", "a", "tau", "gradient") + PARTIALS + BANDS}
        # the independent generator
        want = np.array(st["tau"])
        scale = max(np.abs(want).max(), np.abs(st["tau_contact"]).max())
        assert np.abs(got["v"][1] - np.array(st["v"])).max() < 1e-12 and np.abs(got["a"][0] - np.array(st["a"])).max() < 1e-10, what
        err = np.abs(got["tau"][0] - want).max() / scale
        worst = max(worst, err)
        assert err <= fix["tolerance_rel"], (what, err)
        # the oracle, bit for bit
        v, a, tau, cost = orc.eval_traj(q)
        assert same(got["v"], v) and same(got["a"], a), what
        assert same(got["tau"], tau), (what, np.abs(got["tau"] - tau).max())
        P = orc.eval_partials(q)
        for k in PARTIALS:
            assert same(got[k], P[k]), (what, k, np.nanmax(np.abs(got[k] - P[k])))
        g, bands = orc.grad_hess(q)
        assert same(got["gradient"], g), what
        for k, band in zip(BANDS, bands):
            assert same(got[k], band), (what, k)
        dev.eval_tau()
        assert same(dev.get("tau"), tau), (what, "eval_tau")
        assert dev.get("cost") == cost, (what, "cost")
    dev.close()
    print(name, role, fd_fast, method, len(fix["states"]), "states; worst |tau - golden| / scale", worst)


@pytest.mark.parametrize("fd_fast", [1, 0])
@pytest.mark.parametrize("role", ROLES)
@pytest.mark.parametrize("name", MODELS)
def test_device_on_every_region_and_branch(name, role, fd_fast):
    run_states(name, role, fd_fast)


@pytest.mark.parametrize("method", ["central_differences", "central_differences4"])
@pytest.mark.parametrize("role", ROLES)
def test_device_on_every_region_and_branch_central_differences(role, method):
    """gradients_method central / central4 on the cheetah's states: the box on the moving common body"""
    run_states("mini_cheetah", role, 1, method)
