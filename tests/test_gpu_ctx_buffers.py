"""A context's staging and grown buffers, each with one owner (csrc/host/ctx_buffers.h; the CPU side of it is
tests/test_ctx_buffers.py): on the device, two acrobots' worth of every entry that makes a buffer on first use or grows one.

One context of one acrobot and one of a batch of two, N = 3.  Every grow-on-demand entry is called small, larger, small again;
the bar is == (NaNs matched) against the same call on a fresh context - the statistics rows without their device clock,
column 10, which no test of the project compares.  Then the steady state allocates nothing (free device memory, the bound of
tests/test_gpu_trust_region.py), a growing buffer keeps no superseded generation, "begin again" and destroy return everything,
and a context that has touched every buffer closes in an order the next context survives.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import lin_cases as lc
import track_cases as tc
from idto_amd import hip

pytestmark = pytest.mark.gpu

NAME, B, R, H, M = "acrobot", 2, 2, 1e-3, 2
MIB = 1 << 20
NO_CLOCK = [c for c in range(17) if c != 10]       # a trust-region row without TRR_CLOCK
LS_NO_CLOCK = [c for c in range(hip.LS_ROW) if c != 10]   # a linesearch row without LSR_CLOCK
MANY = ("q", "v", "gradient", "cost")


def _case():
    model, _, prob, sp, _, _ = lc.case(NAME)
    return model, prob, sp


def _q(b=0):
    return _case()[1].q_nom + 0.01 * (b + 1)


def _single():
    model, prob, sp = _case()
    dev = hip.HipPath(model, prob, sp)
    dev.set_unactuated_dofs(model.unactuated_dofs)
    return dev


def _batch():
    model, prob, sp = _case()
    dev = hip.HipPath(model, [prob] * B, sp)
    dev.set_unactuated_dofs(model.unactuated_dofs)
    return dev


def _rhs(nrhs):
    model, prob, _ = _case()
    return np.random.default_rng(11).uniform(-1, 1, (nrhs, (prob.num_steps + 1) * model.nq))


def _track_inputs(S):
    per = [tc.inputs(NAME, S, R, seed=b) for b in range(B)]
    return tuple(np.array([p[k] for p in per]) for k in range(4)) + (per[0][4],)


# ---- the entries: each sets up what it needs, so that its result is a function of its argument alone
def tr_solve(dev, iters):
    dev.set_q(_q()); dev.eval_tau()
    rows, delta = dev.tr_solve(iters, 2, True, False, 1e-1, 1e5)
    return [rows[:, NO_CLOCK], delta, dev.get("q")]


def ls_solve(dev, iters):
    dev.set_q(_q())
    out = dev.ls_solve(iters, 0, 10, False)
    return [out["rows"][:, LS_NO_CLOCK], out["q"], out["v"], out["tau"]]


def costs_along(dev, m):
    dev.set_q(_q()); dev.eval_tau(); dev.gn_step()
    return [dev.costs_along(hip.ls_alphas(0, 6)[:m])]


def solve_host(dev, nrhs):
    dev.set_q(_q()); dev.eval_partials(); dev.grad_hess()
    return [dev.solve_host(_rhs(nrhs))]


def get_many(dev, n):
    dev.set_q(_q()); dev.eval_tau(); dev.gn_step()
    out = [np.zeros(dev.array_size(name)) for name in MANY[:n]]
    what = (C.c_int * n)(*[hip.ARR[name] for name in MANY[:n]])
    ptrs = (C.POINTER(C.c_double) * n)(*[a.ctypes.data_as(C.POINTER(C.c_double)) for a in out])
    assert hip.lib().idto_hip_get_many(dev.h, C.c_int(n), what, ptrs) == 0, hip.lib().idto_hip_last_error()
    return out


def prefetch(dev, n):
    dev.set_q(_q()); dev.eval_tau(); dev.gn_step()
    names = ("gradient", "v")[:n]
    for name in names:
        dev.prefetch(name)
    return [dev.get(name) for name in names]


def constraint_schur(dev, dofs):
    dev.set_q(_q()); dev.eval_partials(); dev.grad_hess()
    return list(dev.constraint_schur(dofs))


def ls_solve_batch(dev, iters):
    dev.set_q_batch(np.array([_q(b) for b in range(B)]))
    out = dev.ls_solve_batch(iters, 0, 10, False)
    return [out["rows"][:, :, LS_NO_CLOCK]] + [out[k] for k in ("q", "v", "tau", "final_cost", "status")]


def tr_solve_batch_fetch(dev, iters):
    dev.set_q_batch(np.array([_q(b) for b in range(B)])); dev.eval_tau()
    out = dev.tr_solve_batch_fetch(iters, 2, True, False, [0.1] * B, 1e5)
    return [out["rows"][:, :, NO_CLOCK]] + [out[k] for k in ("delta", "q", "v", "tau", "dq", "w", "final_cost", "status")] + [out["best"]]


def scene_report(dev, S):
    r = dev.scene_report(_track_inputs(S)[0][:, :S], pair_rows=True)
    return [r.bodies, r.pairs, r.tau_contact, r.tau_pairs]


def plant_linearize(dev, S):
    x, tau = _track_inputs(S)[:2]
    return list(dev.plant_linearize(x[:, :S], tau, H, M))


def plant_track(dev, S):
    x, tau, K, x0, act = _track_inputs(S)
    r = dev.plant_track(x, tau, K, x0, H, M, act)
    return [r.x, r.u, r.dx, r.status]


# (entry, its arguments small / larger / small again)
SINGLE = [(tr_solve, (2, 5, 2)), (ls_solve, (2, 5, 2)), (costs_along, (2, 6)), (solve_host, (1, 3)), (get_many, (1, 4)),
          (prefetch, (1, 2)), (constraint_schur, ((0,), (0, 1), (0,)))]
BATCH = [(ls_solve_batch, (2, 5, 2)), (tr_solve_batch_fetch, (2, 4)), (scene_report, (1, 3)), (plant_linearize, (1, 3)),
         (plant_track, (1, 3))]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _round(one, two):
    """every entry with every argument, in turn -> {(entry, argument, position): arrays}"""
    out = {}
    for dev, table in ((one, SINGLE), (two, BATCH)):
        for entry, args in table:
            for i, arg in enumerate(args):
                out[entry.__name__, arg, i] = entry(dev, arg)
    return out


@pytest.fixture(scope="module")
def fresh():
    """the same calls, each on a context of its own: computed once, left unchanged"""
    out = {}
    for make, table in ((_single, SINGLE), (_batch, BATCH)):
        for entry, args in table:
            for arg in set(args):
                dev = make()
                out[entry.__name__, arg] = entry(dev, arg)
                dev.close()
    return out


def _free():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_growth_keeps_results(fresh):
    one, two = _single(), _batch()
    got = _round(one, two)
    one.close(); two.close()
    assert len(got) == sum(len(args) for _, args in SINGLE + BATCH)
    for (name, arg, i), arrays in got.items():
        ref = fresh[name, arg]
        assert len(arrays) == len(ref)
        for k, (a, b) in enumerate(zip(arrays, ref)):
            assert _same(a, b), (name, arg, i, k)
    # (the calls did something)
    assert np.nanmax(np.abs(fresh["tr_solve", 5][0])) > 0 and np.abs(fresh["solve_host", 3][0]).max() > 0
    assert np.abs(fresh["scene_report", 3][0]).max() > 0 and np.isfinite(fresh["plant_track", 3][1]).all()


def test_steady_state_allocates_nothing_and_growth_keeps_no_generation(fresh):
    model, prob, _ = _case()
    N, nq = prob.num_steps, model.nq
    one, two = _single(), _batch()
    for _ in range(2):
        _round(one, two)
    free0 = _free()
    for _ in range(20):
        got = _round(one, two)
    free1 = _free()
    print(f"steady state: free device memory fell by {free0 - free1} bytes over 20 rounds")
    assert free0 - free1 < MIB
    assert all(_same(a, b) for key, arrays in got.items() for a, b in zip(arrays, fresh[key[0], key[1]]))
    # the statistics rows and the solve's staging grow at every step: 20 generations of each, which sum to more than 4 MiB
    # of rows and 6 MiB of staging - the context may hold the last generation of each, not the ones before it
    iters, nrhs = 150, 200
    row_bytes, rhs_bytes = 17 * 8, (N + 1) * nq * 8
    generations = sum(k * (iters * row_bytes + 2 * nrhs * rhs_bytes) for k in range(1, 21))
    final = 20 * (iters * row_bytes + 2 * nrhs * rhs_bytes)
    assert generations > 8 * MIB and final < MIB
    for k in range(1, 21):
        one.set_q(_q()); one.eval_tau()
        try:
            one.tr_solve(k * iters, 2, True, False, 1e-1, 1e5)
        except hip.FactorizationFailed:   # (only the memory is looked at here)
            pass
        solve_host(one, k * nrhs)
    free2 = _free()
    print(f"growth: free device memory fell by {free1 - free2} bytes; the last generation is {final} bytes, all of them {generations}")
    assert free1 - free2 <= final + MIB
    one.close(); two.close()


def _begin(dev, times=1):
    """MPC storage and plants in hold mode begun `times` times each -> the stored plans and the plants' states after a step"""
    model, prob, _ = _case()
    N, nq, nv = prob.num_steps, model.nq, model.nv
    rng = np.random.default_rng(3)
    q_plan = np.array([_case()[1].q_nom + 0.01 * b for b in range(B)])
    v_plan, tau_plan = rng.uniform(-0.3, 0.3, (B, N + 1, nv)), rng.uniform(-2, 2, (B, N, nv))
    for _ in range(times):
        dev.mpc_batch_begin(np.zeros(nq, dtype=np.int32), tc.actuated(NAME))
    plans = dev.mpc_batch_store(q_plan, v_plan, tau_plan, np.array([0.0, 0.1]))
    for _ in range(times):
        dev.plant_begin(H)
    dev.plant_set_state(np.zeros(B), np.array([np.concatenate([q_plan[b, 0], v_plan[b, 0]]) for b in range(B)]))
    _, status = dev.plant_step(3, tau_plan[:, 0])
    return [plans, status] + list(dev.plant_get_state())


def test_begin_again_and_destroy_return_everything():
    once = _batch()
    ref = _begin(once)
    once.close()
    dev = _batch()
    for rep in range(10):   # on one context: the storage of the begin before is returned at the next
        got = _begin(dev, times=2)
        if rep == 0:
            free0 = _free()
    free1 = _free()
    assert all(_same(a, b) for a, b in zip(got, ref))
    dev.close()
    print(f"begin again: free device memory changed by {free0 - free1} bytes over 9 repetitions")
    assert abs(free0 - free1) < MIB
    for rep in range(10):   # ... and a context's end returns it all
        dev = _batch()
        got = _begin(dev, times=2)
        dev.close()
        if rep == 0:
            free0 = _free()
    free1 = _free()
    assert all(_same(a, b) for a, b in zip(got, ref))
    print(f"destroy and create: free device memory changed by {free0 - free1} bytes over 9 repetitions")
    assert abs(free0 - free1) < MIB


def test_close_with_everything_made(fresh):
    one, two = _single(), _batch()
    _round(one, two)
    _begin(two)
    one.trial_cost(_q())
    for dev in (one, two):   # (the staging of the uploads that do not wait, both buffers)
        dev.set_option("async_uploads", 1)
        for _ in range(3):
            dev.set_problem(_case()[1])
        dev.sync()
    one.close(); two.close()
    one, two = _single(), _batch()
    got = _round(one, two)
    assert all(_same(a, b) for key, arrays in got.items() for a, b in zip(arrays, fresh[key[0], key[1]]))
    one.close(); two.close()
