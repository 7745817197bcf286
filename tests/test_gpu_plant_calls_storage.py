"""The plant family's calls share one kind of storage - a device buffer with a pinned mirror, grown on demand (csrc/idto_hip.hip
GrownBuffer; the layouts are csrc/host/plant_calls.h's): the scene report, the linearisation, the gains, the tracked rollouts and
the two in one pass on ONE context of two acrobots, each with 1 state, then 3 (every buffer grows, while the others' are live),
then 1 again (the larger buffers are reused).  The bar is ==, NaN placement and status words included, against the same call on
a fresh context; afterwards the context still solves a step like a fresh one.  Nothing here is near a limit and no call fails.
"""
import numpy as np
import pytest

import lin_cases as lc
import track_cases as tc
from idto_amd import hip

pytestmark = pytest.mark.gpu

NAME, B, R, H, M = "acrobot", 2, 2, 1e-3, 2
ARRAYS = {hip.SceneReport: ("bodies", "pairs", "tau_contact", "tau_pairs"), hip.Tvlqr: ("x_next", "A", "B", "lin_status", "K", "P", "status"),
          hip.Track: ("x", "u", "dx", "status")}


def _context():
    model, _, prob, sp, _, _ = lc.case(NAME)
    return hip.HipPath(model, [prob] * B, sp)


def _inputs(S):
    """problem b's from seed b -> (x_nom [B, S + 1, w], tau_nom [B, S, nv], K [B, S, nu, n], x0 [B, R, w], actuated, (Q, R, Qf))"""
    per = [tc.inputs(NAME, S, R, seed=b) for b in range(B)]
    act = per[0][4]
    return tuple(np.array([p[k] for p in per]) for k in range(4)) + (act, tc.weights(lc.case(NAME)[0].nv, len(act), 5))


CALLS = {
    "scene_report": lambda dev, S, x, tau, K, x0, act, w: dev.scene_report(x[:, :S], pair_rows=True),
    "plant_linearize": lambda dev, S, x, tau, K, x0, act, w: dev.plant_linearize(x[:, :S], tau, H, M),
    "plant_tvlqr": lambda dev, S, x, tau, K, x0, act, w: dev.plant_tvlqr(x[:, :S], tau, H, M, act, *w),
    "plant_track": lambda dev, S, x, tau, K, x0, act, w: dev.plant_track(x, tau, K, x0, H, M, act),
    "plant_tvlqr_track": lambda dev, S, x, tau, K, x0, act, w: dev.plant_tvlqr_track(x, tau, x0, H, M, act, *w),
}


def _arrays(result):
    """every array of a call's result, by name"""
    if isinstance(result, tuple):
        return {f"[{i}]": a for i, a in enumerate(result)}
    out = {k: getattr(result, k) for k in ARRAYS[type(result)]}
    if getattr(result, "tvlqr", None) is not None:
        out.update({"tvlqr." + k: v for k, v in _arrays(result.tvlqr).items()})
    return out


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all((a == b) | ((a != a) & (b != b))))


def _solve_a_step(dev):
    prob = lc.case(NAME)[2]
    dev.set_q_batch(np.array([prob.q_nom + 0.01 * (b + 1) for b in range(B)]))
    dev.gn_step()
    assert dev.solver_status_batch() == [False] * B
    return [dev.get(arr, b) for b in range(B) for arr in ("gradient", "step", "tau")]


def test_grown_and_reused_buffers_give_what_a_fresh_context_gives():
    fresh = {}
    for S in (1, 3):
        for call, run in CALLS.items():
            one = _context()
            fresh[call, S] = _arrays(run(one, S, *_inputs(S)))
            one.close()
    dev = _context()
    for S in (1, 3, 1):
        for call, run in CALLS.items():
            got = _arrays(run(dev, S, *_inputs(S)))
            assert got.keys() == fresh[call, S].keys()
            for k, ref in fresh[call, S].items():
                assert _same(got[k], ref), (call, S, k)
    # (the calls did something: the law acts, the report has bodies, nothing ended early)
    assert fresh["plant_tvlqr_track", 3]["status"].tolist() == [[[0, 3 * M]] * R] * B and fresh["plant_tvlqr", 3]["status"].tolist() == [0] * B
    assert np.abs(fresh["scene_report", 3]["bodies"]).max() > 0 and np.isfinite(fresh["plant_track", 3]["u"]).all()
    one = _context()
    ref = _solve_a_step(one)
    one.close()
    assert all(_same(a, b) for a, b in zip(_solve_a_step(dev), ref))
    dev.close()
