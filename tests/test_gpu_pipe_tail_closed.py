"""The pipelined solver's producers take their back substitution in closed form (penta_pipe.h pipe_closed_tail,
DESIGN.md 5.2): at the smallest shapes where it can go wrong, against the recursion walked row after row
(`debug_pipe_tail` = 2, the form before) and the row-by-row substitution (= 1) on the same system.

Bars (tests/test_gpu_solver_accuracy.py's): forward error <= 4 x the pivoted LU's + 16 unc + 1e-12 against
oracle_lib.refined_solution; componentwise backward error <= 1e-12 row by row, <= min(1e-11, max(1e-12, LU's / 100)) for
the two recursion-form tails; the three solutions agree to within the sum of their forward-error bars.
tests/test_tail_closed_form.py holds the same arithmetic to 1e-12 on the CPU."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
import solver_cases as sc
from idto_amd import hip
from idto_amd.model import load_model
from idto_amd.problem import load_config, make_problem, synthetic_trajectory
from test_gpu_batch import _problems
from test_gpu_penta import DeviceSolver

pytestmark = pytest.mark.gpu

TAILS = (0, 2, 1)   # closed form for the producers (default), the recursion row after row, row by row
PIPE = dict(gn_small=0, solver_band=0, solver_pipe=1, solver_nd=1)


# ---- solver_layout.h and host/solver_plan.cc nd_split, restated for K = 19: which horizons the closed form takes
def ldl_ks(K):
    return 4 * ((K + 3) // 4) + 2


def pipe_xall(K, spike):
    """pipe_layout<K>(n, spike).xall: where rt of the local rows begins - what the back substitution may use"""
    KE, KR, GS, NCX = K + (K & 1), 4 * ((K + 3) // 4), ldl_ks(K), 3 * K + 1
    oz = 3 * KE + 2 + 2 * K + 3 + 8
    used = oz + 1 + ((oz + 1) & 1) + 2 * KE + 1
    RS = ((used + 15) // 32) * 32 + 16
    rlo = 16 if K >= 17 else ((((K + 1) // 2 + 1) & ~1) if K >= 3 else K)
    nhi = K - rlo
    o = 3 * KR * RS + 2 * NCX * GS + 2 + 2 * (KE + 2 + 2 * K) * GS
    o += (NCX + (2 * K if spike else 0) + 1) * (nhi + (nhi & 1)) + 2
    o += (2 if spike else 1) * 49 * 18 if K >= 17 else 0
    o += (3 * K + 2) * KE if spike else 0
    return o


def back_bs(K, spike):
    KE = K + (K & 1)
    ys0 = max(2 * KE, ldl_ks(K))
    ys = ys0 + (2 if ys0 % 8 == 0 else 0)
    return K * ys * (2 if spike else 1) + KE


def recursion_fits(K, nj, np_):
    KE = K + (K & 1)
    return nj * back_bs(K, True) + 4 * KE + 2 <= pipe_xall(K, True) and np_ * back_bs(K, False) + 4 * KE + 2 <= pipe_xall(K, False)


def closed_fits(K, np_):
    """penta_pipe.h pipe_closed_fits: PipeClosed<K>::end(nloc) <= xall"""
    KE = K + (K & 1)
    ts0 = 2 * KE + 2
    slot = K * (ts0 + (2 if ts0 % 8 == 0 else 0))
    return np_ * back_bs(K, False) + 4 * KE + 2 + (np_ + 2) * slot <= pipe_xall(K, False) and np_ * K <= 512


def chains(n):
    """(longest joiner, longest producer) of nd_split(n, pipe = true)"""
    s = (n - 2) // 2
    rows = lambda half: max(1, min(int(0.52 * (half - 2) + 0.6), half - 3))
    j1, j2 = rows(s), n - rows(n - s - 2) - 2
    return max(s - j1, j2 - s), max(j1, n - j2 - 2)


def test_the_restated_layout_knows_the_documented_carve_up():
    """tests/golden/solver_plan.txt, K = 19 n = 40 on the pipelined kernel: 159280 bytes of LDS (a joiner's carve-up: rt of
    34 local rows, x_sep and the flags behind xall), s = 19, j1 = 9, j2 = 29 - producers of 9 rows, joiners of 10"""
    assert (pipe_xall(19, True) + 34 * 22 + 42 + 32) * 8 == 159280
    assert chains(40) == (10, 9) and recursion_fits(19, 10, 9) and closed_fits(19, 9)


def fit_limit(K=19):
    """(the last horizon whose producers take the closed form, the first that does not although the recursion form still fits)"""
    last = max(n for n in range(16, 64) if recursion_fits(K, *chains(n)) and closed_fits(K, chains(n)[1]))
    assert recursion_fits(K, *chains(last + 1)) and not closed_fits(K, chains(last + 1)[1])
    return last, last + 1


# ---- one cheetah system per (horizon, seed), shared and left unchanged
@functools.lru_cache(maxsize=None)
def cheetah(N, seed=0):
    cfg, model = load_config("mini_cheetah"), load_model("mini_cheetah")
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    q = synthetic_trajectory(cfg, model, N, seed=seed, lower=0.01)
    g, bands = ol.Oracle(model, prob, sp).grad_hess(q)
    H = ol.penta_make_dense(*bands)
    p_ref, unc = ol.refined_solution(H, -g.ravel())
    for a in (q, g, H, p_ref):
        a.setflags(write=False)
    return model, prob, sp, q, g, H, p_ref, unc


def cheetah_steps(N, tails=TAILS):
    """{tail: step} of one context, and the pivoted LU's step"""
    model, prob, sp, q, g, H, p_ref, unc = cheetah(N)
    dev = hip.HipPath(model, prob, sp)
    dev.set_q(q)
    dev.set_option("reference_solver", 1)
    dev.gn_step()
    p_lu = dev.get("step")
    dev.set_option("reference_solver", 0)
    for name, v in PIPE.items():
        dev.set_option(name, v)
    steps = {}
    for tail in tails:
        dev.set_option("debug_pipe_tail", tail)
        dev.gn_step()
        assert dev.get_option("last_solver") == 4 and dev.solver_status() == (False, 0)
        assert np.array_equal(dev.get("gradient"), g)
        steps[tail] = dev.get("step")
    dev.close()
    return steps, p_lu


def held_to_the_bars(H, b, steps, x_lu, x_ref, unc, tag):
    fwd_lu, bwd_lu = sc.errors(H, b, x_lu, x_ref)
    bar = 4 * fwd_lu + 16 * unc + 1e-12
    for tail, x in steps.items():
        fwd, bwd = sc.errors(H, b, x, x_ref)
        cap = 1e-12 if tail == 1 else min(1e-11, max(1e-12, 0.01 * bwd_lu))
        print(f"{tag} tail {tail}: fwd {fwd:.3e} (LU {fwd_lu:.3e}, unc {unc:.1e}) bwd {bwd:.2e} (LU {bwd_lu:.2e}, cap {cap:.1e})")
        assert fwd <= bar, (tag, tail, "forward error", fwd, "LU", fwd_lu, "unc", unc)
        assert bwd <= cap, (tag, tail, "componentwise backward error", bwd, "cap", cap)
    scale = np.abs(x_ref).max()
    tails = list(steps)
    for i, a in enumerate(tails):
        for c in tails[i + 1:]:
            assert np.abs(steps[a].ravel() - steps[c].ravel()).max() / scale <= 2 * bar, (tag, a, c)


@pytest.mark.parametrize("N", [16, 17, 40])
def test_three_tails_on_the_cheetah(N):
    """N = 16, 17: the shortest horizons the pipelined kernel takes (producers of three rows, an even and an odd split)"""
    _, _, _, _, g, H, p_ref, unc = cheetah(N)
    steps, p_lu = cheetah_steps(N)
    assert not np.array_equal(steps[0], steps[2]), "the closed form did not run: the case tests nothing"
    assert not np.array_equal(steps[2], steps[1])
    held_to_the_bars(H, -g.ravel(), steps, p_lu, p_ref, unc, f"cheetah N {N}")


def test_three_tails_on_a_nine_joint_star():
    """revolute_star(9), n = 16 block rows, a directed matrix of cond 1e10: blocks of 9 are padded to 16, which the
    two-workgroup kernel serves - every setting of the option has to leave it alone"""
    c = sc.case(9, 16, 1e10)
    s = DeviceSolver(9, 16)
    s.set_bands(*c.bands[:3])
    x_lu = s.solve(c.b, reference=True)
    steps = {tail: s.solve(c.b, debug_pipe_tail=tail) for tail in TAILS}
    assert s.dev.solver_status() == (False, 0)
    s.close()
    assert np.array_equal(steps[0], steps[2]) and np.array_equal(steps[0], steps[1])
    held_to_the_bars(c.H, c.b, steps, x_lu, c.x_ref, c.unc, "star 9")


def test_fit_fallback_on_either_side_of_the_limit():
    """K = 19: up to nine producer rows the T_i fit behind [Y | Z | c]; the first horizon past that takes the recursion
    row after row in all four chains and equals debug_pipe_tail = 2 bit for bit"""
    last, past = fit_limit()
    assert chains(last)[1] == 9 and chains(past)[1] == 10
    _, _, _, _, g, H, p_ref, unc = cheetah(last)
    steps, p_lu = cheetah_steps(last, (0, 2))
    assert not np.array_equal(steps[0], steps[2])
    held_to_the_bars(H, -g.ravel(), steps, p_lu, p_ref, unc, f"cheetah N {last}")
    steps, _ = cheetah_steps(past, (0, 2))
    assert np.array_equal(steps[0], steps[2])


def test_twenty_solves_give_the_same_bits():
    model, prob, sp, q, *_ = cheetah(16)
    dev = hip.HipPath(model, prob, sp)
    dev.set_q(q)
    dev.gn_step()
    assert dev.get_option("last_solver") == 4
    first = dev.get("step")
    for i in range(19):   # (every launch has its own epoch: flags, counters and flagged words of the last one are stale)
        dev.gn_step() if i & 1 else dev.factor_solve()
        assert np.array_equal(dev.get("step"), first), i
    assert dev.solver_status() == (False, 0)
    dev.close()


def test_a_batch_equals_its_problems_solved_alone():
    model, probs, sp, qs = _problems("mini_cheetah", 16, 3)
    batch = hip.HipPath(model, probs, sp)
    batch.set_q_batch(qs)
    batch.gn_step()
    assert batch.get_option("last_solver") == 4 and batch.solver_status_batch() == [False] * 3
    for b in range(3):
        one = hip.HipPath(model, probs[b], sp)
        one.set_q(qs[b])
        one.gn_step()
        assert one.get_option("last_solver") == 4
        assert np.array_equal(batch.get("step", b), one.get("step")), b
        one.close()
    batch.close()
