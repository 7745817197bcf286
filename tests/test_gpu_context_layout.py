"""The arena plan of host/context_layout.cc and the option table of idto_hip.hip, on the device: the pointers the library
hands to its kernels lie where tests/golden/context_layout.txt says (the fixture tests/test_context_layout.py holds the plan
to on the CPU), a problem of a batch is found at its arena stride, the solver-only context of the KKT step still serves
the constrained loop, and every option keeps its name, its bounds, its messages and its environment variable.  The names
and the places are listed HERE, by hand: the test does not read the library's tables."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from idto_amd import hip
from idto_amd.model import load_model
from idto_amd.problem import SCALING, load_config, make_problem, synthetic_trajectory

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# array id -> (the arena entry it lies in, which band of that entry); None: no contiguous device array
PLACES = {"q": ("q", 0), "v": ("v", 0), "a": ("a", 0), "nplus": ("nplus", 0), "gradient": ("g", 0), "H_A": ("HA", 0),
          "H_B": ("HA", 1), "H_C": ("HA", 2), "step": ("step", 0), "cost": ("cost", 0), "slab": ("slab", 0), "debug": ("dbg", 0),
          "hbands": ("HA", 0), "tr_dq": ("tr_dq", 0), "tr_w": ("tr_w", 0), "tr_scale": ("tr_D", 0), "asm_terms": ("terms", 0),
          "tau": None, "dtau_dqm": None, "dtau_dqt": None, "dtau_dqp": None}


def _fixture_offsets(kind, nq, nv, N):
    head = f"{kind} nq {nq} nv {nv} N {N} :"
    with open(os.path.join(ROOT, "tests", "golden", "context_layout.txt")) as f:
        line = [ln for ln in f if ln.startswith(head)]
    assert len(line) == 1
    tok = line[0][len(head):].split()
    return {tok[i]: int(tok[i + 1]) for i in range(0, len(tok), 2)}


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def test_device_pointers_lie_where_the_fixture_says_and_problem_1_at_the_arena_stride():
    N, B = 3, 2
    cfg, model = load_config("acrobot"), load_model("acrobot")
    probs, qs = [], []
    for b in range(B):
        prob, sp, _ = make_problem(cfg, model, num_steps=N)
        sp.equality_constraints = False
        prob.q_nom = prob.q_nom + 0.01 * b
        prob.Qq = prob.Qq * (1.0 + 0.1 * b)
        probs.append(prob)
        qs.append(synthetic_trajectory(cfg, model, N, seed=b, lower=0.01))
    at = _fixture_offsets("model", model.nq, model.nv, N)
    band = (N + 6) * model.nq * model.nq * 8
    batch = hip.HipPath(model, probs, sp)
    # (before the step: a pointer to the bands or the slab makes the context treat them as written from outside)
    q0 = batch.device_ptr("q")
    for name, place in PLACES.items():
        p = batch.device_ptr(name)
        if place is None:
            assert p is None, name
        else:
            assert p - q0 == at[place[0]] + place[1] * band - at["q"], name
    assert batch.device_ptr("con_S") is None and batch.device_ptr("con_lambda") is None   # (no constraint step yet)
    assert batch.slab_stride == 3 * model.nv * model.nq + model.nv
    batch.close()
    batch, one = hip.HipPath(model, probs, sp), hip.HipPath(model, probs[1], sp)
    # (the step in its separate launches in both: the one-workgroup and the fused launch of a single small problem keep
    # the assembly's per-record products in LDS and never write IDTO_ARR_ASM_TERMS)
    for dev in (batch, one):
        dev.set_option("gn_small", 0)
        dev.set_option("fused", 0)
    batch.set_q_batch(np.array(qs))
    batch.eval_tau()
    batch.gn_step()
    one.set_q(qs[1])
    one.eval_tau()
    one.gn_step()
    assert batch.get_option("last_assembly") == one.get_option("last_assembly") != 0
    for name in PLACES:
        assert batch.array_size(name) == one.array_size(name) >= 1, name
        assert _same(batch.get(name, 1), one.get(name)), name
    assert batch.array_size("con_S") == -1 and batch.array_size("con_lambda") == -1
    assert not _same(batch.get("step", 0), batch.get("step", 1))   # (two different problems)
    one.close()
    batch.close()


def test_constrained_loop_through_the_kkt_context_follows_the_schur_complement_chain():
    """hopper, N = 3, enforced equality constraints: two iterations through the solver-only KKT context (the default)
    against the Schur-complement chain (option con_kkt 0).  Different algorithms, so the tolerances of
    tests/test_gpu_trust_region.py's comparison of the constrained loops: costs, merits and |q| 1e-6 relative, |h| 1e-4,
    the radii the same sequence, the trust ratios' signs, the same steps accepted."""
    N = 3
    cfg, model = load_config("hopper"), load_model("hopper")
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    q = synthetic_trajectory(cfg, model, N, seed=1, lower=0.01)
    rows = {}
    for kkt in (1, 0):
        dev = hip.HipPath(model, prob, sp)
        dev.set_option("con_kkt", kkt)
        dev.set_q(q)
        dev.eval_tau()
        rows[kkt], _ = dev.tr_solve(2, SCALING["double_sqrt"], True, False, 1e-1, 1e5, constrained_dofs=model.unactuated_dofs)
        assert (dev.get_option("kkt_last_solver") != 0) == (kkt == 1)
        dev.close()
    a, b = rows[1], rows[0]
    for col, tol in ((0, 1e-6), (1, 1e-12), (15, 1e-6), (8, 1e-4), (3, 1e-6)):   # cost, radius, merit, |h|, |q|
        assert np.allclose(a[:, col], b[:, col], rtol=tol, atol=1e-12), (col, a[:, col], b[:, col])
    assert np.array_equal(a[:, 2] > 0, b[:, 2] > 0) and np.array_equal(a[:, 9], b[:, 9]) and np.array_equal(a[:, 14], b[:, 14])
    assert (a[:, 14] == 0).all()


# name: (values to set, what get_option returns for each)
READ_WRITE = {name: ((0, 1, 5, 0), (0, 1, 1, 0)) for name in (
    "reference_solver", "two_sided", "fused", "async_uploads", "nd_recursion", "solver_nd", "solver_pipe", "gn_small",
    "asm_in_solver", "asm_fold", "con_kkt", "kkt_fold", "tr_small", "tr_fold", "kkt_in_asm", "decide_in_solver", "fd_fast")}
READ_WRITE.update({"solver_band": ((0, 2, 1), (0, 2, 1)), "ls_waves": ((7, 64, 0), (7, 64, 0)), "gradients_method": ((2, 1, 0), (2, 1, 0)),
                   "nd_min_rows": ((24, 3, 16), (24, 16, 16))})
WRITE_ONLY = {"solver_debug": (1, 2, 0), "debug_skip_role": (2, -1), "debug_pipe_tail": (1, 0), "fused_debug": (1, 0), "asm_stop": (1, 0),
              "fd_stop": (1, 0)}
READ_ONLY = ("last_solver", "weights_diagonal", "solver_timeouts", "ls_solves", "ls_batch_solves", "tr_resident_ok", "kkt_last_solver",
             "last_assembly", "fast_shape", "model_batch")
# the variables that seed a default at create: (option, a value that is not the default, what the option then reads)
ENVIRONMENT = {"IDTO_SOLVER_REFERENCE": ("reference_solver", "1", 1), "IDTO_TWO_SIDED": ("two_sided", "0", 0), "IDTO_FUSED": ("fused", "0", 0),
               "IDTO_ND_MIN_ROWS": ("nd_min_rows", "24", 24), "IDTO_ND_RECURSION": ("nd_recursion", "0", 0),
               "IDTO_SOLVER_ND": ("solver_nd", "0", 0), "IDTO_SOLVER_PIPE": ("solver_pipe", "0", 0), "IDTO_ASM_FOLD": ("asm_fold", "0", 0),
               "IDTO_CON_KKT": ("con_kkt", "0", 0), "IDTO_KKT_FOLD": ("kkt_fold", "0", 0), "IDTO_DEBUG_SKIP_ROLE": (None, "2", None),   # (write-only: nothing reads it back; the child launches nothing)
               "IDTO_TR_SMALL": ("tr_small", "0", 0), "IDTO_TR_FOLD": ("tr_fold", "0", 0), "IDTO_KKT_IN_ASM": ("kkt_in_asm", "0", 0),
               "IDTO_DECIDE_IN_SOLVER": ("decide_in_solver", "0", 0), "IDTO_SOLVER_BAND": ("solver_band", "2", 2)}
DEFAULTS = {"reference_solver": 0, "two_sided": 1, "fused": 1, "nd_min_rows": 16, "nd_recursion": 1, "solver_nd": 1, "solver_pipe": 1,
            "asm_fold": 1, "con_kkt": 1, "kkt_fold": 1, "tr_small": 1, "tr_fold": 1, "kkt_in_asm": 1, "decide_in_solver": 1, "solver_band": 1}


def _acrobot():
    cfg, model = load_config("acrobot"), load_model("acrobot")
    prob, sp, _ = make_problem(cfg, model, num_steps=3)
    return hip.HipPath(model, prob, sp)


def _refused(call, text):
    with pytest.raises(hip.HipError) as e:
        call()
    assert str(e.value).endswith(text), str(e.value)


def test_every_option_keeps_its_name_its_bounds_and_its_messages():
    dev = _acrobot()
    if not any(var in os.environ for var in ENVIRONMENT):
        for name, value in DEFAULTS.items():
            assert dev.get_option(name) == value, name
    for name, (values, reads) in READ_WRITE.items():
        for v, r in zip(values, reads):
            dev.set_option(name, v)
            assert dev.get_option(name) == r, (name, v)
    for name, values in WRITE_ONLY.items():
        for v in values:
            dev.set_option(name, v)
        _refused(lambda: dev.get_option(name), "unknown option " + name)
    for name in READ_ONLY:
        assert isinstance(dev.get_option(name), int)
        _refused(lambda: dev.set_option(name, 1), "unknown option " + name)
    _refused(lambda: dev.set_option("rccl_version", 1), "unknown option rccl_version")
    for bad in (-1, 65):
        _refused(lambda: dev.set_option("ls_waves", bad), "ls_waves: 0 (planned) .. IDTO_LS_MAX_CANDIDATES candidates per wave")
    for bad in (-1, 3):
        _refused(lambda: dev.set_option("gradients_method", bad), "gradients_method: 0 forward, 1 central, 2 central4 (autodiff needs Drake)")
    assert dev.get_option("ls_waves") == 0 and dev.get_option("gradients_method") == 0   # (a refused value changes nothing)
    _refused(lambda: dev.set_option("no_such_option", 1), "unknown option no_such_option")
    _refused(lambda: dev.get_option("no_such_option"), "unknown option no_such_option")
    dev.close()


CHILD = """
import json, sys
from idto_amd import hip
from idto_amd.model import load_model
from idto_amd.problem import load_config, make_problem
cfg, model = load_config("acrobot"), load_model("acrobot")
prob, sp, _ = make_problem(cfg, model, num_steps=3)
dev = hip.HipPath(model, prob, sp)
print("OPTIONS " + json.dumps({name: dev.get_option(name) for name in sys.argv[1:]}))
dev.close()
"""


def test_environment_variables_seed_the_defaults_in_a_fresh_process():
    env = dict(os.environ)
    env.update({var: value for var, (_, value, _) in ENVIRONMENT.items()})
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    names = [name for name, _, _ in ENVIRONMENT.values() if name]
    run = subprocess.run([sys.executable, "-c", CHILD] + names, env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    got = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("OPTIONS ")][0][len("OPTIONS "):])
    assert got == {name: reads for name, _, reads in ENVIRONMENT.values() if name}
    assert all(got[name] != DEFAULTS[name] for name in got)
