"""Shared by tests/test_plant_step.py and tests/test_gpu_plant*.py: the models, three deterministic states each (the first
with an active contact where the model has pairs) and the host restatement of a plant's substep - the oracle's inverse
dynamics for the bias and the mass-matrix columns, libidto_opt.so's exports of csrc/plant_step.h for the solve and the
step.  Everything is computed once per process and never changed."""
import copy
import ctypes as C
import functools
import os

import numpy as np

from idto_amd import optimizer
from idto_amd.model import dptr, iptr, load_model
from idto_amd.problem import load_config, make_problem
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = os.path.join(ROOT, "tests", "golden", "examples")
FLOATING = 3

MODELS = ["acrobot", "hopper", "mini_cheetah", "allegro_hand", "jaco_ball", "dual_jaco"]


def _all_gravity(model):
    m = copy.deepcopy(model)
    m.gravity_enabled = None
    return m.normalize()


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (the device's model, the oracle's model, the configuration).  The example fixtures switch some bodies' weight
    off, which the oracle's one gravity vector cannot say: they run with every weight on.  punyo: zero-length capsules on
    the device (its spheres, bit for bit), spheres in the oracle, as tests/test_gpu_stem.py builds it."""
    if name == "punyo":
        from test_model_stem import all_gravity, as_spheres, punyo, zero_length
        model, cfg = punyo()
        return zero_length(all_gravity(model)), as_spheres(all_gravity(model)), cfg
    if name in ("jaco_ball", "dual_jaco"):
        model = _all_gravity(load_model(os.path.join(EXAMPLES, name + ".model")))
        return model, model, load_config(os.path.join(EXAMPLES, name + ".yaml"))
    model = load_model(name)
    return model, model, load_config(name)


def problem(name, N=3, model=None):
    dev_model, orc_model, cfg = case(name)
    prob, sp, _ = make_problem(cfg, model if model is not None else orc_model, num_steps=N)
    return prob, sp


@functools.lru_cache(maxsize=None)
def oracle(name):
    prob, sp = problem(name)
    return Oracle(case(name)[1], prob, sp)


def _normalized(model, q):
    q = np.array(q, dtype=float)
    for b in range(model.nbodies):
        if int(model.jtype[b]) == FLOATING:
            s = int(model.qstart[b])
            q[s:s + 4] /= np.linalg.norm(q[s:s + 4])
    return q


@functools.lru_cache(maxsize=None)
def states(name):
    """Three (q, v, tau_applied).  The first has an active contact (a pair that penetrates by less than 3 cm; a model without
    pairs: none), found by a fixed-seed scan of offsets from q_init with the oracle's signed distances; the others are
    random offsets of 0.1 from q_init.  Velocities within +-0.5, torques within +-2."""
    model, cfg = case(name)[1], case(name)[2]
    orc = oracle(name)
    rng = np.random.default_rng(20240 + len(name))
    q_init = np.asarray(cfg["q_init"], dtype=float)
    out = []
    if model.npairs:
        for t in range(4000):
            amp = (0.05, 0.2, 0.6, 1.2)[t % 4]
            q = _normalized(model, q_init + rng.uniform(-amp, amp, model.nq))
            phi = orc.signed_distances(q)[0]
            if -0.03 < phi.min() < 0.0:
                out.append(q)
                break
        assert out, name + ": the scan found no state with an active contact"
    while len(out) < 3:
        out.append(_normalized(model, q_init + rng.uniform(-0.1, 0.1, model.nq)))
    return [(q, rng.uniform(-0.5, 0.5, model.nv), rng.uniform(-2.0, 2.0, model.nv)) for q in out]


def solve_host(M, tau, c):
    """idto_plant_solve_host on M [row, col] (its lower triangle is read): (a, the failed pivot or -1)"""
    n = len(c)
    Mc = np.ascontiguousarray(np.asarray(M, dtype=float).T)   # column-major
    a = np.zeros(n)
    piv = optimizer.lib().idto_plant_solve_host(dptr(Mc), dptr(np.ascontiguousarray(tau, dtype=float)),
                                                dptr(np.ascontiguousarray(c, dtype=float)), n, dptr(a))
    return a, piv


def host_fd(orc, q, v, tau):
    """-> (a, M [row, col], c): the oracle's columns and bias, the exported header's solve"""
    nv = orc.nv
    zero = np.zeros(nv)
    M = np.zeros((nv, nv))
    for j in range(nv):
        e = np.zeros(nv)
        e[j] = 1.0
        M[:, j] = orc.inverse_dynamics(q, zero, e, full=False)
    c = orc.inverse_dynamics(q, v, zero)
    a, piv = solve_host(M, tau, c)
    assert piv == -1, piv
    return a, M, c


def advance_host(model, h, q, v, a):
    q, v = np.array(q, dtype=float), np.array(v, dtype=float)
    jt = np.ascontiguousarray(model.jtype, dtype=np.int32)
    qs = np.ascontiguousarray(model.qstart, dtype=np.int32)
    vs = np.ascontiguousarray(model.vstart, dtype=np.int32)
    optimizer.lib().idto_plant_advance_host(model.nbodies, iptr(jt), iptr(qs), iptr(vs), model.nq, float(h), dptr(q), dptr(v),
                                            dptr(np.ascontiguousarray(a, dtype=float)))
    return q, v


def host_rollout(orc, model, h, q, v, tau, substeps):
    """the states behind each of `substeps` substeps under the held torque: [substeps, nq + nv]"""
    out = np.zeros((substeps, model.nq + model.nv))
    for s in range(substeps):
        a = host_fd(orc, q, v, tau)[0]
        q, v = advance_host(model, h, q, v, a)
        out[s] = np.concatenate([q, v])
    return out
