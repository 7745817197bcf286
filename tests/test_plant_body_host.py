"""csrc/plant.h plant_body on the host, as a whole block: the device text compiled by g++ over tests/cpp/lane_emu (a lane is
an OS thread; __syncthreads and the exchange points are barriers) - no GPU.

tests/cpp/plant_body_host_check.cc runs the block with 64 to 256 threads inside exactly the LDS bytes that the host would
request (plant_lds_doubles, plus plant_pd_doubles for PD+): everything behind them is poisoned for the address sanitizer,
everything inside starts as NaN.  The bar is == throughout: M_out and bias_out against the CPU oracle, a_out, the hold
rollout and PD+ against csrc/plant_step.h and csrc/mpc_spline.h run serially on the oracle's numbers, the status words of
a NaN input and of a zero pivot.  It includes plant_body<8, true, true>, the stem route that the device does not
instantiate, on punyo at every block size that fits: the C++ text of that route is right on the
abstract machine; what differed on the device is below the text (lane_emu/hip/hip_runtime.h says what that covers).

The program prints a line per (model, instantiation, mode, block) with the rounds the evaluations went in and equal/compared
plants; the tests assert the whole set of lines.
"""
import copy
import os

import numpy as np
import pytest

import lane_emu as le
import plant_cases as pc
from idto_amd.model import load_model
from idto_amd.problem import SolverParameters

H = 1e-3
MODELS = pc.MODELS + ["punyo"]
INST = {"acrobot": "2", "hopper": "3", "mini_cheetah": "3", "allegro_hand": "4", "jaco_ball": "8", "dual_jaco": "8x", "punyo": "8xs",
        "pendulum": "2"}
BLOCKS = [0, 64, 128, 192, 256]
# what PlantBlock's rule gives (the program restates it from plant_lds_doubles and is told punyo's to assert it) ...
DEFAULT = {"acrobot": 64, "hopper": 64, "mini_cheetah": 128, "allegro_hand": 128, "jaco_ball": 64, "dual_jaco": 64, "punyo": 128,
           "pendulum": 64}
# ... and the forced sizes whose LDS does not fit 160 KiB (the program prints `nofit` for one): none of these models has one
NOFIT = set()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return le.build("plant_body_host_check", tmp_path_factory.mktemp("plant_body_host"))


def write_case(out_dir, label, dev, orc, sp, plants, kind="finite", blocks=BLOCKS, default_block=0, pd=None):
    path = os.path.join(str(out_dir), label + ".case")
    with open(path, "w") as f:
        f.write(f"label {label}\ndev {le.save_model(dev, out_dir, label + '_dev')}\norc {le.save_model(orc, out_dir, label + '_orc')}\n")
        f.write(f"contact {le.fmt(le.contact_values(sp))}\nh {H!r}\nkind {kind}\ndefault_block {default_block}\n")
        f.write(f"blocks {len(blocks)} {' '.join(str(b) for b in blocks)}\n")
        if pd is None:
            f.write("pd 0\n")
        else:
            act, Kp, Kd, ff = pd
            f.write(f"pd 1 {len(act)} {' '.join(str(a) for a in act)}\n{le.fmt(Kp)}\n{le.fmt(Kd)}\n{int(ff)}\n")
        f.write(f"plants {len(plants)}\n")
        for t0, q, v, tau in plants:
            f.write(f"{t0!r}\n{le.fmt(q)}\n{le.fmt(v)}\n{le.fmt(tau)}\n")
    return path


def hopper_gains(model, cfg):
    """Kp [nu][nq], Kd [nu][nv] of the hopper configuration: its gain on each actuated dof's own position / velocity"""
    act = [j for j in range(model.nv) if int(model.actuated[j])]
    Kp, Kd = np.zeros((len(act), model.nq)), np.zeros((len(act), model.nv))
    for r, j in enumerate(act):
        Kp[r, j + model.nq - model.nv], Kd[r, j] = cfg["Kp"][j], cfg["Kd"][j]
    assert np.count_nonzero(Kp) == len(act) == 2 and np.count_nonzero(Kd) == 2
    return act, Kp, Kd, True


def rounds(model, threads):
    groups = threads // model.npaths
    return -(-(model.nv + 1) // groups)


def finite_case(out_dir, name):
    dev, orc, cfg = pc.case(name)
    sp = pc.problem(name)[1]
    plants = [(0.25 + 0.5 * b, q, v, tau) for b, (q, v, tau) in enumerate(pc.states(name))]
    assert len(plants) == 3
    pd = hopper_gains(orc, cfg) if name == "hopper" else None
    path = write_case(out_dir, name, dev, orc, sp, plants, default_block=DEFAULT[name], pd=pd)
    want = []
    for forced in BLOCKS:
        if (name, forced) in NOFIT:
            want.append(f"{name} {INST[name]} nofit {forced}")
            continue
        T = forced or DEFAULT[name]
        for mode in ["fd", "hold"] + (["pd"] if pd else []):
            want.append(f"{name} {INST[name]} {mode} {T} rounds={rounds(orc, T)} 3/3")
    return path, want


def run_and_compare(exe, paths, want):
    rc, lines, err = le.run(exe, paths)
    assert rc == 0 and lines[-1] == "ok: every line equal", "\n".join(lines[-40:]) + err[-6000:]
    assert [l for l in lines[:-1] if not l.startswith("edump ")] == want
    return lines, err


@pytest.mark.parametrize("name", MODELS)
def test_block_equals_the_oracle_and_the_host_restatement(exe, tmp_path, name):
    """forward dynamics at B = 3 (M_out, bias_out == the oracle, a_out == plant_step.h's solve on them), a hold rollout of 3
    substeps and, on the hopper, 2 substeps of PD+ - at the default block and at forced 64, 128, 192, 256 where the LDS fits"""
    path, want = finite_case(tmp_path, name)
    run_and_compare(exe, [path], want)


def test_rounds_and_single_rounds_both_run():
    """a model with more than one wavefront of lanes runs in rounds at 64 threads and in one round from 128 on; punyo's
    default is 128 threads (73,880 B of LDS), the configuration that differed on the device"""
    for name in ("mini_cheetah", "punyo"):
        model = pc.case(name)[1]
        assert (model.nv + 1) * model.npaths > 64
        assert rounds(model, 64) == 2 and rounds(model, 128) == 1
    assert DEFAULT["punyo"] == 128


def zero_pivot_pendulum():
    m = copy.deepcopy(load_model("pendulum"))
    m.mass = np.zeros_like(np.asarray(m.mass, dtype=float))
    m.inertia = np.zeros_like(np.asarray(m.inertia, dtype=float))
    return m.normalize()


def test_status_words(exe, tmp_path):
    """a NaN among the inputs: (2, 0); a mass matrix with a zero pivot (the pendulum with mass and inertia 0): (1, 0) - each
    with the state untouched, and forward dynamics leaves a_out alone"""
    name = "hopper"
    dev, orc, _ = pc.case(name)
    plants = []
    for b, (q, v, tau) in enumerate(pc.states(name)):
        q, v, tau = q.copy(), v.copy(), tau.copy()
        (q, v, tau)[b][1] = np.nan   # (plant 0: a position, plant 1: a velocity, plant 2: a torque)
        plants.append((1.0, q, v, tau))
    paths = [write_case(tmp_path, "hopper_nan", dev, orc, pc.problem(name)[1], plants, kind="nonfinite", blocks=[0])]
    want = ["hopper_nan 3 nonfinite 64 rounds=1 3/3", "hopper_nan 3 nonfinite_fd 64 rounds=1 3/3"]
    pend = zero_pivot_pendulum()
    plants = [(0.0, np.array([0.3]), np.array([0.1]), np.array([0.2]))]
    paths.append(write_case(tmp_path, "pendulum_massless", pend, pend, SolverParameters(verbose=False), plants, kind="pivot", blocks=[0, 128]))
    want += [w for T in (64, 128) for w in (f"pendulum_massless 2 pivot {T} rounds=1 1/1", f"pendulum_massless 2 pivot_fd {T} rounds=1 1/1")]
    run_and_compare(exe, paths, want)


def test_thread_sanitizer_finds_only_the_dump_row(tmp_path):
    """the finite cases again under the thread sanitizer: a missing __syncthreads() or wave_exchange_point() in plant.h or
    id_eval.h is a data race of the emulation's threads.  The one race that plant.h has by design - the surplus groups all
    write the write-only dump row `edump` - is accepted, by address: both accesses writes inside the row.  (The non-finite
    path's flag[0] = 1 from several lanes is a same-value store and is not run here.)"""
    reason = le.tsan_unavailable(tmp_path)
    if reason:
        pytest.skip(reason)
    exe = le.build("plant_body_host_check", tmp_path, le.TSAN)
    for name in MODELS:
        path, want = finite_case(tmp_path, name)
        rc, lines, err = le.run(exe, [path])
        rows = [tuple(int(x, 16) for x in l.split()[1:]) for l in lines if l.startswith("edump ")]
        assert len(rows) == 1
        assert le.unexpected_tsan_reports(err, rows[0]) == [], err[-6000:]
        assert lines[-1] == "ok: every line equal" and [l for l in lines[:-1] if not l.startswith("edump ")] == want
