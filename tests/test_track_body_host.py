"""csrc/plant.h plant_body<..., LAW = true> - track_kernel's body, the plants under the time-varying LQR law - on the host as a
whole block: the device text compiled by g++ over tests/cpp/lane_emu (a lane is an OS thread; __syncthreads and the exchange
points are barriers) - no GPU, nothing loaded into Python.

tests/cpp/track_body_host_check.cc runs the block inside exactly the LDS bytes that the host would request (plant_lds_doubles +
plant_law_doubles): everything behind them is poisoned for the address sanitizer, everything inside starts as NaN.  The bar is
== against the serial composition, step by step: csrc/tvlqr_step.h tvlqr_control, then the host rollout (the oracle's bias and
mass matrix, csrc/plant_step.h's solve and step - tests/plant_cases.py host_rollout's operations) under the resulting torque.
S = 2 steps of m = 2 substeps, R = 2 rollouts, every case cut into two launches by first_step; a rollout whose status word is
not 0 must be left alone by a launch.
"""
import pytest

import lane_emu as le
import lin_cases as lc
import plant_cases as pc
import track_cases as tc

H, S, M, R = 1e-3, 2, 2, 2
# (model, the forced block sizes - 0: the host's rule -, the instantiation, the block the rule gives)
CASES = [("acrobot", [0], "2", 64), ("hopper", [0], "3", 64), ("mini_cheetah", [64, 128], "3", 128), ("dual_jaco", [0], "8x", 64),
         ("punyo", [0], "8xs", 128)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return le.build("track_body_host_check", tmp_path_factory.mktemp("track_body_host"))


def rounds(model, threads):
    groups = threads // model.npaths
    return -(-(model.nv + 1) // groups)


def write_case(out_dir, name, blocks):
    dev, orc, _ = pc.case(name)
    sp = pc.problem(name)[1]
    x_nom, tau_nom, K, x0, act = tc.inputs(name, S, R)
    path = str(out_dir / (name + ".case"))
    with open(path, "w") as f:
        f.write(f"label {name}\ndev {le.save_model(dev, out_dir, name + '_dev')}\norc {le.save_model(orc, out_dir, name + '_orc')}\n")
        f.write(f"contact {le.fmt(le.contact_values(sp))}\nh {H!r}\nblocks {len(blocks)} {' '.join(str(b) for b in blocks)}\n")
        f.write(f"{S} {M} {R} {len(act)} {' '.join(str(int(a)) for a in act)}\n")
        f.write(f"{le.fmt(x_nom)}\n{le.fmt(tau_nom)}\n{le.fmt(K.swapaxes(-1, -2))}\n{le.fmt(x0)}\n")   # (K column-major)
    return path


def expected(name, blocks, inst, default):
    model = pc.case(name)[1]
    return [f"{name} {inst} track {b or default} rounds={rounds(model, b or default)} {R}/{R}" for b in blocks]


def test_the_cases_cover_what_they_are_for():
    """nu = 1; a planar joint with an active contact in the nominal's first state; evaluations in rounds and in one; the exchange
    form and the stem"""
    assert len(tc.actuated("acrobot")) == 1
    q0 = pc.states("hopper")[0][0]
    assert -0.03 < pc.oracle("hopper").signed_distances(q0)[0].min() < 0.0
    cheetah = pc.case("mini_cheetah")[1]
    assert rounds(cheetah, 64) == 2 and rounds(cheetah, 128) == 1
    assert [c[2] for c in CASES] == ["2", "3", "3", "8x", "8xs"]
    assert lc.case("dual_jaco")[0].nq == pc.case("dual_jaco")[0].nq


@pytest.mark.parametrize("name,blocks,inst,default", CASES)
def test_block_equals_the_serial_composition(exe, tmp_path, name, blocks, inst, default):
    rc, lines, err = le.run(exe, [write_case(tmp_path, name, blocks)])
    assert rc == 0 and lines[-1] == "ok: every line equal", "\n".join(lines[-40:]) + err[-6000:]
    assert [l for l in lines[:-1] if not l.startswith("edump ")] == expected(name, blocks, inst, default)


def test_thread_sanitizer_finds_only_the_dump_row(tmp_path):
    """the cases again under the thread sanitizer: a missing __syncthreads() or wave_exchange_point() around the law's staging,
    its deviation or its torque is a data race of the emulation's threads.  The one race that plant.h has by design - the surplus
    groups all write the write-only dump row `edump` - is accepted, by address, as tests/test_plant_body_host.py accepts it."""
    reason = le.tsan_unavailable(tmp_path)
    if reason:
        pytest.skip(reason)
    exe = le.build("track_body_host_check", tmp_path, le.TSAN)
    for name, blocks, inst, default in CASES:
        rc, lines, err = le.run(exe, [write_case(tmp_path, name, blocks)])
        rows = [tuple(int(x, 16) for x in l.split()[1:]) for l in lines if l.startswith("edump ")]
        assert len(rows) == 1
        assert le.unexpected_tsan_reports(err, rows[0]) == [], err[-6000:]
        assert lines[-1] == "ok: every line equal" and [l for l in lines[:-1] if not l.startswith("edump ")] == expected(name, blocks, inst, default)
