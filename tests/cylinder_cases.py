"""The models and states that the cylinder tests share (tests/test_cylinder_host.py, tests/test_gpu_cylinder.py,
tests/test_model_cylinder.py): two small models with a cylinder, the directed states of every region of the
sphere-cylinder rule (include/idto_model.h) placed on them, and the trajectories of the frozen-oracle comparison.

A directed state is a point c in the cylinder's frame where one sphere's centre has to be.  It is placed by choosing the
CYLINDER'S pose for a fixed configuration: p = x - RX c, x the sphere's world centre there - a model per state.
  * hopper_on_cylinder: the hopper's ground box replaced by a world-fixed cylinder; the sphere is geometry 0 of the foot.
  * spinner_with_cylinder: spinner_sphere's spinner carries a cylinder in its sphere's place (a cylinder on a moving
    body); the sphere is finger_two's geometry 1.
The degenerate states - r == 0, the dr == dz tie, c.z == 0 - need c bit for bit.  On the hopper they get it: RX is a
signed permutation, the nonzero coordinates of c are dyadic and lie on world axes where x is in [0.5, 1), so that
x - (x - d) == d exactly, and x itself is one product and one sum of the oracle's body pose, which the device
reproduces bit for bit.  On the spinner the cylinder moves with a body whose rotation has no exact entries, so that it
takes the general states only; tests/test_cylinder_host.py also hands the degenerate states to signed_distance itself
in both role orders and with a rotated frame."""
import copy
import functools
import os

import numpy as np

import cylinder_ref as cyl
from capsule_ref import without_geometry
from idto_amd.model import load_model
from idto_amd.problem import load_config, make_problem, synthetic_trajectory
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = os.path.join(ROOT, "tests", "golden", "cylinder")
ROLES = ("sphere_first", "cylinder_first")
R_DIRECTED, H_DIRECTED = 0.25, 0.5

# name: (c in the cylinder's frame, needs c bit for bit)
STATES = {
    "side": ((0.2, 0.18, 0.3), False),
    "cap": ((0.1, -0.05, 0.52), False),
    "cap_below": ((-0.1, 0.05, -0.52), False),
    "rim": ((0.2, 0.18, 0.51), False),
    "rim_below": ((-0.2, -0.18, -0.51), False),
    "inside_side": ((0.2, 0.1, 0.1), False),
    "inside_cap": ((0.05, 0.02, -0.49), False),
    "r0_above_cap": ((0.0, 0.0, 0.52), True),
    "r0_inside_side": ((0.0, 0.0, 0.125), True),
    "r0_inside_cap": ((0.0, 0.0, 0.375), True),
    "tie": ((0.125, 0.0, 0.375), True),
    "tie_below": ((-0.125, 0.0, -0.375), True),
    "z0_outside": ((0.28125, 0.0, 0.0), True),
    "z0_inside": ((0.21875, 0.0, 0.0), True),
}
REGION = {"side": "side", "cap": "cap", "cap_below": "cap", "rim": "rim", "rim_below": "rim", "inside_side": "inside-side",
          "inside_cap": "inside-cap", "r0_above_cap": "cap", "r0_inside_side": "inside-side", "r0_inside_cap": "inside-cap",
          "tie": "inside-side", "tie_below": "inside-side", "z0_outside": "side", "z0_inside": "inside-side"}
GENERAL = [k for k, (_, exact) in STATES.items() if not exact]

# the cylinder's axis along world x, its x along world z: lying on its side, every entry exact
R_EXACT = np.array([[0.0, 0.0, 1.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0]])


def rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    M = np.eye(3)
    M[i, i], M[i, j], M[j, i], M[j, j] = c, -s, s, c
    return M


R_GENERAL = rot(2, 0.3) @ rot(0, np.pi / 2 + 0.2) @ rot(2, 0.7)


def base_problem(name):
    cfg = load_config("hopper" if name == "hopper" else "spinner")
    return cfg, load_model("hopper" if name == "hopper" else "spinner_sphere")


def with_cylinder(model, g_cyl, body, X_BG, R, H, role):
    """`model` with geometry g_cyl (its last) a cylinder on `body` at X_BG [12]; cylinder_first: registered first, so that
    it is side A of every pair it is in"""
    m = copy.deepcopy(model)
    assert g_cyl == m.ngeoms - 1 and all(int(b) == g_cyl for b in m.pair_b)
    m.geom_type[g_cyl], m.geom_body[g_cyl] = cyl.CYLINDER, body
    m.geom_size[g_cyl], m.geom_X[g_cyl] = [R, H, 0.0], X_BG
    if role == "cylinder_first":
        order = [g_cyl] + list(range(g_cyl))
        m.geom_type, m.geom_body = m.geom_type[order], m.geom_body[order]
        m.geom_size, m.geom_X = m.geom_size[order], m.geom_X[order]
        m.pair_b, m.pair_a = m.pair_a + 1, np.zeros_like(m.pair_a)
    else:
        assert role == "sphere_first"
    return m.normalize()


@functools.lru_cache(maxsize=None)
def _poses(name):
    cfg, model = base_problem(name)
    prob, sp, _ = make_problem(cfg, model, num_steps=2)
    return Oracle(without_geometry(model), prob, sp), sp


def body_poses(name, q):
    return _poses(name)[0].body_poses(np.asarray(q, float))


Q_DIRECTED = {"hopper": np.array([1.35, -0.62, 0.3, -0.5, 0.2]), "spinner": np.array([-0.4, 1.2, 0.35])}
# (slow enough that no pair separates at twice the dissipation velocity, where the force law gives zero)
V_DIRECTED = {"hopper": np.array([0.03, -0.02, 0.04, -0.05, 0.06]), "spinner": np.array([0.05, -0.07, 0.04])}
A_DIRECTED = {"hopper": np.array([1.0, -2.0, 0.5, 1.5, -1.0]), "spinner": np.array([-1.0, 2.0, 0.7])}
PLACED = {"hopper": (0, 2, 2), "spinner": (1, 1, 12)}   # the placed sphere, its body, the geometry the cylinder replaces


def sphere_centre(model, X_body, g):
    """the world centre of a sphere whose offset in its body has a z coordinate only: one product and one sum per
    coordinate, in whichever order the three terms are added"""
    off = np.asarray(model.geom_X[g][9:], float)
    assert off[0] == 0 and off[1] == 0
    b = int(model.geom_body[g])
    Rb, pb = X_body[b][:9].reshape(3, 3), X_body[b][9:]
    return pb + Rb[:, 2] * off[2]


def directed(name, state, role):
    """-> (model, q, v, a): the cylinder posed so that the placed sphere's centre is at STATES[state] in its frame"""
    c, exact = STATES[state]
    assert name == "hopper" or not exact
    c = np.array(c)
    cfg, base = base_problem(name)
    q = Q_DIRECTED[name]
    X = body_poses(name, q)
    g_sph, b_sph, g_cyl = PLACED[name]
    assert int(base.geom_body[g_sph]) == b_sph
    x = sphere_centre(base, X, g_sph)
    RX = R_EXACT if exact else R_GENERAL
    d = RX @ c
    if exact:   # (x - d is a double, and x - (x - d) == d: module docstring)
        assert all(0.5 <= x[i] < 1.0 for i in range(3) if d[i] != 0), x
    p = x - d
    if name == "hopper":
        body, X_BG = -1, np.concatenate([RX.ravel(), p])
    else:   # the cylinder on the spinner: its pose in the body's frame
        body = 2
        Rb, pb = X[body][:9].reshape(3, 3), X[body][9:]
        X_BG = np.concatenate([(Rb.T @ RX).ravel(), Rb.T @ (p - pb)])
    model = with_cylinder(base, g_cyl, body, X_BG, R_DIRECTED, H_DIRECTED, role)
    return model, q, V_DIRECTED[name], A_DIRECTED[name]


def directed_labels():
    return [("hopper", s) for s in STATES] + [("spinner", s) for s in GENERAL]


def expected_pairs(model, q, name):
    """cylinder_ref's phi, n, Ca, Cb of every pair of `model` at q -> [npairs] dicts"""
    X = body_poses(name, q)
    out = []
    for k in range(model.npairs):
        ga, gb = int(model.pair_a[k]), int(model.pair_b[k])
        a_is_sphere = int(model.geom_type[ga]) == cyl.SPHERE
        gs, gc = (ga, gb) if a_is_sphere else (gb, ga)
        assert int(model.geom_type[gc]) == cyl.CYLINDER
        x = sphere_centre(model, X, gs)
        RX, p = cyl.geom_world(model, X, gc)
        out.append(cyl.sphere_cylinder(x, float(model.geom_size[gs][0]), p, RX, float(model.geom_size[gc][0]),
                                       float(model.geom_size[gc][1]), sphere_is_A=a_is_sphere))
    return out


# ---- the models of the trajectory tests
def hopper_on_cylinder(role="sphere_first", radius=0.5):
    """the hopper above a world-fixed cylinder lying on its side across its path (axis along world y, turned a little
    about it), the top of the cylinder at z = 0 under the hopper's start"""
    _, base = base_problem("hopper")
    RX = rot(0, np.pi / 2) @ rot(2, 0.4)
    return with_cylinder(base, 2, -1, np.concatenate([RX.ravel(), [0.0, 0.0, -radius]]), radius, 2.0, role)


def spinner_with_cylinder(role="sphere_first"):
    """spinner_sphere with the spinner's sphere (radius 0.25 at z = -0.25 of the body) replaced by a cylinder whose axis lies
    in the fingers' plane (the body's x), turned about it: the fingers meet its side, its rims and its caps as it turns"""
    _, base = base_problem("spinner")
    RX = rot(1, np.pi / 2) @ rot(2, 0.6)
    return with_cylinder(base, 12, 2, np.concatenate([RX.ravel(), [0.0, 0.0, -0.25]]), 0.2, 0.3, role)


def hills(heights=None):
    """(model, cfg) of tests/golden/cylinder/mini_cheetah_hills; heights: the hills' heights instead of the fixture's 0.05"""
    model = load_model(os.path.join(FIXTURES, "mini_cheetah_hills.model"))
    cfg = load_config(os.path.join(FIXTURES, "mini_cheetah_hills.yaml"))
    if heights is not None:
        model = copy.deepcopy(model)
        cyls = [g for g in range(model.ngeoms) if int(model.geom_type[g]) == cyl.CYLINDER]
        for g, h in zip(cyls, heights):
            model.geom_X[g][11] = -1.0 + h
        model = model.normalize()
    return model, cfg


def trajectory(name, N):
    """-> (model, cfg, q [N + 1, nq]) of the frozen-oracle comparison: the cylinder pairs act at N / 2 steps or more"""
    if name == "hopper_on_cylinder":
        cfg, model = load_config("hopper"), hopper_on_cylinder()
        q = synthetic_trajectory(cfg, model, N, seed=0, lower=0.01)
        q[:, 1] = np.linspace(0.0, -0.35, N + 1)                 # along the cylinder's top and down its side
        q[:, 0] -= 0.5 - np.sqrt(0.25 - np.minimum(q[:, 1] ** 2, 0.2))
    elif name == "spinner_with_cylinder":
        cfg, model = load_config("spinner"), spinner_with_cylinder()
        q = synthetic_trajectory(cfg, model, N, seed=0)
        q[:, 1] = np.linspace(1.5, 1.25, N + 1)
        q[:, 2] = np.linspace(0.0, 1.0, N + 1)
    else:
        assert name == "mini_cheetah_hills"
        model, cfg = hills()
        q = synthetic_trajectory(cfg, model, N, seed=0, lower=0.02)
        q[:, 4] = np.linspace(0.95, 2.45, N + 1)                 # the base carried across the first hill (x = 2)
    return model, cfg, q


# ---- the frozen-oracle comparison's cases and the conditions on them
FROZEN = {"hopper_on_cylinder": 20, "spinner_with_cylinder": 20, "mini_cheetah_hills": 8}   # the horizons


def frozen_case(name):
    N = FROZEN[name]
    model, cfg, q = trajectory(name, N)
    prob, sp, _ = make_problem(cfg, model, num_steps=N)
    sp.scaling = sp.equality_constraints = False
    sp.gradients_method = "forward_differences"
    return model, prob, sp, q, N


def hill_and_ground_together(model, prob, sp, q):
    """whether at some time step a hill pair and a ground pair are within the threshold together, by the oracle on the
    frozen models"""
    fr = cyl.Frozen(model, prob, sp)
    types = lambda k: (int(model.geom_type[int(model.pair_a[k])]), int(model.geom_type[int(model.pair_b[k])]))
    hill = np.array([cyl.CYLINDER in types(k) for k in range(model.npairs)])
    ground = np.array([int(model.geom_body[int(model.pair_b[k])]) < 0 and types(k)[1] == cyl.BOX for k in range(model.npairs)])
    for t in range(1, prob.num_steps + 1):
        orc = Oracle(cyl.frozen_model(model, fr.base.body_poses(q[t])), prob, sp)
        near = orc.signed_distances(q[t])[0] <= orc.contact_threshold
        if (near & hill).any() and (near & ground).any():
            return True
    return False
