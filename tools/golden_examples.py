"""What tools/make_golden.py and tools/make_golden_traj.py share for the example models of tests/golden/examples/
(jaco, jaco_ball, dual_jaco, spinner_capsule, 2dof_spinner_capsule, punyo): the capsule rules, written from the
specification text of include/idto_model.h, the model variants the set conditions compare with, and the recipes of the
states.  Nothing here is imported from tests/, oracle/ or idto_amd/csrc; the arithmetic works in whatever floating-point
type its inputs have (double or long double).

Capsules.  A capsule side of a pair becomes a sphere of the capsule's radius at a substitute centre on its segment
p + u s, s in [-h, h], u = column 2 of the geometry's world rotation:
  * against a sphere at x: the point of the segment closest to x;
  * against a capsule: the closest points of the two segments, found by minimising the quadratic
    |p1 + u1 s - p2 - u2 t|^2 over the rectangle [-h1, h1] x [-h2, h2]: the interior stationary point, if it lies
    inside, and the minimum along each of the four edges are compared and the smallest kept (not the clamp sequence of
    Ericson 5.1.9 that the kernels use).  Two candidates that are as small to 1e-9 but lie apart stop the generator;
  * against a world-fixed box of identity rotation: the segment end with the lower world z.
What geometry cannot decide - which end on equal heights, what parallel segments do, the 1e-10 threshold for
"parallel" - is not decided here either: `Margins` records how far every stored state stays from those cases, and
the generators refuse a state that comes closer than MIN_DZ / MIN_SIN2.  Only pairs that could act count: a pair whose
signed distance is beyond the contact threshold whichever end or point is taken exerts no force under any convention.

Cylinders (tools/make_golden.py cylinder; tests/golden/cylinder/).  `sphere_cylinder` is the closed form of
include/idto_model.h written out once more: the nearest point of the rectangle [0, R] x [-H, H] in the plane through the
axis and the sphere's centre, and inside the nearer of the side and a cap.  The six stored states of the cheetah on hills
keep every foot far from a hill's axis (r == 0) and from the dr == dz tie - a foot's centre that is inside a hill is
centimetres below its side and metres from its caps -, so that neither unpinned choice of the rule is asked of this
restatement.

States.  The recipes restate the trajectory helpers of the tests (tests/test_model_cross_pairs.py touching_trajectory,
tests/test_model_stem.py punyo_trajectory, tests/test_gpu_capsule.py frozen_case); tests/test_golden_examples.py
rebuilds every stored q from those helpers and compares.

Directed contact states (the last section; tools/make_golden.py contact): the labels of a contact pair's branches, the
margins every stored state keeps from the branch boundaries, and the names of a box's regions."""
import copy
import math
import os

import numpy as np

from idto_amd.model import load_model
from idto_amd.problem import load_config, make_problem, synthetic_trajectory

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
EXAMPLES = os.path.join(ROOT, "tests", "golden", "examples")
SPHERE, BOX, CAPSULE, CYLINDER = 0, 1, 2, 4
MIN_DZ = 1e-3      # capsule-box: least |z(+h end) - z(-h end)| [m]
MIN_SIN2 = 1e-3    # capsule-capsule: least 1 - dot(u1, u2)^2
UNIQUE = 1e-9      # capsule-capsule: two minimisers count as one below this distance in (s, t) [m]
MIN_CHANGE = 1e-3  # a set of pairs acts when it changes tau by more than this (the tests' MIN_CHANGE)
MATTERS = 1e-3     # "the capsules' length / the gravity switch matters": relative change of tau
ARMS = 14          # dual_jaco: DoFs 0-13 are the two arms'
HUMANOID = 14      # punyo: bodies / DoFs 0-13 are the humanoid's, body 14 is the ball
PUNYO_CLASSES = ["arm-ball", "arm-ground", "ball-ground", "ball-torso", "ball-waist", "ground-torso"]
CONTACT_KEYS = ("contact_stiffness", "dissipation_velocity", "stiction_velocity", "friction_coefficient", "smoothing_factor")
TWO_DOF_CFG = dict(q_init=[1.0, 0.0], v_init=[0.0, 0.0], q_nom_start=[1.0, 0.0], q_nom_end=[1.0, 1.0], q_guess=[1.0, 0.0],
                   Qq=[1, 1], Qv=[0.1, 0.1], R=[0.1, 1e3], Qfq=[10, 10], Qfv=[0.1, 0.1], time_step=0.05, num_steps=20,
                   contact_stiffness=200, dissipation_velocity=0.1, smoothing_factor=0.01, friction_coefficient=0.5,
                   stiction_velocity=0.05)


# ---- capsule rules
class Margins:
    """smallest distance of the recorded states from the cases the specification decides by convention"""

    def __init__(self):
        self.capsule_box_dz = None
        self.capsule_capsule_sin2 = None

    def note(self, key, value):
        value = float(value)
        old = getattr(self, key)
        setattr(self, key, value if old is None else min(old, value))

    def as_dict(self):
        return dict(capsule_box_dz=self.capsule_box_dz, capsule_capsule_sin2=self.capsule_capsule_sin2,
                    min_capsule_box_dz=MIN_DZ, min_capsule_capsule_sin2=MIN_SIN2,
                    rule="over the pairs that are within the contact threshold for some point of the segment(s); "
                         "null: the model has no such pair")


def closest_on_segment(x, p, u, h):
    s = (x - p) @ u
    s = min(max(s, -h), h)
    return p + u * s, s


def closest_of_two_segments(p1, u1, h1, p2, u2, h2):
    """(s, t) minimising |p1 + u1 s - p2 - u2 t|^2 over [-h1, h1] x [-h2, h2], and 1 - dot(u1, u2)^2"""
    r = p1 - p2
    b = u1 @ u2
    sin2 = 1 - b * b
    dist2 = lambda s, t: (r + u1 * s - u2 * t) @ (r + u1 * s - u2 * t)
    cands = []
    if sin2 > 0:   # the stationary point of the quadratic: s - b t = -u1.r, -b s + t = u2.r
        c, f = u1 @ r, u2 @ r
        s, t = (b * f - c) / sin2, (f - b * c) / sin2
        if -h1 <= s <= h1 and -h2 <= t <= h2:
            cands.append((s, t))
    for s in (-h1, h1):   # an edge s = const: the point of segment 2 closest to that end of segment 1
        cands.append((s, closest_on_segment(p1 + u1 * s, p2, u2, h2)[1]))
    for t in (-h2, h2):
        cands.append((closest_on_segment(p2 + u2 * t, p1, u1, h1)[1], t))
    vals = [dist2(s, t) for s, t in cands]
    best = int(np.argmin(vals))
    for (s, t), val in zip(cands, vals):
        apart = max(abs(s - cands[best][0]), abs(t - cands[best][1]))
        if apart > UNIQUE and abs(np.sqrt(val) - np.sqrt(vals[best])) <= UNIQUE:
            raise SystemExit(f"capsule-capsule: the closest points are not unique: (s, t) = {cands[best]} and {(s, t)}")
    return cands[best][0], cands[best][1], sin2


def reduce_capsules(tA, XA, sA, bodyA, tB, XB, sB, bodyB, threshold=None, margins=None):
    """(centre of A, centre of B) after the capsule reduction: for a capsule its substitute centre, otherwise the
    geometry's own origin.  XA, XB: 4 x 4 world poses.  With `margins`, the pair's distance from the conventions is
    noted and a pair that could act closer to them than MIN_DZ / MIN_SIN2 stops the generator."""
    pA, pB = XA[:3, 3], XB[:3, 3]
    uA, uB = XA[:3, 2], XB[:3, 2]
    rA, hA, rB, hB = sA[0], sA[1], sB[0], sB[1]
    if tA == CAPSULE and tB == CAPSULE:
        s, t, sin2 = closest_of_two_segments(pA, uA, hA, pB, uB, hB)
        cA, cB = pA + uA * s, pB + uB * t
        if margins is not None and min(hA, hB) > 0:
            # the segments' closest approach bounds every choice of points from below
            if np.sqrt((cB - cA) @ (cB - cA)) - rA - rB <= threshold:
                margins.note("capsule_capsule_sin2", sin2)
                if sin2 < MIN_SIN2:
                    raise SystemExit(f"capsule-capsule: 1 - dot(u1, u2)^2 = {float(sin2)} < {MIN_SIN2}")
        return cA, cB

    def against(t_me, p_me, u_me, h_me, r_me, t_other, X_other, s_other, body_other):
        if t_other == SPHERE:
            return closest_on_segment(X_other[:3, 3], p_me, u_me, h_me)[0]
        assert t_other == BOX and body_other < 0, "capsule-box: the box must be fixed to the world"
        assert np.array_equal(np.asarray(X_other[:3, :3], float), np.eye(3)), "capsule-box: the box must not be rotated"
        ends = [p_me + u_me * h_me, p_me - u_me * h_me]
        dz = abs(ends[0][2] - ends[1][2])
        low = ends[0] if ends[0][2] < ends[1][2] else ends[1]
        if margins is not None and h_me > 0:
            top = X_other[2, 3] + s_other[2]
            if low[2] - top - r_me <= threshold:   # (the lower end is the closer one whatever the convention)
                margins.note("capsule_box_dz", dz)
                if dz < MIN_DZ:
                    raise SystemExit(f"capsule-box: the two ends differ by {float(dz)} m < {MIN_DZ} in height")
        return low

    cA, cB = pA, pB
    if tA == CAPSULE:
        cA = against(tA, pA, uA, hA, rA, tB, XB, sB, bodyB)
    if tB == CAPSULE:
        cB = against(tB, pB, uB, hB, rB, tA, XA, sA, bodyA)
    return cA, cB


# ---- the sphere-cylinder rule, written from include/idto_model.h (Drake's DistanceToPoint for a cylinder: the 2-D box
# [0, R] x [-H, H] of its cross-section in the plane through the axis and the point)
def sphere_cylinder(x, rho, X_cyl, R, H):
    """-> (phi, gW, the witness point on the sphere, the one on the cylinder); gW points from the cylinder's surface to
    the sphere's centre (outside) or from the centre to the nearest surface (inside), in the world"""
    RX, p = np.asarray(X_cyl[:3, :3], float), np.asarray(X_cyl[:3, 3], float)
    c = RX.T @ (np.asarray(x, float) - p)
    r = math.hypot(c[0], c[1])
    radial = np.array([c[0] / r, c[1] / r, 0.0]) if r > 0 else np.array([1.0, 0.0, 0.0])
    axial = np.array([0.0, 0.0, 1.0])
    if r > R or abs(c[2]) > H:   # outside: the nearest point of the rectangle, in (r, z)
        near = np.array([min(r, R), max(-H, min(H, c[2]))])
        away = np.array([r, c[2]]) - near
        dist = math.hypot(away[0], away[1])
        g2, phi = away / dist, dist - rho
    else:                        # inside: the nearer of the side and the cap, the side on a tie
        to_side, to_cap = R - r, H - abs(c[2])
        if to_side <= to_cap:
            g2, near, phi = np.array([1.0, 0.0]), np.array([R, c[2]]), -to_side - rho
        else:
            up = 1.0 if c[2] >= 0 else -1.0
            g2, near, phi = np.array([0.0, up]), np.array([r, up * H]), -to_cap - rho
    gW = RX @ (radial * g2[0] + axial * g2[1])
    return phi, gW, np.asarray(x, float) - gW * rho, p + RX @ (radial * near[0] + axial * near[1])


# ---- the cheetah on hills (tests/golden/cylinder): six states - feet on a hill, on the ground, in the air
CYLINDER_DIR = os.path.join(ROOT, "tests", "golden", "cylinder")
HILLS_STATES = [   # (source, the base's x, its z, pitch about y [rad])
    ("in the air", -1.0, 1.5, 0.0),
    ("on the ground in front of the hills", 0.5, 0.27, 0.0),
    ("front feet on the first hill's flank, rear feet on the ground", 1.55, 0.275, 0.0),
    ("over the first hill's top", 2.0, 0.315, 0.0),
    ("between the hills, pitched", 2.5, 0.28, 0.1),
    ("rear feet on the second hill's far flank, front feet on the ground", 3.42, 0.275, -0.05),
]


def hills_example():
    return (load_model(os.path.join(CYLINDER_DIR, "mini_cheetah_hills.model")),
            load_config(os.path.join(CYLINDER_DIR, "mini_cheetah_hills.yaml")))


def hills_state(cfg, source):
    """q of a state of HILLS_STATES: the YAML's q_init with the base moved and pitched"""
    (x, z, pitch), = [s[1:] for s in HILLS_STATES if s[0] == source]
    q = np.asarray(cfg["q_init"], float).copy()
    q[0:4] = [math.cos(pitch / 2), 0.0, math.sin(pitch / 2), 0.0]
    q[4], q[6] = x, z
    return q


# ---- models
def example(name):
    """(model, config) of tests/golden/examples; the 2-DoF spinner has no YAML of its own"""
    cfg = os.path.join(EXAMPLES, name + ".yaml")
    return load_model(os.path.join(EXAMPLES, name + ".model")), (load_config(cfg) if os.path.exists(cfg) else TWO_DOF_CFG)


def contact_parameters(cfg, model):
    sp = make_problem(cfg, model, num_steps=3)[1]
    return {k: float(getattr(sp, k)) for k in CONTACT_KEYS}


def with_zero_length_capsules(model):
    m = copy.deepcopy(model)
    for g in range(m.ngeoms):
        if int(m.geom_type[g]) == CAPSULE:
            m.geom_size[g] = [m.geom_size[g][0], 0.0, 0.0]
    return m.normalize()


def has_capsules(model):
    return any(int(t) == CAPSULE and model.geom_size[g][1] > 0 for g, t in enumerate(model.geom_type))


def has_switch(model):
    return not all(int(x) for x in model.gravity_enabled)


def pair_bodies(model, k):
    return int(model.geom_body[int(model.pair_a[k])]), int(model.geom_body[int(model.pair_b[k])])


def shared_pairs(model):
    """pairs that join chain bodies of two different paths"""
    out = []
    for k in range(model.npairs):
        paths = {int(model.body_path[b]) for b in pair_bodies(model, k) if b >= 0 and int(model.body_path[b]) >= 0}
        if len(paths) == 2:
            out.append(k)
    return out


def punyo_class(model, k):
    names = []
    for b in pair_bodies(model, k):
        names.append("ground" if b < 0 else "ball" if b == HUMANOID else "waist" if b == 0 else "torso" if b == 3 else "arm")
    return "-".join(sorted(names))


def stem_pairs(model):
    """pairs that touch a stem body below the common body"""
    stem = set(model.stem) - {int(model.common_body)}
    return [k for k in range(model.npairs) if stem & set(pair_bodies(model, k))]


# ---- trajectories: the tests' helpers restated
def punyo_trajectory(cfg, model, N, seed):
    q = synthetic_trajectory(cfg, model, N, seed=seed, lower=0.02)
    q[:, 0] = np.linspace(-0.20, -0.30, N + 1)
    q[:, 19] = np.linspace(0.30, 0.27, N + 1)
    return q


def spinner_capsule_trajectory(cfg, model):
    N = 40
    q = synthetic_trajectory(cfg, model, N, seed=0)
    q[:, 1] = np.linspace(1.5, 1.25, N + 1)
    q[:, 2] = np.linspace(0.0, 1.2, N + 1)
    return q


def two_dof_trajectory(cfg, model):
    N = 20
    q = synthetic_trajectory(cfg, model, N, seed=1)
    q[:, 0] = np.linspace(1.0, 1.4, N + 1)
    q[:, 1] = np.linspace(0.0, 0.3, N + 1)
    return q


def touching_trajectory(model, cfg, N, seed, shared_change, tries=2000):
    """tests/test_model_cross_pairs.py touching_trajectory: the same fixed-seed scan and the same criterion, with the
    change of tau by the shared pairs taken from `shared_change(q_t, v_t)` (the generator's own contact forces)
    instead of two oracle runs.  v_t = (q_t - q_{t-1}) / dt on the arms' revolute joints; the box does not move."""
    prob = make_problem(cfg, model, num_steps=N)[0]
    q_init = np.asarray(cfg["q_init"], dtype=float)
    rng = np.random.default_rng(seed)
    ramp = np.linspace(0.0, 1.0, N + 1)[:, None]
    for _ in range(tries):
        d, drift = np.zeros(model.nq), np.zeros(model.nq)
        d[:ARMS] = rng.uniform(-1.2, 1.2, ARMS)
        drift[:ARMS] = rng.uniform(-0.02, 0.02, ARMS)
        q = q_init + d + ramp * drift
        acting = 0
        for t in range(1, N + 1):
            v = np.zeros(model.nv)
            v[:ARMS] = (q[t, :ARMS] - q[t - 1, :ARMS]) / prob.time_step
            acting += shared_change(q[t], v) > MIN_CHANGE
        if acting >= N // 2:
            return q
    raise SystemExit("no touching state found")


# ---- the states of the state-level fixtures: name -> list of (source, q); `source` tells the test how to rebuild q
KANE_SEED = {"jaco": 31, "jaco_ball": 32, "dual_jaco": 33, "spinner_capsule": 34, "2dof_spinner_capsule": 35, "punyo": 36}


def kane_states(name, model, cfg, shared_change=None):
    """five states of the helpers' trajectories and one clear of every pair: a helper's state with a joint moved away
    (`set`: [index, value] pairs applied to q) and, where bodies float, those raised"""
    def take(helper, q, ts, set=(), **kw):
        out = []
        for t in ts:
            qt = np.array(q[t], float)
            for i, val in set:
                qt[i] = val
            out.append((dict(helper=helper, t=int(t), set=[list(x) for x in set], **kw), qt))
        return out

    if name in ("jaco", "jaco_ball"):
        q = synthetic_trajectory(cfg, model, 10, seed=0, lower=0.02)
        up = synthetic_trajectory(cfg, model, 10, seed=1, lower=-0.5)
        return take("synthetic_trajectory", q, (1, 3, 5, 7, 9), N=10, seed=0, lower=0.02) + \
            take("synthetic_trajectory", up, (4,), set=[(1, 3.14)], N=10, seed=1, lower=-0.5)
    if name == "dual_jaco":
        q = touching_trajectory(model, cfg, 20, 0, shared_change)
        up = synthetic_trajectory(cfg, model, 10, seed=1, lower=-0.5)
        return take("touching_trajectory", q, (2, 6, 10, 14, 18), N=20, seed=0) + \
            take("synthetic_trajectory", up, (4,), N=10, seed=1, lower=-0.5)
    if name == "spinner_capsule":
        q = spinner_capsule_trajectory(cfg, model)
        return take("frozen_case", q, (4, 12, 20, 28, 36)) + take("frozen_case", q, (8,), set=[(1, -1.0)])
    if name == "2dof_spinner_capsule":
        q = two_dof_trajectory(cfg, model)
        return take("frozen_case", q, (2, 6, 10, 14, 18)) + take("frozen_case", q, (4,), set=[(0, -1.0)])
    assert name == "punyo"
    q = punyo_trajectory(cfg, model, 10, 0)
    up = synthetic_trajectory(cfg, model, 10, seed=1, lower=-2.0)
    return take("punyo_trajectory", q, (1, 3, 5, 7, 10), N=10, seed=0) + \
        take("synthetic_trajectory", up, (4,), set=[(0, 0.3)], N=10, seed=1, lower=-2.0)


def traj_states(name, model, cfg, shared_change=None):
    """(source, q[4]) of the N = 3 trajectory fixtures"""
    if name == "dual_jaco":
        # (seed 1: the first seed whose hands reach into each other; seed 0's only come within reach of the force law)
        return dict(helper="touching_trajectory", N=3, seed=1), touching_trajectory(model, cfg, 3, 1, shared_change)
    if name == "spinner_capsule":
        q = spinner_capsule_trajectory(cfg, model)
        return dict(helper="frozen_case", rows=[20, 24]), q[20:24]
    assert name == "punyo"
    # punyo_trajectory keeps the ball 0.04 m from the arms and 0.11 m from the waist: those pairs act there only through
    # the smooth tail of the force law.  Here the ball is pushed 0.16 -> 0.15 m in front of the waist at 0.16 m height,
    # which puts an arm-ball pair ~0.015 m and the ball-waist pair (the stem's) ~0.02 m into penetration
    columns = [[19, 0.16, 0.15], [20, 0.16, 0.16]]
    q = punyo_trajectory(cfg, model, 3, 0)
    for i, start, end in columns:
        q[:, i] = np.linspace(start, end, 4)
    return dict(helper="punyo_trajectory", N=3, seed=0, columns=columns), q


# ---- directed contact states (tests/golden/contact/regions_<model>.json, tools/make_golden.py contact)
# Labels.  Every pair of every stored state is labelled from the generator's own arithmetic (Kane.signed_distance,
# Kane.pair_force), never from the oracle or the kernels:
#   kind         "sphere-sphere" | "sphere-box" | "box-box"
#   region       sphere-box: the clamped axes of the sphere's centre in the box frame with their signs, "+x" a face,
#                "+x-z" an edge, "-x+y+z" a corner; "in+x" the centre inside the box, leaving through +x.  Otherwise "-"
#   tie          "dx==dy" | "dy==dz" where the two smallest depths of an inside centre are EQUAL as doubles, else "-"
#   active       phi <= threshold
#   force        "softplus" | "linear" (exponent = -phi / smoothing_factor >= 37); "-" for an inactive pair
#   dissipation  s = v_n / dissipation_velocity: "approach" s < 0, "separate" 0 <= s < 2, "zero" s >= 2 (the pair is
#                active and its force is exactly zero); "-" inactive
#   friction     |v_t| / stiction_velocity: "none" < 1e-8 (the tangential velocity vanishes up to the generator's
#                numerical derivative), "stick" < 0.1, "slip" > 10, "mid" between; "-" inactive
# Margins.  Each state stays clear of every branch boundary by at least the MIN_* below, except the one boundary a state
# is aimed at ("just below the threshold"), where AIM_* holds instead; both are many orders above what double rounding
# of the few operations between q and the compared value can move (1e-16 relative): a label cannot depend on whose
# arithmetic evaluates it.
MIN_CLAMP = 1e-6     # [m] | |c_i| - h_i | of a sphere's centre from every clamp plane of its box
MIN_AXIS_GAP = 1e-6  # [m] second smallest depth - smallest depth of an inside centre (ties excepted: those are exact)
MIN_PHI = 1e-6       # [m] |phi - threshold|
AIM_PHI = 1e-8       # [m] the same for the states aimed at the threshold
MIN_EXPONENT = 1e-3  # |exponent - 37| of an active pair
AIM_EXPONENT = 1e-6  # the same for the states aimed at 37
MIN_S = 1e-3         # min(|s|, |s - 2|) of an active pair
MIN_VERTEX_DZ = 1e-6  # [m] box-box: second lowest vertex - lowest vertex
MIN_CENTRES = 0.02   # [m] sphere-sphere: distance of the centres (the normal is d / |d|)
REACH = 1e-3         # [m] n, Ca, Cb are stored for the pairs with phi <= threshold + REACH: the active ones and the
                     # ones aimed just above the threshold
STICK, SLIP, NONE = 0.1, 10.0, 1e-8


class ContactMargins:
    """smallest distance of the stored states from each branch boundary; `aimed` is the set of boundaries the state under
    evaluation is aimed at ("phi", "exponent"): AIM_* instead of MIN_* holds there, for the pair `aimed_pair` only"""
    KEYS = ("clamp", "axis_gap", "phi", "phi_aimed", "exponent", "exponent_aimed", "s", "vertex_dz", "centres")

    def __init__(self):
        self.least = {k: None for k in self.KEYS}

    def check(self, key, value, bound, what):
        value = float(value)
        if value < bound:
            raise ValueError(f"{what}: {key} margin {value} < {bound}")
        old = self.least[key]
        self.least[key] = value if old is None else min(old, value)

    def merge(self, other):
        for k, val in other.least.items():
            if val is not None:
                self.least[k] = val if self.least[k] is None else min(self.least[k], val)

    def as_dict(self):
        return dict(least=self.least,
                    bound=dict(clamp=MIN_CLAMP, axis_gap=MIN_AXIS_GAP, phi=MIN_PHI, phi_aimed=AIM_PHI, exponent=MIN_EXPONENT,
                               exponent_aimed=AIM_EXPONENT, s=MIN_S, vertex_dz=MIN_VERTEX_DZ, centres=MIN_CENTRES),
                    rule="least over all pairs of all states; *_aimed: the pair a state aims at that boundary; null: no "
                         "such pair")


def box_region(c, h):
    """(region, tie, distance from the clamp planes, gap of the two smallest depths or None)"""
    c, h = np.asarray(c, float), np.asarray(h, float)
    clamp = float(np.abs(np.abs(c) - h).min())
    out = "".join(("+" if c[i] > h[i] else "-") + "xyz"[i] for i in range(3) if abs(c[i]) > h[i])
    if out:
        return out, "-", clamp, None
    depth = h - np.abs(c)
    order = np.argsort(depth, kind="stable")
    ax = int(order[0])
    tie = "-"
    if depth[order[0]] == depth[order[1]]:
        tie = {(0, 1): "dx==dy", (1, 2): "dy==dz"}.get((int(order[0]), int(order[1])), "other")
    return "in" + ("+" if c[ax] >= 0 else "-") + "xyz"[ax], tie, clamp, float(depth[order[1]] - depth[order[0]])


def contact_labels(kane, model, X, q, v, aimed=None, what=""):
    """per pair: dict(kind, region, tie, active, force, dissipation, friction, phi[, n, Ca, Cb]); and the ContactMargins of
    the state.  X: the generator's body poses at q (make_golden.fk).  aimed: {"phi": pair} / {"exponent": pair}.  Raises
    ValueError when a margin is missed."""
    aimed = aimed or {}
    margins = ContactMargins()
    vs, vd = kane.cp["stiction_velocity"], kane.cp["dissipation_velocity"]
    pairs = []
    for k, (ga, gb) in enumerate(zip(model.pair_a, model.pair_b)):
        ga, gb = int(ga), int(gb)
        types = sorted((int(model.geom_type[ga]), int(model.geom_type[gb])))
        kind = {(SPHERE, SPHERE): "sphere-sphere", (SPHERE, BOX): "sphere-box", (BOX, BOX): "box-box"}[tuple(types)]
        detail = {}
        phi, n, Ca, Cb = kane.signed_distance(ga, gb, X, detail)
        lab = dict(kind=kind, region="-", tie="-", active=bool(phi <= kane.threshold), force="-", dissipation="-",
                   friction="-", phi=float(phi))
        w = f"{what} pair {k}"
        if kind == "sphere-box":
            lab["region"], lab["tie"], clamp, gap = box_region(detail["c"], detail["h"])
            margins.check("clamp", clamp, MIN_CLAMP, w)
            if gap is not None and lab["tie"] == "-":
                margins.check("axis_gap", gap, MIN_AXIS_GAP, w)
        elif kind == "box-box":
            z = detail["vertex_z"]
            margins.check("vertex_dz", z[1] - z[0], MIN_VERTEX_DZ, w)
        else:
            margins.check("centres", phi + model.geom_size[ga][0] + model.geom_size[gb][0], MIN_CENTRES, w)
        if aimed.get("phi") == k:
            margins.check("phi_aimed", abs(phi - kane.threshold), AIM_PHI, w)
        else:
            margins.check("phi", abs(phi - kane.threshold), MIN_PHI, w)
        if lab["active"]:
            pf = kane.pair_force(q, v, X, ga, gb)
            if aimed.get("exponent") == k:
                margins.check("exponent_aimed", abs(pf["exponent"] - 37), AIM_EXPONENT, w)
            else:
                margins.check("exponent", abs(pf["exponent"] - 37), MIN_EXPONENT, w)
            margins.check("s", min(abs(pf["s"]), abs(pf["s"] - 2)), MIN_S, w)
            lab["force"] = "linear" if pf["exponent"] >= 37 else "softplus"
            lab["dissipation"] = "approach" if pf["s"] < 0 else ("separate" if pf["s"] < 2 else "zero")
            r = float(np.sqrt(pf["vt"] @ pf["vt"])) / vs
            lab["friction"] = "none" if r < NONE else ("stick" if r < STICK else ("slip" if r > SLIP else "mid"))
            if lab["dissipation"] == "zero":
                assert pf["fn"] == 0.0 and not np.any(pf["fB"]), "s >= 2 must give a force that is exactly zero"
        if phi <= kane.threshold + REACH:
            lab.update(n=[float(x) for x in n], Ca=[float(x) for x in Ca], Cb=[float(x) for x in Cb])
        pairs.append(lab)
    return pairs, margins


# The labels every fixture must cover (tools/make_golden.py contact asserts them; tests/test_contact_regions.py states
# them again and compares).  "pairs" below: the sphere-box pairs of the model's box under test.
FACES = ["+x", "-x", "+y", "-y", "+z", "-z"]
EDGES = [a + b for a, b in (("+x", "+y"), ("+x", "-y"), ("-x", "+y"), ("-x", "-y"), ("+x", "+z"), ("+x", "-z"), ("-x", "+z"),
                            ("-x", "-z"), ("+y", "+z"), ("+y", "-z"), ("-y", "+z"), ("-y", "-z"))]
CORNERS = [a + b + c for a in ("+x", "-x") for b in ("+y", "-y") for c in ("+z", "-z")]
INSIDE = ["in+x", "in-x", "in+y", "in-y", "in+z", "in-z"]

