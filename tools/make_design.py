#!/usr/bin/env python3
"""Assembles DESIGN.md (the current-state document) from tools/design/DESIGN.in.md, carrying over verbatim the sections of
HISTORY.md that describe stable parts of the design (the path and its boundary, the floating-point specification, the
multi-GPU exchange, the oracle's status): those are not round narrative, and a second hand-maintained copy would drift.
Run after editing a part:  python tools/make_design.py"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = open(os.path.join(ROOT, "HISTORY.md")).read()


def section(start, end):
    a = H.index(start)
    return H[a:H.index(end, a)].rstrip() + "\n"


CARRIED = {
    "@@SECTION_1@@": ("## 1. The path and its boundary (SURVEY.md §8 a, b)", "## 2. Data layout in HBM"),
    "@@SECTION_2@@": ("## 2. Data layout in HBM", "## 3. Kernel 1"),
    "@@SECTION_3_2@@": ("### 3.2 Floating-point specification", "### 3.3 Resources and bound"),
    "@@SECTION_7@@": ("## 7. Multi-GPU (SURVEY.md §8 e)", "## 8. Oracle and parity status"),
    "@@SECTION_8@@": ("## 8. Oracle and parity status (SURVEY.md §8 c)", "## 9. Out of scope"),
}
text = open(os.path.join(ROOT, "tools", "design", "DESIGN.in.md")).read()
for k, (a, b) in CARRIED.items():
    # cross references of a carried section to sub-sections that now live in HISTORY.md only
    body = re.sub(r"§(3\.3|3\.4|4\.3|4\.4|5\.[0-9]+|6\.[0-9]|13\.1|13\.2|14\.1)\b", lambda m: "HISTORY §" + m.group(1), section(a, b))
    text = text.replace(k, body)
# statements of the carried sections that later rounds overtook (the history keeps them as they were written)
for old, new in [
    ("ONE banded solve of the KKT system with blocks of nq + nu (`csrc/kkt.h`, HISTORY §13.1; blocks ≤ 24); the reference's route over S = J H⁻¹ Jᵀ (`csrc/constraints.h`, `dense_ldl.h`) for allegro and behind the stepwise API",
     "ONE banded solve of the KKT system with blocks of nq + nu (`csrc/kkt.h`, §5.5, HISTORY §13.1; blocks ≤ 30: every example, allegro's 23 + 6 included); the reference's route over S = J H⁻¹ Jᵀ (`csrc/constraints.h`, `dense_ldl.h`) behind the stepwise API and for a singular S"),
    ("solve with H run on the device.  Without convergence checks and with the non-adaptive scalings\n  — all five example configurations — the whole trust-region loop incl. the multipliers of enforced\n  equality constraints runs on the device and the host waits once per `Solve` (§13); with\n  convergence checks, the adaptive scalings or `IDTO_OPT_HOST_LOOP=1` the O(num_vars) bookkeeping",
     "solve with H run on the device.  The whole trust-region loop - the multipliers of enforced equality\n  constraints, the convergence criteria and (with diagonal cost weights) the adaptive scalings included - runs on the\n  device and the host waits once per `Solve` (§13: all five example configurations).  Dense cost weights without\n  constraints and with a non-adaptive scaling run the same device loop without its two-set evaluation (`idto_hip_gn_step`\n  again at the iterate every iteration; `tests/test_gpu_dense_weights.py` holds it to the stepwise loop bit for bit, a run\n  with rejected steps included, and to the oracle's iterates); with dense cost weights under\n  an adaptive scaling or with enforced constraints (`idto_hip_tr_solve` declines both, and `DeviceLoopEligible` asks\n  `weights_diagonal` before it chooses), `linear_solver = kDenseLdlt`, the debug switches or `IDTO_OPT_HOST_LOOP=1` the O(num_vars) bookkeeping"),
    ("`tr_iter_kernel`, `tr_decide` in `cost_kernel` (`csrc/trust_region.h`, §13)",
     "`tr_iter_kernel`, `tr_decide` in `cost_kernel` (`csrc/trust_region.h`, §13); acrobot and the spinner: the whole iteration in `gn_small_kernel` (§5.4)"),
]:
    if old in text:
        text = text.replace(old, new)
# rows of §8's convention table that came after the carried text
WELDED_ROW = "| welded links (cheetah feet, allegro `hand_root`)"
CAPSULE_ROWS = (
    "| capsule-box: the sphere at the capsule's segment end with the lower world z, the `-h` end on a tie (a capsule lying flat touches the ground along its length; Drake/FCL's witness point there is not pinned here) | `csrc/id_eval.h capsule_single`, `include/idto_model.h` | none in-tree | `QueryObject::ComputeSignedDistancePairwiseClosestPoints` for a tilted and a flat `Capsule` above the ground `Box`, compare the witness point on the capsule |\n"
    "| (near-)parallel capsule-capsule: `1 - (u1·u2)^2 <= 1e-10` ⇒ the middle of the overlap of the two segments | `csrc/id_eval.h capsule_centres`, `tests/capsule_ref.py` | none in-tree | the same query on two parallel overlapping capsules |\n")
# (punyo: what could not be pinned against Drake - the tree holds no number that depends on them)
PUNYO_ROWS = (
    "| an SDF `<inertial>` without `<inertia>` (every link of `models/punyoid.sdf`): libsdformat's default, ixx = iyy = izz = 1 with zero products - the glue links of 0.1 kg included | `tools/convert_models.py parse_sdf`; independently `tools/make_model_fixture.py` (`tests/golden/examples/world_punyo.json`) | none in-tree (the file gives masses only) | `plant.GetBodyByName(\"waist\").default_rotational_inertia()` after `Parser.AddModels` |\n"
    "| an SDF joint `<pose>` is in the child link's frame, the axis in that joint frame; the body frame here is the joint frame, the link hangs in it at the inverse pose (punyo's shoulder, elbow and wrist joints: 0.05 - 0.16 m off the link origin, two turned by pi, so that `shoulderR_joint2` and `elbowR_joint2` turn about -y of the model) | `tools/convert_models.py parse_sdf` (`X_JC`), `build_model`; independently `tools/make_model_fixture.py read_sdf` | SDFormat 1.7 semantics; `models/punyoid.sdf:575-583, 660-668, 695-703` | FK of `hand_R` at q with `shoulderR_joint2` = 0.5 against the model's `X_PF` chain; the sign of the DoF |\n"
    "| punyo's q: height, three torso joints, the arm of `shoulderL_joint1` (declared first), the arm of `shoulderR_joint1`, the ball - depth-first in joint declaration order; `punyo.yaml` comments the first arm as \"right\" | `tools/convert_models.py build_model` (visiting order), `tests/golden/examples/punyo.model` | every vector of `examples/punyo/punyo.yaml` is the same for both arms, so no number of the fixture depends on it | `plant.GetJointByName(\"shoulderL_joint1\").position_start()` against `shoulderR_joint1`'s |\n")
# (cylinders: Drake is not part of this build; the second row's choices are taken from memory of its source)
CYLINDER_ROWS = (
    "| box-cylinder: the cheetah's torso `Box` against a hill `Cylinder` is a candidate pair in Drake (FCL); this project refuses a cylinder against anything but a sphere, and the converter drops the pair and prints that it did | `tools/convert_models.py build_model`, `host/model_tables.cc CheckGeometry` | none in-tree | `QueryObject::ComputeSignedDistancePairwiseClosestPoints` on `mini_cheetah.cc --hills=2` with the torso lowered onto a hill: whether the pair is reported and from which distance its force matters |\n"
    "| sphere-cylinder: at `r == 0` the radial direction is `(1, 0, 0)` of the cylinder's frame, and inside at `R - r == H - abs(c.z)` the side wins over the cap (`dr <= dz`, the box branch's tie rule) - both from memory of Drake's `DistanceToPoint` for a cylinder, not checked against it | `csrc/id_eval.h cylinder_reduce`, `include/idto_model.h`, `tests/cylinder_ref.py` | none in-tree | `QueryObject::ComputeSignedDistanceToPoint` for points on the axis of a `Cylinder` (above a cap and inside) and at an interior point with equal distance to the side and a cap: compare `grad_W` |\n")
if WELDED_ROW in text:
    i = text.index(WELDED_ROW)
    j = text.index("\n", i) + 1
    text = text[:j] + CAPSULE_ROWS + CYLINDER_ROWS + PUNYO_ROWS + text[j:]
open(os.path.join(ROOT, "DESIGN.md"), "w").write(text)
print("DESIGN.md:", len(text.splitlines()), "lines")
