"""Which branch of the contact code a pair lands in, read off the CPU oracle's OUTPUTS: signed_distances (phi, n, Ca, Cb),
body_poses and the model's geometry tables.  A plain module: tests/test_contact_regions.py holds it to the labels that the
independent generator (tools/golden_examples.py contact_labels) stored in tests/golden/contact/regions_*.json, and runs it
over the trajectories of tests/test_gpu_parity.py for the table of DESIGN.md §8.1.

A sphere-box pair's region is taken from what the oracle returned, not from a second clamp of the sphere's centre: the
normal in the box frame has one non-zero component on a face, two on an edge, three on a corner, and their signs name the
region ("+x", "+x-z", "-x+y+z"); the centre is inside the box exactly when phi + radius < 0, and then the single component
names the face it leaves through ("in+x").  The fixtures keep every state 1e-6 m clear of the clamp planes, which keeps a
clamped component of the unit normal above 1e-6 / (distance of the centres) - five orders above TINY."""
import numpy as np

SPHERE, BOX = 0, 1
TINY = 1e-11   # a component of the unit normal in the box frame below this is a rounded zero (rotating back: ~1e-16)
KINDS = {(SPHERE, SPHERE): "sphere-sphere", (SPHERE, BOX): "sphere-box", (BOX, BOX): "box-box"}


def world_rotation(model, poses, g):
    b = int(model.geom_body[g])
    R = np.asarray(model.geom_X[g], float)[:9].reshape(3, 3)
    return R if b < 0 else poses[b][:9].reshape(3, 3) @ R


def classify(model, orc, q):
    """per pair: dict(kind, region, active, force, phi) at the configuration q"""
    phi, n, _, _ = orc.signed_distances(q)
    poses = orc.body_poses(q)
    sigma = orc.params.smoothing_factor
    out = []
    for k in range(model.npairs):
        ga, gb = int(model.pair_a[k]), int(model.pair_b[k])
        ta, tb = int(model.geom_type[ga]), int(model.geom_type[gb])
        kind = KINDS[tuple(sorted((ta, tb)))]
        region = "-"
        if kind == "sphere-box":
            box, sphere = (ga, gb) if ta == BOX else (gb, ga)
            # n points from A to B; g from the box towards the sphere
            g = world_rotation(model, poses, box).T @ (n[k] if ta == BOX else -n[k])
            region = "".join(("+" if g[i] > 0 else "-") + "xyz"[i] for i in range(3) if abs(g[i]) > TINY)
            if phi[k] + float(model.geom_size[sphere][0]) < 0:
                assert len(region) == 2, "an inside centre leaves through one face"
                region = "in" + region
        active = bool(phi[k] <= orc.contact_threshold)
        force = "-" if not active else ("linear" if -phi[k] / sigma >= 37 else "softplus")
        out.append(dict(kind=kind, region=region, active=active, force=force, phi=float(phi[k])))
    return out


def census(model, orc, qs, table=None):
    """counts of (kind, face | edge | corner | inside-<axis> | -, region, active, force) over the configurations qs"""
    table = {} if table is None else table
    for q in qs:
        for k, lab in enumerate(classify(model, orc, q)):
            r = lab["region"]
            cls = "-" if r == "-" else "inside" if r.startswith("in") else {2: "face", 4: "edge", 6: "corner"}[len(r)]
            moving_box = lab["kind"] == "sphere-box" and any(
                int(model.geom_type[g]) == BOX and int(model.geom_body[g]) >= 0 for g in (model.pair_a[k], model.pair_b[k]))
            key = (lab["kind"] + (" (box on a moving body)" if moving_box else ""), cls, r, lab["active"], lab["force"])
            table[key] = table.get(key, 0) + 1
    return table
