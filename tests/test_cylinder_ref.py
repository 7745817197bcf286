"""The sphere-cylinder closed form of include/idto_model.h, as tests/cylinder_ref.py restates it, is a distance: against
the minimum over a dense sampling of the cylinder's surface, and at directed states of every region."""
import numpy as np
import pytest

import cylinder_cases as cc
import cylinder_ref as cyl

R, H = 0.3, 0.45
NTH, NZ, NR = 720, 241, 121


def surface():
    """points of the cylinder's surface in its own frame, and the farthest any surface point is from its nearest sample:
    half the diagonal of the largest cell (side: R dtheta by dz; caps: dr by at most R dtheta)"""
    th = np.linspace(0.0, 2 * np.pi, NTH, endpoint=False)
    z = np.linspace(-H, H, NZ)
    r = np.linspace(0.0, R, NR)
    T, Z = np.meshgrid(th, z, indexing="ij")
    side = np.stack([R * np.cos(T), R * np.sin(T), Z], axis=-1).reshape(-1, 3)
    T, Rr = np.meshgrid(th, r, indexing="ij")
    caps = [np.stack([Rr * np.cos(T), Rr * np.sin(T), np.full_like(T, s * H)], axis=-1).reshape(-1, 3) for s in (1, -1)]
    arc, dz, dr = R * 2 * np.pi / NTH, 2 * H / (NZ - 1), R / (NR - 1)
    return np.concatenate([side] + caps), 0.5 * np.hypot(arc, max(dz, dr))


SURFACE, RESOLUTION = surface()


def random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def poses(n, inside, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        c = rng.uniform(-1, 1, 3) * ([R, R, H] if inside else [2.5 * R, 2.5 * R, 2.0 * H])
        is_in = np.hypot(c[0], c[1]) <= R and abs(c[2]) <= H
        if is_in != inside:
            continue
        RX, p = random_rotation(rng), rng.uniform(-1, 1, 3)
        out.append((c, p + RX @ c, float(rng.uniform(0.0, 0.1)), p, RX, bool(rng.integers(2))))
    return out


def brute_force(c):
    return float(np.sqrt(((SURFACE - c) ** 2).sum(axis=1).min()))


def check_witnesses(res, x, rho, p, RX):
    """n is the unit vector from Ca to Cb (by phi's sign), |Ca - Cb| = |phi|, the witness points lie on the two surfaces"""
    n, Ca, Cb, phi = res["n"], res["Ca"], res["Cb"], res["phi"]
    assert abs(np.linalg.norm(n) - 1.0) <= 1e-14
    assert abs(np.linalg.norm(Ca - Cb) - abs(phi)) <= 1e-14
    if abs(phi) > 1e-6:
        assert np.abs((Cb - Ca) / phi - n).max() <= 1e-9


def test_outside_phi_is_the_distance_to_the_surface():
    assert RESOLUTION < 2.5e-3
    seen = set()
    for c, x, rho, p, RX, sphere_is_A in poses(200, False, 11):
        res = cyl.sphere_cylinder(x, rho, p, RX, R, H, sphere_is_A)
        seen.add(res["region"])
        d = brute_force(c)   # (>= the true distance; a sample lies within RESOLUTION of the nearest surface point)
        assert -1e-12 <= d - (res["phi"] + rho) <= RESOLUTION, (c, d, res["phi"] + rho)
        check_witnesses(res, x, rho, p, RX)
        on_cyl, on_sph = (res["Cb"], res["Ca"]) if sphere_is_A else (res["Ca"], res["Cb"])
        cw = RX.T @ (on_cyl - p)   # the cylinder's witness point is on its surface, the sphere's on the sphere
        assert min(abs(np.hypot(cw[0], cw[1]) - R), abs(abs(cw[2]) - H)) <= 1e-14
        assert np.hypot(cw[0], cw[1]) <= R + 1e-14 and abs(cw[2]) <= H + 1e-14
        assert abs(np.linalg.norm(on_sph - x) - rho) <= 1e-14
        assert np.abs(res["n"] * (1 if sphere_is_A else -1) - (on_cyl - x) / np.linalg.norm(on_cyl - x)).max() <= 1e-9
    assert seen == {"side", "cap", "rim"}


def test_inside_minus_phi_minus_rho_is_the_distance_to_the_surface():
    seen = set()
    for c, x, rho, p, RX, sphere_is_A in poses(200, True, 12):
        res = cyl.sphere_cylinder(x, rho, p, RX, R, H, sphere_is_A)
        seen.add(res["region"])
        d = brute_force(c)
        assert -1e-12 <= d - (-res["phi"] - rho) <= RESOLUTION, (c, d, res["phi"])
        check_witnesses(res, x, rho, p, RX)
    assert seen == {"inside-side", "inside-cap"}


@pytest.mark.parametrize("sphere_is_A", [True, False])
@pytest.mark.parametrize("frame", ["own", "rotated"])
@pytest.mark.parametrize("state", sorted(cc.STATES))
def test_directed_states(state, frame, sphere_is_A):
    c, exact = cc.STATES[state]
    c = np.array(c)
    Rd, Hd, rho = cc.R_DIRECTED, cc.H_DIRECTED, 0.03
    RX = np.eye(3) if frame == "own" else (cc.R_EXACT if exact else cc.R_GENERAL)
    p = np.array([0.5, -0.25, 1.0])
    x = p + RX @ c
    res = cyl.sphere_cylinder(x, rho, p, RX, Rd, Hd, sphere_is_A)
    assert res["region"] == cc.REGION[state]
    r, az = np.hypot(c[0], c[1]), abs(c[2])
    e = np.array([c[0], c[1], 0.0]) / r if r else np.array([1.0, 0.0, 0.0])
    sz = np.array([0.0, 0.0, 1.0 if c[2] >= 0 else -1.0])
    want = {   # region: (phi + rho, g in the cylinder's frame, the cylinder's witness point in its frame)
        "side": (r - Rd, e, e * Rd + [0, 0, c[2]]),
        "inside-side": (r - Rd, e, e * Rd + [0, 0, c[2]]),
        "cap": (az - Hd, sz, e * r + sz * Hd),
        "inside-cap": (az - Hd, sz, e * r + sz * Hd),
        "rim": (np.hypot(r - Rd, az - Hd), (e * (r - Rd) + sz * (az - Hd)) / np.hypot(r - Rd, az - Hd), e * Rd + sz * Hd),
    }[res["region"]]
    # a general state's c is rebuilt from x = p + RX c: a few ulp of coordinates of size 1 off, ~1e-15; a direction divides
    # that by the distance it is formed from, at least 0.02 m here
    tol = 1e-16 if exact else 1e-14
    assert abs(res["phi"] + rho - want[0]) <= tol
    gW, on_cyl = RX @ want[1], p + RX @ np.asarray(want[2], float)
    n, Ca, Cb = res["n"], res["Ca"], res["Cb"]
    assert np.abs(n - (-gW if sphere_is_A else gW)).max() <= (1e-15 if exact else 1e-14 / 0.02)
    assert np.abs((Cb if sphere_is_A else Ca) - on_cyl).max() <= 1e-14
    assert np.abs((Ca if sphere_is_A else Cb) - (x - gW * rho)).max() <= 1e-14
    if state.startswith("r0"):   # r == 0: the direction is the cylinder's own x where the side is chosen
        assert r == 0
        if res["region"] == "inside-side":
            assert np.array_equal(gW, RX[:, 0])
    if state.startswith("tie"):
        assert Rd - r == Hd - az and res["region"] == "inside-side"   # (the lower axis wins: the side)
    if state.startswith("z0"):
        assert c[2] == 0 and (RX.T @ (on_cyl - p))[2] == 0
