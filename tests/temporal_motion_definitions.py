"""Float64 statement of the moved-sphere map of the temporal history (include/mirt.h, "keeping the history across sphere moves"), written from that
text independently of temporal_motion_twin.py, with the rounding bound DESIGN.md section 2 derives for the binary32 chain.

Inputs are the binary32 values the kernel reads, widened; every operation here is float64.  Points are rows: px, py, z of shape (n,), tables (n, 4)
(each point's own sphere now and then)."""
import numpy as np

import temporal_definitions as td

U = td.U


def ray_dirs(cam, px, py):
    """Unit directions through the pixel centres (px, py), (n, 3)."""
    v = np.stack([px + 0.5 - cam["half_width"], py + 0.5 - cam["half_height"], np.full_like(px, cam["z"])], axis=-1)
    r = td.rotate(cam["orient"], v)
    return r / np.linalg.norm(r, axis=-1, keepdims=True)


def moved_map(cam, prev, px, py, z, now, then):
    """A point of a sphere that moved from `then` = (c0, rsq0) to `now` = (c, rsq), seen at depth z through pixel centre (px, py) of `cam`, carried back
    to where it was and projected into `prev`: P = cam.pos + d z;  P' = c0 + (P - c) s,  s = sqrt(rsq0 / rsq) where the two rsq differ and rsq > 0,
    else 1;  r = P' - prev.pos;  z' = |r|;  q = R(prev.orient)^-1 r;  behind: q.z / prev.z <= 0;  f = q.xy (prev.z / q.z) + half - 0.5.
    -> dict with fx, fy, zr, behind and the bounds delta_f (of fx and fy) and delta_z (of z')."""
    cam, prev = td.cam64(cam), td.cam64(prev)
    px, py, z = (np.asarray(a, dtype=np.float64) for a in (px, py, z))
    now, then = np.asarray(now, dtype=np.float64), np.asarray(then, dtype=np.float64)
    d = ray_dirs(cam, px, py)
    P = cam["pos"] + d * z[:, None]
    o = P - now[:, :3]
    with np.errstate(all="ignore"):
        s = np.where((now[:, 3] != then[:, 3]) & (now[:, 3] > 0), np.sqrt(then[:, 3] / now[:, 3]), 1.0)
    Pp = then[:, :3] + o * s[:, None]
    r = Pp - prev["pos"]
    zr = np.linalg.norm(r, axis=-1)
    q = td.rotate(td.conj(prev["orient"]), r)
    with np.errstate(all="ignore"):
        behind = q[:, 2] / prev["z"] <= 0
        t = prev["z"] / q[:, 2]
        fx, fy = q[:, 0] * t + prev["half_width"] - 0.5, q[:, 1] * t + prev["half_height"] - 0.5
    # DESIGN.md section 2, "the moved-sphere map": the error of P is the camera-only chain's, 45 u z + u |P|.  o = P - c adds u |o|; s carries 1.5 u
    # relative (a division, then a square root that halves what it is handed and adds its own rounding); o s adds one more rounding: the scaled offset
    # is off by s dP + 3.5 u s |o|.  P' = c0 + o s adds u |P'|, r = P' - prev.pos adds u z', the inverse rotation 40 u z'.
    norm = lambda a: np.linalg.norm(a, axis=-1)
    E = 41.0 * zr + s * (45.0 * z + norm(P)) + 3.5 * s * norm(o) + norm(Pp)
    R2 = (fx + 0.5 - prev["half_width"]) ** 2 + (fy + 0.5 - prev["half_height"]) ** 2
    with np.errstate(all="ignore"):
        delta_f = U * (np.sqrt(2.0) * (R2 + prev["z"] ** 2) / (zr * abs(prev["z"])) * E + 3.0 * np.sqrt(R2) + 2.0 * np.maximum(np.abs(fx), np.abs(fy)) + 2.0 * max(abs(prev["half_width"]), abs(prev["half_height"])))
    # z' = sqrt(dot(r, r)): the error of r (E without the rotation's 40 z'), and 3 u z' for the dot product's three roundings and the root's own
    delta_z = U * ((E - 40.0 * zr) + 3.0 * zr)
    return {"fx": fx, "fy": fy, "zr": zr, "behind": behind, "delta_f": delta_f, "delta_z": delta_z, "P": P, "Pp": Pp, "s": s, "R": np.sqrt(R2)}
