"""Float64 definition of steps 2-3 of the temporal history (include/mirt.h, "temporal history for the denoised resolve"), written from that text
independently of temporal_twin.py, with the rounding bounds DESIGN.md section 2 derives for the binary32 chain, and the analytic scene the CPU
tests use: a sphere over a ground plane seen through the pinhole camera of Camera.hpp:80-88.

Inputs are the binary32 values the kernel reads, widened; every operation here is float64."""
import numpy as np

U = 2.0 ** -24            # unit roundoff of binary32


def rotate(q, v):
    """glm operator*(quat, vec3): v + 2 (w (qv x v) + qv x (qv x v)); q = (x, y, z, w), v = (..., 3)."""
    qv = np.asarray(q[:3], dtype=np.float64)
    uv = np.cross(qv, v)
    return v + 2.0 * (q[3] * uv + np.cross(qv, uv))


def conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]], dtype=np.float64)


def ray_dirs(cam, w, h):
    """Unit directions of the pixel centres, (h, w, 3)."""
    py, px = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    v = np.stack([px + 0.5 - cam["half_width"], py + 0.5 - cam["half_height"], np.full_like(px, cam["z"])], axis=-1)
    r = rotate(cam["orient"], v)
    return r / np.linalg.norm(r, axis=-1, keepdims=True)


def cam64(cam):
    return {k: np.asarray(v, dtype=np.float64) for k, v in cam.items()}


# ---- the analytic scene -------------------------------------------------------------------------------------------------------------------------
SPHERE_C, SPHERE_R, GROUND_Y = np.array([0.0, 0.5, 0.0]), 0.5, 0.0


def first_hit(cam, w, h):
    """-> (depth (h, w), normal (h, w, 3), on_sphere (h, w), hit (h, w)): the sphere, else the ground plane y = 0, else a miss (depth 1e4, normal 0)."""
    o, d = cam["pos"], ray_dirs(cam, w, h)
    oc = o - SPHERE_C
    bq = d @ oc
    disc = bq * bq - (oc @ oc - SPHERE_R ** 2)
    ts = np.where(disc > 0, -bq - np.sqrt(np.maximum(disc, 0)), np.inf)
    ts = np.where(ts > 0, ts, np.inf)
    with np.errstate(divide="ignore"):
        tg = np.where(d[..., 1] < 0, (GROUND_Y - o[1]) / d[..., 1], np.inf)
    on_sphere = ts < tg
    t = np.minimum(ts, tg)
    hit = np.isfinite(t)
    P = o + d * np.where(hit, t, 0.0)[..., None]
    n = np.where(on_sphere[..., None], (P - SPHERE_C) / SPHERE_R, np.array([0.0, 1.0, 0.0]))
    return np.where(hit, t, 1e4), np.where(hit[..., None], n, 0.0), on_sphere, hit


# ---- steps 2-3 ------------------------------------------------------------------------------------------------------------------------------------
def reproject_blend(cur, n, cam, hist, tp):
    """cur: {"x": (h, w, 3), "v", "z", "N": (h, w, 3), "usable"}; hist likewise plus "n" and "cam"; n = the tile count (a scalar here).
    -> dict of per-pixel results and of the quantities the bounds are made of."""
    cam, prev = cam64(cam), cam64(hist["cam"])
    h, w = cur["z"].shape
    z, N = cur["z"].astype(np.float64), cur["N"].astype(np.float64)
    py, px = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    d = ray_dirs(cam, w, h)
    P = cam["pos"] + d * z[..., None]
    r = P - prev["pos"]
    zr = np.linalg.norm(r, axis=-1)
    q = rotate(conj(prev["orient"]), r)
    with np.errstate(all="ignore"):
        behind = q[..., 2] / prev["z"] <= 0
        t = prev["z"] / q[..., 2]
        fx, fy = q[..., 0] * t + prev["half_width"] - 0.5, q[..., 1] * t + prev["half_height"] - 0.5
    ix, iy = np.floor(fx), np.floor(fy)
    wx, wy = fx - ix, fy - iy
    applies = cur["usable"] & (np.abs(N).sum(axis=-1) != 0)
    # the scale of the rounding error of fx, fy: delta_f = U (sqrt 2 (R^2 + hz^2) / (z' |hz|) E + 3 R + 2 max(w, h)),  E = 41 z' + 45 z + |P|
    R2 = (fx + 0.5 - prev["half_width"]) ** 2 + (fy + 0.5 - prev["half_height"]) ** 2
    E = 41.0 * zr + 45.0 * z + np.linalg.norm(P, axis=-1)
    delta_f = U * (np.sqrt(2.0) * (R2 + prev["z"] ** 2) / (zr * abs(prev["z"])) * E + 3.0 * np.sqrt(R2) + 2.0 * max(w, h))
    eps_z = 2.0 * U * (45.0 * z + np.linalg.norm(P, axis=-1) + 4.0 * zr)            # of |z_tap - z'| - depth_tol z'
    eps_n = 4.0 * U                                                                     # of dot(N_p, N_tap)
    near = (np.minimum(wx, 1.0 - wx) <= delta_f) | (np.minimum(wy, 1.0 - wy) <= delta_f)      # floor may come out the other way in binary32
    B = np.zeros((h, w)); X = np.zeros((h, w, 3)); V = np.zeros((h, w)); L = np.zeros((h, w))
    any_in = np.zeros((h, w), dtype=bool); any_taken = np.zeros((h, w), dtype=bool)
    lo, hi = np.full((h, w, 3), np.inf), np.full((h, w, 3), -np.inf)
    taps = []
    for j in (0, 1):
        for i in (0, 1):
            tx, ty = ix + i, iy + j
            inside = (tx >= 0) & (ty >= 0) & (tx < w) & (ty < h) & ~behind
            cx, cy = np.clip(np.nan_to_num(tx), 0, w - 1).astype(int), np.clip(np.nan_to_num(ty), 0, h - 1).astype(int)
            tz, tn, tN = hist["z"][cy, cx].astype(np.float64), hist["n"][cy, cx].astype(np.float64), hist["N"][cy, cx].astype(np.float64)
            mz = np.abs(tz - zr) - tp["depth_tol"] * zr
            mn = (N * tN).sum(axis=-1) - tp["normal_min"]
            live = inside & hist["usable"][cy, cx] & (tn > 0)
            taken = live & (mz <= 0) & (mn >= 0)
            near |= live & ((np.abs(mz) <= eps_z) | (np.abs(mn) <= eps_n))
            b = (wx if i else 1.0 - wx) * (wy if j else 1.0 - wy)
            tx_ = hist["x"][cy, cx].astype(np.float64)
            B += np.where(taken, b, 0.0); V += np.where(taken, b * hist["v"][cy, cx], 0.0); L += np.where(taken, b * tn, 0.0)
            X += np.where(taken[..., None], b[..., None] * tx_, 0.0)
            lo = np.where(taken[..., None], np.minimum(lo, tx_), lo); hi = np.where(taken[..., None], np.maximum(hi, tx_), hi)
            any_in |= inside; any_taken |= taken
            taps.append({"taken": taken, "b": b, "cx": cx, "cy": cy})
    with np.errstate(all="ignore"):
        xh, vh, nh = X / B[..., None], V / B, L / B
        nh = np.minimum(nh, tp["max_ratio"] * n)
        a = n / (n + nh)
        bx = xh + a[..., None] * (cur["x"] - xh)
        bv = a * a * cur["v"] + (1 - a) ** 2 * vh
    cls = np.where(~cur["usable"], 4, np.where(~applies, 1, np.where(~any_in, 2, np.where(~any_taken | (B == 0), 3, 0))))
    re = cls == 0
    # |x32 - x64| for a reprojected pixel away from every threshold
    with np.errstate(all="ignore"):
        spread = np.where(re[..., None], hi - lo, 0.0)
        d_xh = spread * ((4.0 * delta_f + 12.0 * U) / B)[..., None] + 8.0 * U * np.maximum(np.abs(hi), np.abs(lo))
        d_a = a * 12.0 * U                                                            # hn constant over the taps taken: nh carries rounding only
        bound = (1 - a)[..., None] * d_xh + np.abs(cur["x"] - xh) * d_a[..., None] + 4.0 * U * (np.abs(cur["x"]) + np.abs(xh))
    return {"fx": fx, "fy": fy, "P": P, "cls": cls, "near": near & applies, "xh": xh, "x": np.where(re[..., None], bx, cur["x"]), "v": np.where(re, bv, cur["v"]),
            "len": np.where(re, n + nh, np.where(cur["usable"], n, 0.0)), "bound": bound, "a": a, "B": B, "taps": taps, "delta_f": delta_f}
