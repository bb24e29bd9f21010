"""Binary32 numpy twin of the temporal history kept across sphere moves, written from the text of include/mirt.h ("keeping the history across sphere
moves": the definition), operation for operation, on top of temporal_twin.py (the camera-only steps, which it imports and does not edit).

Besides temporal_twin's inputs a call takes `ids`, the id map of its camera ((h, w) int32: the BVH-order sphere of every pixel centre, -1 for none),
and `spheres`, the BVH-order table now ((n, 4) float32 rows {pos, radius_sq}).  A history also holds "ids" and "spheres": the id map of the call that
wrote it and the table it was taken under."""
import numpy as np

import denoise_twin as dt
import temporal_twin as tt

f32 = np.float32
DEFAULTS, CLASSES = tt.DEFAULTS, tt.CLASSES
REPROJECTED, NO_HISTORY, OUTSIDE, REJECTED, UNUSABLE = range(5)


def words(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def moved_and_scaled(ids, now, then):
    """Per pixel: the sphere moved (i >= 0 and any of its four words differs between the tables); its radius_sq word differs."""
    i = np.clip(ids, 0, max(len(now) - 1, 0))
    a, b = words(now)[i], words(then)[i]
    scaled = (ids >= 0) & (a[..., 3] != b[..., 3])
    return (ids >= 0) & (a != b).any(axis=-1), scaled


def project(cam, prev, z, px, py, ids, now, then):
    """The map up to (fx, fy, z', behind) for every pixel, whatever its usability.  px, py, z: float32 arrays of one shape; ids: int32 of that shape."""
    now, then = np.asarray(now, dtype=f32).reshape(-1, 4), np.asarray(then, dtype=f32).reshape(-1, 4)
    if len(now) == 0:
        now = then = np.zeros((1, 4), dtype=f32)
    moved, scaled = moved_and_scaled(ids, now, then)
    i = np.clip(ids, 0, len(now) - 1)
    d = tt.camera_ray_dir(cam, px, py)
    P = [cam["pos"][c] + d[c] * z for c in range(3)]
    o = [P[c] - now[i, c] for c in range(3)]
    with np.errstate(all="ignore"):
        s = np.sqrt(then[i, 3] / now[i, 3])
    scale = scaled & (now[i, 3] > f32(0.0))
    o = [np.where(scale, o[c] * s, o[c]) for c in range(3)]
    P = [np.where(moved, then[i, c] + o[c], P[c]) for c in range(3)]
    r = [P[c] - prev["pos"][c] for c in range(3)]
    zr = np.sqrt(tt.dot3(r, r))
    q = tt.rotate([-prev["orient"][0], -prev["orient"][1], -prev["orient"][2]], prev["orient"][3], r)
    behind = (q[2] / prev["z"]) <= f32(0.0)
    t = prev["z"] / q[2]
    fx = (q[0] * t + prev["half_width"]) - f32(0.5)
    fy = (q[1] * t + prev["half_height"]) - f32(0.5)
    if np.array_equal(tt.camera_words(cam), tt.camera_words(prev)):              # the identity exception: not for a sphere that moved
        fx, fy, zr, behind = np.where(moved, fx, px), np.where(moved, fy, py), np.where(moved, zr, z), behind & moved
    return fx.astype(f32), fy.astype(f32), zr.astype(f32), behind


def reproject_blend(st, n_img, cam, hist, dparams, tparams, ids, spheres):
    """Steps 2-3 on a prepared state -> (x (3), v, len, class image): temporal_twin.reproject_blend with the moved map and the id condition on a tap."""
    h, w = st["v"].shape
    x, v, z, N, ok = st["x"], st["v"], st["z"], st["N"], st["usable"]
    cls = np.where(ok, NO_HISTORY, UNUSABLE).astype(np.int32)
    length = np.where(ok, n_img, f32(0.0)).astype(f32)
    if not tt.takes_history(hist, cam, dparams, tparams, (h, w)):
        return [c.copy() for c in x], v.copy(), length, cls
    py, px = np.meshgrid(np.arange(h, dtype=f32), np.arange(w, dtype=f32), indexing="ij")
    with np.errstate(all="ignore"):
        fx, fy, zr, behind = project(cam, hist["cam"], z, px, py, ids, spheres, hist["spheres"])
        applies = ok & ~((N[0] == 0) & (N[1] == 0) & (N[2] == 0))
        ixf, iyf = np.floor(fx), np.floor(fy)
        window = (ixf >= f32(-1.0)) & (ixf <= f32(w - 1)) & (iyf >= f32(-1.0)) & (iyf <= f32(h - 1))
        outside = behind | ~window
        wx, wy = fx - ixf, fy - iyf
        ux, uy = f32(1.0) - wx, f32(1.0) - wy
        ix = np.where(window, ixf, f32(0.0)).astype(np.int64)
        iy = np.where(window, iyf, f32(0.0)).astype(np.int64)
        zero = np.zeros_like(v)
        B, V, L, X = zero.copy(), zero.copy(), zero.copy(), [zero.copy() for _ in range(3)]
        started = np.zeros(v.shape, dtype=bool)
        depth_tol, normal_min = f32(tparams["depth_tol"]), f32(tparams["normal_min"])
        for j in (0, 1):
            for i in (0, 1):
                tx, ty = ix + i, iy + j
                inside = (tx >= 0) & (ty >= 0) & (tx < w) & (ty < h)
                cx, cy = np.clip(tx, 0, w - 1), np.clip(ty, 0, h - 1)
                tz, tn = hist["z"][cy, cx], hist["n"][cy, cx]
                tN = [hist["N"][c][cy, cx] for c in range(3)]
                taken = (inside & hist["usable"][cy, cx] & (tn > f32(0.0)) & (np.abs(tz - zr) <= depth_tol * zr) & (tt.dot3(N, tN) >= normal_min)
                         & (hist["ids"][cy, cx] == ids))
                b = (wx if i else ux) * (wy if j else uy)
                B = dt._add(B, started, taken, b)
                for c in range(3):
                    X[c] = dt._add(X[c], started, taken, b * hist["x"][c][cy, cx])
                V = dt._add(V, started, taken, b * hist["v"][cy, cx])
                L = dt._add(L, started, taken, b * tn)
                started = started | taken
        rejected = ~started | (B == f32(0.0))
        xh = [X[c] / B for c in range(3)]
        vh, nh = V / B, L / B
        cap = f32(tparams["max_ratio"]) * n_img
        nh = np.where(cap < nh, cap, nh)
        a = n_img / (n_img + nh)
        oma = f32(1.0) - a
        bx = [xh[c] + a * (x[c] - xh[c]) for c in range(3)]
        bv = (a * a) * v + (oma * oma) * vh
        blen = n_img + nh
    cls = np.where(applies, np.where(outside, OUTSIDE, np.where(rejected, REJECTED, REPROJECTED)), cls).astype(np.int32)
    re = cls == REPROJECTED
    out_x = [np.where(re, bx[c], x[c]).astype(f32) for c in range(3)]
    return out_x, np.where(re, bv, v).astype(f32), np.where(re, blen, length).astype(f32), cls


def render(acc, aov, counts, exposure, dparams, tparams, width, height, cam, hist, ids, spheres):
    """mirt_render_temporal under mirt_set_sphere_motion(1) -> (frame, len, stats, the history afterwards, the class image)."""
    dp = dict(dt.DEFAULTS)
    dp.update(dparams)
    tp = dict(DEFAULTS)
    tp.update(tparams)
    spheres = np.array(spheres, dtype=f32).reshape(-1, 4)
    st = dt.prepare(acc, aov, counts, exposure, dp, width, height)
    h_img, w_img = st["v"].shape                                                  # mirt_id_map covers width x height; the history's id plane is read over the tiled pixels
    ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32)[:h_img, :w_img])
    n_img = dt.to_image(np.repeat(np.asarray(counts, dtype=np.uint32).reshape(-1, 1), 256, axis=1), width, height).astype(f32)
    st["x"], st["v"], length, cls = reproject_blend(st, n_img, cam, hist, dp, tp, ids, spheres)
    if int(tp["update"]):
        hist = {"x": [c.copy() for c in st["x"]], "v": st["v"].copy(), "N": [c.copy() for c in st["N"]], "z": st["z"].copy(), "usable": st["usable"].copy(),
                "n": length.copy(), "cam": cam, "demodulate": int(dp["demodulate"]), "albedo_floor": f32(dp["albedo_floor"]), "shape": tuple(st["v"].shape),
                "ids": ids.copy(), "spheres": spheres.copy()}
    for i in range(int(dp["iterations"])):
        st["x"], st["v"] = dt.atrous_pass(st, 1 << i, dp)
    return dt.finish(st, width, height), length, tt.stats_of(cls), hist, cls
