"""Binary32 numpy twin of the temporal history of the denoised resolve, written from the text of include/mirt.h ("temporal history for the denoised
resolve", THE DEFINITION, steps 1-5), operation for operation; steps 1 and 5 are denoise_twin.py's.  numpy evaluates every array operation on
float32 arrays with one rounding and never fuses two.

A camera is the eleven words mirt_set_camera takes: {"pos": 3, "orient": 4 (x, y, z, w), "half_width", "half_height", "z", "exposure"}.
A history is what a call with update = 1 leaves: {"x": 3 images, "v", "N": 3 images, "z", "usable", "n" (the length image), "cam", "demodulate",
"albedo_floor", "shape"}."""
import numpy as np

import denoise_twin as dt

f32 = np.float32
DEFAULTS = {"max_ratio": 7.0, "depth_tol": 0.02, "normal_min": 0.9, "update": 1}
CLASSES = ("reprojected", "no_history", "outside", "rejected", "unusable")
REPROJECTED, NO_HISTORY, OUTSIDE, REJECTED, UNUSABLE = range(5)


def camera(pos, orient, half_width, half_height, z, exposure=1.0):
    return {"pos": np.asarray(pos, dtype=f32), "orient": np.asarray(orient, dtype=f32), "half_width": f32(half_width), "half_height": f32(half_height),
            "z": f32(z), "exposure": f32(exposure)}


def camera_words(cam):
    return np.concatenate([cam["pos"], cam["orient"], [cam["half_width"], cam["half_height"], cam["z"], cam["exposure"]]]).astype(f32).view(np.uint32)


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross3(x, y):
    return [x[1] * y[2] - y[1] * x[2], x[2] * y[0] - y[2] * x[0], x[0] * y[1] - y[0] * x[1]]


def rotate(qv, w, v):
    """glm operator*(quat, vec3) as device_math.hpp camera_axis spells it: v + ((uv * w) + uuv) * 2."""
    uv = cross3(qv, v)
    uuv = cross3(qv, uv)
    return [v[c] + ((uv[c] * w) + uuv[c]) * f32(2.0) for c in range(3)]


def camera_ray_dir(cam, px, py):
    """camera_ray_dir(cam, px, py, 0.5f, 0.5f); px, py float32 images of pixel coordinates."""
    v = [(px + f32(0.5)) - cam["half_width"], (py + f32(0.5)) - cam["half_height"], np.full_like(px, cam["z"])]
    r = rotate([cam["orient"][0], cam["orient"][1], cam["orient"][2]], cam["orient"][3], v)
    inv = f32(1.0) / np.sqrt(dot3(r, r))
    return [r[c] * inv for c in range(3)]


def unit_orient(cam):
    o = cam["orient"]
    qn = ((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]) + o[3] * o[3]
    return bool(np.abs(qn - f32(1.0)) < f32(1e-4))


def takes_history(hist, cam, dparams, tparams, shape):
    """Step 2's conditions on the call."""
    return (hist is not None and f32(tparams["max_ratio"]) > 0 and hist["shape"] == tuple(shape) and int(hist["demodulate"]) == int(dparams["demodulate"])
            and f32(hist["albedo_floor"]).view(np.uint32) == f32(dparams["albedo_floor"]).view(np.uint32)
            and f32(hist["cam"]["exposure"]).view(np.uint32) == f32(cam["exposure"]).view(np.uint32) and unit_orient(cam) and unit_orient(hist["cam"]))


def project(cam, prev, z, px, py):
    """Step 2 up to (fx, fy, z', behind) for every pixel, whatever its usability."""
    if np.array_equal(camera_words(cam), camera_words(prev)):
        return px.copy(), py.copy(), z.copy(), np.zeros(z.shape, dtype=bool)
    d = camera_ray_dir(cam, px, py)
    P = [cam["pos"][c] + d[c] * z for c in range(3)]
    r = [P[c] - prev["pos"][c] for c in range(3)]
    zr = np.sqrt(dot3(r, r))
    o = prev["orient"]
    q = rotate([-o[0], -o[1], -o[2]], o[3], r)
    behind = (q[2] / prev["z"]) <= f32(0.0)
    t = prev["z"] / q[2]
    fx = (q[0] * t + prev["half_width"]) - f32(0.5)
    fy = (q[1] * t + prev["half_height"]) - f32(0.5)
    return fx, fy, zr, behind


def reproject_blend(st, n_img, cam, hist, dparams, tparams):
    """Steps 2-3 on a prepared state (denoise_twin.prepare) -> (x (3), v, len, class image).  n_img: the tile count of every pixel, float32."""
    h, w = st["v"].shape
    x, v, z, N, ok = st["x"], st["v"], st["z"], st["N"], st["usable"]
    cls = np.where(ok, NO_HISTORY, UNUSABLE).astype(np.int32)
    length = np.where(ok, n_img, f32(0.0)).astype(f32)
    if not takes_history(hist, cam, dparams, tparams, (h, w)):
        return [c.copy() for c in x], v.copy(), length, cls
    py, px = np.meshgrid(np.arange(h, dtype=f32), np.arange(w, dtype=f32), indexing="ij")
    with np.errstate(all="ignore"):
        fx, fy, zr, behind = project(cam, hist["cam"], z, px, py)
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
                taken = inside & hist["usable"][cy, cx] & (tn > f32(0.0)) & (np.abs(tz - zr) <= depth_tol * zr) & (dot3(N, tN) >= normal_min)
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


def stats_of(cls):
    return {name: int((cls == k).sum()) for k, name in enumerate(CLASSES)}


def render(acc, aov, counts, exposure, dparams, tparams, width, height, cam, hist):
    """mirt_render_temporal -> (frame (height, width, 4), len (16 v_tiles, 16 h_tiles), stats, the history afterwards)."""
    dp = dict(dt.DEFAULTS)
    dp.update(dparams)
    tp = dict(DEFAULTS)
    tp.update(tparams)
    st = dt.prepare(acc, aov, counts, exposure, dp, width, height)
    n_img = dt.to_image(np.repeat(np.asarray(counts, dtype=np.uint32).reshape(-1, 1), 256, axis=1), width, height).astype(f32)
    st["x"], st["v"], length, cls = reproject_blend(st, n_img, cam, hist, dp, tp)
    if int(tp["update"]):
        hist = {"x": [c.copy() for c in st["x"]], "v": st["v"].copy(), "N": [c.copy() for c in st["N"]], "z": st["z"].copy(), "usable": st["usable"].copy(),
                "n": length.copy(), "cam": cam, "demodulate": int(dp["demodulate"]), "albedo_floor": f32(dp["albedo_floor"]), "shape": tuple(st["v"].shape)}
    for i in range(int(dp["iterations"])):
        st["x"], st["v"] = dt.atrous_pass(st, 1 << i, dp)
    return dt.finish(st, width, height), length, stats_of(cls), hist
