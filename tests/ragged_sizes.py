"""Shared pieces of the ragged-size tests (test_ragged_sizes_cpu.py, test_ragged_sizes_gpu.py): image sizes that are no whole number of 16 x 16
tiles, where three quantities that are otherwise equal come apart — width x height (the row pitch of every full-image plane, and what the camera is
built from), w_img x h_img = 16 (width // 16) x 16 (height // 16) (the area the stencils and the reprojection may read) and 256 x tiles against
width x height.

The twins of denoise_twin.py / temporal_twin.py work on the w_img x h_img image, which is what include/mirt.h defines.  The `wide_*` functions here
run the same twins AS IF w_img = width: the prepared planes are padded to width x height with finite, usable values, the twin's own passes run on the
padded planes, and the result is cropped.  They exist only to show that the inputs tell the two readings apart."""
import numpy as np

import denoise_twin as dt
import temporal_twin as tt

f32 = np.float32
#        size      tiles   what it isolates
SIZES = [(70, 40),  # 4 x 2   both remainders, width no multiple of 4 pixels
         (40, 70),  # 2 x 4   the transpose
         (17, 16),  # 1 x 1   a one-column remainder only
         (16, 31),  # 1 x 1   a row remainder only, the largest (15)
         (79, 33)]  # 4 x 2   the largest column remainder, a one-row remainder
COLUMN_REMAINDER = [s for s in SIZES if s[0] % 16]
TEMPORAL_SIZES = SIZES[:2]


def img(w, h):
    """(w_img, h_img): the pixels the tiles cover."""
    return 16 * (w // 16), 16 * (h // 16)


def tiles(w, h):
    return (w // 16) * (h // 16)


# ---- synthetic slabs (the recipe of test_denoise_gpu.synthetic, for any tile count; NaN words in the last owned column and row) ---------------------
def synthetic(w, h, k, seed):
    """-> (accumulator slab, AOV slab, accumulations).  Positive radiance over smooth guides — every pixel a hit, normals within a few degrees of +z,
    depths 4 .. 5 — so that a tap's weight is far from 0 and whether it is taken shows in the words.  One NaN bucket word sits in the last owned
    column (x = w_img - 1) and one in the last owned row (y = h_img - 1): their pixels are unusable and pass through."""
    rng = np.random.default_rng(seed)
    n, acc_n = tiles(w, h), 3 * k
    slab = (10.0 ** rng.uniform(-1, 0.5, (n, 1, 3, 256)) * rng.uniform(0.5, 1.5, (n, k, 3, 256))).astype(f32)
    h_tiles = w // 16
    slab[h_tiles - 1, 0, 1, 5 * 16 + 15] = np.nan                                  # tile row 0, last tile column: pixel (w_img - 1, 5)
    slab[n - h_tiles, 0, 1, 15 * 16 + 3] = np.nan                                  # last tile row, first tile column: pixel (3, h_img - 1)
    # (both in bucket 0, as test_denoise_gpu.synthetic plants its own: with the NaN in the last bucket the noise map's NaN word for that pixel differs
    # between the device and numpy — IEEE 754 leaves the sign of a NaN result open — so that word is not pinned)
    aov = np.zeros((n, 7, 256), dtype=f32)
    nrm = np.array([0.0, 0.0, 1.0]) + rng.normal(scale=0.03, size=(n, 256, 3))
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    aov[:, 0] = rng.uniform(4.0, 5.0, (n, 256)) * acc_n
    aov[:, 1:4] = np.moveaxis(nrm, 2, 1) * acc_n
    aov[:, 4:7] = rng.uniform(0.3, 0.9, (n, 3, 256)) * acc_n
    return slab, aov.astype(f32), acc_n


# ---- "as if w_img = width" ----------------------------------------------------------------------------------------------------------------------------
def _pad(a, w, h):
    """(h_img, w_img) -> (h, w): the remainder mirrors the owned pixels next to it, made finite."""
    hi, wi = a.shape
    out = np.pad(a, ((0, h - hi), (0, w - wi)), mode="symmetric")
    if out.dtype == bool:
        out[hi:, :] = True
        out[:, wi:] = True
    else:
        rest = np.ones(out.shape, dtype=bool)
        rest[:hi, :wi] = False
        out = np.where(rest & ~np.isfinite(out), out.dtype.type(1.0), out)
    return out


def pad_state(st, w, h):
    """A prepared state (denoise_twin.prepare) with every plane padded to (h, w); the remainder is usable."""
    return {key: [_pad(c, w, h) for c in v] if isinstance(v, list) else _pad(v, w, h) for key, v in st.items()}


def crop_state(st, w, h):
    wi, hi = img(w, h)
    return {key: [c[:hi, :wi] for c in v] if isinstance(v, list) else v[:hi, :wi] for key, v in st.items()}


def wide_denoise(acc, aov, counts, exposure, params, w, h):
    """denoise_twin.denoise with the stencil reading the planes' remainder: what a k_atrous bounded by width x height would give."""
    p = dict(dt.DEFAULTS)
    p.update(params)
    st = pad_state(dt.prepare(acc, aov, counts, exposure, p, w, h), w, h)
    for i in range(int(p["iterations"])):
        st["x"], st["v"] = dt.atrous_pass(st, 1 << i, p)
    return dt.finish(crop_state(st, w, h), w, h)


def landers(st, cam, prev, w, h):
    """Pixels of a prepared state to which step 2 applies, whose point projects (temporal_twin.project) outside the w_img x h_img window of the
    history but inside the width x height one: the twin classes them `outside`; a k_reproject bounded by width x height would read the planes'
    remainder for them."""
    wi, hi = img(w, h)
    py, px = np.meshgrid(np.arange(hi, dtype=f32), np.arange(wi, dtype=f32), indexing="ij")
    with np.errstate(all="ignore"):
        fx, fy, _, behind = tt.project(cam, prev, st["z"], px, py)
        ixf, iyf = np.floor(fx), np.floor(fy)
    N = st["N"]
    applies = st["usable"] & ~((N[0] == 0) & (N[1] == 0) & (N[2] == 0))
    window = lambda ww, hh: (ixf >= -1) & (ixf <= ww - 1) & (iyf >= -1) & (iyf <= hh - 1)
    return applies & ~behind & ~window(wi, hi) & window(w, h)


# ---- camera moves (test_temporal_gpu's yaw and strafe, and a dolly away from the scene) --------------------------------------------------------------
def quat_mul(a, b):
    ax, ay, az, aw = [float(v) for v in a]
    bx, by, bz, bw = [float(v) for v in b]
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def yaw_camera(cam, degrees):
    """Scene camera, in place: turned about the world's +y through its own position."""
    half = np.radians(degrees) / 2.0
    q = quat_mul([0.0, np.sin(half), 0.0, np.cos(half)], cam.orient)
    cam.orient = (q / np.linalg.norm(q)).astype(f32)


def strafe_camera(cam, dx, dy=0.0, dz=0.0):
    cam.pos = (np.asarray(cam.pos, dtype=np.float64) + [dx, dy, dz]).astype(f32)


def dolly_camera(cam, back):
    """Along the camera's own axis, away from what it looks at: every point moves towards the centre of the new image, so the new image's border
    pixels come from beyond the old one's."""
    q = np.asarray(cam.orient, dtype=np.float64)
    v = np.array([0.0, 0.0, 1.0])
    behind = v + 2.0 * (q[3] * np.cross(q[:3], v) + np.cross(q[:3], np.cross(q[:3], v)))
    strafe_camera(cam, *(back * behind))


MOVES = {"yaw": lambda cam: yaw_camera(cam, -2.0), "strafe": lambda cam: strafe_camera(cam, 0.05, 0.01), "dolly": lambda cam: dolly_camera(cam, 0.3)}


def twin_camera(cam):
    return tt.camera(cam.pos, cam.orient, cam.half_width, cam.half_height, cam.z, cam.exposure)
