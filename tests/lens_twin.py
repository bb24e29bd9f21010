"""numpy twin of the thin-lens camera ray (csrc/device_math.hpp lens_ray) and the float64 thin-lens definition it is held to.

The reference defines no lens (Camera.hpp:80-88 ignores focus_distance / f_number), so there is no reference text behind this mode.
The oracle carries the project's own lens all the same (orc_set_lens: the operation order below in C++, as it carries mode 2 and the caller's
gloss_decay); tests/test_lens_cpu.py holds Oracle.raygen under a lens to this twin bit for bit, and the twin to the float64 thin lens.
The twin starts from the oracle's own pinhole rays (Oracle.raygen: the unchanged arithmetic of Camera::generate_ray) and restates, in
binary32 array arithmetic with one rounding per operation, exactly what lens_ray does after them:

    rng = hash_2d(acc, seed[ID] + 2 * max_bounces);  u0, u1 = rand_unit_float(rng) twice
    (lx, ly) = disk(u0, u1):  rho = sqrt(u0);  (sin, cos) = fast_sincos(u1 * two_pi);  lx = rho * cos;  ly = rho * sin
    t = focus_depth / dot3(d, fwd);      P = pos + d * t
    ax = A * lx;  ay = A * ly;           O = pos + (right * ax + up * ay)
    D = normalize3(P - O)                dot3 = (x*x + y*y) + z*z,  normalize3 = v * (1 / sqrt(dot3(v, v)))

right / up / fwd = the camera's +x, +y, -z rotated by view.orient with the quat * vec3 formula of camera_ray_dir, in binary32.
Its integer generator and its fast_sincos are pinned in tests/test_lens_cpu.py against the known answers and golden vectors the oracle
tests use."""
import numpy as np

f32 = np.float32
f64 = np.float64
u32 = np.uint32
U = 2.0 ** -24                                    # binary32 unit roundoff
M32 = np.uint64(0xFFFFFFFF)

TWO_PI = f32(6.28318530717958647692528676655900576)
INV_PI = f32(0.318309886183790671537767526745028724)
HALF_PI = f32(1.57079632679489661923132169163975144)


# ---- Random.hpp:5-50 on uint32 arrays ------------------------------------------------------------------------------------------
def _u64(a):
    return np.asarray(a).astype(np.uint64) & M32


def hash_2d(x, y):
    x, y = _u64(x), _u64(y)
    k = np.uint64(0x41C64E6D)
    qx = (k * ((x >> np.uint64(1)) ^ y)) & M32
    qy = (k * ((y >> np.uint64(1)) ^ x)) & M32
    return ((k * (qx ^ (qy >> np.uint64(3)))) & M32).astype(u32)


def pcg_generate(state):
    """-> (output, next state), both uint32 arrays."""
    p = _u64(state)
    nxt = (p * np.uint64(747796405) + np.uint64(2891336453)) & M32
    p = ((((p >> ((p >> np.uint64(28)) + np.uint64(4))) ^ p) * np.uint64(277803737)) & M32)
    return ((p >> np.uint64(22)) ^ p).astype(u32), nxt.astype(u32)


def rand_unit_float(state):
    """-> (float32 in [0, 1], next state): static_cast<float>(x) * 2^-32 (round to nearest even, then an exact scaling)."""
    out, nxt = pcg_generate(state)
    return out.astype(f32) * f32(2.0 ** -32), nxt


# ---- VectorMath.hpp:644-662 ----------------------------------------------------------------------------------------------------
def fast_sincos(x):
    x = np.asarray(x, dtype=f32).copy()
    qf = np.rint(x * INV_PI).astype(f32)
    sign = (qf.astype(np.int32).astype(u32) << u32(31)).astype(u32)
    for c in (-0.78515625, -0.00024187564849853515625, -3.7747668102383613586e-08, -1.2816720341285448015e-12):
        x = x + qf * (f32(c) * f32(4.0))
    x = HALF_PI - (HALF_PI - x)
    x2 = x * x
    x = (x.view(u32) ^ sign).view(f32)
    su = f32(2.6083159809786593541503e-06); cu = f32(-2.71811842367242206819355e-07)
    su = su * x2 - f32(0.0001981069071916863322258); cu = cu * x2 + f32(2.47990446951007470488548e-05)
    su = su * x2 + f32(0.00833307858556509017944336); cu = cu * x2 - f32(0.00138888787478208541870117)
    su = su * x2 - f32(0.166666597127914428710938); cu = cu * x2 + f32(0.0416666641831398010253906)
    su = x2 * (su * x) + x
    cu = cu * x2 - f32(0.5); cu = cu * x2 + f32(1.0)
    cu = (cu.view(u32) ^ sign).view(f32)
    su = np.where(np.abs(su) > f32(1.0), f32(0.0), su).astype(f32)
    cu = np.where(np.abs(cu) > f32(1.0), f32(0.0), cu).astype(f32)
    return su, cu


def disk(t, s):
    """Sampling.hpp:85-104: -> (x, y) = sqrt(t) * (cos, sin)(s * two_pi)."""
    sin_phi, cos_phi = fast_sincos(np.asarray(s, dtype=f32) * TWO_PI)
    rho = np.sqrt(np.asarray(t, dtype=f32))
    return rho * cos_phi, rho * sin_phi


# ---- camera --------------------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return [a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]]      # glm::cross, as device_math.hpp cross3


def quat_rotate(orient, v, dtype=f32):
    """glm operator*(quat, vec3) as camera_ray_dir spells it: v + ((uv * w) + uuv) * 2; v = three scalars or arrays."""
    q = [dtype(orient[0]), dtype(orient[1]), dtype(orient[2])]
    w = dtype(orient[3])
    v = [np.asarray(c, dtype=dtype) for c in v]
    uv = _cross(q, v)
    uuv = _cross(q, uv)
    return [v[k] + ((uv[k] * w) + uuv[k]) * dtype(2.0) for k in range(3)]


def camera_axes(cam, dtype=f32):
    """-> right, up, fwd as (3,) arrays: the camera's +x, +y, -z rotated by cam.orient."""
    return tuple(np.array([dtype(c) for c in quat_rotate(cam.orient, axis, dtype)], dtype=dtype) for axis in ((1, 0, 0), (0, 1, 0), (0, 0, -1)))


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def normalize3(v):
    inv = f32(1.0) / np.sqrt(dot3(v, v))
    return [v[0] * inv, v[1] * inv, v[2] * inv]


def pinhole_dir(cam, x, y, s0=0.5, s1=0.5):
    """Camera::generate_ray's direction (Camera.hpp:80-88) for pixel arrays x, y (after cam.resize): -> (3, n) float32."""
    x = np.atleast_1d(np.asarray(x)); y = np.atleast_1d(np.asarray(y))
    v = [x.astype(f32) + f32(s0) - f32(cam.half_width), y.astype(f32) + f32(s1) - f32(cam.half_height), np.full(x.shape, f32(cam.z), dtype=f32)]
    return np.stack(normalize3(quat_rotate(cam.orient, v))).astype(f32)


def seeds(tiles, max_bounces):
    """seed[ID] of Renderer.hpp:107 for the rays tile * 256 + ID of the global LaunchIndices `tiles` (wraps like the uint32 product)."""
    idx = (np.asarray(tiles, dtype=np.uint64)[:, None] * np.uint64(256) + np.arange(256, dtype=np.uint64)[None, :]).reshape(-1)
    return ((idx * np.uint64(2 * max_bounces + 1)) & M32).astype(u32)


def lens_offset(max_bounces):
    return 2 * max_bounces


def draw_offsets(max_bounces):
    """Seed offsets a path draws from without a lens: raygen and the NEE of bounce 0 at 0 (Renderer.hpp:117,255), the NEE of bounce b at 2b and
    its BRDF sample at 2b + 1 for the bounces that shade a hit at all, b <= max_bounces - 2 (the last bounce only drops, Renderer.hpp:358)."""
    used = {0}
    for b in range(max_bounces - 1):
        used.update((2 * b, 2 * b + 1))
    return used


def lens_points(acc, seed, max_bounces):
    """-> (lx, ly, u0, u1) of accumulation `acc` for the seeds of `seeds()`."""
    rng = hash_2d(np.full(seed.shape, acc, dtype=u32), (_u64(seed) + np.uint64(lens_offset(max_bounces))) & M32)
    u0, rng = rand_unit_float(rng)
    u1, rng = rand_unit_float(rng)
    lx, ly = disk(u0, u1)
    return lx, ly, u0, u1


def lens_rays(cam, d, acc, seed, max_bounces, aperture, focus_depth):
    """The lens rays derived from the pinhole directions d (3, n) float32 of the rays with seeds `seed`: -> O (3, n), D (3, n) float32."""
    A, fd = f32(aperture), f32(focus_depth)
    right, up, fwd = camera_axes(cam)
    pos = np.asarray(cam.pos, dtype=f32)
    d = [np.asarray(d[k], dtype=f32) for k in range(3)]
    lx, ly, _, _ = lens_points(acc, seed, max_bounces)
    t = fd / dot3(d, fwd)
    P = [pos[k] + d[k] * t for k in range(3)]
    ax, ay = A * lx, A * ly
    O = [pos[k] + (right[k] * ax + up[k] * ay) for k in range(3)]
    D = normalize3([P[k] - O[k] for k in range(3)])
    O, D = np.stack(O).astype(f32), np.stack(D).astype(f32)
    assert O.dtype == f32 and D.dtype == f32
    return O, D


def oracle_lens_rays(oracle, acc, aperture, focus_depth, tiles=None):
    """Lens rays of Accumulate() number `acc` for an Oracle that has been Resize()d over the whole image; `tiles` = the global LaunchIndices a
    context owns, in its local order (None: all)."""
    p, d = oracle.raygen(acc)
    n_tiles = p.shape[1] // 256
    tiles = np.arange(n_tiles) if tiles is None else np.asarray(tiles)
    pick = (tiles[:, None] * 256 + np.arange(256)[None, :]).reshape(-1)
    return lens_rays(oracle.scene.camera, d[:, pick], acc, seeds(tiles, oracle.max_bounces), oracle.max_bounces, aperture, focus_depth)


# ---- float64 thin lens, from the textbook (e.g. Pharr, Jakob, Humphreys, "Physically Based Rendering", 6.2.3) -----------------------------
def focus_points64(cam, d, focus_depth):
    """Where the pinhole ray pos + s d meets the plane of focus {x : (x - pos) . fwd = focus_depth}: -> F (n, 3), cos(theta) (n,).  Every ray
    from any lens point through F belongs to that pixel sample: this is the thin-lens construction."""
    _, _, fwd = camera_axes(cam, f64)
    d = np.asarray(d, dtype=f64).T
    cos = d @ fwd
    return np.asarray(cam.pos, dtype=f64)[None, :] + d * (f64(focus_depth) / cos)[:, None], cos


FOCUS_K = 30.0
"""Distance from the float64 focus point F to the binary32 ray (O, D), in units of u (|pos| + focus_depth / cos(theta)); u = 2^-24, t = focus_depth / cos.
  fwd in binary32: 5 roundings per component behind unit-size terms -> |fwd32 - fwd64| <= 8u, a relative error 8u / cos of dot(d, fwd);
  the dot itself: 3 roundings over terms that sum to at most 1 in magnitude -> 3u / cos; the division: u.          t32 = t (1 + (11 / cos + 1) u)
  P_k = pos_k + d_k t: one rounding of the product, one of the sum -> |P - F| <= (11 / cos + 1) u t + u t + u (|pos| + t)
  v = P - O: u |v| per component, <= 2u |v| in norm; D = v * inv: a common factor does not turn the line, the three products round by u each,
  <= 2u in angle -> the line through O along D passes P within 4u |v|, |v| <= t + A <= 2t.
  Sum: u ((11 / cos + 3) t + |pos| + 8t) <= u (11 / cos + 11)(|pos| + t); with cos >= 0.58 (asserted by the test: the cameras' corners) <= 30 u (|pos| + t).
  O itself is taken as given (the ray starts where the binary32 O says), so its rounding does not enter."""


def distance_to_line(F, O, D):
    O = np.asarray(O, dtype=f64).T; D = np.asarray(D, dtype=f64).T
    D = D / np.linalg.norm(D, axis=1)[:, None]
    w = F - O
    return np.linalg.norm(w - (w * D).sum(axis=1)[:, None] * D, axis=1)
