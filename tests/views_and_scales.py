"""Scenes, cameras and transforms of tests/test_views_and_scales.py: a seeded cloud of spheres looked at from every side, from inside, from
far away, through very long and very short lenses and through quaternions that do not rotate; and a second cloud scaled and shifted until
the binary16 boxes of the tree become subnormal, coarse or unusable.  Everything here is float64 numpy rounded once to binary32: inputs,
not arithmetic under test."""
import copy
import math

import numpy as np

f32 = np.float32
W, H, N_ACC, MAX_BOUNCES, BUCKETS = 64, 48, 5, 3, 5
CLOUD_SEED, SCALED_SEED = 11, 12
BIG_CENTRE, BIG_RADIUS = (1.75, -2.25, 0.75), 2.0             # the sphere the "inside a sphere" views sit in; nothing else reaches into it
ROUTE_LIMIT = 1e-4                                            # mirt_launch.hip launch_batch: ||q|^2 - 1| >= 1e-4 -> no lists, every camera ray walks the tree
BUNDLE_MARGIN = 0.01                                          # bundle_half_angle: 0.7072 / |z| * 1.01


# ---- quaternions (x, y, z, w), float64 ----------------------------------------------------------------------------------------------
def quat_axis(axis, degrees):
    a = np.asarray(axis, dtype=np.float64); a = a / np.linalg.norm(a)
    h = math.radians(degrees) / 2.0
    return np.concatenate([a * math.sin(h), [math.cos(h)]])


def quat_mul(a, b):
    av, aw, bv, bw = a[:3], a[3], b[:3], b[3]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), [aw * bw - av @ bv]])


def quat_apply(q, v):
    """glm operator*(quat, vec3) as camera_ray_dir spells it (device_math.hpp), in float64: v + 2 (w (qv x v) + qv x (qv x v))."""
    q = np.asarray(q, dtype=np.float64); v = np.asarray(v, dtype=np.float64)
    uv = np.cross(q[:3], v)
    uuv = np.cross(q[:3], uv)
    return v + (uv * q[3] + uuv) * 2.0


def quat_matrix(q):
    """The linear map v -> quat_apply(q, v), column by column."""
    return np.stack([quat_apply(q, e) for e in np.eye(3)], axis=1)


def rotation_matrix(q):
    """The rotation of the NORMALISED quaternion, from the textbook formula (not through quat_apply)."""
    x, y, z, w = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def forward(q):
    """Where the camera looks: the image of -z, normalised (camera_ray_dir normalises after the map)."""
    d = quat_apply(q, (0.0, 0.0, -1.0))
    return d / np.linalg.norm(d)


def shortest_arc(direction):
    """The unit quaternion that turns -z into `direction` by the shorter way."""
    d = np.asarray(direction, dtype=np.float64); d = d / np.linalg.norm(d)
    a = np.array([0.0, 0.0, -1.0])
    q = np.concatenate([np.cross(a, d), [1.0 + a @ d]])
    return q / np.linalg.norm(q)


def norm_sq_f32(q):
    """|q|^2 as launch_batch sums it: binary32, x^2 + y^2 + z^2 + w^2 from the left."""
    q = np.asarray(q, dtype=f32)
    return float(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])


R = math.sqrt(0.5)
AXIS_QUATS = {"-z": (0.0, 0.0, 0.0, 1.0), "+z": (0.0, 1.0, 0.0, 0.0), "-x": (0.0, R, 0.0, R), "+x": (0.0, -R, 0.0, R),
              "+y": (R, 0.0, 0.0, R), "-y": (-R, 0.0, 0.0, R)}
AXIS_DIRS = {"-z": (0, 0, -1), "+z": (0, 0, 1), "-x": (-1, 0, 0), "+x": (1, 0, 0), "+y": (0, 1, 0), "-y": (0, -1, 0)}
# yaw 25 degrees about y, then pitch -15 about the turned x, then roll 37 about the view axis
COMPOUND = quat_mul(quat_mul(quat_axis((0, 1, 0), 25.0), quat_axis((1, 0, 0), -15.0)), quat_axis((0, 0, 1), 37.0))


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def _materials(S):
    mats = np.zeros(4, dtype=S.MATERIAL)
    mats["albedo"][:3] = [(0.8, 0.3, 0.3), (0.3, 0.8, 0.3), (0.6, 0.6, 0.9)]
    mats["albedo"][3] = 1.0; mats["emission"][3] = 15.0
    return mats


def _assign_materials(rng, geo):
    n = len(geo)
    geo["material_ID"] = rng.integers(0, 3, n)
    geo["material_ID"][rng.choice(n, max(1, n // 16), replace=False)] = 3


def cloud(mirt, seed=CLOUD_SEED, n=600):
    """n spheres, centres uniform in [-6, 6]^3, radii 0.15 .. 0.9.  Sphere 0 has radius 2 and an empty inside (spheres that would reach into
    it are drawn again); spheres 1 and 2 are the same sphere twice.  Three diffuse materials, an emissive one on n / 16 spheres, ambient 0.3."""
    S = mirt.scene
    rng = np.random.default_rng(seed)
    geo = np.zeros(n, dtype=S.SPHERE)
    big = np.asarray(BIG_CENTRE, dtype=np.float64)
    pos = np.zeros((n, 3)); rad = np.zeros(n)
    pos[0], rad[0] = big, BIG_RADIUS
    for i in range(1, n):
        while True:
            c, r = rng.uniform(-6.0, 6.0, 3), rng.uniform(0.15, 0.9)
            if np.linalg.norm(c - big) > BIG_RADIUS + r + 0.05:
                break
        pos[i], rad[i] = c, r
    pos[2], rad[2] = pos[1], rad[1]
    geo["position"] = pos.astype(f32)
    geo["radius_sq"] = (rad ** 2).astype(f32)
    _assign_materials(rng, geo)
    geo["material_ID"][:3] = (0, 1, 1)
    cam = S.Camera(eye=(0.0, 0.0, 14.0), direction=(0.0, 0.0, -1.0), focal_length=50.0, exposure=1.0)
    return S.Scene(geo, _materials(S), cam, np.full(3, 0.3, dtype=f32), name=f"cloud{seed}")


def scaled_cloud(mirt, seed=SCALED_SEED, n=300):
    """n spheres, centres uniform in [-6, 6]^3, radii 0.5 .. 1.2: no leaf box is thinner than 8 binary16 steps up to coordinates of 64."""
    S = mirt.scene
    rng = np.random.default_rng(seed)
    geo = np.zeros(n, dtype=S.SPHERE)
    geo["position"] = rng.uniform(-6.0, 6.0, (n, 3)).astype(f32)
    geo["radius_sq"] = (rng.uniform(0.5, 1.2, n) ** 2).astype(f32)
    _assign_materials(rng, geo)
    cam = S.Camera(eye=(0.0, 0.0, 14.0), direction=(0.0, 0.0, -1.0), focal_length=50.0, exposure=1.0)
    sc = S.Scene(geo, _materials(S), cam, np.full(3, 0.3, dtype=f32), name=f"scaled_cloud{seed}")
    set_camera(sc, -14.0 * forward(COMPOUND), COMPOUND, 50.0)
    return sc


def set_camera(sc, eye, orient, focal):
    """An explicit quaternion, written into the camera as it stands: no look-at, no normalisation."""
    cam = sc.camera
    cam.pos = np.asarray(eye, dtype=np.float64).astype(f32)
    cam.orient = np.asarray(orient, dtype=np.float64).astype(f32)
    cam.focal_length = float(focal)
    cam.resize(1, 1)


def free_eye(sc, seed=5, box=3.0, margin=0.05):
    """A seeded point of [-box, box]^3 that lies outside every sphere of `sc` by at least `margin` (the first of the seeded draws that does)."""
    rng = np.random.default_rng(seed)
    c = sc.geometry["position"].astype(np.float64); r = np.sqrt(sc.geometry["radius_sq"].astype(np.float64))
    for _ in range(10000):
        p = rng.uniform(-box, box, 3)
        if (np.linalg.norm(c - p, axis=1) - r).min() > margin:
            return p
    raise AssertionError("no free point found")


# ---- views ------------------------------------------------------------------------------------------------------------------------
class View:
    """scene: "cloud" | "default9".  orient: a quaternion (written as is), or None with `direction` for Camera(direction=...), whose eye is then
    placed `back` units behind the target along the direction the returned quaternion really looks.  klass: what section D asserts of the
    candidate lists — "listed", "fallback", "far" or "any".  guard: what section C asserts of the oracle's first hits."""

    def __init__(self, scene="cloud", orient=None, direction=None, eye=None, back=14.0, target=(0.0, 0.0, 0.0), focal=50.0, w=W, h=H,
                 klass="listed", guard="three", brute=False):
        self.scene, self.orient, self.direction, self.eye, self.back, self.target = scene, orient, direction, eye, back, target
        self.focal, self.w, self.h, self.klass, self.guard, self.brute = focal, w, h, klass, guard, brute

    def make(self, mirt):
        sc = cloud(mirt) if self.scene == "cloud" else mirt.scene.default9()
        if self.orient is None:
            q = mirt.scene.Camera(eye=(0.0, 0.0, 0.0), direction=self.direction).orient        # exactly what quat_look_at returns
        else:
            q = np.asarray(self.orient, dtype=np.float64)
        if self.eye == "free":
            eye = free_eye(sc)
        elif self.eye is not None:
            eye = np.asarray(self.eye, dtype=np.float64)
        else:
            eye = np.asarray(self.target, dtype=np.float64) - self.back * forward(np.asarray(q, dtype=np.float64))
        set_camera(sc, eye, q, self.focal)
        return sc


D9_TARGET = (0.0, 0.05, 0.1)
# centre + (r, 0, 0), the sum rounded to binary32
BIG_SURFACE = (float(f32(f32(BIG_CENTRE[0]) + f32(BIG_RADIUS))), BIG_CENTRE[1], BIG_CENTRE[2])
VIEWS = {}
for _name, _q in AXIS_QUATS.items():                                                            # 1: the six axis views
    VIEWS[f"axis{_name}"] = View(orient=_q, brute=(_name == "+z"))
VIEWS["compound"] = View(orient=COMPOUND)                                                       # 2
VIEWS["inside_cloud"] = View(orient=shortest_arc((1, 1, 1)), eye="free", brute=True)            # 3
VIEWS["sphere_centre"] = View(orient=COMPOUND, eye=BIG_CENTRE, klass="any", guard="inside")      # 4
VIEWS["sphere_surface"] = View(orient=AXIS_QUATS["-x"], eye=BIG_SURFACE, klass="any", guard="inside")   # 4: looking back through the centre
# 5: 128 rows put a pixel at 7.5 units across where the cloud is — with 48 rows it is 20, and the five samples of the one or two pixels that
# see the cloud meet it twice on average: too few for the guard's three spheres
VIEWS["far"] = View(orient=COMPOUND, back=2000.0, w=32, h=128, klass="far", guard="far")
# 6: planned at 400 units.  There a ray's own cone (alpha = 1.4e-3 per unit, far above this lens's rho = 2.8e-4) is 0.66 units wide, wider than
# most spheres: 2566 of the 3072 pixels overflowed their list on the GPU and none of the rest held fewer than 8.  At 100 units it is a listed view.
VIEWS["tele"] = View(orient=COMPOUND, back=100.0, focal=2000.0)
VIEWS["focal3"] = View(orient=COMPOUND, back=10.0, focal=3.0, klass="fallback")                  # 7
VIEWS["focal12"] = View(orient=COMPOUND, back=10.0, focal=12.0, klass="fallback")
VIEWS["focal13"] = View(orient=COMPOUND, back=10.0, focal=13.0)
VIEWS["row256x16"] = View(orient=COMPOUND, focal=200.0, w=256, h=16)                             # 8
VIEWS["column16x256"] = View(orient=COMPOUND, focal=25.0, w=16, h=256)
VIEWS["look_up"] = View(direction=(0.0, 1.0, 0.0), klass="any", brute=True)                      # 9
VIEWS["look_down"] = View(direction=(0.0, -1.0, 0.0), klass="any")
VIEWS["compound_x1.001"] = View(orient=COMPOUND * (1.0 + 1e-3))                                  # 10
VIEWS["compound_x1.05"] = View(orient=COMPOUND * 1.05)
VIEWS["compound_x0.9"] = View(orient=COMPOUND * 0.9)
VIEWS["+x_x0.8"] = View(orient=np.asarray(AXIS_QUATS["+x"]) * 0.8)
VIEWS["default9_compound_x1.05"] = View(scene="default9", orient=COMPOUND * 1.05, back=1.2, target=D9_TARGET, focal=40.0)
VIEWS["default9_+x_x0.8"] = View(scene="default9", orient=np.asarray(AXIS_QUATS["+x"]) * 0.8, back=1.2, target=D9_TARGET, focal=40.0)
# not in the sweep as first written: the largest scaling the host still serves through lists (|q|^2 - 1 = 8e-5 < 1e-4), so that the
# 1 % margin of bundle_half_angle is exercised by a map that really stretches angles (the cases above are all routed through the tree)
VIEWS["compound_x1.00004"] = View(orient=COMPOUND * (1.0 + 4e-5))
NON_UNIT = ("look_up", "look_down", "compound_x1.001", "compound_x1.05", "compound_x0.9", "+x_x0.8", "compound_x1.00004")
MUST_EXCEED_MARGIN = ("compound_x1.05", "+x_x0.8")
TWIN_VIEWS = ("axis+z", "inside_cloud", "look_up")


def routed(sc):
    """True when launch_batch gives this camera no lists (its quaternion is too far from unit for the bundle bound)."""
    return abs(norm_sq_f32(sc.camera.orient) - 1.0) >= ROUTE_LIMIT


# ---- transforms -------------------------------------------------------------------------------------------------------------------
# name -> (k of the scale 2^k, offset)
TRANSFORMS = {"2^-14": (-14, None), "2^-6": (-6, None), "2^+8": (8, None), "2^+12": (12, None),
              "offset16": (0, (16.0, -16.0, 16.0)), "offset48": (0, (48.0, 48.0, -48.0)), "offset70000": (0, (70000.0, -70000.0, 3000.0))}
HALF_BOXES_FIXED = {"2^-14": 1, "2^-6": 1, "2^+8": 1, "offset16": 1, "offset70000": 0}          # fixed beforehand; the rest by the rule alone
TWIN_TRANSFORMS = ("2^-14", "offset70000")


def transformed(sc, k=0, offset=None):
    """A copy of `sc` with positions and eye times 2^k (exact in binary32), radius_sq times 2^2k, then shifted by `offset` (rounded)."""
    out = copy.deepcopy(sc)
    s = f32(2.0) ** f32(k)
    geo = np.array(out.geometry)
    geo["position"] = geo["position"] * s
    geo["radius_sq"] = geo["radius_sq"] * s * s
    out.camera.pos = (out.camera.pos * s).astype(f32)
    if offset is not None:
        o = np.asarray(offset, dtype=f32)
        geo["position"] = geo["position"] + o
        out.camera.pos = (out.camera.pos + o).astype(f32)
    out.geometry = geo
    out.name = f"{sc.name} * 2^{k} + {offset}"
    return out


# ---- bvh_layout.hpp:120-125, restated ----------------------------------------------------------------------------------------------
def half_ulp_at(m):
    """Spacing of binary16 values around |m| (bvh_layout.hpp half_ulp_at)."""
    if m < 6.103515625e-05:
        return 5.9604644775390625e-08
    return math.ldexp(1.0, math.frexp(m)[1] - 11)


def half_box_adequate(amax, min_extent):
    """A LEAF box: binary16 is adequate unless a coordinate lies beyond +-60000 or the smallest extent is under 8 quantisation steps."""
    return amax <= 60000.0 and not min_extent < 8.0 * half_ulp_at(amax)


def predicted_half_boxes(sc, pad=True):
    """1 when every leaf box [c - r, c + r] of the scene passes the rule.  pad: the boxes as build_records grows them (by 2^-18 (max|c| + r),
    then one step outward); without it the bare spheres.  A prediction is only used where both agree (test_scale_sweep_is_not_borderline)."""
    c = sc.geometry["position"].astype(f32); r = np.sqrt(sc.geometry["radius_sq"].astype(f32))
    ok = True
    for ci, ri in zip(c, r):
        lo, hi = ci - ri, ci + ri
        if pad:
            p = f32(2.0 ** -18) * (np.abs(ci).max() + ri)
            lo, hi = np.nextafter(lo - p, f32(-np.inf)), np.nextafter(hi + p, f32(np.inf))
        amax = float(max(np.abs(lo).max(), np.abs(hi).max()))
        ok = ok and half_box_adequate(amax, float((hi - lo).min()))
    return int(ok)
