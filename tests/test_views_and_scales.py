"""The traversal and the camera rays' candidate lists over a sweep of views and scales.

The candidate lists (kernels.hpp kCollect, collect_leaf, k_primary_cand, k_primary_hits; mirt_launch.hip bundle_half_angle) are complete only
while several hand-chosen margins hold together, and they have no CPU twin; the binary16 boxes (bvh_layout.hpp half_box_adequate,
float_to_half_down / up) and sqrt_trav's slow branch are reached by the other suites only in passing.  Here one seeded cloud of spheres is
seen along every axis, rolled, from inside, from a sphere's centre and surface, from 2000 units away, through focal lengths of 3 to 2000,
as a single tile row and a single tile column and through quaternions that are not unit; a second cloud is scaled by 2^-14 .. 2^+12 and
shifted by up to 70000 (views_and_scales.py).

The reference is the brute-force oracle (ob.TRAV_BRUTE) everywhere and every comparison is on the raw words: mirt.h promises identical
results for every knob involved, so no tolerance appears in this file.  The CPU tests keep the sweep honest — a view that shows nothing, or
a transform that sits on the edge of the binary16 rule, fails here before it can pass vacuously on the GPU.

What the host does with a quaternion that is not unit (views 9 and 10): glm's quat * vec3 is then the map (1 - s^2) I + s^2 R, s = |q|,
which stretches angles by up to its condition number, and the bundle half-angle allows for 1 %.  launch_batch therefore gives a camera
with ||q|^2 - 1| >= 1e-4 no lists at all — its camera rays walk the tree like any other ray — so these views are served, bit for bit, by
the path trace_primary_rays = 1 takes.  mirt_debug_primary_lists still builds and reports lists for them (that is what section D reads);
that no batch reads those lists is asserted separately, through the box-test counter, which then equals the traced renderer's.  The view
"compound_x1.00004" (|q|^2 - 1 = 8e-5) is the largest scaling the lists do serve.

test_default_bundle_is_unchanged pins the box tests of the default, benched path on S(1000) 128 x 128 x 5, five iterations, lists on,
count_traffic: `nodes` = 2 175 226 (NODES_S1000), measured on an MI355X with the host layer this suite was written against.  The count includes k_primary_cand's cone traversal, so it
moves with bundle_half_angle and the cover cut; a change to either for unit quaternions shows here."""
import math

import numpy as np
import pytest

import oracle_binding as ob
import views_and_scales as vs
from test_aov import twin as aov_twin
from test_gpu_parity import assert_same
from views_and_scales import MAX_BOUNCES, N_ACC, BUCKETS, TRANSFORMS, VIEWS, f32

COUNTERS = ("rays", "shadow_rays", "terminated", "dropped")
NODES_S1000 = 2175226       # (see the module docstring)


# ---- the oracle, once per case --------------------------------------------------------------------------------------------------
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def oracle_run(sc, w, h, trav_mode=ob.TRAV_BRUTE):
    """-> accumulator, frame, counters, the camera rays of accumulation 1 and their brute-force hits (all from one Oracle)."""
    o = ob.Oracle(sc, max_bounces=MAX_BOUNCES, buckets=BUCKETS, trav_mode=trav_mode)
    o.Resize(w, h)
    o.Accumulate(N_ACC)
    counters = o.counters()                                                              # (before trace_closest, which counts its rays too)
    p, d = o.raygen(1)
    tfar, prim = o.trace_closest(p, d, ob.TRAV_BRUTE)
    out = dict(acc=o.accumulator().copy(), frame=o.Render().copy(), counters=counters, p=p, d=d, tfar=tfar, prim=prim, prims=o.bvh()[1])
    o.close()
    return out


def view_oracle(mirt, name):
    v = VIEWS[name]
    return cached(("view", name), lambda: oracle_run(v.make(mirt), v.w, v.h))


def transform_scene(mirt, name):
    k, offset = TRANSFORMS[name]
    return vs.transformed(vs.scaled_cloud(mirt), k, offset)


def transform_oracle(mirt, name):
    return cached(("transform", name), lambda: oracle_run(transform_scene(mirt, name), vs.W, vs.H))


def first_hits_all_accumulations(mirt, sc, w, h):
    """Hit distance and BVH-order prim id of every camera ray of accumulations 1 .. N_ACC: [N_ACC][pixel]."""
    o = ob.Oracle(sc, max_bounces=MAX_BOUNCES, buckets=BUCKETS, trav_mode=ob.TRAV_BRUTE)
    o.Resize(w, h)
    out = [o.trace_closest(*o.raygen(a), ob.TRAV_BRUTE) for a in range(1, N_ACC + 1)]
    o.close()
    return np.stack([t for t, _ in out]), np.stack([i for _, i in out])


# ---- C: the sweep itself (CPU) -----------------------------------------------------------------------------------------------------
def test_cloud_is_what_the_views_assume(mirt):
    sc = vs.cloud(mirt)
    geo = sc.geometry
    c = geo["position"].astype(np.float64); r = np.sqrt(geo["radius_sq"].astype(np.float64))
    assert len(geo) == 600 and np.abs(c).max() <= 6.0 and 0.15 <= r[1:].min() and r[1:].max() <= 0.9 and r[0] == vs.BIG_RADIUS
    assert np.array_equal(geo[1:2].view(np.uint8), geo[2:3].view(np.uint8)), "spheres 1 and 2 are one sphere twice"
    assert (np.linalg.norm(c[1:] - c[0], axis=1) - r[1:] > vs.BIG_RADIUS).all(), "a sphere reaches into the radius-2 sphere"
    mats = np.asarray(sc.material)
    lights = (mats["emission"][geo["material_ID"]] > 0).any(axis=1).sum()
    assert lights == 600 // 16 and (sc.ambient == f32(0.3)).all()
    # view 3: the eye lies outside every sphere
    eye = VIEWS["inside_cloud"].make(mirt).camera.pos.astype(np.float64)
    assert (np.linalg.norm(c - eye, axis=1) - r).min() > 0.04 and np.abs(eye).max() <= 3.0
    # view 4: the surface eye is centre + (r, 0, 0) to within one rounding
    eye = VIEWS["sphere_surface"].make(mirt).camera.pos.astype(np.float64)
    assert abs(np.linalg.norm(eye - c[0]) - vs.BIG_RADIUS) < 2.0 ** -22
    # view 1: each axis quaternion looks down its axis from 14 units away
    for name, axis in vs.AXIS_DIRS.items():
        cam = VIEWS[f"axis{name}"].make(mirt).camera
        assert np.abs(vs.forward(cam.orient) - np.asarray(axis)).max() < 1e-7, name
        assert np.abs(cam.pos + 14.0 * np.asarray(axis)).max() < 1e-5, name
    # view 2: yaw 25, pitch -15, roll 37
    fwd, up = vs.forward(vs.COMPOUND), vs.quat_apply(vs.COMPOUND, (0, 1, 0))
    assert abs(math.degrees(math.asin(fwd[1])) + 15.0) < 1e-9 and abs(math.degrees(math.atan2(-fwd[0], -fwd[2])) - 25.0) < 1e-9
    level = np.cross(np.cross(fwd, (0, 1, 0)), fwd); level /= np.linalg.norm(level)
    assert abs(math.degrees(math.acos(np.clip(up @ level, -1, 1))) - 37.0) < 1e-6
    # view 7: |z| = 2 focal at 48 rows; rho plus a unit ray's own cone half-width (alpha^2 = 2^-19) straddles kAlphaFat = 0.03
    alpha_unit = math.sqrt(2.0 ** -19)
    rho = lambda focal: 0.7072 / (2.0 * focal) * 1.01 + 1e-4                           # noqa: E731  bundle_half_angle
    assert rho(12.0) + alpha_unit > 0.03 > rho(13.0) + alpha_unit and rho(3.0) > 0.03
    for name, focal in (("focal3", 3.0), ("focal12", 12.0), ("focal13", 13.0)):
        cam = VIEWS[name].make(mirt).camera; cam.resize(VIEWS[name].w, VIEWS[name].h)
        assert abs(float(cam.z)) == 2.0 * focal


@pytest.mark.parametrize("name", list(VIEWS))
def test_view_shows_what_it_is_for(mirt, name):
    """No view may pass vacuously: the oracle's first hits contain at least three distinct spheres, except for the two views from inside
    the radius-2 sphere (every pixel hits that sphere) and the far view (hits in at most 64 pixels, from at least three spheres).  A view
    whose lists must be non-empty on a quarter of its pixels hits something on a quarter of its pixels: a pixel with a hit has a list."""
    v = VIEWS[name]
    sc = v.make(mirt)
    tfar, prim = first_hits_all_accumulations(mirt, sc, v.w, v.h)
    o = view_oracle(mirt, name)
    assert np.array_equal(prim[0], o["prim"])
    n_pix = prim.shape[1]
    hit_pixels = (prim >= 0).any(axis=0)
    print(f"{name}: {len(np.unique(prim[prim >= 0]))} distinct spheres hit, {hit_pixels.sum()} of {n_pix} pixels hit, |q|^2 = {vs.norm_sq_f32(sc.camera.orient):.6f}")
    if v.guard == "inside":
        big = int(np.flatnonzero((o["prims"]["radius_sq"] == f32(4.0)))[0])
        assert (prim == big).all(), "a pixel does not see the sphere the eye is in"
        if name == "sphere_centre":
            assert np.abs(tfar - 2.0).max() < 1e-5
    elif v.guard == "far":
        assert 0 < hit_pixels.sum() <= 64 and len(np.unique(prim[prim >= 0])) >= 3
    else:
        assert len(np.unique(prim[0][prim[0] >= 0])) >= 3
    if v.klass == "listed":
        assert hit_pixels.sum() >= n_pix // 4
    assert sum(1 for u in VIEWS.values() if u.guard != "three") <= 3


@pytest.mark.parametrize("name", list(TRANSFORMS))
def test_transform_shows_what_it_is_for(mirt, name):
    o = transform_oracle(mirt, name)
    assert len(np.unique(o["prim"][o["prim"] >= 0])) >= 3
    assert (o["prim"] >= 0).mean() > 0.25 and np.isfinite(o["acc"]).all()


def test_scale_sweep_is_not_borderline(mirt):
    """half_box_adequate (bvh_layout.hpp:120-125) over the leaf boxes, restated: the prediction the GPU test asserts.  It must not hang on how a
    leaf box is padded — the host builder asks the rule about build_records' padded boxes, the GPU builder about max|c| + 1.0001 r and 2 r —
    and it must give the values that are fixed beforehand."""
    base = vs.scaled_cloud(mirt)
    r = np.sqrt(base.geometry["radius_sq"].astype(np.float64))
    assert len(r) == 300 and 0.5 <= r.min() and r.max() <= 1.2
    for name in TRANSFORMS:
        sc = transform_scene(mirt, name)
        padded, bare = vs.predicted_half_boxes(sc, pad=True), vs.predicted_half_boxes(sc, pad=False)
        c = sc.geometry["position"].astype(f32); rad = np.sqrt(sc.geometry["radius_sq"].astype(f32))
        gpu_rule = int(all(vs.half_box_adequate(float(np.abs(ci).max() + ri * f32(1.0001)), float(f32(2.0) * ri)) for ci, ri in zip(c, rad)))
        print(f"{name}: half_boxes predicted {padded} (bare spheres {bare}, GPU builder's form {gpu_rule}); largest coordinate {np.abs(c).max():.6g}")
        assert padded == bare == gpu_rule, name
        if name in vs.HALF_BOXES_FIXED:
            assert padded == vs.HALF_BOXES_FIXED[name], f"{name}: the documented rule contradicts the expected layout"
    # the sweep reaches what it is for: binary16 subnormals, coarse steps, the +-60000 limit
    assert np.abs(transform_scene(mirt, "2^-14").geometry["position"]).min() < 6.1e-5
    assert vs.half_ulp_at(48.0) == 2.0 ** -5 and 8 * vs.half_ulp_at(48.0 + 6.0 + 1.2) <= 2 * 0.5
    assert 20000 < np.abs(transform_scene(mirt, "2^+12").geometry["position"]).max() < 60000
    assert np.abs(transform_scene(mirt, "offset70000").geometry["position"]).max() > 60000


@pytest.mark.parametrize("name", vs.NON_UNIT)
def test_non_unit_quaternion_is_a_shear(name, mirt):
    """quat * vec3 for |q| = s is (1 - s^2) I + s^2 R: it does not keep angles, and the angle between a sample and its pixel's axis can
    grow by the map's condition number, of which bundle_half_angle covers 1 %."""
    q = VIEWS[name].make(mirt).camera.orient.astype(np.float64)
    s2 = float(q @ q)
    M = vs.quat_matrix(q)
    want = (1.0 - s2) * np.eye(3) + s2 * vs.rotation_matrix(q)
    assert np.abs(M - want).max() < 1e-14
    sv = np.linalg.svd(M, compute_uv=False)
    cond = sv.max() / sv.min()
    is_routed = abs(vs.norm_sq_f32(q) - 1.0) >= vs.ROUTE_LIMIT
    print(f"{name}: |q|^2 = {s2:.6f}, condition number {cond:.6f}, {'beyond' if cond - 1 > vs.BUNDLE_MARGIN else 'within'} the 1 % margin, "
          f"{'walks the tree' if is_routed else 'served through lists'}")
    if name in vs.MUST_EXCEED_MARGIN:
        assert cond - 1.0 > vs.BUNDLE_MARGIN
    if name == "compound_x1.001":
        assert cond - 1.0 < vs.BUNDLE_MARGIN
    if name in ("look_up", "look_down"):
        assert abs(s2 - 0.5) < 1e-6, "quat_look_at along +-up: right is clamped, the quaternion has norm sqrt(1/2)"
    # a camera the lists serve must lie within the margin, with room: that is what the 1e-4 limit of launch_batch is for
    assert is_routed == (name != "compound_x1.00004")
    if not is_routed:
        assert 1e-5 < cond - 1.0 < vs.BUNDLE_MARGIN / 10
    else:
        assert cond - 1.0 > 5e-4


@pytest.mark.parametrize("case", [("view", n) for n in vs.TWIN_VIEWS] + [("transform", n) for n in vs.TWIN_TRANSFORMS], ids=lambda c: f"{c[0]}-{c[1]}")
def test_oracle_twin_traversal_equals_brute_force(mirt, case):
    """The oracle's own per-ray BVH traversal (the kernels' twin, its default tree) is held to the same sweep."""
    kind, name = case
    if kind == "view":
        v = VIEWS[name]; sc, w, h, want = v.make(mirt), v.w, v.h, view_oracle(mirt, name)
    else:
        sc, w, h, want = transform_scene(mirt, name), vs.W, vs.H, transform_oracle(mirt, name)
    got = oracle_run(sc, w, h, trav_mode=ob.TRAV_PER_RAY_BVH)
    assert_same(got["acc"], want["acc"], f"{name}: TRAV_PER_RAY_BVH vs TRAV_BRUTE")
    assert_same(got["frame"], want["frame"], f"{name}: frame")
    for k in ("rays", "terminated"):                # (shadow_rays is counted per mode: the brute-force loop counts the slots of a stream, the twin its rays)
        assert got["counters"][k] == want["counters"][k], k
    o = ob.Oracle(sc, max_bounces=MAX_BOUNCES, buckets=BUCKETS); o.Resize(w, h)
    tt, ti = o.trace_closest(want["p"], want["d"], ob.TRAV_PER_RAY_BVH)
    o.close()
    assert np.array_equal(ti, want["prim"]); assert_same(tt, want["tfar"], f"{name}: camera rays through the twin")


# ---- the trace-only case at 2^-52 ------------------------------------------------------------------------------------------------------
TINY_K = -52


def tiny_rays(mirt):
    """The scaled cloud times 2^-52 with its camera rays and 20000 incoherent rays (built as in test_trace_kernels_bit_exact, scaled alike),
    the oracle's brute-force answers and the float64 discriminant of every reported hit."""
    def make():
        sc = vs.transformed(vs.scaled_cloud(mirt), TINY_K)
        s = 2.0 ** TINY_K
        o = ob.Oracle(sc); o.Resize(128, 128)
        cp, cd = o.raygen(1)
        rng = np.random.default_rng(3)
        n = 20000
        geo = sc.geometry
        pick = rng.integers(0, len(geo), n)
        nrm = rng.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        rad = np.sqrt(geo["radius_sq"][pick].astype(np.float64))[:, None] * rng.choice([0.5, 1.0, 1.0 + 1e-4, 1.5, 3.0], size=(n, 1))
        p = (geo["position"][pick] + nrm * rad).astype(f32).T
        d = rng.normal(size=(n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32).T
        d[0, :5] = 0.0
        q = n // 4
        d[:, :q] *= rng.choice(np.array([0.9, 0.999, 1.00001, 1.00004, 1.0002, 1.002, 1.06, 1.125, 1.5], dtype=f32), size=q)[None, :]
        P = np.ascontiguousarray(np.concatenate([cp, p], axis=1)); D = np.ascontiguousarray(np.concatenate([cd, d], axis=1))
        wt, wi = o.trace_closest(P, D, ob.TRAV_BRUTE)
        tmax = np.where(wi >= 0, wt * rng.uniform(0.5, 1.5, wt.shape), 10.0 * s).astype(f32)
        wo = o.trace_shadow(P, D, tmax, ob.TRAV_BRUTE)
        prims = o.bvh()[1]
        o.close()
        k = np.flatnonzero(wi >= 0)
        oc = prims["position"][wi[k]].astype(np.float64) - P[:, k].T
        b = (oc * D[:, k].T).sum(axis=1)
        disc = b * b - (oc * oc).sum(axis=1) + prims["radius_sq"][wi[k]].astype(np.float64)
        return dict(sc=sc, P=P, D=D, wt=wt, wi=wi, tmax=tmax, wo=wo, disc=disc)
    return cached("tiny", make)


def test_tiny_scene_reaches_the_slow_square_root(mirt):
    """sqrt_trav takes the library path when a wave holds a discriminant in [0, 2^-100).  At 2^-52 the squared radii are 2^-104 times
    0.25 .. 1.44, so every hit's discriminant is such a value while the misses' are negative: both kinds share waves."""
    t = tiny_rays(mirt)
    n = len(t["wi"])
    small = int(((t["disc"] >= 0) & (t["disc"] < 2.0 ** -100)).sum())
    print(f"2^{TINY_K}: {n} rays, {(t['wi'] >= 0).sum()} hit, {small} hit discriminants below 2^-100, {int(t['wo'].sum())} shadow rays occluded")
    assert small >= n // 100
    assert (t["wi"] >= 0).mean() >= 0.2
    assert 0 < t["wo"].sum() < n and np.isfinite(t["wt"][t["wi"] >= 0]).all() and (t["wt"][t["wi"] >= 0] > 0).any()


# ---- A + D: the view sweep (GPU) ---------------------------------------------------------------------------------------------------
def render(mirt, sc, w, h, **kw):
    r = mirt.Renderer(sc, max_bounces=MAX_BOUNCES, buckets=BUCKETS, **kw)
    r.Resize(w, h)
    r.Accumulate(N_ACC)
    return r


def check_against_oracle(r, o, what):
    assert_same(r.accumulator(), o["acc"], f"{what}: accumulator")
    assert r.Render()
    assert_same(r.GetFrame(), o["frame"], f"{what}: frame")
    assert r.counters()["rays"] == o["counters"]["rays"], f"{what}: rays"
    assert r.counters()["terminated"] == o["counters"]["terminated"], f"{what}: terminated"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VIEWS))
def test_view_lists_traced_and_gpu_built_equal_the_oracle(mirt, name):
    v = VIEWS[name]
    sc = v.make(mirt)
    o = view_oracle(mirt, name)
    n_pix = (v.w // 16) * (v.h // 16) * 256
    kw = dict(use_bvh=True, aov=True, count_traffic=True)
    lists = render(mirt, sc, v.w, v.h, trace_primary_rays=False, **kw)
    traced = render(mirt, sc, v.w, v.h, trace_primary_rays=True, **kw)
    built = render(mirt, sc, v.w, v.h, trace_primary_rays=False, gpu_build=True, **kw)
    for label, r in (("lists", lists), ("traced", traced), ("lists on a GPU-built tree", built)):
        check_against_oracle(r, o, f"{name}, {label}")
    # first hits: the sharp check.  lists == traced == the numpy twin over the oracle's brute-force hits
    assert_same(lists.aov(), traced.aov(), f"{name}: AOV sums, lists vs traced")
    assert_same(built.aov(), traced.aov(), f"{name}: AOV sums, lists on a GPU-built tree vs traced")
    want_aov, _ = aov_twin(sc, v.w, v.h, N_ACC, MAX_BOUNCES)
    assert_same(lists.aov(), want_aov, f"{name}: AOV sums vs the twin")
    cl, ct = lists.counters(), traced.counters()
    for k in COUNTERS:
        assert cl[k] == ct[k], f"{name}: {k} {cl[k]} (lists) vs {ct[k]} (traced)"
    assert_same(lists.GetFrame(), traced.GetFrame(), f"{name}: frame, lists vs traced")
    # stage level: ray generation and the traversal on exactly those rays
    gp, gd = lists.debug_raygen(1)
    assert_same(gp, o["p"], f"{name}: ray origins"); assert_same(gd, o["d"], f"{name}: ray directions")
    gt, gi = lists.debug_trace_closest(o["p"], o["d"])
    assert np.array_equal(gi, o["prim"]), f"{name}: primID of {(gi != o['prim']).sum()} camera rays"
    assert_same(gt, o["tfar"], f"{name}: tfar of the camera rays")
    # D: the path the view is for
    hist = lists.debug_primary_lists()
    is_routed = vs.routed(sc)
    print(f"{name}: lists {hist}; nodes lists {cl['nodes']} traced {ct['nodes']}; {'no batch reads them' if is_routed else 'read by every batch'}")
    assert sum(hist) == n_pix
    if v.klass == "listed":
        assert sum(hist[1:9]) >= n_pix // 4, f"{name}: {sum(hist[1:9])} of {n_pix} pixels have a non-empty list"
    elif v.klass == "fallback":
        assert hist[9] == n_pix
    elif v.klass == "far":
        assert hist[9] > 0
    if is_routed:                                                                       # the same launches as trace_primary_rays = 1
        assert (cl["nodes"], cl["spheres"]) == (ct["nodes"], ct["spheres"]), f"{name}: a camera with |q|^2 off 1 by 1e-4 or more must get no lists"
    elif v.klass == "listed":
        assert (cl["nodes"], cl["spheres"]) != (ct["nodes"], ct["spheres"]), f"{name}: the lists were not used"
    for r in (lists, traced, built):
        r.close()
    if v.brute:
        r = render(mirt, sc, v.w, v.h, use_bvh=False, aov=True)
        check_against_oracle(r, o, f"{name}, use_bvh=False")
        assert_same(r.aov(), want_aov, f"{name}: AOV sums, use_bvh=False")
        r.close()


# ---- B: scales and offsets (GPU) ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TRANSFORMS))
def test_scaled_and_shifted_scene_equals_the_oracle(mirt, name):
    sc = transform_scene(mirt, name)
    o = transform_oracle(mirt, name)
    want_half = vs.predicted_half_boxes(sc)
    if name in vs.HALF_BOXES_FIXED:
        assert want_half == vs.HALF_BOXES_FIXED[name]
    got = {}
    for gpu_build in (False, True):
        r = render(mirt, sc, vs.W, vs.H, use_bvh=True, gpu_build=gpu_build, count_traffic=True)
        what = f"{name}, gpu_build={gpu_build}"
        check_against_oracle(r, o, what)
        info = r.debug_info()
        hist = r.debug_primary_lists()
        print(f"{what}: half_boxes {info['half_boxes']} wide {info['wide']} records {info['records']}; lists {hist}")
        assert info["half_boxes"] == want_half, f"{what}: half_boxes {info['half_boxes']}, the documented rule gives {want_half}"
        assert sum(hist[1:9]) >= vs.W * vs.H // 4, f"{what}: the lists are not in use"
        gt, gi = r.debug_trace_closest(o["p"], o["d"])
        assert np.array_equal(gi, o["prim"]), f"{what}: primID of {(gi != o['prim']).sum()} camera rays"
        assert_same(gt, o["tfar"], f"{what}: tfar of the camera rays")
        got[gpu_build] = (r.accumulator().copy(), r.GetFrame().copy(), {k: r.counters()[k] for k in COUNTERS}, info["half_boxes"])
        r.close()
    assert_same(got[True][0], got[False][0], f"{name}: both builders, accumulator"); assert_same(got[True][1], got[False][1], f"{name}: both builders, frame")
    assert got[True][2:] == got[False][2:], f"{name}: both builders: {got[True][2:]} vs {got[False][2:]}"


@pytest.mark.gpu
def test_tiny_scene_traces_through_the_slow_square_root(mirt):
    t = tiny_rays(mirt)
    for use_bvh in (0, 1):
        r = mirt.Renderer(t["sc"], use_bvh=bool(use_bvh))
        gt, gi = r.debug_trace_closest(t["P"], t["D"])
        assert np.array_equal(gi, t["wi"]), f"primID mismatch use_bvh={use_bvh}: {(gi != t['wi']).sum()}"
        assert_same(gt, t["wt"], f"tfar use_bvh={use_bvh}")
        go = r.debug_trace_shadow(t["P"], t["D"], t["tmax"])
        assert np.array_equal(go, t["wo"]), f"occlusion mismatch use_bvh={use_bvh}: {(go != t['wo']).sum()}"
        r.close()


@pytest.mark.gpu
def test_default_bundle_is_unchanged(mirt):
    """See the module docstring: the box tests of the default path on an existing scene, lists on."""
    r = mirt.Renderer(mirt.scene.synthetic(1000, ambient=0.5), max_bounces=5, use_bvh=True, count_traffic=True)
    r.Resize(128, 128); r.Accumulate(5)
    c = r.counters()
    hist = r.debug_primary_lists()
    print(f"S(1000) 128x128x5, lists: nodes {c['nodes']} spheres {c['spheres']} lists {hist}")
    assert sum(hist[1:9]) > 128 * 128 // 2
    assert c["nodes"] == NODES_S1000
    r.close()
