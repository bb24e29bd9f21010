"""First-hit AOVs (mirt_set_aov; the reference's compiled-out FIRST BOUNCE OUTPUTS, Renderer.hpp:216-231): per pixel, the f32 sums over the
accumulations 1, 2, 3, ... of the camera ray's hit distance (1e4 on a miss), its flipped world-space normal and the colour its closure is
set up with, in a slab [tile][plane 0..6][256] beside the accumulator.

The yardstick is a numpy twin in this file: Oracle.raygen + Oracle.trace_closest (brute force, the FMA form every camera ray takes) give
ray and hit; everything after is float32 array arithmetic with the glm definitions of device_math.hpp (dot = (x*x + y*y) + z*z,
normalize = v * (1 / sqrt(dot))), one rounding per operation.  GPU results are compared with it on the raw words (`view(uint32)`)."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
from oracle_binding import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
MIRT_NOT_READY, MIRT_ERR_ARG, MIRT_ERR_STATE = 1, -1, -3
MISS_DEPTH = f32(1e4)
NEW_NAMES = ("mirt_set_aov", "mirt_get_aov", "mirt_aov_floats", "mirt_read_aov", "mirt_aov_device", "mirt_load_aov", "mirt_render_aov",
             "mirt_group_set_aov", "mirt_group_aov_floats", "mirt_group_read_aov", "mirt_group_render_aov")


def assert_same(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} words differ"


# ---- scenes built here ---------------------------------------------------------------------------------------------------------
def flip_scene(mirt):
    """The camera INSIDE one large sphere (its far wall is hit from within: dot(N, D) >= 0, the normal is flipped) with three small
    spheres in view (hit from outside: not flipped).  None of the shipped scenes flips a normal at bounce 0."""
    s = mirt.scene
    mats = [s._material(albedo=(0.5, 0.25, 0.125), F0=(0.0625, 0.125, 0.25), roughness=0.5),
            s._material(albedo=(0.75, 0.75, 0.25), F0=(0.9, 0.6, 0.3), roughness=0.2),
            s._material(albedo=(0.1, 0.9, 0.4), emission=(5, 5, 5), F0=(0.04, 0.04, 0.04), roughness=1.0)]
    geo = [s._sphere((0.0, 0.0, 0.0), 20.0 * 20.0, 0),
           s._sphere((-0.8, 0.0, 0.0), 0.4 * 0.4, 1), s._sphere((0.8, 0.3, -1.0), 0.4 * 0.4, 1), s._sphere((0.0, -0.6, 0.5), 0.3 * 0.3, 2)]
    cam = s.Camera(eye=(0.0, 0.0, 3.0), direction=(0.0, 0.0, -1.0), focal_length=50.0, exposure=1.0)
    return s.Scene(np.array(geo, dtype=s.SPHERE), np.array(mats, dtype=s.MATERIAL), cam, np.full(3, 0.5, dtype=f32), name="flip")


ONE_ALBEDO = (0.25, 0.5, 0.75)       # exact in binary32: n hits sum to n * albedo without rounding


def one_sphere_scene(mirt):
    s = mirt.scene
    cam = s.Camera(eye=(0.0, 0.0, 6.0), direction=(0.0, 0.0, -1.0), focal_length=50.0, exposure=1.0)
    return s.Scene(np.array([s._sphere((0.0, 0.0, 0.0), 1.0, 0)], dtype=s.SPHERE), np.array([s._material(albedo=ONE_ALBEDO, F0=(0.5, 0.5, 0.5))], dtype=s.MATERIAL),
                   cam, np.ones(3, dtype=f32), name="one_sphere")


# ---- the twin ----------------------------------------------------------------------------------------------------------------
def twin(sc, w, h, n_acc, max_bounces=16, brdf=0):
    """-> (sums [tile][7][256] f32 over accumulations 1..n_acc in order, {"miss", "hit", "flip"} counts)."""
    o = ob.Oracle(sc, max_bounces=max_bounces, trav_mode=ob.TRAV_BRUTE)
    o.Resize(w, h)
    prims = o.bvh()[1]                                            # BVH order: what primID indexes
    centre = np.ascontiguousarray(prims["position"], dtype=f32)
    colour_of_prim = np.ascontiguousarray(np.asarray(sc.material, dtype=o.MATERIAL)["F0" if brdf else "albedo"], dtype=f32)[prims["material_ID"]]
    n = (w // 16) * (h // 16) * 256
    sums = np.zeros((7, n), dtype=f32)
    counts = {"miss": 0, "hit": 0, "flip": 0}
    for a in range(1, n_acc + 1):
        p, d = o.raygen(a)
        tfar, prim = o.trace_closest(p, d, ob.TRAV_BRUTE)
        hit = prim >= 0
        k = np.flatnonzero(hit)
        O, D, t = p[:, k], d[:, k], tfar[k]
        H = O + D * t                                             # hit = O + D * depth, unfused (two roundings)
        v = H - centre[prim[k]].T
        dot = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        N = v * (f32(1.0) / np.sqrt(dot))                         # glm::normalize
        flip = ((N[0] * D[0] + N[1] * D[1]) + N[2] * D[2]) >= f32(0.0)
        N = np.where(flip, -N, N)
        sums[0, ~hit] += MISS_DEPTH
        sums[0, k] += t
        sums[1:4, k] += N
        sums[4:7, k] += colour_of_prim[prim[k]].T
        counts["miss"] += int((~hit).sum()); counts["hit"] += len(k); counts["flip"] += int(flip.sum())
    o.close()
    assert sums.dtype == f32 and np.isfinite(sums).all()
    return np.ascontiguousarray(sums.reshape(7, n // 256, 256).transpose(1, 0, 2)), counts


def twin_resolve(sums, w, h, n_acc):
    """mirt_render_aov of a whole-image slab: -> depth (h, w), normal (h, w, 3), albedo (h, w, 3)."""
    h_tiles = w // 16
    img = np.zeros((7, h, w), dtype=f32)
    for t in range(sums.shape[0]):
        x0, y0 = 16 * (t % h_tiles), 16 * (t // h_tiles)
        img[:, y0:y0 + 16, x0:x0 + 16] = sums[t].reshape(7, 16, 16)
    nf = f32(n_acc)
    depth = img[0] / nf
    albedo = np.moveaxis(img[4:7] / nf, 0, -1)
    v = img[1:4]
    dot = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        nrm = v * (f32(1.0) / np.sqrt(dot))
    nrm = np.where(dot == f32(0.0), f32(0.0), nrm).astype(f32)
    return np.ascontiguousarray(depth), np.ascontiguousarray(np.moveaxis(nrm, 0, -1)), np.ascontiguousarray(albedo)


_twin_cache = {}


def cached_twin(key, make):
    if key not in _twin_cache:
        _twin_cache[key] = make()
    return _twin_cache[key]


# name -> (scene factory, width, height, accumulations, max_bounces, brdf, renderer kwargs)
CASES = {
    "default9": (lambda m: m.scene.default9(), 64, 64, 10, 16, 0, {}),
    "S1000_bvh": (lambda m: m.scene.synthetic(1000, ambient=0.5), 128, 128, 10, 5, 0, {"use_bvh": True}),
    "white_furnace": (lambda m: m.scene.white_furnace(), 64, 48, 10, 16, 0, {}),
    "flip": (flip_scene, 64, 64, 10, 8, 0, {"use_bvh": True}),
    "brdf_test_ggx": (lambda m: m.scene.brdf_test(), 96, 64, 10, 6, 1, {"use_bvh": True}),
}


def case_twin(mirt, name):
    make, w, h, n, mb, brdf, _ = CASES[name]
    return cached_twin(name, lambda: twin(make(mirt), w, h, n, mb, brdf))


def case_renderer(mirt, name, **more):
    make, w, h, _, mb, brdf, kw = CASES[name]
    r = mirt.Renderer(make(mirt), max_bounces=mb, brdf=brdf, aov=True, **{**kw, **more})
    r.Resize(w, h)
    return r


def s1000(mirt):
    return mirt.scene.synthetic(1000, ambient=0.5)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_aov_interface_is_declared_at_every_layer(mirt):
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    declared = set(re.findall(r"^int\s+(mirt_\w+)\s*\(", header, flags=re.M))
    lib = mirt.load_library()
    raw = C.CDLL(mirt.LIB_PATH)
    for n in NEW_NAMES:
        assert n in declared, f"{n} is not declared (on one line) in include/mirt.h"
        assert hasattr(raw, n), f"{n} is not exported by libmirt.so"
        assert n in lib._declared, f"{n} is not bound in Python"
    assert {n for n in declared if "aov" in n} == set(NEW_NAMES)
    for text in ("MIRT_AOV_DEPTH = 0, MIRT_AOV_NORMAL = 1, MIRT_AOV_ALBEDO = 2", "#define MIRT_AOV_PLANES 7u", "Renderer.hpp:216-231", "exact stream order", "has not been run"):
        assert text in header
    assert C.sizeof(mirt.Policy) == 48                                           # a setter of its own: mirt_policy keeps its layout
    for cls in (mirt.Renderer, mirt.GroupRenderer):
        assert inspect.signature(cls).parameters["aov"].default is False
        for method in ("set_aov", "aov", "render_aov"):
            assert callable(getattr(cls, method))
    assert callable(mirt.Renderer.load_aov)
    assert (mirt.AOV_DEPTH, mirt.AOV_NORMAL, mirt.AOV_ALBEDO, mirt.AOV_PLANES) == (0, 1, 2, 7)


def test_aov_calls_fail_without_a_context(mirt):
    lib = mirt.load_library()
    assert lib.mirt_set_aov(None, 1) < 0
    assert lib.mirt_render_aov(None, 0, None) < 0
    assert lib.mirt_read_aov(None, None) < 0 and lib.mirt_load_aov(None, None, 0) < 0 and lib.mirt_aov_floats(None, None) < 0
    assert lib.mirt_group_set_aov(None, 1) < 0 and lib.mirt_group_render_aov(None, 0, None) < 0 and lib.mirt_group_read_aov(None, None) < 0


def test_twin_on_one_sphere(mirt):
    """Unit sphere at the origin seen from (0, 0, 6) down -z, 32 x 32, 6 accumulations.  Pixel (16, 16) is the one whose un-jittered ray
    (s = 0) runs along the axis through the centre.  Its samples lie at image-plane offsets in [0, 1)^2, so their angle to the axis has
    tan(theta) < sqrt(2) / |z|; a ray at angle theta hits at L cos(theta) - sqrt(r^2 - L^2 sin^2(theta)), which grows with theta from
    L - r = 5.  Hence every sample's depth lies in [5, depth(theta_max)] (+- 1e-5 for the f32 arithmetic of a distance of about 5)."""
    sc = one_sphere_scene(mirt)
    n_acc, w, h = 6, 32, 32
    sums, counts = twin(sc, w, h, n_acc)
    assert counts["hit"] > 0 and counts["miss"] > 0 and counts["flip"] == 0
    x, y = w // 2, h // 2
    tile, ID = (y // 16) * (w // 16) + x // 16, (y % 16) * 16 + x % 16
    px = sums[tile, :, ID].astype(np.float64)
    L, r = 6.0, 1.0
    z = float(sc.camera.z)                                                               # half_height * (-2 / 24) * focal_length = -66.67
    assert abs(z + 16.0 * 50.0 / 12.0) < 1e-3
    sin_max = math.sin(math.atan(math.sqrt(2.0) / abs(z)))
    depth_max = L * math.sqrt(1.0 - sin_max ** 2) - math.sqrt(r * r - (L * sin_max) ** 2)
    assert 5.0 < depth_max < 5.01
    assert n_acc * (L - r - 1e-5) <= px[0] <= n_acc * (depth_max + 1e-5), px[0]
    assert px[3] > 0 and px[3] == np.abs(px[1:4]).max()                                  # the normal's largest component points at the eye (+z from the centre)
    assert px[4:7].tolist() == [n_acc * a for a in ONE_ALBEDO]                           # all six samples hit
    # a corner pixel misses every time: depth n * 1e4, nothing else
    corner = sums[0, :, 0]
    assert corner[0] == f32(n_acc * 1e4) and not corner[1:].any()
    # every pixel: albedo sum = albedo * its hit count, hit count from the depth plane's misses
    depth, nrm, alb = twin_resolve(sums, w, h, n_acc)
    assert depth.shape == (h, w) and nrm.shape == (h, w, 3) and alb.shape == (h, w, 3)
    length = np.sqrt((nrm.astype(np.float64) ** 2).sum(-1))
    assert np.all((np.abs(length - 1.0) < 1e-6) | (length == 0.0)) and (length == 0.0).any() and (length > 0).any()


def test_twin_flip_scene_covers_both_signs(mirt):
    """The flip scene must keep covering `dot(N, D) >= 0`: flipped and unflipped hits both occur (at the size the GPU test uses)."""
    _, counts = case_twin(mirt, "flip")
    assert counts["flip"] > 0, counts
    assert counts["hit"] - counts["flip"] > 0, counts
    assert counts["miss"] == 0, counts                                                  # the camera is inside a sphere


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_sums_and_images_equal_the_twin(mirt, name):
    _, w, h, n, _, _, _ = CASES[name]
    want, counts = case_twin(mirt, name)
    assert counts["hit"] > 0
    r = case_renderer(mirt, name)
    assert r.aov_enabled
    r.Accumulate(n)
    got = r.aov()
    assert got.shape == want.shape == ((w // 16) * (h // 16), 7, 256)
    assert_same(got, want, f"{name}: AOV sums vs the numpy twin")
    for which, img in zip((mirt.AOV_DEPTH, mirt.AOV_NORMAL, mirt.AOV_ALBEDO), twin_resolve(want, w, h, n)):
        assert_same(r.render_aov(which), img, f"{name}: render_aov({which}) vs the twin's resolve")
    r.close()


INVARIANCE = {
    "max_batch=1": dict(max_batch=1), "max_batch=5": dict(max_batch=5), "max_batch=0": dict(max_batch=0),
    "streams=1": dict(streams=1), "streams=3": dict(streams=3), "streams=3,max_batch=2": dict(streams=3, max_batch=2),
    "trace_primary_rays=0": dict(trace_primary_rays=False), "trace_primary_rays=1": dict(trace_primary_rays=True),
    "use_bvh=0": dict(use_bvh=False), "use_bvh=1": dict(use_bvh=True), "gpu_build=1": dict(gpu_build=True), "reference_tree=1": dict(reference_tree=True),
}


@pytest.mark.gpu
def test_gpu_sums_do_not_depend_on_launch_shape(mirt):
    """synthetic(1000) 128 x 128 x 13: one slab, whatever the batch size, the streams in flight, the way camera rays are traced, the tree,
    and whether the 13 accumulations arrive as one call or as 13 asynchronous ones."""
    w, h, n, mb = 128, 128, 13, 5
    want, _ = cached_twin("S1000x13", lambda: twin(s1000(mirt), w, h, n, mb))
    for label, kw in INVARIANCE.items():
        for asynchronous in (False, True):
            r = mirt.Renderer(s1000(mirt), max_bounces=mb, aov=True, **{"use_bvh": True, **kw})
            r.Resize(w, h)
            if asynchronous:
                for _ in range(n):
                    r.AccumulateAsync(1)
            else:
                r.Accumulate(n)
            assert_same(r.aov(), want, f"{label}, {'13 x AccumulateAsync(1)' if asynchronous else 'Accumulate(13)'}")
            assert r.accumulations == n
            r.close()


@pytest.mark.gpu
def test_gpu_aov_has_no_side_effect(mirt):
    """Accumulator, frame and every counter are the same words with AOVs on and off; the kernel counts nothing."""
    res = {}
    for on in (False, True):
        r = mirt.Renderer(s1000(mirt), max_bounces=5, use_bvh=True, count_traffic=True, aov=on, max_batch=4, streams=3)
        r.Resize(128, 128)
        r.Accumulate(10)
        assert r.Render()
        res[on] = (r.accumulator().copy(), r.GetFrame().copy(), r.counters())
        n = C.c_size_t(99)
        assert r._lib.mirt_aov_floats(r._ctx, C.byref(n)) == 0 and n.value == (64 * 7 * 256 if on else 0)
        if not on:
            buf = np.zeros(64 * 7 * 256, dtype=f32)
            assert r._lib.mirt_read_aov(r._ctx, buf.ctypes.data_as(C.c_void_p)) == MIRT_ERR_STATE
            assert r._lib.mirt_render_aov(r._ctx, 0, buf.ctypes.data_as(C.c_void_p)) == MIRT_ERR_STATE
        r.close()
    assert_same(res[True][0], res[False][0], "accumulator with AOVs on vs off")
    assert_same(res[True][1], res[False][1], "frame with AOVs on vs off")
    assert res[True][2] == res[False][2] and res[True][2]["rays"] > 0 and res[True][2]["spheres"] > 0


@pytest.mark.gpu
def test_gpu_aov_sharding(mirt):
    w, h, n, mb = 128, 128, 13, 5
    want, _ = cached_twin("S1000x13", lambda: twin(s1000(mirt), w, h, n, mb))
    single = mirt.Renderer(s1000(mirt), max_bounces=mb, use_bvh=True, aov=True)
    single.Resize(w, h); single.Accumulate(n)
    whole = single.aov()
    assert_same(whole, want, "single context")
    images = [single.render_aov(k) for k in range(3)]
    single.close()
    h_tiles, v_tiles = w // 16, h // 16
    merged = np.zeros((v_tiles, h_tiles, 7, 256), dtype=f32)
    painted = [np.full_like(img, -7.0) for img in images]
    for rank in range(2):
        r = mirt.Renderer(s1000(mirt), max_bounces=mb, use_bvh=True, aov=True)
        r.Resize(w, h); r.SetTileRows(rank, 2); r.Accumulate(n)
        part = r.aov()
        assert part.shape == (v_tiles // 2 * h_tiles, 7, 256)
        merged[rank::2] = part.reshape(v_tiles // 2, h_tiles, 7, 256)
        for k in range(3):
            assert r.render_aov(k, out=painted[k]) is painted[k]                          # only the context's own tiles are written
        r.close()
    assert_same(merged.reshape(-1, 7, 256), whole, "two contexts with interleaved tile rows")
    for k in range(3):
        assert_same(painted[k], images[k], f"render_aov({k}) painted by two contexts into one buffer")
    g = mirt.GroupRenderer(s1000(mirt), devices=[0, 0, 0], max_bounces=mb, use_bvh=True, aov=True)
    g.Resize(w, h); g.Accumulate(n)
    assert_same(g.read_aov(), whole, "GroupRenderer(devices=[0, 0, 0]).read_aov()")
    for k in range(3):
        assert_same(g.render_aov(k), images[k], f"GroupRenderer.render_aov({k})")
    g.Accumulate(2)                                                                      # the gather is repeated after more accumulations
    assert g.aov()[:, 4:7].max() > whole[:, 4:7].max()
    g.close()


@pytest.mark.gpu
def test_gpu_aov_state_rules(mirt):
    sc = mirt.scene.default9()
    r = mirt.Renderer(sc, max_bounces=4)
    r.Resize(64, 64)
    lib, ctx = r._lib, r._ctx
    assert not r.aov_enabled
    assert lib.mirt_set_aov(ctx, 2) == MIRT_ERR_ARG
    r.Accumulate(1)
    assert lib.mirt_set_aov(ctx, 1) == MIRT_ERR_STATE and b"before the first accumulation" in lib.mirt_last_error(ctx)
    r.ResetAccumulator()
    r.set_aov(True)
    assert r.aov().shape == (16, 7, 256) and not r.aov().any()
    # render_aov before any accumulation: MIRT_NOT_READY, the buffer untouched
    buf = np.full((64, 64, 3), 5.0, dtype=f32)
    assert lib.mirt_render_aov(ctx, mirt.AOV_NORMAL, buf.ctypes.data_as(C.c_void_p)) == MIRT_NOT_READY and (buf == 5.0).all()
    assert r.render_aov(mirt.AOV_DEPTH) is None
    assert lib.mirt_render_aov(ctx, 3, buf.ctypes.data_as(C.c_void_p)) == MIRT_ERR_ARG
    r.Accumulate(3)
    first = r.aov().copy()
    assert first.any() and lib.mirt_set_aov(ctx, 1) == 0                                  # already on: nothing changes
    assert_same(r.aov(), first, "set_aov(1) while on")
    assert r.render_aov(mirt.AOV_DEPTH) is not None                                       # 3 accumulations of 5 buckets: no multiple needed
    # exact stream order and AOVs refuse each other, and say why
    assert lib.mirt_set_stream_order(ctx, 1) == MIRT_ERR_STATE and b"hit records" in lib.mirt_last_error(ctx)
    assert r.stream_order == 0
    # reset zeroes, resize reallocates (and zeroes)
    r.ResetAccumulator()
    assert not r.aov().any() and r.accumulations == 0
    r.Accumulate(3)
    assert_same(r.aov(), first, "after a reset the same three accumulations")
    r.Resize(96, 32)
    assert r.aov().shape == (12, 7, 256) and not r.aov().any()
    r.Resize(64, 64)
    # load_aov round-trips from host and from device
    r.Accumulate(3)
    r.load_aov(np.zeros_like(first))
    assert not r.aov().any()
    r.load_aov(first)
    assert_same(r.aov(), first, "load_aov from host")
    other = mirt.Renderer(sc, max_bounces=4, aov=True)
    other.Resize(64, 64)
    ptr, nbytes = r.aov_device()
    assert nbytes == first.nbytes
    other.load_aov(ptr, is_device=True)
    assert_same(other.aov(), first, "load_aov from device")
    other.close()
    # off: frees the slab at any time, deferred calls are launched first
    r.AccumulateAsync(1)
    r.set_aov(False)
    assert not r.aov_enabled and r.accumulations == 4
    assert lib.mirt_set_aov(ctx, 1) == MIRT_ERR_STATE
    r.close()
    e = mirt.Renderer(sc, max_bounces=4, exact_stream_order=True)
    assert e._lib.mirt_set_aov(e._ctx, 1) == MIRT_ERR_STATE and b"hit records" in e._lib.mirt_last_error(e._ctx)
    e.set_stream_order(False)
    e.set_aov(True)
    e.close()
    with pytest.raises(mirt.MirtError):
        mirt.Renderer(sc, max_bounces=4, exact_stream_order=True, aov=True)


def read_pfm(path):
    with open(path, "rb") as f:
        kind = f.readline().strip()
        w, h = (int(v) for v in f.readline().split())
        assert float(f.readline()) < 0                                                   # little-endian
        data = np.frombuffer(f.read(), dtype="<f4")
    ch = {b"Pf": 1, b"PF": 3}[kind]
    assert data.size == w * h * ch
    return kind, data.reshape((h, w) if ch == 1 else (h, w, 3))


@pytest.mark.gpu
def test_gpu_headless_writes_the_three_aovs(mirt, tmp_path):
    exe = os.path.join(mirt.CSRC, "mirt_headless")
    prefix = str(tmp_path / "first_hit")
    subprocess.run([exe, "--scene", "default9", "--size", "64x64", "--spp", "10", "--aov", prefix], check=True, capture_output=True, text=True)
    r = mirt.Renderer(mirt.scene.default9(), use_bvh=True, aov=True)
    r.Resize(64, 64); r.Accumulate(10)
    for which, name, kind in ((mirt.AOV_DEPTH, "depth", b"Pf"), (mirt.AOV_NORMAL, "normal", b"PF"), (mirt.AOV_ALBEDO, "albedo", b"PF")):
        got_kind, got = read_pfm(f"{prefix}.{name}.pfm")
        assert got_kind == kind
        assert_same(got, r.render_aov(which), f"{name}.pfm vs render_aov")
    r.close()
