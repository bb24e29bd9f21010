"""Thin-lens depth of field on the device (mirt_set_lens, mirt_pick_focus): the LENS kernels against the numpy twin of tests/lens_twin.py on
the raw words, the pinhole path untouched by a closed aperture, the invariances of the lens-on accumulator, closed forms, the circle of
confusion and the focus pick.  The reference defines no lens; the oracle carries the project's (orc_set_lens, held to the twin bit for bit in
tests/test_lens_cpu.py), and the whole path under a lens - every LENS kernel, with and without light RIS, dense and sparse - is held to it word for
word here.  The AOVs under a lens keep their own twin."""
import ctypes as C
import math

import numpy as np
import pytest

import definitions as df
import lens_twin as lt
import oracle_binding as ob
import test_definitions_cpu as cpu
import test_light_ris_gpu as rg
from oracle_binding import bits

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
MIRT_ERR_ARG, MIRT_ERR_STATE = -1, -3
MISS_DEPTH = f32(1e4)


def assert_same(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} words differ"


def s1000(mirt):
    return mirt.scene.synthetic(1000, ambient=0.5)


SCENES = {"default9": (lambda m: m.scene.default9(), 16, (0.03, 1.1)), "S1000": (s1000, 5, (0.15, 25.0))}     # factory, max_bounces, (A, focus_depth)


def raw_raygen(r, acc, n_tiles):
    n = n_tiles * 256
    p = np.empty((3, n), dtype=f32); d = np.empty((3, n), dtype=f32)
    r._check(r._lib.mirt_debug_raygen(r._ctx, acc, p.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p)))
    return p, d


# ---- rays ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_lens_rays_equal_the_twin(mirt, name):
    make, mb, (A, fd) = SCENES[name]
    sc = make(mirt)
    o = ob.Oracle(sc, max_bounces=mb); o.Resize(64, 64)
    r = mirt.Renderer(make(mirt), max_bounces=mb); r.Resize(64, 64)
    r.set_lens(A, fd)
    assert r.lens() == (float(f32(A)), float(f32(fd)))
    partitions = ((None, np.arange(16)), ((1, 2), np.array([4, 5, 6, 7, 12, 13, 14, 15])))       # whole image; tile rows 1, 3
    for rows, tiles in partitions:
        if rows:
            r.SetTileRows(*rows)
        for acc in (1, 2, 9):
            p, d = raw_raygen(r, acc, len(tiles))
            O, D = lt.oracle_lens_rays(o, acc, A, fd, tiles)
            assert_same(p, O, f"{name} origins, accumulation {acc}, rows {rows}")
            assert_same(d, D, f"{name} directions, accumulation {acc}, rows {rows}")
    assert len(np.unique(bits(p)[0])) > 1000                          # the origins do differ from ray to ray
    r.close(); o.close()


# ---- AOVs: k_trace<primary, LENS> and k_first_hit_aov<LENS> ------------------------------------------------------------------------------
def aov_twin(sc, w, h, n_acc, mb, A, fd):
    """tests/test_aov.py's twin with the lens rays in place of the pinhole rays."""
    o = ob.Oracle(sc, max_bounces=mb, trav_mode=ob.TRAV_BRUTE); o.Resize(w, h)
    prims = o.bvh()[1]
    centre = np.ascontiguousarray(prims["position"], dtype=f32)
    colour = np.ascontiguousarray(np.asarray(sc.material, dtype=o.MATERIAL)["albedo"], dtype=f32)[prims["material_ID"]]
    n = (w // 16) * (h // 16) * 256
    sums = np.zeros((7, n), dtype=f32)
    for a in range(1, n_acc + 1):
        p, d = lt.oracle_lens_rays(o, a, A, fd)
        tfar, prim = o.trace_closest(p, d, ob.TRAV_BRUTE)
        hit = prim >= 0
        k = np.flatnonzero(hit)
        O, D, t = p[:, k], d[:, k], tfar[k]
        H = O + D * t
        v = H - centre[prim[k]].T
        N = v * (f32(1.0) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))
        flip = ((N[0] * D[0] + N[1] * D[1]) + N[2] * D[2]) >= f32(0.0)
        N = np.where(flip, -N, N)
        sums[0, ~hit] += MISS_DEPTH
        sums[0, k] += t
        sums[1:4, k] += N
        sums[4:7, k] += colour[prim[k]].T
    o.close()
    return np.ascontiguousarray(sums.reshape(7, n // 256, 256).transpose(1, 0, 2))


@pytest.mark.parametrize("name,kw", [("default9", {}), ("S1000", {"use_bvh": True}), ("S1000", {"use_bvh": True, "max_batch": 3, "streams": 3})])
def test_lens_aovs_equal_the_twin(mirt, name, kw):
    make, mb, (A, fd) = SCENES[name]
    want = aov_twin(make(mirt), 64, 64, 7, mb, A, fd)
    r = mirt.Renderer(make(mirt), max_bounces=mb, aov=True, **kw); r.Resize(64, 64)
    r.set_lens(A, fd)
    r.Accumulate(7)
    assert_same(r.aov(), want, f"{name} {kw} AOV sums under a lens")
    r.close()


# ---- a closed aperture is the pinhole path -------------------------------------------------------------------------------------------------
def state_of(r, n):
    r.Accumulate(n)
    assert r.Render()
    return dict(acc=r.accumulator(), frame=r.GetFrame().copy(), counters=r.counters(), aov=r.aov())


def test_closed_aperture_is_the_pinhole_path(mirt):
    kw = dict(max_bounces=5, use_bvh=True, aov=True, max_batch=5)
    fresh = mirt.Renderer(s1000(mirt), **kw); fresh.Resize(64, 64)
    want = state_of(fresh, 10); fresh.close()
    r = mirt.Renderer(s1000(mirt), **kw); r.Resize(64, 64)
    r.set_lens(0.0, 123.0)
    got = state_of(r, 10)
    for k in ("acc", "frame", "aov"):
        assert_same(got[k], want[k], f"closed aperture: {k}")
    assert got["counters"] == want["counters"]
    # lens on -> accumulate -> lens off -> accumulate: the lists of this view, built before the lens or not at all, serve the pinhole batches again
    r.ResetAccumulator(); r.set_lens(0.15, 25.0); r.Accumulate(5)
    assert r.accumulations == 5
    r.set_lens(0.0, 25.0); r.ResetAccumulator()
    again = state_of(r, 10)
    for k in ("acc", "frame", "aov"):
        assert_same(again[k], want[k], f"lens on -> off: {k}")
    r.close()
    # ... and with the lens set BEFORE the first pinhole batch could build any list
    r = mirt.Renderer(s1000(mirt), **kw); r.Resize(64, 64)
    r.set_lens(0.15, 25.0); r.Accumulate(5); r.set_lens(0.0, 1.0); r.ResetAccumulator()
    again = state_of(r, 10)
    for k in ("acc", "frame", "aov"):
        assert_same(again[k], want[k], f"lens first, then off: {k}")
    r.close()


# ---- invariances with the lens on ------------------------------------------------------------------------------------------------------
LENS_A, LENS_FD, N_ACC = 0.15, 25.0, 13


def lens_renderer(mirt, sc=None, **kw):
    kw = {**dict(max_bounces=5, use_bvh=True), **kw}
    r = mirt.Renderer(sc if sc is not None else s1000(mirt), **kw); r.Resize(64, 64)
    r.set_lens(LENS_A, LENS_FD)
    return r


@pytest.fixture(scope="module")
def lens_reference(mirt):
    r = lens_renderer(mirt); r.Accumulate(N_ACC)
    out = dict(acc=r.accumulator(), counters=r.counters())
    r.close()
    return out


@pytest.mark.parametrize("kw", [dict(use_bvh=False), dict(gpu_build=True), dict(reference_tree=True), dict(trace_primary_rays=True), dict(trace_primary_rays=False),
                                dict(max_batch=1), dict(max_batch=5), dict(max_batch=0), dict(streams=1), dict(streams=3, max_batch=2), dict(aov=True)],
                         ids=lambda kw: ",".join(f"{k}={int(v)}" for k, v in kw.items()))
def test_lens_accumulator_does_not_depend_on(mirt, lens_reference, kw):
    """Brute force against the trees is the check that the traversal accepts off-centre origins."""
    r = lens_renderer(mirt, **kw); r.Accumulate(N_ACC)
    assert_same(r.accumulator(), lens_reference["acc"], str(kw))
    c = r.counters()
    for k in ("rays", "shadow_rays", "terminated", "dropped"):
        assert c[k] == lens_reference["counters"][k], (kw, k)
    assert r.get_policy()["trace_primary_rays"] == int(kw.get("trace_primary_rays", False))       # the caller's value, whatever route the rays take
    r.close()


def test_lens_accumulator_does_not_depend_on_async_calls_partition_or_group(mirt, lens_reference):
    r = lens_renderer(mirt)
    for _ in range(N_ACC):
        r.AccumulateAsync(1)
    assert_same(r.accumulator(), lens_reference["acc"], "13 x async(1)")
    r.close()
    parts = []
    for first in (0, 1):                                               # two contexts with interleaved tile rows
        r = lens_renderer(mirt); r.SetTileRows(first, 2); r.Accumulate(N_ACC)
        parts.append(r.accumulator()); r.close()
    whole = np.empty_like(lens_reference["acc"])
    for first in (0, 1):
        rows = np.arange(first, 4, 2)
        whole[(rows[:, None] * 4 + np.arange(4)[None, :]).reshape(-1)] = parts[first]
    assert_same(whole, lens_reference["acc"], "two contexts, interleaved tile rows")
    g = mirt.GroupRenderer(s1000(mirt), devices=(0, 0, 0), max_bounces=5, use_bvh=True); g.Resize(64, 64)
    g.set_lens(LENS_A, LENS_FD); g.Accumulate(N_ACC)
    assert g.lens() == (float(f32(LENS_A)), float(f32(LENS_FD)))
    assert_same(g.accumulator(), lens_reference["acc"], "three-member group")
    g.close()


def test_lens_ggx_with_decay_does_not_depend_on_traversal(mirt):
    decay = [0.0, 0.25, 0.5, 1.0]
    accs = []
    for kw in (dict(use_bvh=False), dict(use_bvh=True), dict(use_bvh=True, max_batch=3, streams=3)):
        r = mirt.Renderer(mirt.scene.brdf_test(), max_bounces=6, brdf=1, gloss_decay=decay, **kw); r.Resize(96, 64)
        r.set_lens(0.4, 28.0); r.Accumulate(10)
        accs.append(r.accumulator()); r.close()
    assert_same(accs[1], accs[0], "GGX under a lens: tree vs brute force")
    assert_same(accs[2], accs[0], "GGX under a lens: batches and streams")
    assert np.isfinite(accs[0]).all() and accs[0].max() > 0


# ---- the whole path under a lens is the oracle's ----------------------------------------------------------------------------------------------
GGX_DECAY = [0.0, 0.25, 0.5, 1.0]
LENS_PATHS = {   # scene, width, height, accumulations, max_bounces, lens, keywords shared with the oracle
    "S1000": (s1000, 64, 64, 10, 5, (0.15, 25.0), {}),
    "default9": (lambda m: m.scene.default9(), 96, 64, 5, 16, (0.03, 1.1), {}),
    "brdf_test_ggx": (lambda m: m.scene.brdf_test(), 96, 64, 5, 16, (0.4, 28.0), dict(brdf=1, gloss_decay=GGX_DECAY)),
}
LENS_ROUTES = (("tree", dict(use_bvh=True)), ("brute", dict(use_bvh=False)), ("tree built on the device", dict(use_bvh=True, gpu_build=True)))


@pytest.mark.parametrize("candidates", [0, 7])
@pytest.mark.parametrize("name", list(LENS_PATHS))
def test_whole_path_under_a_lens_is_the_oracle(mirt, name, candidates):
    """k_trace<*, LENS> / k_shade<FIRST, GGX, LENS> and, with seven candidates, k_shade<FIRST, GGX, LENS, false, RIS = true>: accumulator, frame and counters."""
    make, w, h, n, mb, lens, kw = LENS_PATHS[name]
    sc = make(mirt)
    want = rg.oracle_states(sc, (name, "lens", candidates), w, h, (n,), max_bounces=mb, lens=lens, light_ris=candidates, **kw)[n]
    pinhole = rg.oracle_states(sc, (name, "pinhole", candidates), w, h, (n,), max_bounces=mb, light_ris=candidates, **kw)[n]
    assert (bits(want["acc"]) != bits(pinhole["acc"])).any()
    for label, route in LENS_ROUTES:
        r = mirt.Renderer(sc, max_bounces=mb, buckets=5, light_ris=candidates, **route, **kw); r.Resize(w, h)
        r.set_lens(*lens); r.Accumulate(n)
        rg.check_against_oracle(r, want, f"{name} under a lens, M = {candidates}, {label}")
        r.close()


@pytest.mark.parametrize("candidates", [0, 7])
@pytest.mark.parametrize("name", list(LENS_PATHS))
def test_sparse_lens_kernels_are_the_oracle(mirt, name, candidates):
    """k_trace<*, kPrimaryActive, LENS = true> and k_shade<true, GGX, LENS = true, SPARSE = true, RIS>: 5 accumulations, every third tile frozen, 5 more."""
    make, w, h, _, mb, lens, kw = LENS_PATHS[name]
    rg.check_frozen_against_oracle(mirt, make(mirt), (name, "lens", candidates), w, h, LENS_ROUTES, max_bounces=mb, lens=lens, light_ris=candidates, **kw)


# ---- closed forms ----------------------------------------------------------------------------------------------------------------------
def test_white_furnace_under_a_lens_is_exactly_one(mirt):
    for kw in (dict(use_bvh=False), dict(use_bvh=True)):
        r = mirt.Renderer(mirt.scene.white_furnace(), **kw); r.Resize(32, 32)
        r.set_lens(0.2, 2.0); r.Accumulate(5)
        acc = r.accumulator()
        assert (bits(acc) == bits(f32(1.0))).all(), kw
        o = ob.Oracle(mirt.scene.white_furnace(), lens=(0.2, 2.0)); o.Resize(32, 32); o.Accumulate(5)
        assert_same(acc, o.accumulator(), f"white furnace under a lens against the oracle, {kw}")
        assert r.Render(); assert_same(r.GetFrame(), o.Render(), f"white furnace under a lens, frame, {kw}")
        assert r.counters()["rays"] == o.counters()["rays"] and r.counters()["terminated"] == o.counters()["terminated"]
        o.close(); r.close()


class LensBackend:
    """tests/test_definitions_gpu.py's render(), with a lens."""
    name = "gpu+lens"

    def __init__(self, mirt):
        self.mirt = mirt

    def render(self, sc, w, h, n_acc, max_bounces, buckets=5, mis=True, variant=0):
        r = self.mirt.Renderer(sc, max_bounces=max_bounces, buckets=buckets, mis=mis, use_bvh=bool(variant)); r.Resize(w, h)
        r.set_lens(0.03, 0.3)                                           # eye at 1.25 from the unit sphere's centre: focused just behind its near pole
        r.Accumulate(n_acc)
        out = dict(acc=r.accumulator(), frame=None, counters=r.counters())
        r.close()
        return out


@pytest.mark.parametrize("w,h,n_acc,variant", [(64, 64, 50, 0), (256, 256, 20, 1)])
def test_filling_sphere_under_a_lens(mirt, w, h, n_acc, variant):
    """The filling-sphere rows of DESIGN.md §2 (E): a lens moves the camera rays, not the closed form — every ray still hits the sphere that
    fills the frame.  Same expectations, same 5 sigma."""
    cpu.check_filling_sphere(LensBackend(mirt), mirt, w, h, n_acc, variant=variant)


# ---- circle of confusion ----------------------------------------------------------------------------------------------------------------
COC = dict(w=64, h=64, focal=50.0, r=0.05, d=2.0, A=0.09, f=1.0, n_acc=128, E=4.0)


def coc_scene(mirt):
    S = mirt.scene
    cam = S.Camera(eye=(0.0, 0.0, 0.0), direction=(0.0, 0.0, -1.0), focal_length=COC["focal"], exposure=1.0)
    return S.Scene(np.array([S._sphere((0.0, 0.0, -COC["d"]), COC["r"] ** 2, 0)], dtype=S.SPHERE),
                   np.array([S._material(albedo=(0, 0, 0), emission=(COC["E"],) * 3)], dtype=S.MATERIAL), cam, np.zeros(3, dtype=f32), name="coc")


def coc_render(mirt, A, f, use_bvh=True):
    """-> hits per pixel (h, w): the bucket sums / E (each sample is exactly E or 0, so the sums are exact small multiples of E)."""
    r = mirt.Renderer(coc_scene(mirt), max_bounces=2, use_bvh=use_bvh); r.Resize(COC["w"], COC["h"])
    if A is not None:
        r.set_lens(A, f)
    r.Accumulate(COC["n_acc"])
    acc = r.accumulator().astype(f64)
    r.close()
    per_tile = acc.sum(axis=1)[:, 0, :] / COC["E"]                     # [tile][256], red
    assert np.array_equal(per_tile, np.rint(per_tile))
    img = np.zeros((COC["h"], COC["w"]))
    for t in range(per_tile.shape[0]):
        img[16 * (t // 4):16 * (t // 4) + 16, 16 * (t % 4):16 * (t % 4) + 16] = per_tile[t].reshape(16, 16)
    return img


def footprint_radius(img):
    y, x = np.nonzero(img)
    return float(np.hypot(x + 0.5 - COC["w"] / 2, y + 0.5 - COC["h"] / 2).max())


def test_circle_of_confusion(mirt):
    """One emissive sphere (radius r, albedo 0) on the axis at depth d, ambient 0.  max_bounces = 2, not 1: with one bounce every hit is the
    path's last and is dropped (Q5), and the image is black; with two, a hit adds E (bounce 0: no throughput, Q9), the albedo-0 throughput ends
    the path in the roulette, the one light is the hit sphere itself (no NEE): each sample is exactly E or 0.
    Geometry, camera at the origin, |z| = pixels per unit tangent: a lens point a (|a| <= A) and a pixel offset q (in pixels) give the focus-plane
    point q f / |z|; at depth d that ray stands at a (1 - d / f) + q d / |z| from the axis and hits when this is within the silhouette radius.
    The lit footprint therefore reaches |z| (A |1/f - 1/d| + r / d).  Finite depth of the sphere: (i) the silhouette is the tangent cone,
    tan = r / sqrt(d^2 - r^2) instead of r / d; (ii) the tangent points lie at depths within d +- r, where the blur A |1/f - 1/(d +- r)| differs from
    the one at d by at most A r / (d (d - r)).  Allowed: +- (1 px + |z| (r / sqrt(d^2 - r^2) - r / d + A r / (d (d - r)))).
    Sum: every sample is a Bernoulli draw worth E; E[N] = n_acc x silhouette area in px^2 for the pinhole, and the same for the lens up to the
    factor by which the shadow of the sphere thrown from an off-axis lens point onto the plane of focus grows: a cone of half-angle alpha about
    an axis tilted by phi, tan(phi) = a / d, cuts the plane in an ellipse of area pi f^2 tan^2(alpha) / cos^3(phi), and tan(alpha) = (r / d) cos(phi):
    relative growth 1 / cos(phi) - 1 <= (A / d)^2 / 2 = 0.1 %.  Var[N] = sum p (1 - p) <= E[N] for either run, so sigma <= sqrt(2 E[N]) for the
    difference: E[N] = 128 pi 3.33^2 = 4470, sigma <= 94.6, the geometric term 4.5 = 0.05 sigma (checked with the twin and the oracle's brute-force
    traversal on the CPU before the sizes were fixed: 4478 hits pinhole, 4432 defocused, 4479 focused; footprint 9.62 px against 9.33 + 0.16)."""
    c = COC
    z = (c["h"] / 2) * (2.0 / 24.0) * c["focal"]
    pin = coc_render(mirt, None, None)
    blur = coc_render(mirt, c["A"], c["f"])
    sharp = coc_render(mirt, c["A"], c["d"])
    want = z * (c["A"] * abs(1 / c["f"] - 1 / c["d"]) + c["r"] / c["d"])
    fin = z * (c["r"] / math.sqrt(c["d"] ** 2 - c["r"] ** 2) - c["r"] / c["d"] + c["A"] * c["r"] / (c["d"] * (c["d"] - c["r"])))
    got = footprint_radius(blur)
    print(f"lens/coc: footprint {got:.2f} px, closed form {want:.2f} px, finite-depth term {fin:.3f} px; pinhole {footprint_radius(pin):.2f}, focused {footprint_radius(sharp):.2f}")
    assert abs(got - want) <= 1.0 + fin
    assert footprint_radius(sharp) <= footprint_radius(pin) + 1.0
    expect = c["n_acc"] * math.pi * (z * c["r"] / math.sqrt(c["d"] ** 2 - c["r"] ** 2)) ** 2
    sigma = math.sqrt(2 * expect)
    geometric = 0.5 * (c["A"] / c["d"]) ** 2 * expect
    assert geometric < sigma
    print(f"lens/coc: hits pinhole {pin.sum():.0f}, defocused {blur.sum():.0f}, focused {sharp.sum():.0f}; E[N] {expect:.0f}, 5 sigma {5 * sigma:.0f}, geometric {geometric:.1f}")
    for label, img in (("defocused", blur), ("focused", sharp)):
        assert abs(img.sum() - pin.sum()) <= 5 * sigma + geometric, label
    assert_same(coc_render(mirt, c["A"], c["f"], use_bvh=False), blur, "circle of confusion: brute force vs tree")


# ---- pick --------------------------------------------------------------------------------------------------------------------------------
def test_pick_focus(mirt):
    sc = mirt.scene.default9()
    for kw in (dict(use_bvh=False), dict(use_bvh=True)):
        r = mirt.Renderer(sc, **kw); r.Resize(64, 64)
        cam = sc.camera
        _, _, fwd = lt.camera_axes(cam)
        geo = np.asarray(sc.geometry)
        centre, r2 = geo["position"].astype(f64), geo["radius_sq"].astype(f64)
        seen_hit = seen_sky = False
        for (x, y) in ((32, 32), (0, 0), (63, 63), (20, 40), (45, 10), (32, 50), (10, 32)):
            d = lt.pinhole_dir(cam, [x], [y])
            p = np.asarray(cam.pos, dtype=f32).reshape(3, 1)
            tfar, prim = r.debug_trace_closest(p, d)
            dist, depth = r.pick_focus(x, y)
            if prim[0] < 0:
                assert dist == math.inf and depth == math.inf; seen_sky = True
                continue
            seen_hit = True
            cos = f32(lt.dot3([d[0, 0], d[1, 0], d[2, 0]], fwd))
            assert bits(f32(dist)) == bits(tfar[0]), (x, y)
            assert bits(f32(depth)) == bits(f32(tfar[0] * min(cos, f32(1.0)))), (x, y)
            assert depth <= dist
            P, D = p.T.astype(f64), d.T.astype(f64)
            b, oc2, disc = df.sphere_roots(P, D, centre, r2)
            t_all = np.where(disc >= 0, b - np.sqrt(np.maximum(disc, 0)), np.inf); t_all = np.where(t_all < 0, b + np.sqrt(np.maximum(disc, 0)), t_all)
            t_all = np.where((disc >= 0) & (t_all >= 0), t_all, np.inf)
            k = int(np.argmin(t_all[0]))
            E = df.sphere_error_model(P, D, centre, r2, b, oc2, disc)[2][0, k] + df.u * abs(t_all[0, k])
            assert abs(dist - t_all[0, k]) <= E, (x, y, dist, t_all[0, k], E)
            r.set_lens(0.05, 2.0)                                          # the pick is a pinhole ray, lens or no lens, and changes no state
            assert r.pick_focus(x, y) == (dist, depth) and r.lens() == (float(f32(0.05)), 2.0)
            r.set_lens(0.0, 1.0)
        assert seen_hit
        # a pixel outside this context's tiles, and one outside the image
        before = r.pick_focus(40, 40)
        r.SetTileRange(0, 1)
        assert r.pick_focus(40, 40) == before
        a, b_ = C.c_float(0), C.c_float(0)
        assert r._lib.mirt_pick_focus(r._ctx, 64, 0, C.byref(a), C.byref(b_)) == MIRT_ERR_ARG
        assert r._lib.mirt_pick_focus(r._ctx, 0, 64, C.byref(a), C.byref(b_)) == MIRT_ERR_ARG
        r.close()
    r = mirt.Renderer(coc_scene(mirt), max_bounces=2, use_bvh=True); r.Resize(64, 64)
    assert r.pick_focus(2, 2) == (math.inf, math.inf)                    # sky
    dist, depth = r.pick_focus(32, 32)
    assert abs(dist - (COC["d"] - COC["r"])) < 5e-3 and depth <= dist          # half a pixel off the axis: the front pole + a sag of 1.1e-3
    g = mirt.GroupRenderer(coc_scene(mirt), devices=(0, 0), max_bounces=2); g.Resize(64, 64)
    assert g.pick_focus(32, 32) == (dist, depth)
    g.close(); r.close()


def test_picked_depth_focuses_the_sphere(mirt):
    """After set_lens(A, depth of the pick) the circle-of-confusion sphere at that pixel is sharp: no wider than the pinhole image + 1 px (its front
    pole is in focus; the silhouette, r behind it, blurs by |z| A r / (d (d - r)) = 0.08 px)."""
    r = mirt.Renderer(coc_scene(mirt), max_bounces=2, use_bvh=True); r.Resize(64, 64)
    _, depth = r.pick_focus(32, 32)
    r.close()
    assert footprint_radius(coc_render(mirt, COC["A"], depth)) <= footprint_radius(coc_render(mirt, None, None)) + 1.0


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_lens_refusals(mirt):
    r = mirt.Renderer(mirt.scene.default9()); r.Resize(32, 32)
    lib, ctx = r._lib, r._ctx
    for a, d in ((-0.1, 1.0), (0.1, 0.0), (0.1, -2.0), (math.nan, 1.0), (0.1, math.nan), (math.inf, 1.0), (0.1, math.inf), (0.0, math.inf)):
        assert lib.mirt_set_lens(ctx, a, d) == MIRT_ERR_ARG, (a, d)
    assert r.lens() == (0.0, 0.0)
    assert lib.mirt_set_lens(ctx, 0.0, 0.0) == 0 and lib.mirt_set_lens(ctx, 0.0, -3.0) == 0       # a closed aperture asks nothing of the depth
    r.set_stream_order(True)
    assert lib.mirt_set_lens(ctx, 0.1, 1.0) == MIRT_ERR_STATE and b"no lens" in lib.mirt_last_error(ctx)
    assert lib.mirt_set_lens(ctx, 0.0, 1.0) == 0
    r.set_stream_order(False)
    r.set_lens(0.1, 1.0)
    assert lib.mirt_set_stream_order(ctx, 1) == MIRT_ERR_STATE and b"no lens" in lib.mirt_last_error(ctx)
    assert r.stream_order == 0
    r.set_lens(0.0, 1.0)
    assert lib.mirt_set_stream_order(ctx, 1) == 0
    r.close()
    # set_lens launches deferred async calls first, under the old lens, and does not reset
    a = mirt.Renderer(mirt.scene.default9(), max_batch=8); a.Resize(32, 32)
    a.AccumulateAsync(3); a.set_lens(0.05, 1.2); a.AccumulateAsync(2)
    b = mirt.Renderer(mirt.scene.default9(), max_batch=8); b.Resize(32, 32)
    b.Accumulate(3); b.set_lens(0.05, 1.2); b.Accumulate(2)
    assert a.accumulations == 5
    assert_same(a.accumulator(), b.accumulator(), "deferred calls render under the lens they were issued under")
    a.close(); b.close()
    r = mirt.Renderer(mirt.scene.default9(), lens=True); r.Resize(32, 32)
    cam = r.scene.camera
    assert r.lens() == (float(cam.aperture_radius), float(f32(cam.focus_distance)))
    r.close()
