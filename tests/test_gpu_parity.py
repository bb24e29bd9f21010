"""GPU parity tests (-m gpu): every check calls the HIP path through the C-ABI (libmirt.so) and compares with the
CPU oracle on the same seeded inputs — bit-exact for the integer/bit work AND for the f32 radiance (the kernels
reproduce the reference's IEEE operation sequence), which is far inside north_star's 1e-4 relative tolerance.
Full-size checks use size-independent properties (BVH == brute force, shard == whole, batch == sequential)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_binding as ob
from oracle_binding import bits, fnv1a
from test_oracle_cpu import CASES, GOLDEN, make_scene

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4          # north_star tolerance; the assertions below are bit-exact and only fall back to this in messages


def assert_same(got, want, what):
    got = np.ascontiguousarray(got, dtype=np.float32); want = np.ascontiguousarray(want, dtype=np.float32)
    if np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        return
    diff = np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1e-30)
    bad = (got.view(np.uint32) != want.view(np.uint32)).sum()
    raise AssertionError(f"{what}: {bad} of {got.size} words differ; max rel err {diff.max():.3e} (tolerance {REL_TOL})")


@pytest.fixture(scope="module")
def gpu(mirt):
    r = mirt.Renderer(mirt.scene.default9(), device=0)
    yield r
    r.close()


# ---- device math vs the oracle's unit functions ----------------------------------------------------------------
def test_device_math_bit_exact(mirt, gpu, oracle_lib):
    lib = oracle_lib
    rng = np.random.default_rng(7)
    n = 20000
    # fast_sincos
    x = np.concatenate([rng.uniform(0, 6.2832, n - 6), [0.0, 6.2831855, 3.1415927, 1e-38, -0.0, 100.0]]).astype(np.float32)
    out = gpu.debug_math(0, x[None, :], 2)
    s, c = C.c_float(), C.c_float()
    for i in range(0, n, 1):
        lib.orc_fast_sincos(float(x[i]), C.byref(s), C.byref(c))
        assert np.float32(s.value).view(np.uint32) == out[0, i].view(np.uint32) and np.float32(c.value).view(np.uint32) == out[1, i].view(np.uint32), x[i]
    # atan2 / asin
    y = rng.uniform(-2, 2, n).astype(np.float32); xx = rng.uniform(-2, 2, n).astype(np.float32)
    y[:4] = [0.0, -0.0, 1.0, 0.0]; xx[:4] = [0.0, -1.0, 0.0, 1.0]
    out = gpu.debug_math(1, np.stack([y, xx]), 1)
    want = np.array([lib.orc_fast_atan2(float(a), float(b)) for a, b in zip(y, xx)], dtype=np.float32)
    assert_same(out[0], want, "fast_atan2")
    xa = np.concatenate([rng.uniform(-1, 1, n - 4), [1.0, -1.0, 0.0, 1.25]]).astype(np.float32)
    out = gpu.debug_math(2, xa[None, :], 1)
    want = np.array([lib.orc_fast_asin(float(a)) for a in xa], dtype=np.float32)
    assert_same(out[0], want, "fast_asin")
    # IEEE division / sqrt on the device (correctly rounded, denormals kept)
    a = np.concatenate([rng.uniform(-1e3, 1e3, n - 3), [1e-40, 3.0, 1e38]]).astype(np.float32)
    b = np.concatenate([rng.uniform(-1e3, 1e3, n - 3), [3.0, 1e-40, 1e-3]]).astype(np.float32)
    out = gpu.debug_math(3, np.stack([a, b]), 3)
    with np.errstate(all="ignore"):
        assert_same(out[0], np.float32(1.0) / a, "1/x")
        assert_same(out[1], np.sqrt(np.abs(a)), "sqrt")
        assert_same(out[2], a / b, "a/b")
    # the traversal's own sqrt (kernels.hpp sqrt_trav: hipcc's correctly rounded expansion minus its denormal scaling) is IEEE sqrt
    # wherever the sphere tests use it (inputs >= 0; every bit pattern: profiles/experiments/sqrt_check.hip)
    xs = np.concatenate([np.exp(rng.uniform(-80, 80, n)), rng.uniform(0, 4, n), (np.arange(1, 4097, dtype=np.float64) / 64.0) ** 2,
                         [0.0, 1e-45, 1e-40, 1.1754944e-38, 7e-31, 8e-31, 1.2e30, 1.3e30, 3.4e38, np.inf, 1.0, 4.0, 2.0]]).astype(np.float32)
    got = gpu.debug_math(10, xs[None, :], 1)
    assert_same(got[0], np.sqrt(xs), "sqrt_trav")
    # hemisphere, tangent frame, light sampling
    t = rng.uniform(0, 1, n).astype(np.float32); u = rng.uniform(0, 1, n).astype(np.float32)
    t[:2] = [1.0, 0.0]
    out = gpu.debug_math(4, np.stack([t, u]), 3)
    h = np.empty(3, dtype=np.float32)
    for i in range(0, n, 5):
        lib.orc_hemisphere(float(t[i]), float(u[i]), h.ctypes.data_as(C.c_void_p))
        assert np.array_equal(h.view(np.uint32), out[:, i].view(np.uint32))
    N = rng.normal(size=(3, n)).astype(np.float32); N /= np.linalg.norm(N, axis=0, keepdims=True).astype(np.float32)
    N[:, 0] = [0, 0, -1]; N[:, 1] = [0, 0, 1]
    v = rng.normal(size=(3, n)).astype(np.float32)
    out = gpu.debug_math(5, np.concatenate([N, v]), 10)
    q = np.empty(4, dtype=np.float32); l = np.empty(3, dtype=np.float32); w = np.empty(3, dtype=np.float32)
    for i in range(0, n, 5):
        nn = np.ascontiguousarray(N[:, i]); vv = np.ascontiguousarray(v[:, i])
        lib.orc_tangent_space(nn.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p))
        lib.orc_to_local(q.ctypes.data_as(C.c_void_p), vv.ctypes.data_as(C.c_void_p), l.ctypes.data_as(C.c_void_p))
        lib.orc_to_world(q.ctypes.data_as(C.c_void_p), vv.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p))
        assert np.array_equal(np.concatenate([q, l, w]).view(np.uint32), out[:, i].view(np.uint32)), i
    Wc = rng.normal(size=(3, n)).astype(np.float32); Wc /= np.linalg.norm(Wc, axis=0, keepdims=True).astype(np.float32)
    dist = rng.uniform(0.2, 50, n).astype(np.float32); r2 = (rng.uniform(0.01, 0.15, n).astype(np.float32) * dist) ** 2
    r2[: n // 4] = (np.float32(0.01) * dist[: n // 4]) ** 2                    # small-angle branch (sinThetaMax2 < 0.00068523)
    sin2 = r2 / (dist * dist)
    inp = np.concatenate([Wc, sin2[None], dist[None], r2[None], t[None], u[None]])
    out = gpu.debug_math(6, inp, 5)
    o5 = np.empty(5, dtype=np.float32)
    for i in range(0, n, 5):
        wc = np.ascontiguousarray(Wc[:, i])
        lib.orc_sample_direction_to_sphere(wc.ctypes.data_as(C.c_void_p), float(sin2[i]), float(dist[i]), float(r2[i]), float(t[i]), float(u[i]), o5.ctypes.data_as(C.c_void_p))
        assert np.array_equal(o5.view(np.uint32), out[:, i].view(np.uint32)), i
    # RNG
    xs = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32); ys = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    rg = rng.integers(1, 1000, n).astype(np.uint32)
    xs[:3] = [1, 1, 5]; ys[:3] = [0, 33, 8455]
    out = gpu.debug_math(7, np.stack([xs, ys, rg]).view(np.float32), 5).view(np.uint32)
    assert out[0, 0] == 0xEF386249 and out[0, 1] == 0x56410662 and out[0, 2] == 0xD9B98C80
    assert out[1:4, 0].view(np.float32).tolist() == [np.float32(0.1417161226272583), np.float32(0.9638892412185669), np.float32(0.3188127279281616)]
    for i in range(0, n, 11):
        st = C.c_uint32(lib.orc_hash_2d(int(xs[i]), int(ys[i])))
        assert st.value == out[0, i]
        f = [lib.orc_make_unit_float(lib.orc_pcg_generate(C.byref(st))) for _ in range(2)]
        st2 = C.c_uint32(st.value)
        f.append(lib.orc_make_unit_float(lib.orc_pcg_generate(C.byref(st))))
        assert np.array_equal(np.array(f, dtype=np.float32).view(np.uint32), out[1:4, i])
        assert lib.orc_rand_bounded_int(C.byref(st2), int(rg[i])) == out[4, i]


# ---- single kernels ------------------------------------------------------------------------------------------------
def test_ggx_closure_functions_bit_exact(mirt, gpu, oracle_lib):
    """SURVEY.md §8f rank 4, function level: Closure<GGX>::eval / ::sample (DataStreams.hpp:184-219) and everything under them
    (Sampling.hpp:254-309) on the device vs the oracle, bit for bit.  The reference's PATH with this closure does not build
    (`#define BRDF 0`; `gloss_decay_table` is declared nowhere; pdf() returns 0), so the closure is not wired into k_shade."""
    lib = oracle_lib
    rng = np.random.default_rng(21)
    n = 4000
    def unit_upper(k):
        v = rng.normal(size=(k, 3)); v[:, 2] = np.abs(v[:, 2]) + 1e-3
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    F0 = rng.uniform(0.02, 1.0, (n, 3)).astype(np.float32)
    alpha = (rng.uniform(0.0, 1.0, n) ** 2).astype(np.float32); alpha[:8] = [0.0, 1.0, 1e-4, 0.5, 0.0, 1e-3, 0.25, 0.04]
    L, V = unit_upper(n), unit_upper(n)
    V[:4] = [(0, 0, 1), (1e-3, 0, 1), (0.6, 0.0, 0.8), (0.0, 0.8, 0.6)]
    u = rng.uniform(0, 1, (n, 2)).astype(np.float32); u[:4] = [(0, 0), (1, 1), (0.5, 0.25), (0.999, 0.001)]
    inp = np.concatenate([F0.T, alpha[None, :], L.T, V.T]).astype(np.float32)
    got = gpu.debug_math(8, inp, 3)
    want = np.zeros((n, 3), dtype=np.float32)
    for i in range(n):
        lib.orc_ggx_eval(F0[i].ctypes.data_as(C.c_void_p), float(alpha[i]), L[i].ctypes.data_as(C.c_void_p), V[i].ctypes.data_as(C.c_void_p), want[i].ctypes.data_as(C.c_void_p))
    assert_same(got.T, want, "Closure<GGX>::eval")
    assert np.isfinite(want).all() and (want >= 0).all()
    inp = np.concatenate([F0.T, alpha[None, :], V.T, u.T]).astype(np.float32)
    got = gpu.debug_math(9, inp, 6)
    wd, we = np.zeros((n, 3), dtype=np.float32), np.zeros((n, 3), dtype=np.float32)
    for i in range(n):
        lib.orc_ggx_sample(F0[i].ctypes.data_as(C.c_void_p), float(alpha[i]), V[i].ctypes.data_as(C.c_void_p), float(u[i, 0]), float(u[i, 1]),
                           wd[i].ctypes.data_as(C.c_void_p), we[i].ctypes.data_as(C.c_void_p))
    assert_same(got[:3].T, wd, "Closure<GGX>::sample direction"); assert_same(got[3:].T, we, "Closure<GGX>::sample estimator")
    mirror = alpha == 0.0                                  # alpha 0: perfect mirror about the normal (DataStreams.hpp:203-209)
    assert np.array_equal(wd[mirror], V[mirror] * np.float32([-1, -1, 1]))


def test_raygen_bit_exact(mirt):
    sc = mirt.scene.default9()
    r = mirt.Renderer(sc, max_bounces=16); r.Resize(96, 64)
    o = ob.Oracle(sc, max_bounces=16); o.Resize(96, 64)
    for acc in (1, 2, 77):
        gp, gd = r.debug_raygen(acc)
        wp, wd = o.raygen(acc)
        assert_same(gp, wp, "ray origins"); assert_same(gd, wd, "ray directions")
    r.close()


@pytest.mark.parametrize("scene_name,n_rays", [("default9", 40000), ("S1000a", 60000), ("S8a", 20000)])
def test_trace_kernels_bit_exact(mirt, scene_name, n_rays):
    sc = make_scene(mirt, scene_name)
    o = ob.Oracle(sc); o.Resize(128, 128)
    cp, cd = o.raygen(1)
    rng = np.random.default_rng(3)
    # camera rays + incoherent rays from points near sphere surfaces (incl. inside, on the surface, far away)
    geo = sc.geometry
    pick = rng.integers(0, len(geo), n_rays)
    nrm = rng.normal(size=(n_rays, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    rad = np.sqrt(geo["radius_sq"][pick])[:, None] * rng.choice([0.5, 1.0, 1.0 + 1e-4, 1.5, 3.0], size=(n_rays, 1))
    p = (geo["position"][pick] + nrm * rad).astype(np.float32).T
    d = rng.normal(size=(n_rays, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32).T
    d[0, :5] = 0.0                                          # axis-parallel rays: 1/0 slabs
    # non-unit directions, as the reference's tangent frame produces near N.z = -1 (|D| up to 1.125 seen in cfg2): the sphere
    # tests become "fat"; slightly stretched rays take the cone slab test, strongly stretched ones the brute-force detour (k_trace_fat)
    q = n_rays // 4
    d[:, :q] *= rng.choice(np.array([0.9, 0.999, 1.00001, 1.00004, 1.0002, 1.002, 1.06, 1.125, 1.5], dtype=np.float32), size=q)[None, :]
    P = np.ascontiguousarray(np.concatenate([cp, p], axis=1)); D = np.ascontiguousarray(np.concatenate([cd, d], axis=1))
    wt, wi = o.trace_closest(P, D, ob.TRAV_BRUTE)
    tmax = np.where(wi >= 0, wt * rng.uniform(0.5, 1.5, wt.shape), 10.0).astype(np.float32)
    wo = o.trace_shadow(P, D, tmax, ob.TRAV_BRUTE)
    for use_bvh in (0, 1):
        r = mirt.Renderer(sc, use_bvh=bool(use_bvh))
        gt, gi = r.debug_trace_closest(P, D)
        assert np.array_equal(gi, wi), f"primID mismatch use_bvh={use_bvh}: {(gi != wi).sum()}"
        assert_same(gt, wt, f"tfar use_bvh={use_bvh}")
        go = r.debug_trace_shadow(P, D, tmax)
        assert np.array_equal(go, wo), f"occlusion mismatch use_bvh={use_bvh}: {(go != wo).sum()}"
        r.close()
    assert (wi >= 0).mean() > 0.2


# ---- the whole path against the golden vectors and the live oracle -----------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("use_bvh", [False, True])
def test_accumulate_matches_golden(mirt, name, use_bvh):
    cfg = CASES[name]
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    r = mirt.Renderer(make_scene(mirt, cfg["scene"]), max_bounces=cfg["mb"], buckets=cfg.get("buckets", 5), mis=cfg.get("mis", True), use_bvh=use_bvh)
    r.Resize(cfg["w"], cfg["h"])
    r.Accumulate(cfg["spp"])
    assert r.accumulations == cfg["spp"]
    assert_same(r.accumulator(), g["accumulator"], f"{name} accumulator")
    ready = r.Render()
    if g["frame"].size:
        assert ready
        assert_same(r.GetFrame(), g["frame"], f"{name} frame")
    else:
        assert not ready and not r.GetFrame().any()          # Renderer.hpp:437: no output until accumulations % 5 == 0
    c = r.counters()
    assert c["rays"] == int(g["rays"]) and c["terminated"] == int(g["terminated"])
    assert c["terminated"] + c["dropped"] == cfg["spp"] * (cfg["w"] // 16) * (cfg["h"] // 16) * 256
    r.close()


@pytest.mark.parametrize("scene_name,w,h,spp,mb", [("default9", 160, 96, 15, 16), ("S1000a", 256, 128, 10, 5), ("S8a", 512, 512, 1, 2)])
def test_accumulate_matches_live_oracle(mirt, scene_name, w, h, spp, mb):
    sc = make_scene(mirt, scene_name)
    o = ob.Oracle(sc, max_bounces=mb, trav_mode=ob.TRAV_BRUTE); o.Resize(w, h); o.Accumulate(spp)
    r = mirt.Renderer(sc, max_bounces=mb, use_bvh=(scene_name != "S8a"), count_traffic=True, trace_primary_rays=True); r.Resize(w, h); r.Accumulate(spp)
    assert_same(r.accumulator(), o.accumulator(), "accumulator")
    if spp % 5 == 0:
        assert r.Render(); assert_same(r.GetFrame(), o.Render(), "frame")
    co, cg = o.counters(), r.counters()
    assert cg["rays"] == co["rays"] and cg["terminated"] == co["terminated"]
    if scene_name != "S8a":
        # same traversal algorithm as the oracle's mode 2 -> same visit counts (feeds the roofline's algorithmic bytes)
        t = ob.Oracle(sc, max_bounces=mb, trav_mode=ob.TRAV_PER_RAY_BVH); t.match_product(r); t.Resize(w, h); t.Accumulate(spp)
        ct = t.counters()
        assert cg["nodes"] == ct["nodes"] and cg["spheres"] == ct["spheres"]
        assert cg["shadow_rays"] == ct["shadow_rays"] and cg["shadow_nodes"] == ct["shadow_nodes"] and cg["shadow_spheres"] == ct["shadow_spheres"]
    r.close()


@pytest.mark.parametrize("allow_half", [True, False])
@pytest.mark.parametrize("reference_tree", [False, True])
def test_tree_and_record_variants_agree(mirt, allow_half, reference_tree):
    """The GPU-internal BVH is only a conservative culling structure: binary16 (32-B) or f32 (64-B) records, the internal
    SAH tree or the caller's reference tree — all must give the brute-force accumulators, and visit exactly the boxes and
    spheres the oracle's twin visits for the same variant."""
    sc = mirt.scene.synthetic(1000, ambient=0.5)
    o = ob.Oracle(sc, max_bounces=5, trav_mode=ob.TRAV_BRUTE); o.Resize(128, 128); o.Accumulate(5)
    r = mirt.Renderer(sc, max_bounces=5, use_bvh=True, allow_half_boxes=allow_half, reference_tree=reference_tree, count_traffic=True, trace_primary_rays=True)
    r.Resize(128, 128); r.Accumulate(5)
    info = r.debug_info()
    assert info["half_boxes"] == int(allow_half) and info["wide"] == int(allow_half) and info["lds_records"] == info["records"]
    assert info["lds_spheres"] == (1000 if info["records"] * (64 if info["wide"] or not allow_half else 32) + 16000 <= (48 if allow_half else 96) * 1024 else 0)    # records AND spheres staged when both fit
    assert info["records"] == 999 if not allow_half else 333 <= info["records"] < 999       # binary16 records hold up to four children: a node and its inner children
    assert info["trace_workgroups_per_cu"] == (2 if allow_half else 1)
    assert_same(r.accumulator(), o.accumulator(), f"accumulator (half={allow_half}, reference_tree={reference_tree})")
    t = ob.Oracle(sc, max_bounces=5, trav_mode=ob.TRAV_PER_RAY_BVH); t.match_product(r); t.Resize(128, 128); t.Accumulate(5)
    cg, ct = r.counters(), t.counters()
    assert cg["nodes"] == ct["nodes"] and cg["spheres"] == ct["spheres"]
    assert cg["shadow_nodes"] == ct["shadow_nodes"] and cg["shadow_spheres"] == ct["shadow_spheres"]
    if not reference_tree:
        ref = mirt.Renderer(sc, max_bounces=5, use_bvh=True, reference_tree=True, count_traffic=True, trace_primary_rays=True); ref.Resize(128, 128); ref.Accumulate(5)
        assert cg["nodes"] < 0.6 * ref.counters()["nodes"]          # the internal SAH tree roughly halves the box tests
        ref.close()
    r.close()


def test_deep_stack_and_wide_references(mirt):
    """Two corners of the traversal stack (kernels.hpp stack_put / stack_get): (1) a caller's chain-shaped tree over spheres lined up
    behind each other, ordered so that every camera ray enters the nearer inner child and stacks the farther LEAF at every level —
    47 entries deep, far past the 12-16 entries kept in LDS, through the scratch spill; (2) a scene of 40 000 spheres, where record
    and prim indices no longer fit the 15 + 1 bits of the u16 stack entries and the u32 stack is used with binary16 records."""
    n = 48
    sc = mirt.scene.synthetic(n, ambient=0.5)
    sc.geometry["position"] = np.stack([np.zeros(n), np.zeros(n), -3.0 * np.arange(n)], axis=1).astype(np.float32)
    sc.geometry["radius_sq"] = np.float32(1.0)
    sc.camera = mirt.scene.Camera(eye=(0.0, 0.0, 12.0), direction=(0.0, 0.0, -1.0), focal_length=200.0, exposure=1.0)
    o = ob.Oracle(sc, max_bounces=5, trav_mode=ob.TRAV_BRUTE); o.Resize(64, 48); o.Accumulate(5)
    for primary in (True, False):
        r = mirt.Renderer(sc, max_bounces=5, use_bvh=True, reference_tree=True, count_traffic=True, trace_primary_rays=primary)
        slot_z = r.prims["position"][:, 2]
        order = np.argsort(slot_z)                                   # farthest slot first: leaf k of the chain is the farthest sphere left
        chain = np.zeros(2 * n - 1, dtype=mirt.scene.NODE)
        chain["min_bound"] = [-1.0, -1.0, slot_z.min() - 1.0]; chain["max_bound"] = [1.0, 1.0, slot_z.max() + 1.0]      # (the product derives its own boxes)
        for k in range(n - 1):                                       # inner node 2k -> children 2k+1 (leaf) and 2k+2 (the rest: inner, or the last leaf)
            chain["first_id"][2 * k] = 2 * k + 1; chain["prim_count"][2 * k] = 0
            chain["first_id"][2 * k + 1] = order[k]; chain["prim_count"][2 * k + 1] = 1
        chain["first_id"][2 * n - 2] = order[n - 1]; chain["prim_count"][2 * n - 2] = 1
        r.UpdateScene(nodes=chain)
        assert r.debug_info()["depth"] >= n and r.debug_info()["wide"] == 0          # too deep for the 4-wide records (three stack entries per level): child-pair records
        r.Resize(64, 48); r.Accumulate(5)
        assert_same(r.accumulator(), o.accumulator(), f"chain tree, stack {n - 1} deep (trace_primary_rays={primary})")
        c = r.counters()
        assert c["rays"] == o.counters()["rays"] and c["nodes"] > 2 * (n - 1) * 64 * 48      # the camera rays alone walk the whole chain
        r.close()
    big = mirt.scene.synthetic(40000)
    r = mirt.Renderer(big, max_bounces=4, use_bvh=True, count_traffic=True, trace_primary_rays=True); r.Resize(64, 48); r.Accumulate(5)
    info = r.debug_info()
    assert info["half_boxes"] == 1 and info["wide"] == 1 and info["records"] < 39999 and info["lds_records"] == 512          # 32 KB of staged 64-B records: the u32-stack plan
    t = ob.Oracle(big, max_bounces=4, trav_mode=ob.TRAV_PER_RAY_BVH); t.match_product(r); t.Resize(64, 48); t.Accumulate(5)
    assert_same(r.accumulator(), t.accumulator(), "S(40000) vs the twin")
    cg, ct = r.counters(), t.counters()
    for k in ("rays", "nodes", "spheres", "shadow_rays", "shadow_nodes", "shadow_spheres"):
        assert cg[k] == ct[k], k
    r.close()


@pytest.mark.parametrize("scene_name,allow_half,w,h,spp,mb", [("default9", True, 64, 64, 5, 16), ("S8a", True, 64, 64, 5, 5), ("S1000a", True, 128, 128, 5, 5),
                                                             ("S1000a", False, 128, 128, 5, 5), ("S20000", True, 256, 128, 5, 6)])
def test_gpu_built_tree_gives_the_same_results(mirt, scene_name, allow_half, w, h, spp, mb):
    """policy.gpu_build: the traversal tree is built on the GPU (Morton-order LBVH, lbvh_build.hip) instead of the host SAH
    sweep.  A different tree must not change a single bit of the result (DESIGN.md "Traversal semantics"); it only costs
    more box tests per ray."""
    sc = mirt.scene.synthetic(20000) if scene_name == "S20000" else make_scene(mirt, scene_name)
    a = mirt.Renderer(sc, max_bounces=mb, use_bvh=True, allow_half_boxes=allow_half, count_traffic=True); a.Resize(w, h); a.Accumulate(spp)
    g = mirt.Renderer(sc, max_bounces=mb, use_bvh=True, allow_half_boxes=allow_half, count_traffic=True, gpu_build=True); g.Resize(w, h); g.Accumulate(spp)
    n = len(sc.geometry)
    ia, ig = a.debug_info(), g.debug_info()
    assert ig["half_boxes"] == ia["half_boxes"] and ig["depth"] <= 64 and ig["wide"] == ia["wide"] == int(allow_half and n >= 2)
    for info in (ig, ia):                                    # binary16 records are 4-wide (a node and its inner children), from either builder
        assert info["records"] == n - 1 if not info["wide"] else (n - 1) // 3 <= info["records"] < max(n - 1, 2)
    assert_same(g.accumulator(), a.accumulator(), f"{scene_name}: GPU-built tree vs host SAH tree")
    ca, cg = a.counters(), g.counters()
    assert cg["rays"] == ca["rays"] and cg["shadow_rays"] == ca["shadow_rays"] and cg["terminated"] == ca["terminated"]
    assert cg["nodes"] < 4 * ca["nodes"]                         # an LBVH costs more box tests, not an order of magnitude more
    if scene_name in ("default9", "S1000a"):
        o = ob.Oracle(sc, max_bounces=mb, trav_mode=ob.TRAV_BRUTE); o.Resize(w, h); o.Accumulate(spp)
        assert_same(g.accumulator(), o.accumulator(), f"{scene_name}: GPU-built tree vs brute-force oracle")
    # an edit: same context, scene handed over again -> rebuilt on the GPU
    sc.geometry["position"][1, 1] += 0.25
    for r in (a, g):
        r.UpdateScene(); r.ResetAccumulator(); r.Accumulate(spp)
    assert_same(g.accumulator(), a.accumulator(), f"{scene_name}: after an edit")
    a.close(); g.close()


def test_caller_tree_with_multi_prim_leaves(mirt):
    """policy.reference_tree walks whatever Node[] the caller hands over.  The reference's builder only makes one-prim leaves
    (BVH.hpp:201-205), but its traversal loops over prim_count (BVH.hpp:343-345): a hand-made tree with up to 5 prims per
    leaf (median splits of the BVH-order range) must give the brute-force result, with binary16 and f32 records."""
    sc = mirt.scene.synthetic(300, ambient=0.5)
    o = ob.Oracle(sc, max_bounces=5, trav_mode=ob.TRAV_BRUTE); o.Resize(96, 96); o.Accumulate(5)
    for allow_half in (True, False):
        r = mirt.Renderer(sc, max_bounces=5, use_bvh=True, reference_tree=True, allow_half_boxes=allow_half, count_traffic=True)
        prims = r.prims
        rad = np.sqrt(prims["radius_sq"])[:, None]
        lo, hi = prims["position"] - rad, prims["position"] + rad
        nodes = []
        def build(a, b):                                    # returns the index of the node covering prims [a, b)
            i = len(nodes); nodes.append(None)
            fill(i, a, b)
            return i
        def fill(i, a, b):
            if b - a <= 5:
                nodes[i] = (lo[a:b].min(0), a, hi[a:b].max(0), b - a)
                return
            m = (a + b) // 2
            k = len(nodes); nodes.append(None); nodes.append(None)     # children adjacent: first_id, first_id + 1
            nodes[i] = (lo[a:b].min(0), k, hi[a:b].max(0), 0)
            fill(k, a, m); fill(k + 1, m, b)
        build(0, len(prims))
        arr = np.zeros(len(nodes), dtype=mirt.scene.NODE)
        for i, (mn, first, mx, cnt) in enumerate(nodes):
            arr[i] = (mn, first, mx, cnt)
        assert (arr["prim_count"] > 1).any() and arr["prim_count"].max() == 5
        r.UpdateScene(nodes=arr)
        r.Resize(96, 96); r.Accumulate(5)
        assert r.debug_info()["half_boxes"] == int(allow_half)
        assert_same(r.accumulator(), o.accumulator(), f"multi-prim leaves, half={allow_half}")
        assert r.debug_info()["records"] == len(prims) - 1 if not allow_half else r.debug_info()["records"] < len(prims) - 1   # every k-prim leaf became a subtree of k one-prim leaves (bvh_layout.hpp); binary16 records are 4-wide
        r.close()


def _awkward_scene(mirt, seed, n):
    """Spheres chosen to stress the tree builders and the tie rule: exact duplicates, concentric shells, a sphere around the
    camera, tiny and huge radii side by side, many centres on one plane / one line (equal Morton codes, zero-extent axes)."""
    S = mirt.scene
    rng = np.random.default_rng(seed)
    geo = np.zeros(n, dtype=S.SPHERE)
    geo["position"] = rng.uniform(-6, 6, (n, 3)).astype(np.float32)
    geo["radius_sq"] = (rng.uniform(0.05, 1.2, n) ** 2).astype(np.float32)
    if n >= 8:
        geo["position"][1] = geo["position"][0]; geo["radius_sq"][1] = geo["radius_sq"][0]          # exact duplicate: equal distances, prim index decides
        geo["position"][2] = geo["position"][0]; geo["radius_sq"][2] = geo["radius_sq"][0] * 4       # concentric shell
        geo["position"][3] = (0.0, 1.0, 14.0); geo["radius_sq"][3] = 4.0                              # contains the camera
        geo["radius_sq"][4] = 1e-6; geo["radius_sq"][5] = 400.0                                      # tiny / huge
    if seed % 2:
        geo["position"][n // 2:, 1] = 0.5                                                            # half the centres on one plane
    if seed % 3 == 0:
        geo["position"][n // 2:, 0] = 1.0; geo["position"][n // 2:, 1] = 0.5                         # ... on one line
    mats = np.zeros(4, dtype=S.MATERIAL)
    mats["albedo"][:3] = [(0.8, 0.3, 0.3), (0.3, 0.8, 0.3), (0.6, 0.6, 0.9)]
    mats["albedo"][3] = 1.0; mats["emission"][3] = 15.0
    geo["material_ID"] = rng.integers(0, 3, n)
    geo["material_ID"][rng.integers(0, n, max(1, n // 16))] = 3
    cam = S.Camera(eye=(0.0, 1.0, 14.0), direction=(0.0, -0.05, -1.0), focal_length=35.0, exposure=1.0)
    return S.Scene(geo, mats, cam, np.full(3, 0.3, dtype=np.float32), name=f"awkward{seed}")


@pytest.mark.parametrize("seed,n", [(1, 2), (2, 3), (3, 17), (4, 64), (5, 257), (6, 1500)])
def test_awkward_scenes_all_tree_builders_equal_brute_force(mirt, seed, n):
    sc = _awkward_scene(mirt, seed, n)
    o = ob.Oracle(sc, max_bounces=6, trav_mode=ob.TRAV_BRUTE); o.Resize(96, 64); o.Accumulate(5)
    want = o.accumulator()
    for kw in (dict(use_bvh=False), dict(use_bvh=True), dict(use_bvh=True, reference_tree=True), dict(use_bvh=True, gpu_build=True),
               dict(use_bvh=True, gpu_build=True, allow_half_boxes=False)):
        r = mirt.Renderer(sc, max_bounces=6, **kw); r.Resize(96, 64); r.Accumulate(5)
        assert_same(r.accumulator(), want, f"seed {seed} n {n} {kw}")
        assert r.counters()["rays"] == o.counters()["rays"]
        r.close()


@pytest.mark.parametrize("hw", [(19, 37), (1, 5), (64, 128)])
def test_sky_lookup_with_a_real_equirect_image(mirt, hw):
    """Sky::operator() (Primitives.hpp:35-46): nearest-texel lookup into an RGBA-f32 equirect image through fast_atan2 /
    fast_asin, scaled by ambient_color, times throughput.r on all three channels (Q10).  The repo ships no env.hdr, so the
    image is synthetic; every texel is different, so a wrong row, column or channel shows."""
    h, w = hw
    sc = mirt.scene.default9()
    rng = np.random.default_rng(h * 1000 + w)
    sc.hdri = rng.uniform(0.0, 4.0, (h, w, 4)).astype(np.float32)
    sc.ambient = np.array([0.7, 0.5, 0.9], dtype=np.float32)
    o = ob.Oracle(sc, max_bounces=6, trav_mode=ob.TRAV_BRUTE); o.Resize(96, 64); o.Accumulate(10)
    for use_bvh in (False, True):
        r = mirt.Renderer(sc, max_bounces=6, use_bvh=use_bvh); r.Resize(96, 64); r.Accumulate(10)
        assert_same(r.accumulator(), o.accumulator(), f"hdri {h}x{w} use_bvh={use_bvh}")
        assert r.Render(); assert_same(r.GetFrame(), o.Render(), "resolved frame")
        r.close()
    assert o.accumulator().max() > 0.5


def test_frame_loop_with_deferred_batches(mirt):
    """The reference's UI loop calls Accumulate(); Render(); once per frame (Application.cpp:379-380) and moves the camera in
    between.  mirt_accumulate_async defers partial batches: frames between two due Render()s are traced together, deferred
    frames keep the camera they were issued under, and every observer sees all issued frames."""
    sc = mirt.scene.synthetic(1000, ambient=0.5)
    r = mirt.Renderer(sc, max_bounces=5, use_bvh=True); r.Resize(96, 64)
    o = ob.Oracle(sc, max_bounces=5, trav_mode=ob.TRAV_BRUTE); o.Resize(96, 64)
    frames_shown = 0
    for frame in range(1, 24):
        if frame == 8:                                       # camera move: the app resets (Application.cpp:332)
            sc.camera.pos = sc.camera.pos + np.array([0.5, 0.0, 0.0], dtype=np.float32)
            for x in (r, o):
                x.UpdateCamera() if x is r else x.update_camera()
                x.ResetAccumulator()
        if frame == 15:                                      # camera change WITHOUT reset: frames issued before keep the old camera
            sc.camera.pos = sc.camera.pos + np.array([0.0, 0.25, 0.0], dtype=np.float32)
            r.UpdateCamera(); o.update_camera()
        r.UpdateCamera()                                     # the host mirror re-sends the camera before every Accumulate(): unchanged -> no flush
        r.AccumulateAsync(1); o.Accumulate(1)
        assert r.accumulations == o.accumulations            # issued frames are counted at once
        shown = r.Render()
        want = o.Render()
        assert shown == (want is not None)
        if shown:
            frames_shown += 1
            assert_same(r.GetFrame(), want, f"frame {frame}")
    assert frames_shown >= 3
    assert_same(r.accumulator(), o.accumulator(), "accumulator after the loop")
    assert r.counters()["rays"] == o.counters()["rays"]
    r.close()


def test_white_furnace_gpu(mirt):
    r = mirt.Renderer(mirt.scene.white_furnace(), use_bvh=True); r.Resize(64, 64); r.Accumulate(5)
    assert np.all(r.accumulator() == 1.0)
    assert r.Render() and np.ptp(r.GetFrame()[..., :3].reshape(-1, 3), axis=0).max() == 0.0
    r.close()


# ---- size-independent properties at larger sizes ---------------------------------------------------------------------------
def test_bvh_equals_brute_force_on_gpu_cfg2_shape(mirt):
    """BASELINE cfg2 geometry (1024x1024, 1k spheres, 5 bounce iterations) at 5 accumulations: the BVH path must give
    the brute-force path's accumulators bit for bit (10 M rays)."""
    sc = mirt.scene.synthetic(1000, ambient=0.5)
    out = []
    for use_bvh in (False, True):
        r = mirt.Renderer(sc, max_bounces=5, use_bvh=use_bvh); r.Resize(1024, 1024); r.Accumulate(5)
        out.append((r.accumulator(), r.counters())); r.close()
    assert_same(out[1][0], out[0][0], "BVH vs brute force")
    assert out[0][1]["rays"] == out[1][1]["rays"] > 10_000_000


def test_sharded_contexts_reproduce_the_whole(mirt):
    sc = mirt.scene.synthetic(1000, ambient=0.5)
    w, h, spp = 256, 192, 10
    whole = mirt.Renderer(sc, max_bounces=5, use_bvh=True); whole.Resize(w, h); whole.Accumulate(spp)
    want = whole.accumulator(); whole.close()
    tiles = (w // 16) * (h // 16)
    parts = []
    for rank in range(3):
        first, count = mirt.distributed.tile_range(tiles, rank, 3)
        r = mirt.Renderer(sc, max_bounces=5, use_bvh=True); r.Resize(w, h); r.SetTileRange(first, count); r.Accumulate(spp)
        parts.append(r.accumulator()); r.close()
    assert_same(np.concatenate(parts), want, "sharded vs whole")


@pytest.mark.parametrize("world", [2, 5])
def test_interleaved_tile_rows_reproduce_the_whole(mirt, world):
    """mirt_set_tile_rows: rank r renders tile rows r, r+N, ... (what bench.py --gpus N uses: every GPU gets sky and ground
    alike).  Slabs put back row by row give the single-context accumulator bit for bit, and each context's Render() fills
    exactly its own rows of the frame."""
    sc = mirt.scene.synthetic(1000, ambient=0.5)
    w, h, spp = 208, 192, 10                                 # 13 x 12 tiles: 12 rows do not divide by 5
    h_tiles, v_tiles = w // 16, h // 16
    whole = mirt.Renderer(sc, max_bounces=5, use_bvh=True); whole.Resize(w, h); whole.Accumulate(spp)
    want = whole.accumulator().reshape(v_tiles, h_tiles, -1); assert whole.Render(); want_frame = whole.GetFrame().copy(); whole.close()
    got = np.zeros_like(want); frame = np.zeros_like(want_frame)
    for rank in range(world):
        first_row, stride, n_rows = mirt.distributed.tile_rows(v_tiles, rank, world)
        r = mirt.Renderer(sc, max_bounces=5, use_bvh=True); r.Resize(w, h); r.SetTileRows(first_row, stride); r.Accumulate(spp)
        acc = r.accumulator()
        assert acc.size == n_rows * h_tiles * 5 * 3 * 256
        got[rank::world] = acc.reshape(n_rows, h_tiles, -1)
        assert r.Render()
        mine = r.GetFrame()
        rows = np.concatenate([np.arange(16 * tr, 16 * tr + 16) for tr in range(rank, v_tiles, world)])
        other = np.setdiff1d(np.arange(h), rows)
        assert not mine[other].any()                         # rows of other ranks stay untouched
        frame[rows] = mine[rows]
        r.close()
    assert_same(got, want, f"interleaved rows over {world} contexts vs whole")
    assert_same(frame, want_frame, "frames assembled from the ranks' rows")


def test_batching_and_call_splitting_do_not_change_results(mirt):
    sc = mirt.scene.default9()
    a = mirt.Renderer(sc, use_bvh=True); a.Resize(128, 64); a.Accumulate(13)
    b = mirt.Renderer(sc, use_bvh=True, max_batch=1); b.Resize(128, 64)
    for n in (1, 4, 0, 8):
        b.Accumulate(n)
    assert a.accumulations == b.accumulations == 13
    assert_same(b.accumulator(), a.accumulator(), "batch 1 vs default batch")
    assert not a.Render()                                  # 13 % 5 != 0
    a.Accumulate(2); assert a.Render()
    a.close(); b.close()


@pytest.mark.parametrize("streams", [1, 3])
def test_batches_larger_than_the_bucket_count(mirt, streams):
    """A batch may carry more accumulations than there are buckets (default: about 512 M primary rays per batch, at most 256 accumulations): paths add
    into a per-slot contribution buffer and the merge applies the slots to their buckets in accumulation order, so every
    batch size gives the oracle's accumulator bit for bit — including sizes that do not divide the bucket count or the call."""
    sc = mirt.scene.synthetic(1000, ambient=0.5)
    o = ob.Oracle(sc, max_bounces=5, trav_mode=ob.TRAV_BRUTE); o.Resize(192, 96); o.Accumulate(23)
    want, wc = o.accumulator(), o.counters()
    for max_batch in (0, 1, 3, 5, 7, 16, 64, 200):
        r = mirt.Renderer(sc, max_bounces=5, use_bvh=True, streams=streams, max_batch=max_batch); r.Resize(192, 96)
        eff = r.get_policy()
        assert eff["max_batch"] == (max_batch or 256) and eff["streams"] == streams      # 0 = auto: 512 M rays / 18 k pixels, capped at 256 (path ids: slot << 15 | pixel)
        r.Accumulate(9); r.Accumulate(14)
        assert_same(r.accumulator(), want, f"max_batch={max_batch} streams={streams}")
        c = r.counters()
        assert c["rays"] == wc["rays"] and c["terminated"] == wc["terminated"] and c["terminated"] + c["dropped"] == 23 * 192 * 96   # every path accounted for
        r.close()
    # a context with few pixels has room for many batch slots in its path ids: 150 accumulations of a 64x48 image as ONE batch
    sc = mirt.scene.default9()
    o = ob.Oracle(sc, max_bounces=6, trav_mode=ob.TRAV_BRUTE); o.Resize(64, 48); o.Accumulate(150)
    r = mirt.Renderer(sc, max_bounces=6, use_bvh=True, streams=streams); r.Resize(64, 48)
    assert r.get_policy()["max_batch"] == 256
    r.AccumulateAsync(150); r.Synchronize()
    assert_same(r.accumulator(), o.accumulator(), f"150 accumulations in one batch, streams={streams}")
    assert r.Render(); assert_same(r.GetFrame(), o.Render(), "its frame")
    r.close()


def test_stream_pipelining_does_not_change_results(mirt):
    """policy.streams batches run concurrently on separate HIP streams; the in-order merge of their contribution buffers
    must reproduce the strictly sequential result bit for bit (every bucket sees its adds in accumulation order)."""
    sc = mirt.scene.synthetic(1000, ambient=0.5)
    out = {}
    for streams in (1, 2, 3, 5):
        r = mirt.Renderer(sc, max_bounces=5, use_bvh=True, streams=streams); r.Resize(256, 160)
        for n in (7, 30, 3):                                # uneven calls: partial batches, many batches in flight
            r.AccumulateAsync(n)
        r.Synchronize()
        out[streams] = (r.accumulator(), r.counters()); r.close()
    o = ob.Oracle(sc, max_bounces=5, trav_mode=ob.TRAV_BRUTE); o.Resize(256, 160); o.Accumulate(40)
    for streams, (acc, ctr) in out.items():
        assert_same(acc, o.accumulator(), f"streams={streams}")
        assert ctr["rays"] == o.counters()["rays"] and ctr["terminated"] == o.counters()["terminated"]


def test_resume_from_loaded_accumulator(mirt):
    sc = mirt.scene.default9()
    a = mirt.Renderer(sc); a.Resize(64, 64); a.Accumulate(10)
    b = mirt.Renderer(sc); b.Resize(64, 64); b.Accumulate(5)
    c = mirt.Renderer(sc); c.Resize(64, 64); c.load_accumulator(b.accumulator(), 5); c.Accumulate(5)
    assert_same(c.accumulator(), a.accumulator(), "resume")
    a.ResetAccumulator()
    assert a.accumulations == 0 and not a.accumulator().any()
    for r in (a, b, c):
        r.close()


def test_edge_cases_and_errors(mirt):
    sc = mirt.scene.default9()
    r = mirt.Renderer(sc)
    with pytest.raises(mirt.MirtError):
        r.Accumulate(1)                                    # Resize not called
    r.Resize(70, 40)                                       # truncates to 4 x 2 tiles (Renderer.hpp:59-60)
    r.Accumulate(5)
    assert r.accumulator().shape == (8, 5, 3, 256)
    assert r.Render()
    fb = r.GetFrame()
    assert fb.shape == (40, 70, 4) and not fb[32:].any() and not fb[:, 64:].any() and np.all(fb[:32, :64, 3] == 1.0)
    o = ob.Oracle(sc); o.Resize(70, 40); o.Accumulate(5)
    assert_same(r.accumulator(), o.accumulator(), "ragged size")
    with pytest.raises(mirt.MirtError):
        r.set_policy(buckets=0)
    with pytest.raises(mirt.MirtError):
        r.SetTileRange(7, 5)
    r.Resize(8, 8)                                         # no whole tile: ++accumulations over an empty parallel_for (Renderer.hpp:59-60,74-75), like the reference
    r.Accumulate(3)
    assert r.accumulations == 3 and r.accumulator().size == 0
    r.close()
    bad = mirt.scene.default9(); bad.geometry["material_ID"][3] = 99
    with pytest.raises(mirt.MirtError):
        mirt.Renderer(bad)
    # a caller's tree whose inner nodes share children (node 1 -> {2,3}, node 2 -> {3,4}) is refused, not walked
    r = mirt.Renderer(mirt.scene.default9(), reference_tree=True, use_bvh=True)
    nodes = r.nodes.copy()
    bad_nodes = np.zeros(7, dtype=mirt.scene.NODE)
    bad_nodes["min_bound"] = -10.0; bad_nodes["max_bound"] = 10.0
    bad_nodes["first_id"] = [1, 3, 3, 0, 1, 2, 3]; bad_nodes["prim_count"] = [0, 0, 0, 1, 1, 1, 1]
    bad_nodes["first_id"][2] = 4                                             # node 1 -> {3,4}, node 2 -> {4,5}: node 4 has two parents
    with pytest.raises(mirt.MirtError, match="more than one parent"):
        r.UpdateScene(nodes=bad_nodes)
    r.UpdateScene(nodes=nodes)                                               # the context stays usable
    r.close()
    for field, value in (("position", np.nan), ("position", np.inf), ("radius_sq", -1.0), ("radius_sq", np.nan)):
        bad = mirt.scene.default9()
        if field == "position": bad.geometry["position"][2, 1] = value
        else: bad.geometry["radius_sq"][2] = value
        with pytest.raises(mirt.MirtError):                  # non-finite geometry is refused (host builder and mirt_set_scene), not traced
            mirt.Renderer(bad)


def test_cpp_host_matches_golden_and_oracle(mirt, tmp_path):
    """The C++ host mirror (csrc/mirt_host.hpp + mirt_headless, reference call protocol: Accumulate(); Render() per frame):
    its accumulator (FNV-1a of the raw words) and its PFM frame must equal the committed golden vector / the live oracle."""
    import json
    import subprocess
    exe = os.path.join(mirt.CSRC, "mirt_headless")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", mirt.CSRC, "mirt_headless"], check=True)

    g = np.load(os.path.join(GOLDEN, "default9_64x64_10spp_b16.npz"))
    o = ob.Oracle(mirt.scene.synthetic(1000, ambient=0.5), max_bounces=5, trav_mode=ob.TRAV_BRUTE); o.Resize(64, 32); o.Accumulate(5)
    ob9 = ob.Oracle(mirt.scene.bvh_test(), max_bounces=16, trav_mode=ob.TRAV_BRUTE); ob9.Resize(64, 48); ob9.Accumulate(10)
    cases = [(["--scene", "default9"], 64, 64, 10, g["accumulator"], g["frame"], int(g["rays"])),
             (["--scene", "synthetic:1000", "--ambient", "0.5", "--bounces", "5"], 64, 32, 5, o.accumulator(), o.Render(), o.counters()["rays"]),
             (["--scene", "bvh_test"], 64, 48, 10, ob9.accumulator(), ob9.Render(), ob9.counters()["rays"])]
    for args, w, hgt, spp, want_acc, want_frame, want_rays in cases:
        pfm = str(tmp_path / "frame.pfm")
        out = subprocess.run([exe, *args, "--size", f"{w}x{hgt}", "--spp", str(spp), "--out", pfm], check=True, capture_output=True, text=True).stdout
        rep = json.loads(out)
        assert rep["accumulations"] == spp and rep["rays"] == want_rays and rep["frame_ready"], args
        assert rep["accumulator_fnv1a"] == fnv1a(want_acc), args
        raw = open(pfm, "rb").read()
        assert raw.startswith(b"PF\n") and len(raw) == len(f"PF\n{w} {hgt}\n-1.0\n") + w * hgt * 12
        img = np.frombuffer(raw[-w * hgt * 12:], dtype="<f4").reshape(hgt, w, 3)
        assert np.array_equal(img.view(np.uint32), np.ascontiguousarray(want_frame[..., :3]).view(np.uint32)), args


def test_cpp_host_frame_loop(mirt):
    """--frames N: the reference's UI loop (Application.cpp:373-380) — every frame Accumulate(); Render(); — reported per frame:
    a frame is due on every 5th call (Renderer.hpp:437) and the last due frame equals the oracle's."""
    import json
    import subprocess
    exe = os.path.join(mirt.CSRC, "mirt_headless")
    out = subprocess.run([exe, "--scene", "default9", "--size", "64x48", "--frames", "12"], check=True, capture_output=True, text=True).stdout
    rep = json.loads(out)
    assert rep["accumulations"] == 12 and rep["frames_due"] == [5, 10] and rep["frame_ready"]
    o = ob.Oracle(mirt.scene.default9(), max_bounces=16, trav_mode=ob.TRAV_BRUTE); o.Resize(64, 48)
    o.Accumulate(10); frame10 = o.Render(); o.Accumulate(2)
    assert rep["accumulator_fnv1a"] == fnv1a(o.accumulator())
    assert rep["last_frame_fnv1a"] == fnv1a(frame10)


@pytest.mark.parametrize("n,w,h,spp,mb", [(10000, 256, 192, 5, 9), (100000, 192, 128, 5, 9)])
def test_large_scenes_bvh_equals_brute_force(mirt, n, w, h, spp, mb):
    """cfg3 / cfg4 geometry (10k / 100k spheres, 9 bounce iterations): only the top of the tree fits in LDS, the rest of the
    records and all spheres come from L2/HBM.  The BVH path must still give the brute-force accumulators bit for bit."""
    sc = mirt.scene.synthetic(n)
    b = mirt.Renderer(sc, max_bounces=mb, use_bvh=False); b.Resize(w, h); b.Accumulate(spp)
    want, wc = b.accumulator(), b.counters(); b.close()
    for reference_tree in (False, True):
        r = mirt.Renderer(sc, max_bounces=mb, use_bvh=True, reference_tree=reference_tree); r.Resize(w, h); r.Accumulate(spp)
        info = r.debug_info()
        assert info["wide"] == 1 and n // 3 <= info["records"] < n - 1 and 0 < info["lds_records"] < info["records"] and info["lds_spheres"] == 0
        assert_same(r.accumulator(), want, f"S({n}) BVH (reference_tree={reference_tree}) vs brute force")
        assert r.counters()["rays"] == wc["rays"] and r.counters()["terminated"] == wc["terminated"]
        r.close()


@pytest.mark.parametrize("name,n,mb,buckets,w,h,spp", [("cfg3", 10000, 9, 5, 256, 192, 5), ("cfg4", 100000, 9, 5, 128, 96, 5), ("cfg5", 100000, 17, 16, 96, 64, 16)])
def test_baseline_scenes_and_policies_vs_brute_force_oracle(mirt, name, n, mb, buckets, w, h, spp):
    """BASELINE cfg3 / cfg4 / cfg5: their own scene S(n) and their own policy (bounce iterations, buckets, MIS), at a resolution
    the oracle's brute-force loops (the reference as shipped, BVH.hpp:312 / :365) finish in seconds on the host threads.
    The shipped GPU pipeline must reproduce the oracle's accumulators and frame bit for bit."""
    sc = mirt.scene.synthetic(n)
    o = ob.Oracle(sc, max_bounces=mb, buckets=buckets, trav_mode=ob.TRAV_BRUTE); o.Resize(w, h); o.Accumulate(spp)
    r = mirt.Renderer(sc, max_bounces=mb, buckets=buckets, use_bvh=True); r.Resize(w, h); r.Accumulate(spp)
    assert_same(r.accumulator(), o.accumulator(), f"{name} scene and policy, {w}x{h}x{spp}: HIP BVH pipeline vs brute-force oracle")
    if spp % buckets == 0:
        assert r.Render(); assert_same(r.GetFrame(), o.Render(), f"{name} frame")
    cg, co = r.counters(), o.counters()
    assert cg["rays"] == co["rays"] and cg["terminated"] == co["terminated"]
    assert cg["shadow_rays"] <= co["shadow_rays"]           # the reference also traces NEE rays of last-bounce hits, whose paths it then drops (Q5)
    assert cg["terminated"] + cg["dropped"] == spp * (w // 16) * (h // 16) * 256
    r.close()


@pytest.mark.parametrize("name,n_tiles,spp", [("cfg3", 64, 5), ("cfg4", 40, 5), ("cfg5", 16, 16)])
def test_full_size_spot_checks_vs_oracle(mirt, name, n_tiles, spp):
    """BASELINE cfg3 / cfg4 / cfg5 at their FULL image size (1920x1088, 4096x4096): the shipped pipeline (batches, streams,
    contribution buffers) renders the whole image; the oracle renders a spread of its 16x16 tiles with the brute-force loops
    (every random draw depends only on the global LaunchIndex, pixel and accumulation: Renderer.hpp:107,117).  Those tiles'
    accumulator slabs must agree bit for bit, every path of the image must be accounted for."""
    cfg = mirt.scene.CONFIGS[name]
    w, h, mb, buckets = cfg["width"], cfg["height"], cfg["max_bounces"], cfg["buckets"]
    sc = mirt.scene.synthetic(cfg["n"], ambient=cfg["ambient"])
    h_tiles, v_tiles = w // 16, h // 16
    rng = np.random.default_rng(11)
    tiles = np.unique(np.concatenate([[0, h_tiles - 1, (v_tiles - 1) * h_tiles, v_tiles * h_tiles - 1, (v_tiles // 2) * h_tiles + h_tiles // 2],
                                      rng.integers(0, h_tiles * v_tiles, n_tiles - 5)])).astype(np.uint32)
    r = mirt.Renderer(sc, max_bounces=mb, buckets=buckets, use_bvh=True); r.Resize(w, h); r.Accumulate(spp)
    c = r.counters()
    assert c["terminated"] + c["dropped"] == spp * h_tiles * v_tiles * 256
    got = r.accumulator()[tiles]
    r.close()
    o = ob.Oracle(sc, max_bounces=mb, buckets=buckets, trav_mode=ob.TRAV_BRUTE); o.Resize(w, h, tiles=tiles); o.Accumulate(spp)
    assert_same(got, o.accumulator(), f"{name} full size {w}x{h}: {len(tiles)} tiles vs brute-force oracle")
    assert got.any()


@pytest.mark.parametrize("name,spp", [("cfg3", 5), ("cfg4", 2)])
def test_full_size_bvh_equals_brute_force(mirt, name, spp):
    """BASELINE cfg3 / cfg4 at full size: the BVH pipeline and the brute-force path (the reference as shipped) agree on every word
    of the whole accumulator, and every path is accounted for (size-independent property; the oracle covers a spread of tiles
    of the same images in test_full_size_spot_checks_vs_oracle)."""
    cfg = mirt.scene.CONFIGS[name]
    w, h, mb = cfg["width"], cfg["height"], cfg["max_bounces"]
    sc = mirt.scene.synthetic(cfg["n"], ambient=cfg["ambient"])
    fast = mirt.Renderer(sc, max_bounces=mb, use_bvh=True); fast.Resize(w, h); fast.AccumulateAsync(spp)
    slow = mirt.Renderer(sc, max_bounces=mb, use_bvh=False, streams=1); slow.Resize(w, h); slow.Accumulate(spp)
    fast.Synchronize()
    cf, cs = fast.counters(), slow.counters()
    assert cf["rays"] == cs["rays"] and cf["shadow_rays"] == cs["shadow_rays"]
    assert cf["terminated"] + cf["dropped"] == spp * (w // 16) * (h // 16) * 256 == cs["terminated"] + cs["dropped"]
    a, b = fast.accumulator(), slow.accumulator()
    fast.close(); slow.close()
    assert_same(a, b, f"{name} full size: BVH pipeline vs brute force")
    assert np.isfinite(a).all() and (a >= 0).all()


@pytest.mark.parametrize("scene_name,w,h,spp,mb", [("default9", 160, 96, 10, 16), ("S1000a", 256, 128, 16, 5), ("S20000", 320, 192, 8, 6), ("bvh_test", 128, 96, 10, 16), ("S1000a", 32, 16, 5, 5)])
def test_primary_rays_through_pixel_candidate_lists(mirt, scene_name, w, h, spp, mb):
    """The camera rays of a batch share one cone traversal per pixel that lists the spheres its jittered samples can hit
    (kernels.hpp kCollect / k_primary_cand / k_primary_hits); pixels whose list overflows are traced normally.  Same
    accumulators bit for bit as with every primary ray walking the tree (policy.trace_primary_rays) and as the brute-force
    oracle, the same ray counts, and far fewer box tests.  32x16: a bundle wider than the tree can take -> every pixel falls back."""
    sc = mirt.scene.synthetic(20000) if scene_name == "S20000" else mirt.scene.bvh_test() if scene_name == "bvh_test" else make_scene(mirt, scene_name)
    a = mirt.Renderer(sc, max_bounces=mb, use_bvh=True, count_traffic=True); a.Resize(w, h); a.Accumulate(spp)
    b = mirt.Renderer(sc, max_bounces=mb, use_bvh=True, count_traffic=True, trace_primary_rays=True); b.Resize(w, h); b.Accumulate(spp)
    assert_same(a.accumulator(), b.accumulator(), f"{scene_name}: candidate lists vs traced primary rays")
    ca, cb = a.counters(), b.counters()
    for k in ("rays", "shadow_rays", "terminated", "dropped", "shadow_nodes"):
        assert ca[k] == cb[k], k
    if w >= 128:
        assert ca["nodes"] < cb["nodes"]                     # the primary rays' box tests are gone (one cone per pixel instead)
    if scene_name != "S20000":
        o = ob.Oracle(sc, max_bounces=mb, trav_mode=ob.TRAV_BRUTE); o.Resize(w, h); o.Accumulate(spp)
        assert_same(a.accumulator(), o.accumulator(), f"{scene_name}: candidate lists vs brute-force oracle")
    a.close(); b.close()


def test_cfg5_policy_16_buckets_17_bounces(mirt):
    """BASELINE cfg5 policy (16 buckets, Policy.max_bounces 17) on S(10000) at a size the oracle's brute force finishes."""
    sc = mirt.scene.synthetic(10000)
    o = ob.Oracle(sc, max_bounces=17, buckets=16, trav_mode=ob.TRAV_BRUTE); o.Resize(96, 64); o.Accumulate(32)
    r = mirt.Renderer(sc, max_bounces=17, buckets=16, use_bvh=True); r.Resize(96, 64); r.Accumulate(32)
    assert_same(r.accumulator(), o.accumulator(), "cfg5 policy accumulator")
    assert r.Render(); assert_same(r.GetFrame(), o.Render(), "cfg5 policy frame (even-k median)")
    assert r.counters()["rays"] == o.counters()["rays"]
    r.close()


@pytest.mark.parametrize("scene_name,w,h,n_members,spp,mb", [("default9", 160, 96, 3, 10, 16), ("S1000a", 128, 80, 2, 5, 5), ("S1000a", 96, 80, 4, 5, 5)])
def test_group_in_the_library_reproduces_the_single_renderer(mirt, scene_name, w, h, n_members, spp, mb):
    """mirt_group_*: one renderer object on n devices — scene replicated, tile rows interleaved, ONE gather to the first device,
    device-side un-interleave, Render() of the whole frame there.  Members sharing this box's one GPU exchange their slabs with
    device copies (RCCL needs distinct devices; its calls are covered by test_rccl_selftest); everything else is the multi-GPU
    path.  Accumulator and frame must equal the single context's and the oracle's bit for bit (80 rows = 5 tile rows: uneven split)."""
    sc = make_scene(mirt, scene_name)
    o = ob.Oracle(sc, max_bounces=mb, trav_mode=ob.TRAV_BRUTE); o.Resize(w, h); o.Accumulate(spp)
    g = mirt.GroupRenderer(sc, devices=[0] * n_members, max_bounces=mb, use_bvh=True); g.Resize(w, h)
    assert not g.Render()                                  # nothing accumulated yet
    g.Accumulate(spp - 1); g.Accumulate(1)
    assert g.accumulations == spp
    assert_same(g.accumulator(), o.accumulator(), f"group of {n_members}: gathered accumulator vs oracle")
    assert g.Render(); assert_same(g.GetFrame(), o.Render(), "group frame vs oracle")
    c = g.counters()
    assert c["rays"] == o.counters()["rays"] and c["terminated"] + c["dropped"] == spp * (w // 16) * (h // 16) * 256
    assert g.gather_ms() > 0
    # a second frame after more accumulations: the gather is repeated, not reused
    g.Accumulate(5); o.Accumulate(5)
    assert g.Render(); assert_same(g.GetFrame(), o.Render(), "group frame after more accumulations")
    g.ResetAccumulator(); assert g.accumulations == 0 and not g.accumulator().any()
    g.close()
    one = mirt.GroupRenderer(sc, devices=[0], max_bounces=mb, use_bvh=True); one.Resize(w, h); one.Accumulate(spp)
    o1 = ob.Oracle(sc, max_bounces=mb, trav_mode=ob.TRAV_BRUTE); o1.Resize(w, h); o1.Accumulate(spp)
    assert_same(one.accumulator(), o1.accumulator(), "group of one")
    one.close()


def test_rccl_selftest(mirt):
    """The RCCL calls mirt_group_gather makes between distinct devices (dlopen of librccl, ncclCommInitAll, grouped ncclSend /
    ncclRecv on a HIP stream), exercised on this box's one GPU by sending 4 MB to itself."""
    mirt.rccl_selftest(0, 1 << 20)


def test_cpp_host_on_a_group(mirt):
    """mirt_headless --devices 0,0: the C++ Renderer mirror drives a two-member group through mirt.h alone; same golden accumulator."""
    import json
    import subprocess
    exe = os.path.join(mirt.CSRC, "mirt_headless")
    g = np.load(os.path.join(GOLDEN, "default9_64x64_10spp_b16.npz"))
    out = subprocess.run([exe, "--scene", "default9", "--size", "64x64", "--spp", "10", "--devices", "0,0"], check=True, capture_output=True, text=True).stdout
    rep = json.loads(out)
    assert rep["gpus"] == 2 and rep["accumulations"] == 10 and rep["rays"] == int(g["rays"]) and rep["frame_ready"]
    assert rep["accumulator_fnv1a"] == fnv1a(g["accumulator"]) and rep["last_frame_fnv1a"] == fnv1a(g["frame"])


def test_accumulator_device_view_for_rccl(mirt):
    """The multi-GPU gather wraps the context's accumulator slab as a torch tensor without a copy."""
    import torch
    r = mirt.Renderer(mirt.scene.default9(), use_bvh=True); r.Resize(64, 48); r.Accumulate(5)
    ptr, nbytes = r.accumulator_device()
    t = mirt.distributed.device_tensor(ptr, nbytes, shape=(12, 5, 3, 256))
    assert t.is_cuda and t.dtype == torch.float32 and t.data_ptr() == ptr
    assert np.array_equal(t.cpu().numpy().view(np.uint32), r.accumulator().view(np.uint32))
    assert mirt.distributed.gather_accumulator(t, 12, 0, 1, 5) is t
    r.close()


def _bench_line(cmd, env, timeout):
    import json
    import subprocess
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1, out.stdout[-500:]
    return json.loads(line[0]), out.stderr


def test_bench_two_ranks_rehearsal(tmp_path):
    """bench.py's torch.distributed path (env parsing, tile sharding, barriers, MAX/SUM reductions, gather) with two ranks
    sharing this box's single GPU over gloo; on an 8-GPU node the same code runs over RCCL.  The N > 1 --full line carries what the
    N = 1 line carries: a roofline for rank 0's share from the rocprofv3 --pmc child passes that rank 0 runs before it joins
    the process group, the CPU baseline, and `group_host` — the library's own multi-GPU host run as a child over the same devices."""
    import shutil
    import sys
    from conftest import ROOT
    env = dict(os.environ, MIRT_BENCH_SHARE_GPU="1", MIRT_BENCH_BACKEND="gloo")
    port = 29700 + os.getpid() % 200
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--config", "cfg2", "--spp", "5", "--full"]
    d, err = _bench_line(cmd, env, 900)
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["image"] == "1024x1024" and d["gather_ms"] is not None
    assert d["value"] > 0 and d["roofline"]["bound"] == "valu" and d["roofline"]["hbm"]["frac"] > 0 and d["rays_per_step"] > 9e6
    assert d["cpu_baseline"] is not None and d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["cores"] >= 1 and d["cpu_baseline"]["host_hardware_threads"] >= d["cpu_baseline"]["cores"]
    assert "4 accumulations" in d["cpu_baseline"]["sample"] or int(d["cpu_baseline"]["sample"].split()[0]) >= 4
    if shutil.which("rocprofv3") or os.path.exists("/opt/rocm/bin/rocprofv3"):
        rf = d["roofline"]
        assert rf["frac"] is not None and 0.0 < rf["frac"] == rf["useful_lane_frac"] <= rf["issue_frac"] <= 1.0, err[-1500:]
        assert 0.0 < rf["arithmetic_frac"] < 1.0 and rf["traffic"] > 0 and rf["pmc"]["batch"] >= 5
    gh = d["group_host"]
    assert "error" not in gh, gh
    assert gh["n_gpus"] == 2 and gh["value"] > 0 and gh["gather_ms"] is not None and gh["gather_ms"] > 0 and gh["devices"] == [0, 0]


def test_bench_group_host_rehearsal():
    """bench.py --group: one process, mirt_group_* over two members that share this box's GPU (slabs move by device copies; on distinct
    devices the same call is the RCCL gather)."""
    import sys
    from conftest import ROOT
    env = dict(os.environ, MIRT_BENCH_DEVICES="0,0")
    d, _ = _bench_line([sys.executable, os.path.join(ROOT, "bench.py"), "--group", "--gpus", "2", "--steps", "1", "--warmup", "1", "--config", "cfg2", "--spp", "5"], env, 600)
    assert d["n_gpus"] == 2 and d["devices"] == [0, 0] and d["value"] > 0 and d["gather_ms"] > 0 and d["rays_per_step"] > 9e6 and d["scaling"] == "strong"


def test_bench_plain_line_and_dump_outputs(mirt, tmp_path):
    """A plain bench run (no --full) times exactly --steps steps and carries none of the --full legs; --dump-outputs writes the accumulator
    the timed steps left, bit for bit what a Renderer driven through the same calls holds, and the same from run to run."""
    import sys
    from conftest import ROOT
    cfg = mirt.scene.CONFIGS["cfg2"]
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--config", "cfg2", "--spp", "5", "--dump-outputs"]
    d, _ = _bench_line(base + [str(tmp_path / "a")], dict(os.environ), 600)
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "Mray/s" and d["dtype"] == "f32"
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["kernel_ms_per_step"] is None and d["value_with_every_primary_ray_walking_the_tree"] is None
    tiles, sums = np.load(tmp_path / "a" / "accumulator_tiles.npy"), np.load(tmp_path / "a" / "accumulator_tile_sums.npy")
    n_tiles = (cfg["width"] // 16) * (cfg["height"] // 16)
    assert tiles.dtype == np.float32 and tiles.shape == (1024, cfg["buckets"], 3, 256) and sums.dtype == np.float64 and sums.shape == (n_tiles, 3)
    r = mirt.Renderer(mirt.scene.synthetic(cfg["n"], ambient=cfg["ambient"]), max_bounces=cfg["max_bounces"], buckets=cfg["buckets"], use_bvh=True)
    r.Resize(cfg["width"], cfg["height"]); r.Accumulate(3 * 5)
    acc = r.accumulator()
    r.close()
    idx = np.sort(np.random.default_rng(0).choice(n_tiles, len(tiles), replace=False))
    assert_same(tiles, acc[idx], "bench --dump-outputs sample vs a Renderer after the same 15 accumulations")
    assert np.allclose(sums, acc.astype(np.float64).sum(axis=(1, 3)), rtol=1e-12, atol=0) and sums.sum() > 0
    _bench_line(base + [str(tmp_path / "b")], dict(os.environ), 600)
    for name in ("accumulator_tiles.npy", "accumulator_tile_sums.npy"):
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), name


def test_cfg2_full_size_properties(mirt):
    """BASELINE cfg2 at full size (1024x1024, 64 accumulations, S(1000), 5 bounce iterations; 132 M closest-hit rays):
    the shipped configuration (internal SAH tree, binary16 records, 3 batches in flight) must reproduce the brute-force
    path's accumulators bit for bit; every path is accounted for; Render() gates on accumulations % 5."""
    sc = mirt.scene.synthetic(1000, ambient=0.5)
    fast = mirt.Renderer(sc, max_bounces=5, use_bvh=True); fast.Resize(1024, 1024); fast.AccumulateAsync(64)
    slow = mirt.Renderer(sc, max_bounces=5, use_bvh=False, streams=1); slow.Resize(1024, 1024); slow.Accumulate(64)
    fast.Synchronize()
    cf, cs = fast.counters(), slow.counters()
    assert cf["rays"] == cs["rays"] > 130_000_000 and cf["shadow_rays"] == cs["shadow_rays"]
    assert cf["terminated"] + cf["dropped"] == 64 * 1024 * 1024 == cs["terminated"] + cs["dropped"]
    assert_same(fast.accumulator(), slow.accumulator(), "cfg2 full size: BVH pipeline vs brute force")
    assert not fast.Render()                              # 64 % 5 != 0
    fast.Accumulate(1); slow.Accumulate(1)
    assert fast.Render() and slow.Render()
    assert_same(fast.GetFrame(), slow.GetFrame(), "cfg2 full size frame")
    acc = fast.accumulator()
    assert np.isfinite(acc).all() and (acc >= 0).all()
    fast.close(); slow.close()


def test_edit_protocol_scene_and_camera_changes(mirt):
    """The reference's edit loop (Application.cpp:299-333, 508-510): change the scene or the camera, rebuild BVH + light
    list, ResetAccumulator, keep accumulating.  After each edit the result must equal a fresh render of the edited scene."""
    sc = mirt.scene.synthetic(200, ambient=0.5)
    r = mirt.Renderer(sc, max_bounces=6, use_bvh=True); r.Resize(96, 64); r.Accumulate(7)
    # geometry + material edit
    sc.geometry["position"][17] += np.float32([0.5, 0.25, -0.75]); sc.geometry["radius_sq"][33] *= np.float32(2.0)
    sc.geometry["material_ID"][40] = 16                                   # becomes a light -> light list changes
    sc.material["albedo"][3] = np.float32([0.9, 0.1, 0.2])
    r.UpdateScene(); r.ResetAccumulator(); r.Accumulate(10)
    o = ob.Oracle(sc, max_bounces=6, trav_mode=ob.TRAV_BRUTE); o.Resize(96, 64); o.Accumulate(10)
    assert np.array_equal(r.lights, o.lights()) and len(r.lights) == 200 // 64 + 1
    assert_same(r.accumulator(), o.accumulator(), "after scene edit")
    # camera move (View::Translate / Rotate results are host-side; the path only sees pos + orient)
    sc.camera.pos = sc.camera.pos + np.float32([1.0, -0.5, 2.0])
    sc.camera.orient = mirt.scene.quat_look_at(mirt.scene._normalize((0.2, -0.4, -1.0)))
    r.UpdateCamera(); r.ResetAccumulator(); r.Accumulate(5)
    o.update_camera(); o.ResetAccumulator(); o.Accumulate(5)
    assert_same(r.accumulator(), o.accumulator(), "after camera move")
    assert r.Render(); assert_same(r.GetFrame(), o.Render(), "frame after camera move")
    # resize keeps the scene, resets the accumulation
    r.Resize(64, 96); o.Resize(64, 96); r.Accumulate(5); o.Accumulate(5)
    assert r.accumulations == 5
    assert_same(r.accumulator(), o.accumulator(), "after resize")
    # policy change of the bucket count reallocates and resets
    r.set_policy(buckets=3); r.Accumulate(6)
    o3 = ob.Oracle(sc, max_bounces=6, buckets=3, trav_mode=ob.TRAV_BRUTE); o3.Resize(64, 96); o3.Accumulate(6)
    assert_same(r.accumulator(), o3.accumulator(), "after bucket-count change"); assert r.Render()
    assert_same(r.GetFrame(), o3.Render(), "3-bucket median frame")
    r.close()


@pytest.mark.parametrize("name,n_tiles", [("cfg4", 8), ("cfg3", 10), ("cfg2", 10)])
def test_bench_launch_shapes_vs_oracle(mirt, name, n_tiles):
    """The launch shapes bench.py's driver line is produced with, against the brute-force oracle: cfg4 4096x4096 as ONE
    batch of 63 accumulations (path ids slot << 24 | pixel with slots up to 62, 1.06 G-entry stream planes, the contribution-buffer path);
    cfg3 1920x1088 as one batch of the 192 accumulations of three 64-accumulation steps issued with AccumulateAsync; cfg2 1024x1024 as one
    batch of 256.  The oracle's cost is bounded by the number of tiles it renders (Oracle.Resize(w, h, tiles=...)), not by a smaller batch."""
    cfg = mirt.scene.CONFIGS[name]
    w, h, mb, buckets = cfg["width"], cfg["height"], cfg["max_bounces"], cfg["buckets"]
    sc = mirt.scene.synthetic(cfg["n"], ambient=cfg["ambient"])
    h_tiles, v_tiles = w // 16, h // 16
    rng = np.random.default_rng(29)
    tiles = np.unique(np.concatenate([[0, v_tiles * h_tiles - 1, (v_tiles // 2) * h_tiles + h_tiles // 2, (3 * v_tiles // 4) * h_tiles + h_tiles // 3],
                                      rng.integers(0, h_tiles * v_tiles, n_tiles - 4)])).astype(np.uint32)
    r = mirt.Renderer(sc, max_bounces=mb, buckets=buckets, use_bvh=True); r.Resize(w, h)
    eff = r.get_policy()
    if name == "cfg4":
        assert eff["max_batch"] == 63 and eff["streams"] == 1          # the plan bench.py logs: 1 G primary rays per batch (what path ids and stream slots hold: 63), one batch in flight
        spp = 63
        r.Accumulate(spp)
    elif name == "cfg3":
        assert eff["max_batch"] == 256 and eff["streams"] == 1
        spp = 192
        for _ in range(3):
            r.AccumulateAsync(64)                                      # bench.py's timed region: three steps, launched as one batch at the synchronisation
        r.Synchronize()
    else:
        assert eff["max_batch"] == 256
        spp = 256
        r.Accumulate(spp)
    assert r.accumulations == spp
    c = r.counters()
    assert c["terminated"] + c["dropped"] == spp * h_tiles * v_tiles * 256
    got = r.accumulator()[tiles]
    r.close()
    o = ob.Oracle(sc, max_bounces=mb, buckets=buckets, trav_mode=ob.TRAV_BRUTE); o.Resize(w, h, tiles=tiles); o.Accumulate(spp)
    assert_same(got, o.accumulator(), f"{name} at bench.py's launch shape ({spp} accumulations in one batch): {len(tiles)} tiles vs brute-force oracle")
    assert got.any()


def test_max_batch_at_its_documented_maximum(mirt):
    """policy.max_batch is clamped to what path ids AND stream slots hold (mirt.h) instead of failing at the first launch.  Checked
    where the clamp binds with little memory — a context that owns 2^22 pixels asks for 256 accumulations per batch and gets 255 — and, when
    the device has the 200 GB free, on the whole 4096x4096 image with max_batch = 64 -> 63 (one Accumulate() call: the arena is carved for the limit)."""
    sc = mirt.scene.synthetic(1000, ambient=0.5)
    r = mirt.Renderer(sc, max_bounces=2, use_bvh=True, max_batch=256); r.Resize(2048, 2048)
    assert r.get_policy()["max_batch"] == 255
    r.set_policy(max_batch=4)                                                  # (the arena of 255 x 2^22 rays is never allocated)
    assert r.get_policy()["max_batch"] == 4
    r.Accumulate(5)
    o = ob.Oracle(sc, max_bounces=2, trav_mode=ob.TRAV_BRUTE); o.Resize(2048, 2048, tiles=np.array([5, 9000], dtype=np.uint32)); o.Accumulate(5)
    assert_same(r.accumulator()[[5, 9000]], o.accumulator(), "2048x2048 after the clamp")
    r.close()
    import torch
    free_b, _ = torch.cuda.mem_get_info(0)
    r = mirt.Renderer(sc, max_bounces=2, use_bvh=True, max_batch=64); r.Resize(4096, 4096)
    assert r.get_policy()["max_batch"] == 63
    if free_b > 230 * (1 << 30):
        r.Accumulate(1)
        assert r.accumulations == 1 and r.counters()["terminated"] + r.counters()["dropped"] == 4096 * 4096
    r.close()


def test_policy_is_planned_before_the_first_launch(mirt):
    """mirt_get_policy reports the batch plan launches will use (not a provisional 256) before anything was accumulated,
    and a policy change the plan does not depend on keeps it."""
    sc = mirt.scene.synthetic(1000, ambient=0.5)
    r = mirt.Renderer(sc, max_bounces=3, use_bvh=True); r.Resize(1024, 1024)
    before = r.get_policy()
    r.Accumulate(2)
    after = r.get_policy()
    assert before["max_batch"] == after["max_batch"] == 256 and before["streams"] == after["streams"]
    r.set_policy(trace_primary_rays=1)
    assert r.get_policy()["max_batch"] == after["max_batch"]
    r.close()


def test_group_with_more_members_than_tile_rows(mirt):
    """members beyond the last tile row own nothing; they count the Accumulate() calls and the group still renders the image."""
    sc = mirt.scene.default9()
    w, h, spp = 96, 32, 5                                                       # two tile rows, four members
    o = ob.Oracle(sc, max_bounces=6, trav_mode=ob.TRAV_BRUTE); o.Resize(w, h); o.Accumulate(spp)
    g = mirt.GroupRenderer(sc, devices=[0, 0, 0, 0], max_bounces=6, use_bvh=True); g.Resize(w, h); g.Accumulate(spp)
    assert g.accumulations == spp
    assert_same(g.accumulator(), o.accumulator(), "group of 4 on 2 tile rows")
    assert g.Render(); assert_same(g.GetFrame(), o.Render(), "its frame")
    g.close()


@pytest.mark.parametrize("n", [16384, 40000])
def test_wide_records_with_a_stack_deeper_than_lds(mirt, n):
    """the spill path of node_step_wide (kernels.hpp: up to three pushes per 4-wide level past the 16 u16 / 12 u32 stack entries kept in
    LDS).  n overlapping spheres on a line: a ray along the line meets all four child boxes of every 4-wide node on its way down, so the stack grows
    by three per level — 7 levels (n = 16384, u16 entries) and 8 levels (n = 40000, u32 entries) pass the LDS-resident part.  Rays along the line,
    against it and oblique ones, closest-hit and any-hit, vs the oracle's brute-force loops."""
    sc = mirt.scene.synthetic(n, ambient=0.5)
    length = 240.0                                                               # |x| <= 120: binary16 planes are precise enough for radius 0.5, so the 4-wide records are used
    sc.geometry["position"] = np.stack([np.linspace(-0.5 * length, 0.5 * length, n), np.zeros(n), np.zeros(n)], axis=1).astype(np.float32)
    sc.geometry["radius_sq"] = np.float32(0.25)
    r = mirt.Renderer(sc, max_bounces=3, use_bvh=True)
    info = r.debug_info()
    assert info["wide"] == 1 and info["depth"] >= (14 if n == 16384 else 16)
    rng = np.random.default_rng(3)
    m = 3000
    px = np.concatenate([np.full(m // 3, -0.5 * length - 3.0), np.full(m // 3, 0.5 * length + 3.0), rng.uniform(-0.5 * length - 2.0, 0.5 * length + 2.0, m - 2 * (m // 3))]).astype(np.float32)
    p = np.stack([px, rng.uniform(-0.3, 0.3, m), rng.uniform(-0.3, 0.3, m)]).astype(np.float32)
    d = np.stack([np.concatenate([np.ones(m // 3), -np.ones(m // 3), rng.uniform(-1, 1, m - 2 * (m // 3))]), rng.normal(0, 0.02, m), rng.normal(0, 0.02, m)])
    d[:, 2 * (m // 3):] += rng.normal(0, 0.5, (3, m - 2 * (m // 3)))
    d = (d / np.linalg.norm(d, axis=0)).astype(np.float32)
    # start the axis-parallel rays inside the row as well: every box on the way is entered before any sphere in front prunes it
    p[0, : m // 6] = rng.uniform(-0.5 * length, 0.5 * length, m // 6).astype(np.float32)
    o = ob.Oracle(sc, max_bounces=3, trav_mode=ob.TRAV_BRUTE)
    tg, ig = r.debug_trace_closest(p, d)
    to, io = o.trace_closest(p, d, ob.TRAV_BRUTE)
    assert np.array_equal(ig, io) and np.array_equal(tg.view(np.uint32), to.view(np.uint32))
    tfar = rng.uniform(0.01, 5.0, m).astype(np.float32)
    assert np.array_equal(r.debug_trace_shadow(p, d, tfar), o.trace_shadow(p, d, tfar, ob.TRAV_BRUTE))
    r.close()


def test_cpp_host_reads_and_writes_radiance_hdr(mirt, tmp_path):
    """mirt_headless --hdri env.hdr --out frame.hdr: the reference's own file formats at both ends of the harness (Application.cpp:225-231
    environment map, Image.cpp:71-74 flipped screenshot).  The environment is written by the Python host, decoded by the C++ one; the sky
    lookups of the render must equal the oracle's on the same decoded texels (accumulator bit for bit), and the stored frame, read back by
    Python, must be the RGBE quantisation of the oracle's frame."""
    import json
    import subprocess
    exe = os.path.join(mirt.CSRC, "mirt_headless")
    rng = np.random.default_rng(77)
    env = (rng.uniform(0.0, 1.0, (24, 48, 4)) ** 3 * 6.0).astype(np.float32)
    env_path, out_path = str(tmp_path / "env.hdr"), str(tmp_path / "frame.hdr")
    mirt.hdr.write_hdr(env_path, env[::-1])                                  # (write_hdr flips: hand the rows over bottom-up so that the file's top row is env[0])
    sc = mirt.scene.default9()
    sc.hdri = mirt.hdr.read_hdr(env_path)
    assert sc.hdri.shape == (24, 48, 4) and np.array_equal(sc.hdri.view(np.uint32), mirt.hdr.rgbe_to_float(mirt.hdr.float_to_rgbe(env)).view(np.uint32))
    sc.ambient = np.array([0.8, 0.8, 0.8], dtype=np.float32)
    o = ob.Oracle(sc, max_bounces=16, trav_mode=ob.TRAV_BRUTE); o.Resize(96, 64); o.Accumulate(10)
    rep = json.loads(subprocess.run([exe, "--scene", "default9", "--size", "96x64", "--spp", "10", "--hdri", env_path, "--ambient", "0.8", "--out", out_path],
                                    check=True, capture_output=True, text=True).stdout)
    assert rep["accumulator_fnv1a"] == fnv1a(o.accumulator()) and rep["frame_ready"]
    frame = o.Render()
    assert frame[..., :3].max() > 0.05
    got = mirt.hdr.read_hdr(out_path)                                       # top-down
    want = mirt.hdr.rgbe_to_float(mirt.hdr.float_to_rgbe(frame))[::-1]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
