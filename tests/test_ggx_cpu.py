"""policy.brdf = 1 (the reference's `#define BRDF 1`, Closure<GGX>) on the CPU: the oracle's GGX closure (`ob.Oracle(brdf=1)`, what
the GPU tests check against) is pinned by golden vectors recorded before the closure switch moved into oracle/oracle.cpp, by an
analytic known answer, and by the Lambertian closure ignoring the decay table."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_binding as ob
from oracle_binding import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def mirror_furnace(mirt):
    """The white furnace (Application.cpp:218-223) with its one material made a perfect mirror: albedo 0, F0 = 1, roughness 0."""
    sc = mirt.scene.white_furnace()
    sc.material["albedo"] = 0.0
    sc.material["F0"] = 1.0
    sc.material["roughness"] = 0.0
    return sc


@pytest.mark.parametrize("scene_name,w,h,spp,mb", [("default9", 64, 64, 5, 16), ("S1000", 64, 48, 5, 5)])
@pytest.mark.parametrize("trav_mode", [ob.TRAV_BRUTE, ob.TRAV_PER_RAY_BVH])
def test_twin_with_brdf0_is_the_oracle(mirt, scene_name, w, h, spp, mb, trav_mode):
    """brdf = 0 with a decay table set equals the oracle as every other test constructs it, bit for bit (accumulator, frame,
    counters): the table is read by Closure<GGX> alone."""
    sc = mirt.scene.default9() if scene_name == "default9" else mirt.scene.synthetic(1000)
    o = ob.Oracle(sc, max_bounces=mb, trav_mode=trav_mode); o.Resize(w, h); o.Accumulate(spp)
    t = ob.Oracle(sc, brdf=0, gloss_decay=[0.5, 0.25], max_bounces=mb, trav_mode=trav_mode); t.Resize(w, h); t.Accumulate(spp)
    assert np.array_equal(bits(t.accumulator()), bits(o.accumulator()))
    assert np.array_equal(bits(t.Render()), bits(o.Render()))
    assert t.counters() == o.counters()
    assert o.counters()["shadow_rays"] > 0


GGX_CASES = {
    "ggx_brdf_test_64x32_10spp_b16_decay": dict(scene="brdf_test", w=64, h=32, spp=10, mb=16, decay=[0.0, 0.1, 0.3, 0.6, 1.0]),
    "ggx_default9_64x64_5spp_b16": dict(scene="default9", w=64, h=64, spp=5, mb=16),
    "ggx_brdf_test_64x32_5spp_b6_nomis": dict(scene="brdf_test", w=64, h=32, spp=5, mb=6, mis=False, decay=[0.0, 0.5]),
}


@pytest.mark.parametrize("name", sorted(GGX_CASES))
@pytest.mark.parametrize("mode", [ob.TRAV_BRUTE, ob.TRAV_PER_RAY_BVH])
def test_oracle_ggx_matches_golden(mirt, name, mode):
    """The golden vectors were recorded (brute force, one thread) from the separate copy of the tile loop that carried the GGX closure
    before it was folded into oracle/oracle.cpp; make_golden.py regenerates the same arrays from `ob.Oracle(brdf=1)`."""
    cfg = GGX_CASES[name]
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    o = ob.Oracle(getattr(mirt.scene, cfg["scene"])(), brdf=1, gloss_decay=cfg.get("decay"), max_bounces=cfg["mb"], mis=cfg.get("mis", True), trav_mode=mode)
    o.Resize(cfg["w"], cfg["h"])
    o.Accumulate(cfg["spp"])
    assert np.array_equal(bits(o.accumulator()), bits(g["accumulator"]))
    img = o.Render()
    if g["frame"].size:
        assert np.array_equal(bits(img), bits(g["frame"]))
    else:
        assert img is None                                # accumulations % buckets != 0 (Renderer.hpp:437)
    c = o.counters()
    assert c["rays"] == int(g["rays"]) and c["terminated"] == int(g["terminated"])
    if mode == ob.TRAV_BRUTE:
        assert c["shadow_rays"] == int(g["shadow_rays"])
    else:                                                 # mode 2, like the product, emits no NEE rays for last-bounce hits (dropped anyway, Q5)
        assert c["shadow_rays"] <= int(g["shadow_rays"])


def test_debug_path_goes_through_the_closure_switch(mirt):
    """orc_debug_path records one pixel's ray and hit per bounce under either closure; the camera ray and its first hit do not depend
    on the closure."""
    sc = mirt.scene.brdf_test()
    recs = {}
    for brdf in (0, 1):
        o = ob.Oracle(sc, brdf=brdf, max_bounces=6, trav_mode=ob.TRAV_BRUTE, threads=1); o.Resize(64, 32)
        recs[brdf] = o.debug_path(6, 0, 1)                 # tile 6, pixel 0: the image centre, which the camera looks at
        assert 1 <= len(recs[brdf]) <= 6
    assert np.array_equal(bits(recs[1][0]), bits(recs[0][0]))
    assert recs[1][0][7] >= 0                             # a hit (a miss records primID -1)


def test_mirror_furnace_is_exactly_one(mirt):
    """alpha = 0 takes the mirror branch of Closure<GGX>::sample; Fresnel(F0 = 1, .) = 1 and G1 = 2 / (1 + sqrt(x / x)) = 1 exactly, so
    the estimator is 1, roulette's q is 0 and the reflected ray leaves the convex sphere for the sky of 1: every accumulator word is
    exactly 1.0.  The Lambertian closure with albedo 0 ends the same paths black."""
    sc = mirror_furnace(mirt)
    t = ob.Oracle(sc, brdf=1, max_bounces=4, trav_mode=ob.TRAV_BRUTE); t.Resize(64, 64); t.Accumulate(5)
    acc = t.accumulator()
    assert np.array_equal(bits(acc), bits(np.ones_like(acc)))
    lam = ob.Oracle(sc, brdf=0, max_bounces=4, trav_mode=ob.TRAV_BRUTE); lam.Resize(64, 64); lam.Accumulate(5)
    assert not lam.accumulator().any()               # the unit sphere fills this camera's view: every pixel is the sphere's


def test_ggx_differs_from_lambertian_and_uses_the_decay(mirt):
    """GGX reads F0 and roughness, not albedo, and the decay table changes alpha from the bounce it names on."""
    sc = mirt.scene.brdf_test()
    runs = {}
    for key, brdf, decay in (("lam", 0, None), ("ggx", 1, None), ("decay", 1, [0.0, 0.5])):
        t = ob.Oracle(sc, brdf=brdf, gloss_decay=decay, max_bounces=6, trav_mode=ob.TRAV_PER_RAY_BVH); t.Resize(64, 32); t.Accumulate(5)
        runs[key] = t.accumulator()
        assert np.isfinite(runs[key]).all()
    assert not np.array_equal(runs["lam"], runs["ggx"])
    assert not np.array_equal(runs["ggx"], runs["decay"])


def test_brdf_test_scene(mirt):
    """Scenes::BRDF_test (Application.cpp:123-217), Properties::Roughness."""
    sc = mirt.scene.brdf_test()
    f = np.float32
    assert len(sc.geometry) == 12 and len(sc.material) == 12
    assert np.array_equal(sc.camera.pos, np.array([0, 0, f(10) * f(2.8)], dtype=f))
    assert np.array_equal(sc.camera.orient, mirt.scene.white_furnace().camera.orient)
    assert sc.geometry[0]["position"].tolist() == [0, -1001, 0] and sc.geometry[0]["radius_sq"] == f(1e6)
    assert sc.material[0]["albedo"].tolist() == [f(0.1)] * 3 and sc.material[0]["roughness"] == 1
    assert sc.geometry[1]["position"].tolist() == [0, 10, 0] and sc.geometry[1]["radius_sq"] == 5
    assert sc.material[1]["emission"].tolist() == [100] * 3
    for i in range(10):
        g, m = sc.geometry[2 + i], sc.material[2 + i]
        assert g["position"][0] == f(2 * i - 10) * f(1.25) + f(1) and g["position"][1] == f(i) * f(0.1) and g["position"][2] == 0
        assert g["radius_sq"] == 1 and g["material_ID"] == 2 + i
        assert m["roughness"] == f(i) / f(9) and m["F0"].tolist() == [1] * 3 and m["F80"].tolist() == [1] * 3 and m["albedo"].tolist() == [0] * 3
    assert sc.ambient.tolist() == [1, 1, 1]
    assert mirt.light_list(sc.geometry, sc.material).tolist() == [1]


def test_default9_carries_every_material_member(mirt):
    """Application.cpp:37-98: the GGX members are filled in; what the Lambertian path reads is unchanged."""
    m = mirt.scene.default9().material
    assert m["roughness"].tolist() == pytest.approx([0.2, 1, 1, 1, 0.85, 0.05, 0.15, 0.1, 0.8])
    assert m["F0"][6].tolist() == pytest.approx([0.944, 0.776, 0.373]) and m["IOR_minus_one"][7] == np.float32(0.762)
    assert m["albedo"][4].tolist() == pytest.approx([0.793, 0.793, 0.664]) and m["emission"][3].tolist() == [200, 17, 25]


def test_policy_has_brdf_at_offset_44(mirt):
    assert C.sizeof(mirt.Policy) == 48 and mirt.Policy.brdf.offset == 44
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    assert "uint32_t brdf;" in header and "_reserved" not in header
    lib = mirt.load_library()
    assert "mirt_set_gloss_decay" in lib._declared and "mirt_group_set_gloss_decay" in lib._declared
    assert lib.mirt_set_gloss_decay(None, None, 0) < 0
