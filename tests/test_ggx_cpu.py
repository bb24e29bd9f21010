"""policy.brdf = 1 (the reference's `#define BRDF 1`, Closure<GGX>) on the CPU: the twin that the GPU tests check against
(tests/native/ggx_twin.cpp) is first shown to be the oracle itself with brdf = 0, then pinned by an analytic known answer."""
import ctypes as C
import os

import numpy as np
import pytest

import ggx_binding as gb
import oracle_binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def ggx_twin(tmp_path_factory):
    """The twin, compiled once per session with oracle/Makefile's CXXFLAGS into a temporary directory."""
    if gb._lib is None:
        gb.load(gb.build(str(tmp_path_factory.mktemp("ggx_twin"))))
    return gb


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def mirror_furnace(mirt):
    """The white furnace (Application.cpp:218-223) with its one material made a perfect mirror: albedo 0, F0 = 1, roughness 0."""
    sc = mirt.scene.white_furnace()
    sc.material["albedo"] = 0.0
    sc.material["F0"] = 1.0
    sc.material["roughness"] = 0.0
    return sc


@pytest.mark.parametrize("scene_name,w,h,spp,mb", [("default9", 64, 64, 5, 16), ("S1000", 64, 48, 5, 5)])
@pytest.mark.parametrize("trav_mode", [ob.TRAV_BRUTE, ob.TRAV_PER_RAY_BVH])
def test_twin_with_brdf0_is_the_oracle(mirt, ggx_twin, scene_name, w, h, spp, mb, trav_mode):
    """The restated tile loop with brdf = 0 equals liboracle.so bit for bit (accumulator, frame, counters): the only thing the twin
    adds is the closure switch."""
    sc = mirt.scene.default9() if scene_name == "default9" else mirt.scene.synthetic(1000)
    o = ob.Oracle(sc, max_bounces=mb, trav_mode=trav_mode); o.Resize(w, h); o.Accumulate(spp)
    t = gb.GgxTwin(sc, brdf=0, gloss_decay=[0.5, 0.25], max_bounces=mb, trav_mode=trav_mode); t.Resize(w, h); t.Accumulate(spp)
    assert np.array_equal(bits(t.accumulator()), bits(o.accumulator()))
    assert np.array_equal(bits(t.Render()), bits(o.Render()))
    assert t.counters() == o.counters()
    assert o.counters()["shadow_rays"] > 0


def test_mirror_furnace_is_exactly_one(mirt, ggx_twin):
    """alpha = 0 takes the mirror branch of Closure<GGX>::sample; Fresnel(F0 = 1, .) = 1 and G1 = 2 / (1 + sqrt(x / x)) = 1 exactly, so
    the estimator is 1, roulette's q is 0 and the reflected ray leaves the convex sphere for the sky of 1: every accumulator word is
    exactly 1.0.  The Lambertian closure with albedo 0 ends the same paths black."""
    sc = mirror_furnace(mirt)
    t = gb.GgxTwin(sc, brdf=1, max_bounces=4, trav_mode=ob.TRAV_BRUTE); t.Resize(64, 64); t.Accumulate(5)
    acc = t.accumulator()
    assert np.array_equal(bits(acc), bits(np.ones_like(acc)))
    lam = gb.GgxTwin(sc, brdf=0, max_bounces=4, trav_mode=ob.TRAV_BRUTE); lam.Resize(64, 64); lam.Accumulate(5)
    assert not lam.accumulator().any()               # the unit sphere fills this camera's view: every pixel is the sphere's


def test_ggx_twin_differs_from_lambertian_and_uses_the_decay(mirt, ggx_twin):
    """GGX reads F0 and roughness, not albedo, and the decay table changes alpha from the bounce it names on."""
    sc = mirt.scene.brdf_test()
    runs = {}
    for key, brdf, decay in (("lam", 0, None), ("ggx", 1, None), ("decay", 1, [0.0, 0.5])):
        t = gb.GgxTwin(sc, brdf=brdf, gloss_decay=decay, max_bounces=6, trav_mode=ob.TRAV_PER_RAY_BVH); t.Resize(64, 32); t.Accumulate(5)
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
