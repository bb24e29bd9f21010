"""mirt_set_material_closures without a GPU: the exported symbols, the Python hosts' validation, the header's wording, and — with the
oracle alone — the power of the GPU test of the sampler's flag (test_material_closures_gpu.py, test 4) on scene X below."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mirt_set_material_closures", "mirt_get_material_closures", "mirt_group_set_material_closures")

X_W, X_H, X_SPP = 64, 64, 16          # test 4's frame: 64 x 64 x 16, buckets = 16


def scene_x(mirt):
    """One ball (material 0: a light Lambertian albedo, a tinted F0, some roughness) that fills most of the frame, and above it, towards the camera and just out of view, one emissive
    sphere (material 1, albedo = F0 = 0): the scene's one light.  No ambient light: a ray that misses ends.  A ray the ball's closure samples
    upwards meets the emitter, and the weight of that hit is Q8's pdf_in — the pdf of the closure that sampled the ray."""
    s = mirt.scene
    mats = [s._material(albedo=(0.9, 0.85, 0.8), F0=(0.9, 0.8, 0.7), roughness=0.4),
            s._material(albedo=(0, 0, 0), F0=(0, 0, 0), emission=(12.0, 10.0, 8.0))]
    geo = [s._sphere((0.0, 0.0, 0.0), 1.0, 0), s._sphere((0.0, 1.7, 1.7), 1.0, 1)]
    return s.Scene(geometry=np.array(geo, dtype=s.SPHERE), material=np.array(mats, dtype=s.MATERIAL),
                   camera=s.Camera(eye=(0.0, 0.0, 4.0), direction=(0.0, 0.0, -1.0), focal_length=50.0), name="closure_x")


def first_hit_prims(o, spp):
    """[acc - 1][tile * 256 + px] -> the primitive (BVH order; -1: none) the camera ray of Accumulate() call `acc` meets first, by the oracle."""
    out = []
    for acc in range(1, spp + 1):
        p, d = o.raygen(acc)
        out.append(o.trace_closest(p, d, ob.TRAV_BRUTE)[1])
    return np.array(out)


def test_symbols_are_exported_and_declared(mirt):
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", mirt.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), f"{name} is not declared in mirt.h"
        assert re.search(rf" T {name}$", nm, re.M), f"{name} is not exported by libmirt.so"
    lib = mirt.load_library()
    assert all(name in lib._declared for name in SYMBOLS)
    # the two host layers: mirt_host.hpp and the headless tool
    assert "SetMaterialClosures" in open(os.path.join(mirt.CSRC, "mirt_host.hpp")).read()
    assert "--closures" in open(os.path.join(mirt.CSRC, "mirt_headless.cpp")).read()


def test_header_documents_both_state_directions():
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    doc = header[header.index("per-material closures"):header.index("int mirt_set_material_closures(")]
    flat = " ".join(doc.replace("*", " ").split())
    assert "a non-empty table under stream order 1" in flat and "mirt_set_stream_order(ctx, 1) with a non-empty table" in flat
    assert "MIRT_ERR_STATE" in flat and "MIRT_ERR_ARG" in flat


@pytest.mark.parametrize("bad", [[2], [0, 1, -1], [0.5], [True], ["1"], [0] * 64, [1] * 100])
def test_python_hosts_refuse_a_bad_table_before_the_library(mirt, bad, monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was reached with a bad table")
    monkeypatch.setattr(mirt, "load_library", no_library)
    for cls in (mirt.Renderer, mirt.GroupRenderer):
        with pytest.raises(ValueError, match="material_closures"):
            cls(mirt.scene.default9(), material_closures=bad)
        obj = cls.__new__(cls)                      # no context: set_material_closures must raise before it looks for one
        with pytest.raises(ValueError, match="material_closures"):
            obj.set_material_closures(bad)


def test_python_hosts_accept_what_the_library_accepts(mirt):
    t = mirt._closure_table([0, 1] * 31 + [1])
    assert t.dtype == np.uint8 and len(t) == mirt.MAX_MATERIALS == 63
    assert len(mirt._closure_table(None)) == 0 and len(mirt._closure_table([])) == 0
    assert mirt._closure_table(np.array([1, 0], dtype=np.int64)).tolist() == [1, 0]


def test_scene_x_gives_gpu_test_4_its_power(mirt):
    """With the oracle alone.  The issue's two conditions at max_bounces = 2: the pure Lambertian run traces secondary rays for at least a quarter of
    the samples whose first hit is the ball, and at least 25 % of all samples hit the ball first.
    max_bounces = 2 alone cannot tell a wrong flag, though: a hit at the last bounce is dropped (Q5), so no emitter hit of bounce 1 is ever
    weighed.  GPU test 4 therefore also runs max_bounces = 3, and for that case this test counts, on the oracle's own paths, the ball-first
    samples whose SECOND hit is the emitter — the hits whose weight is pdf_in: at least 5 % of them."""
    sc = scene_x(mirt)
    nodes, prims = mirt.bvh_build(sc.geometry)
    assert np.array_equal(prims["position"], sc.geometry["position"])              # geometry order = BVH order (Q11 then suppresses the emitter's NEE onto itself)
    o = ob.Oracle(sc, max_bounces=2, buckets=16, mis=True, trav_mode=ob.TRAV_BRUTE)
    o.Resize(X_W, X_H); o.Accumulate(X_SPP)
    rays = o.counters()["rays"]                                                     # (before the classification below traces its own rays)
    first = first_hit_prims(o, X_SPP)
    samples = first.size
    assert samples == X_W * X_H * X_SPP
    ball = int((first == 0).sum())
    primary = samples
    secondary = rays - primary
    print(f"scene X: {ball} of {samples} samples hit the ball first ({ball / samples:.1%}), emitter first {int((first == 1).sum())}, secondary rays {secondary}")
    assert ball >= 0.25 * samples
    assert secondary >= 0.25 * ball
    assert (first == 1).sum() <= 0.75 * samples
    # max_bounces = 3: the second hit of a ball-first sample, on one tile row of accumulation 1
    o3 = ob.Oracle(sc, max_bounces=3, buckets=16, mis=True, trav_mode=ob.TRAV_BRUTE)
    o3.Resize(X_W, X_H); o3.Accumulate(1)
    n_ball = n_emitter_next = 0
    for tile in (5, 6, 9, 10):                                                      # the four middle tiles
        for px in range(256):
            path = o3.debug_path(tile, px, 1)
            if len(path) and int(path[0, 7]) == 0:
                n_ball += 1
                n_emitter_next += len(path) > 1 and int(path[1, 7]) == 1
    print(f"scene X, max_bounces 3: {n_emitter_next} of {n_ball} ball-first samples meet the emitter next")
    assert n_ball >= 512 and n_emitter_next >= 0.05 * n_ball
