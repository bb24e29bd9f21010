"""GPU tests (-m gpu) of the 16-byte ray records (kernels.hpp StreamBuf / ShadowBuf): a shadow record holds its own ray and its path id,
k_trace reads nothing through another stream.  Everything is compared with the CPU oracle bit for bit, counters included.

The four kinds of shadow record — the path survived or ended at the hit (kDestAccum), with or without the emissive add of the
bounce travelling along (kDestFull, plane d) — all occur in the record-kind scenes.  The oracle has no counter of emissive hits
with a pending light record, so their presence is shown from its per-path records (Oracle.debug_path): hits on an emissive
sphere at a bounce that still shades (where the MIS path samples one of the scene's several lights)."""
import numpy as np
import pytest

import oracle_binding as ob

pytestmark = pytest.mark.gpu


def assert_words(got, want, what):
    got = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32); want = np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    assert got.shape == want.shape, what
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} words differ"


def scene_of(mirt, name, ambient):
    if name == "default9":
        sc = mirt.scene.default9()
        sc.ambient = np.full(3, 0.4 if ambient else 0.0, dtype=np.float32)
        return sc
    return mirt.scene.synthetic(1000, ambient=0.5 if ambient else 0.0)


def emissive_hits_that_shade(sc, o, w, h, max_bounces, accumulations):
    """Hits on an emissive sphere at bounces 1 .. max_bounces - 2 (bounce 0 and the last bounce send no record with E), from the oracle's paths."""
    _, prims = o.bvh()
    emissive = (sc.material["emission"].max(axis=1) > np.finfo(np.float32).eps)[prims["material_ID"]]
    n = 0
    for acc in range(1, accumulations + 1):
        for tile in range((w // 16) * (h // 16)):
            for px in range(256):
                rec = o.debug_path(tile, px, acc)
                prim = rec[1:max_bounces - 1, 7].astype(np.int64)
                n += int(emissive[prim[prim >= 0]].sum())
    return n


# ---- 1. record kinds ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("brdf", [0, 1])
@pytest.mark.parametrize("ambient", [False, True])
@pytest.mark.parametrize("scene_name,w,h", [("default9", 64, 48), ("S1000", 64, 64)])
def test_record_kinds_match_the_oracle(mirt, scene_name, w, h, ambient, brdf):
    mb, spp = 5, 7
    decay = [0.0, 0.1, 0.3, 0.6, 1.0] if brdf else None
    sc = scene_of(mirt, scene_name, ambient)
    o = ob.Oracle(sc, max_bounces=mb, buckets=5, mis=True, trav_mode=ob.TRAV_BRUTE, brdf=brdf, gloss_decay=decay); o.Resize(w, h); o.Accumulate(spp)
    r = mirt.Renderer(sc, max_bounces=mb, buckets=5, mis=True, use_bvh=True, count_traffic=True, trace_primary_rays=True, max_batch=spp, streams=1,
                      brdf=brdf, gloss_decay=decay)
    r.Resize(w, h); r.Accumulate(spp)
    assert_words(r.accumulator(), o.accumulator(), f"{scene_name} ambient={ambient} brdf={brdf}: accumulator")
    t = ob.Oracle(sc, max_bounces=mb, buckets=5, mis=True, trav_mode=ob.TRAV_PER_RAY_BVH, brdf=brdf, gloss_decay=decay); t.match_product(r); t.Resize(w, h); t.Accumulate(spp)
    assert_words(t.accumulator(), o.accumulator(), "the twin itself")
    cg, ct = r.counters(), t.counters()
    paths = spp * (w // 16) * (h // 16) * 256
    for k in ("rays", "shadow_rays", "terminated", "nodes", "spheres", "shadow_nodes", "shadow_spheres"):
        assert cg[k] == ct[k], (k, cg[k], ct[k])
    assert cg["dropped"] == paths - ct["terminated"], (cg["dropped"], paths, ct["terminated"])     # every path ends or is dropped after the last bounce
    assert cg["shadow_rays"] > 0 and 0 < cg["terminated"] <= paths
    if scene_name == "default9" and brdf == 0:
        # plane d is exercised: emissive hits on bounces that shade (the scene has three lights, so such a hit samples a light and sends a record)
        assert emissive_hits_that_shade(sc, o, w, h, mb, 2) > 0
    r.close()


# ---- 2. stage level -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_bvh", [False, True])
def test_130_rays_through_the_trace_stage(mirt, use_bvh):
    """130 rays = two full waves and a ragged third (two lanes), the last 16-B group of the list partial: mirt_debug_trace_shadow against the
    oracle's sphere_occludes loop and mirt_debug_trace_closest against its closest-hit loop."""
    n = 130
    sc = mirt.scene.synthetic(1000, ambient=0.5)
    o = ob.Oracle(sc); o.Resize(64, 64)
    rng = np.random.default_rng(130)
    geo = sc.geometry
    pick = rng.integers(0, len(geo), n)
    nrm = rng.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    P = np.ascontiguousarray((geo["position"][pick] + nrm * np.sqrt(geo["radius_sq"][pick])[:, None] * rng.choice([1.0 + 1e-4, 1.5, 3.0], size=(n, 1))).astype(np.float32).T)
    d = rng.normal(size=(n, 3)); D = np.ascontiguousarray((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32).T)
    wt, wi = o.trace_closest(P, D, ob.TRAV_BRUTE)
    tmax = np.where(wi >= 0, wt * rng.uniform(0.5, 1.5, n), 10.0).astype(np.float32)
    wo = o.trace_shadow(P, D, tmax, ob.TRAV_BRUTE)
    assert 0 < wo.sum() < n and 0 < (wi >= 0).sum() < n                         # both outcomes of both stages occur
    r = mirt.Renderer(sc, use_bvh=use_bvh)
    go = r.debug_trace_shadow(P, D, tmax)
    assert np.array_equal(go, wo), f"occlusion: {(go != wo).sum()} of {n} differ"
    gt, gi = r.debug_trace_closest(P, D)
    assert np.array_equal(gi, wi), f"primID: {(gi != wi).sum()} of {n} differ"
    assert_words(gt, wt, "tfar")
    r.close()


# ---- 3. streams across segments -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,spp", [(16, 16, 9), (96, 96, 33)])
def test_streams_across_queue_segments(mirt, w, h, spp):
    """16 x 16 x 9: the late-bounce streams hold fewer rays than one workgroup takes.  96 x 96 x 33: the bounce-1 stream (about 300 k rays, 590
    block iterations) fills all of the queue's segments, so stream and shadow slots of every segment are written and read."""
    sc = mirt.scene.synthetic(1000, ambient=0.5)
    o = ob.Oracle(sc, max_bounces=6, trav_mode=ob.TRAV_BRUTE); o.Resize(w, h); o.Accumulate(spp)
    r = mirt.Renderer(sc, max_bounces=6, use_bvh=True, max_batch=spp, streams=1); r.Resize(w, h); r.Accumulate(spp)
    assert_words(r.accumulator(), o.accumulator(), f"{w}x{h}x{spp}")
    co, cg = o.counters(), r.counters()
    assert cg["rays"] == co["rays"] and cg["terminated"] == co["terminated"] and cg["shadow_rays"] > 0
    assert cg["terminated"] + cg["dropped"] == spp * (w // 16) * (h // 16) * 256
    r.close()
