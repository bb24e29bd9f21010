#!/usr/bin/env python3
"""What a sphere drag costs, and what a refitted tree costs to walk (profiles/update_spheres.txt), on BASELINE cfg4's scene (100 000 spheres).

cost     host clock around synchronous calls, median of `repeats` (the first call of each kind is left out: allocation, the links kernel):
         mirt_update_spheres for 1 sphere and for all of them, beside mirt_set_scene on the same context with the host SAH builder and with
         gpu_build, and mirt_bvh_build alone (the caller's share of a rebuild).
walk     cfg4's policy on a 2048 x 2048 image (a quarter of cfg4's pixels: the figure is a rate), 16 accumulations per timing, best of 3: Mray/s
         of the refitted SAH tree beside a fresh SAH tree and a fresh gpu_build tree over the same spheres in the same order, after 1 %, 10 % and
         100 % of the ordinary spheres have moved by one radius and by ten radii (seeded directions); boxes per ray from count_traffic on 512 x 512.
Run from the repository root on the GPU box; one JSON line per figure."""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
mirt = importlib.import_module("cpu-raytracing-experiments_amd")
CFG = dict(mirt.scene.CONFIGS["cfg4"])
f32 = np.float32


def median_ms(fn, repeats=7):
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def scene():
    return mirt.scene.synthetic(CFG["n"], ambient=CFG["ambient"])


def renderer(sc, **kw):
    return mirt.Renderer(sc, max_bounces=CFG["max_bounces"], buckets=CFG["buckets"], mis=True, use_bvh=True, **kw)


def set_scene_again(r):
    """mirt_set_scene alone, with the arrays the renderer holds: the caller's mirt_bvh_build and light list are not in the figure."""
    P = mirt._ptr
    amb = np.ascontiguousarray(r.scene.ambient, dtype=f32); hdri = np.ascontiguousarray(r.scene.hdri, dtype=f32)
    lights = r.lights if len(r.lights) else np.zeros(1, dtype=np.int32)
    r._call("set_scene", P(r.geometry), P(r.prims), len(r.geometry), P(r.nodes), len(r.nodes), P(r.material), len(r.material), P(lights), len(r.lights), P(amb), P(hdri),
            hdri.shape[1], hdri.shape[0])


def cost():
    out = {}
    for name, kw in (("host SAH", {}), ("gpu_build", {"gpu_build": True})):
        r = renderer(scene(), **kw)
        r.Resize(64, 64)
        n = len(r.geometry)
        everyone = np.arange(n)
        out[f"{name}: update_spheres, 1 sphere, ms"] = median_ms(lambda: r.update_spheres([n // 2]))
        out[f"{name}: update_spheres, all {n}, ms"] = median_ms(lambda: r.update_spheres(everyone))
        b, g = np.ascontiguousarray(r._bvh_of_geometry), everyone.astype(np.uint32)
        packet = np.concatenate([r.geometry["position"], r.geometry["radius_sq"][:, None]], axis=1).astype(f32)
        P = mirt._ptr
        out[f"{name}: mirt_update_spheres alone (no numpy), all {n}, ms"] = median_ms(lambda: r._call("update_spheres", n, P(b), P(g), P(packet)))
        out[f"{name}: mirt_set_scene, ms"] = median_ms(lambda: set_scene_again(r), 3)
        r.close()
    geo = np.ascontiguousarray(scene().geometry, dtype=mirt.scene.SPHERE)
    out["mirt_bvh_build alone (the caller's reference builder), ms"] = median_ms(lambda: mirt.bvh_build(geo), 3)
    print(json.dumps({"cost": out}), flush=True)


def rate(r, side=2048, acc=16):
    r.Resize(side, side)
    r.Accumulate(acc)                                             # warm-up: buffers, camera-ray lists
    best = 0.0
    for _ in range(3):
        r.ResetAccumulator()
        c0 = r.counters()["rays"]
        t0 = time.perf_counter(); r.Accumulate(acc); r.Synchronize(); dt = time.perf_counter() - t0
        best = max(best, (r.counters()["rays"] - c0) / dt / 1e6)
    return best


def boxes_per_ray(sc, prims=None, nodes=None, edit=None, **kw):
    r = renderer(sc, count_traffic=True, **kw)
    if prims is not None:
        r.UpdateScene(nodes=nodes, prims=prims)
    if edit is not None:
        r.update_spheres(*edit)
    r.Resize(512, 512); r.Accumulate(CFG["buckets"])
    c = r.counters()
    r.close()
    return (c["nodes"] + c["shadow_nodes"]) / (c["rays"] + c["shadow_rays"])


def walk():
    base = scene()
    radius = np.sqrt(base.geometry["radius_sq"])
    ordinary = np.nonzero(radius < 100.0)[0]
    rng = np.random.default_rng(1)
    direction = rng.normal(size=(len(radius), 3)); direction /= np.linalg.norm(direction, axis=1)[:, None]
    order = rng.permutation(ordinary)
    for fraction in (0.01, 0.1, 1.0):
        for radii in (1.0, 10.0):
            idx = np.sort(order[: max(1, int(round(fraction * len(ordinary))))])
            position = (base.geometry["position"][idx] + (radii * radius[idx])[:, None] * direction[idx]).astype(f32)
            a = renderer(scene())                                  # the SAH tree of the unmoved scene, refitted
            a.update_spheres(idx, position)
            moved = scene(); moved.geometry = a.geometry.copy()
            row = {"moved": f"{fraction:.0%} by {radii:g} radii", "refitted SAH Mray/s": rate(a)}
            for name, kw in (("fresh SAH", {}), ("fresh gpu_build", {"gpu_build": True})):
                b = renderer(moved, **kw)
                b.UpdateScene(nodes=a.nodes, prims=a.prims)       # the same spheres in the same order: the same rays
                row[f"{name} Mray/s"] = rate(b)
                b.close()
                row[f"{name} boxes/ray"] = boxes_per_ray(moved, prims=a.prims, nodes=a.nodes, **kw)
            row["refitted SAH boxes/ray"] = boxes_per_ray(scene(), edit=(idx, position))
            a.close()
            print(json.dumps({"walk": row}), flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["cost", "walk"]
    if "cost" in which:
        cost()
    if "walk" in which:
        walk()
