#!/usr/bin/env python3
"""What a sun drag costs (profiles/sun_sky.txt): mirt_set_sun_sky end to end, with and without the sky table rebuild, beside mirt_set_scene of
BASELINE cfg4's scene (100 000 spheres) with the same map.  Host clock around synchronous calls (each one ends with the main stream
synchronised), median of `repeats`; the first call of each kind is left out (allocation).  Run from the repository root on the GPU box."""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
mirt = importlib.import_module("cpu-raytracing-experiments_amd")


def median_ms(fn, repeats=7):
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    sc = mirt.scene.synthetic(100000, ambient=1.0)
    out = {}
    for (w, h) in ((2049, 1025), (8193, 4097)):
        for sky in (False, True):
            r = mirt.Renderer(sc, max_bounces=9, use_bvh=True, sky_sampling=sky)
            r.Resize(64, 64)
            key = f"{w - 1}x{h - 1}, sky sampling {'on' if sky else 'off'}"
            out[key] = {"set_sun_sky_ms": median_ms(lambda: r.set_sun_sky(width=w, height=h))}
            baked = r.environment()[1]
            out[key]["set_environment_same_map_ms"] = median_ms(lambda: r.set_environment(None, baked), 3)
            amb = np.ascontiguousarray(sc.ambient, dtype=np.float32)
            lights = r.lights if len(r.lights) else np.zeros(1, dtype=np.int32)
            P = mirt._ptr                                  # mirt_set_scene alone: the host's BVH build and light list are not in the figure
            out[key]["set_scene_same_map_ms"] = median_ms(lambda: r._call("set_scene", P(r.geometry), P(r.prims), len(r.geometry), P(r.nodes), len(r.nodes), P(r.material),
                                                                            len(r.material), P(lights), len(r.lights), P(amb), P(baked), baked.shape[1], baked.shape[0]), 3)
            r.close()
            print(json.dumps({key: out[key]}), flush=True)


if __name__ == "__main__":
    main()
