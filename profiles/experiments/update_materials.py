#!/usr/bin/env python3
"""What a material edit costs in place, beside the parent commit's path for the same edit (profiles/update_materials.txt), on BASELINE cfg4's
scene (100 000 spheres, 17 materials, material 16 emitting on every 64th sphere).

Host clock around synchronous calls; 3 calls of each kind left out (allocations, first launches), then `REPEATS` timed: median [min .. max].
Every timed call changes something: two states are alternated, and only the direction named is timed.
  in place   mirt_update_materials itself, arrays prepared beforehand: (1) material 16 takes another emission, the light count stays;
             (2) 1 % of the spheres (seeded) take material 16 and become lights; (3) one sphere takes material 16.
  parent     the same three edits the only way the parent commit offers: mirt_light_list over the edited arrays, then mirt_set_scene with them,
             on a context with the host SAH builder (gpu_build 0) and with gpu_build 1.  The caller's mirt_bvh_build is NOT counted: a material
             edit does not need it.
  set_scene  mirt_set_scene alone with unchanged arrays: it now uploads the geometry-order table (20 B per sphere).  `--lib PATH` times the
             same call against another build of libmirt.so (the parent commit's) and nothing else.
Run from the repository root on the GPU box; one JSON line per group of figures."""
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
WARMUP, REPEATS = 3, 15
P = mirt._ptr


def stats(samples):
    return {"median": round(float(np.median(samples)), 4), "min": round(float(np.min(samples)), 4), "max": round(float(np.max(samples)), 4)}


def alternate(there, back):
    """`there` timed, `back` not; both run WARMUP times first."""
    for _ in range(WARMUP):
        there(); back()
    t = []
    for _ in range(REPEATS):
        t0 = time.perf_counter(); there(); t.append((time.perf_counter() - t0) * 1e3)
        back()
    return stats(t)


def renderer(**kw):
    r = mirt.Renderer(mirt.scene.synthetic(CFG["n"], ambient=CFG["ambient"]), max_bounces=CFG["max_bounces"], buckets=CFG["buckets"], mis=True, use_bvh=True, **kw)
    r.Resize(64, 64)
    return r


def set_scene(r, geometry, prims, material, lights):
    amb = np.ascontiguousarray(r.scene.ambient, dtype=f32); hdri = np.ascontiguousarray(r.scene.hdri, dtype=f32)
    some = lights if len(lights) else np.zeros(1, dtype=np.int32)
    r._call("set_scene", P(geometry), P(prims), len(geometry), P(r.nodes), len(r.nodes), P(material), len(material), P(some), len(lights), P(amb), P(hdri), hdri.shape[1], hdri.shape[0])


def states(r):
    """The three edits as (name, in-place call there, in-place call back, arrays there, arrays back)."""
    n = len(r.geometry)
    mat_b = r.material.copy(); mat_b["emission"][16] = (5.0, 40.0, 10.0)
    rng = np.random.default_rng(1)
    dark = np.nonzero(r.geometry["material_ID"] != 16)[0]
    many = np.sort(rng.permutation(dark)[: n // 100]).astype(np.uint32)
    one = np.array([dark[len(dark) // 2]], dtype=np.uint32)
    out = []
    mi = np.array([16], dtype=np.uint32)
    row_a, row_b = np.ascontiguousarray(r.material[[16]]), np.ascontiguousarray(mat_b[[16]])
    out.append(("one material's emission, light count unchanged",
                lambda: r._call("update_materials", 1, P(mi), P(row_b), 0, None, None, None), lambda: r._call("update_materials", 1, P(mi), P(row_a), 0, None, None, None),
                (r.geometry, r.prims, mat_b), (r.geometry, r.prims, r.material)))
    for name, g in ((f"1 % of the spheres ({len(many)}) become lights", many), ("one sphere becomes a light", one)):
        b = np.ascontiguousarray(r._bvh_of_geometry[g])
        to, fro = np.full(len(g), 16, dtype=np.int32), np.ascontiguousarray(r.geometry["material_ID"][g])
        geo_b, prims_b = r.geometry.copy(), r.prims.copy()
        geo_b["material_ID"][g] = 16; prims_b["material_ID"][b] = 16
        call = lambda ids, b=b, g=g: r._call("update_materials", 0, None, None, len(g), P(b), P(g), P(ids))
        out.append((name, lambda call=call, to=to: call(to), lambda call=call, fro=fro: call(fro), (geo_b, prims_b, r.material), (r.geometry, r.prims, r.material)))
    return out


def measure():
    for gpu_build in (0, 1):
        r = renderer(gpu_build=bool(gpu_build))
        row = {"gpu_build": gpu_build, "spheres": len(r.geometry), "lights": len(r.lights)}
        for name, there, back, arrays_there, arrays_back in states(r):
            if gpu_build == 0:                                     # the in-place path does not touch the tree: one builder is enough
                row[f"in place: {name}, ms"] = alternate(there, back)
                back()
            parent = lambda a: set_scene(r, a[0], a[1], a[2], mirt.light_list(a[0], a[2]))
            row[f"parent path (mirt_light_list + mirt_set_scene): {name}, ms"] = alternate(lambda: parent(arrays_there), lambda: parent(arrays_back))
        row["mirt_light_list alone, ms"] = alternate(lambda: mirt.light_list(r.geometry, r.material), lambda: None)
        row["mirt_set_scene alone, unchanged arrays, ms"] = alternate(lambda: set_scene(r, r.geometry, r.prims, r.material, r.lights), lambda: None)
        t = r.lights_table()
        row["compaction"] = {"spheres per workgroup": t["block"], "workgroup totals per scan pass": t["scan_pass"]}
        r.close()
        print(json.dumps(row), flush=True)


def set_scene_only(lib_path):
    mirt.LIB_PATH = lib_path                                       # before the first load_library()
    C = mirt.C

    class Missing:                                                 # an older build lacks the newest entry points: declared, never called here
        argtypes = restype = None

    class Tolerant(C.CDLL):
        def __getattr__(self, name):
            try:
                return super().__getattr__(name)
            except AttributeError:
                if not name.startswith("mirt_"):
                    raise
                return Missing()

    C.CDLL = Tolerant
    for gpu_build in (0, 1):
        r = renderer(gpu_build=bool(gpu_build))
        row = {"library": lib_path, "gpu_build": gpu_build,
               "mirt_set_scene alone, unchanged arrays, ms": alternate(lambda: set_scene(r, r.geometry, r.prims, r.material, r.lights), lambda: None)}
        r.close()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--lib":
        set_scene_only(os.path.abspath(sys.argv[2]))
    else:
        measure()
