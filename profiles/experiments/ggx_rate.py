"""What policy.brdf = 1 (Closure<GGX>) costs against the Lambertian path: rays per second (glossy paths survive roulette longer, so
frames are not comparable), per-batch k_shade time from the library's HIP-event brackets, for default9 with every material member at
1920x1088 x 64 accumulations and for BRDF_test.  One warm-up batch, then GGX_REPS timed batches per closure, closures alternated.
Prints one JSON line per (scene, brdf).  For per-instantiation kernel times run it under `rocprofv3 --kernel-trace --stats -- python ...`."""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
mirt = importlib.import_module("cpu-raytracing-experiments_amd")

REPS = int(os.environ.get("GGX_REPS", "3"))
DECAY = [0.0, 0.1, 0.3, 0.6, 1.0]
cases = [("default9", 1920, 1088, 64), ("brdf_test", 1920, 1088, 64)]
for name, w, h, spp in cases:
    sc = getattr(mirt.scene, name)()
    rs = {b: mirt.Renderer(sc, max_bounces=16, use_bvh=True, profile=True, brdf=b, gloss_decay=DECAY) for b in (0, 1)}
    stats = {b: {"rays": 0, "shadow_rays": 0, "s": 0.0, "shade_ms": 0.0, "trace_ms": 0.0} for b in (0, 1)}
    for b, r in rs.items():
        r.Resize(w, h); r.Accumulate(spp)        # warm-up: plan, allocations, code objects
    for _ in range(REPS):
        for b, r in rs.items():
            r.ResetAccumulator(); r.counters(); r.kernel_times(reset=True)
            c0 = r.counters()
            t0 = time.perf_counter(); r.Accumulate(spp); dt = time.perf_counter() - t0
            c1 = r.counters(); kt = r.kernel_times(reset=True)
            st = stats[b]
            st["rays"] += c1["rays"] - c0["rays"]; st["shadow_rays"] += c1["shadow_rays"] - c0["shadow_rays"]; st["s"] += dt
            st["shade_ms"] += kt["shade"]["ms"]; st["trace_ms"] += kt["trace"]["ms"]
    for b, st in stats.items():
        print(json.dumps({"scene": name, "size": f"{w}x{h}", "spp": spp, "brdf": b, "batches": REPS,
                          "rays_per_batch": st["rays"] // REPS, "shadow_rays_per_batch": st["shadow_rays"] // REPS,
                          "mray_per_s": round(st["rays"] / st["s"] / 1e6, 1), "ms_per_batch": round(1e3 * st["s"] / REPS, 2),
                          "k_shade_ms_per_batch": round(st["shade_ms"] / REPS, 2), "k_trace_ms_per_batch": round(st["trace_ms"] / REPS, 2)}), flush=True)
    for r in rs.values():
        r.close()
