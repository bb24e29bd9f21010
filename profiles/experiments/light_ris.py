"""What mirt_set_light_ris costs and buys.  Two parts, one JSON line per row:
  rate        k_shade ms per batch (the library's HIP-event brackets) and Mray/s with M = 0, 1, 4, 8, 16 candidates on default9 and
              S(10000) at 1920x1088 x 64 accumulations; one warm-up batch, then LIGHT_RIS_REPS timed batches per M, the Ms alternated.
  equal_time  wall time of accumulate_until to the same noise target (the 0.95-quantile the plain draw reaches in 1024 accumulations) with M = 0 and with the Ms of LIGHT_RIS_MS on the 600-sphere cloud of
              tests/views_and_scales.py (37 lights) and on S(10000): the comparison that decides whether the feature pays on a scene.
LIGHT_RIS_PARTS=rate,equal_time picks the parts, LIGHT_RIS_RATE_MS=0,16 the Ms of the rate part (one context each, all alive at once:
the brackets of a run with five of them at 1920x1088 were not reliable at M = 16, see profiles/light_ris.txt)."""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
mirt = importlib.import_module("cpu-raytracing-experiments_amd")

REPS = int(os.environ.get("LIGHT_RIS_REPS", "3"))
PARTS = os.environ.get("LIGHT_RIS_PARTS", "rate,equal_time").split(",")
MS = [int(m) for m in os.environ.get("LIGHT_RIS_MS", "4,8").split(",")]
RATE_MS = tuple(int(m) for m in os.environ.get("LIGHT_RIS_RATE_MS", "0,1,4,8,16").split(","))   # every M keeps a context of its own alive: few at a time

if "rate" in PARTS:
    for name, sc in (("default9", mirt.scene.default9()), ("S10000", mirt.scene.synthetic(10000))):
        w, h, spp, ms = 1920, 1088, 64, RATE_MS
        rs = {m: mirt.Renderer(sc, max_bounces=9, use_bvh=True, profile=True, light_ris=m) for m in ms}
        stats = {m: {"rays": 0, "shadow_rays": 0, "s": 0.0, "shade_ms": 0.0, "trace_ms": 0.0} for m in ms}
        for r in rs.values():
            r.Resize(w, h); r.Accumulate(spp)
        for _ in range(REPS):
            for m, r in rs.items():
                r.ResetAccumulator(); r.kernel_times(reset=True)
                c0 = r.counters()
                t0 = time.perf_counter(); r.Accumulate(spp); dt = time.perf_counter() - t0
                c1 = r.counters(); kt = r.kernel_times(reset=True)
                st = stats[m]
                st["rays"] += c1["rays"] - c0["rays"]; st["shadow_rays"] += c1["shadow_rays"] - c0["shadow_rays"]; st["s"] += dt
                st["shade_ms"] += kt["shade"]["ms"]; st["trace_ms"] += kt["trace"]["ms"]
        for m, st in stats.items():
            print(json.dumps({"part": "rate", "scene": name, "size": f"{w}x{h}", "spp": spp, "candidates": m, "batches": REPS,
                              "rays_per_batch": st["rays"] // REPS, "shadow_rays_per_batch": st["shadow_rays"] // REPS,
                              "mray_per_s": round(st["rays"] / st["s"] / 1e6, 1), "ms_per_batch": round(1e3 * st["s"] / REPS, 2),
                              "k_shade_ms_per_batch": round(st["shade_ms"] / REPS, 2), "k_trace_ms_per_batch": round(st["trace_ms"] / REPS, 2)}), flush=True)
        for r in rs.values():
            r.close()

if "equal_time" in PARTS:
    import views_and_scales as vs
    cloud = vs.VIEWS["compound"].make(mirt)
    for name, sc, w, h in (("cloud37", cloud, 512, 384), ("S10000", mirt.scene.synthetic(10000), 960, 544)):
        # the target is what the plain draw reaches in 1024 accumulations: its own 0.95-quantile there
        r = mirt.Renderer(sc, max_bounces=9, buckets=16, use_bvh=True)
        r.Resize(w, h); r.Accumulate(1024)
        target = float(mirt.noise_quantile(r.noise()["hist"], 0.95))
        r.close()
        for m in [0] + MS:
            r = mirt.Renderer(sc, max_bounces=9, buckets=16, use_bvh=True, light_ris=m)
            r.Resize(w, h); r.Accumulate(16); r.ResetAccumulator(); r.Synchronize()      # warm-up
            t0 = time.perf_counter()
            out = r.accumulate_until(target, quantile=0.95, check_every=64, max_accumulations=8192)
            dt = time.perf_counter() - t0
            print(json.dumps({"part": "equal_time", "scene": name, "size": f"{w}x{h}", "target": round(target, 5), "candidates": m, "seconds": round(dt, 3),
                              "accumulations": r.accumulations, "converged": bool(out["converged"]), "noise_mean": float(out.get("mean", float("nan"))),
                              "shadow_rays": r.counters()["shadow_rays"], "rays": r.counters()["rays"]}), flush=True)
            r.close()
