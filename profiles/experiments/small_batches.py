"""Small batches on one stream: Accumulate(1) and Accumulate(5) per launch with streams=1, max_batch=5 (one batch in flight, no more
accumulations than buckets) at 1024x1024, S(1000), 5 bounces.  Every batch writes a contribution buffer and is merged."""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
mirt = importlib.import_module("cpu-raytracing-experiments_amd")
r = mirt.Renderer(mirt.scene.synthetic(1000, ambient=0.5), max_bounces=5, use_bvh=True, streams=1, max_batch=5); r.Resize(1024, 1024)
r.Accumulate(10)
for per_launch, launches in ((1, 200), (5, 80)):
    for rep in range(3):
        c0 = r.counters()["rays"]; t0 = time.perf_counter()
        for _ in range(launches): r.Accumulate(per_launch)
        dt = time.perf_counter() - t0
        print(f"Accumulate({per_launch}) x {launches}: {dt / launches * 1e3:6.3f} ms per launch, {(r.counters()['rays'] - c0) / dt / 1e6:7.0f} Mray/s", flush=True)
r.close()
