"""What mirt_set_sky_sampling costs and what it buys.
  build   the table build (mirt_set_scene with the switch on, minus the same call with it off) for 1 x 1, 2048 x 1024 and 4096 x 2048 maps
  cost    BASELINE cfg2's shape (1024 x 1024, S(1000), max_bounces 5, 64 accumulations per step) under a 65 x 33 sun map with ambient 1:
          (a) switch off, (b) switch on — HIP-event time of the shade and trace classes per step, host clock around Accumulate(64)
  noise   a Lambert ball on a Lambert ground ball under the sun map (tests/test_sky_sampling_gpu.py's scene), 64 x 64 x 80, 16 buckets:
          the mean of mirt_noise with the switch off and on, and their ratio
Every measurement is a fresh child process.
    python profiles/experiments/sky_sampling.py [--rounds 3] [--steps 3] [--out FILE]
    python profiles/experiments/sky_sampling.py --child build|a|b|noise        (one measurement; prints a JSON line)"""
import argparse, importlib, json, os, statistics, subprocess, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SPP = 64


def sun_map(w=65, h=33, sun=(6, 40), power=1e4):
    m = np.ones((h, w, 4), dtype=np.float32)
    m[sun[0], sun[1], :3] = power
    return m


def child(args):
    sys.path.insert(0, ROOT)
    mirt = importlib.import_module("cpu-raytracing-experiments_amd")
    S = mirt.scene
    if args.child == "build":
        out = {}
        for w, h in ((1, 1), (2048, 1024), (4096, 2048)):
            sc = S.default9(); sc.ambient = np.ones(3, dtype=np.float32)
            sc.hdri = sun_map(w, h, sun=(h // 4, w // 3)) if w > 1 else np.ones((1, 1, 4), dtype=np.float32)
            ms = {}
            for on in (False, True):
                r = mirt.Renderer(sc, sky_sampling=on)
                t = []
                for _ in range(4):
                    t0 = time.perf_counter(); r.UpdateScene(); t.append((time.perf_counter() - t0) * 1e3)
                ms[on] = min(t[1:])
                r.close()
            out[f"{w}x{h}"] = {"set_scene_off_ms": ms[False], "set_scene_on_ms": ms[True], "build_ms": ms[True] - ms[False]}
        print(json.dumps(out), flush=True)
        return
    if args.child == "noise":
        geo = [S._sphere((0, -100.0, 0), 100.0 ** 2, 0), S._sphere((0, 0.5, 0), 0.25, 1)]
        mat = [S._material(albedo=(0.7, 0.7, 0.7)), S._material(albedo=(0.8, 0.3, 0.2))]
        cam = S.Camera(eye=(0.0, 1.2, 4.0), direction=(0.0, -0.2, -1.0), focal_length=35.0, exposure=1.0)
        sc = S.Scene(np.array(geo, dtype=S.SPHERE), np.array(mat, dtype=S.MATERIAL), cam, np.ones(3, dtype=np.float32), name="sun")
        sc.hdri = sun_map()
        out = {}
        for on in (False, True):
            r = mirt.Renderer(sc, max_bounces=6, buckets=16, use_bvh=True, sky_sampling=on)
            r.Resize(64, 64); r.Accumulate(80)
            out["on" if on else "off"] = float(r.noise()["mean"])
            r.close()
        out["ratio_on_over_off"] = out["on"] / out["off"]
        print(json.dumps(out), flush=True)
        return
    cfg = S.CONFIGS["cfg2"]
    sc = S.synthetic(cfg["n"], ambient=1.0)
    sc.hdri = sun_map()
    r = mirt.Renderer(sc, max_bounces=cfg["max_bounces"], buckets=cfg["buckets"], use_bvh=True, profile=True, sky_sampling=args.child == "b")
    r.Resize(cfg["width"], cfg["height"])
    r.Accumulate(SPP); r.kernel_times(reset=True)
    ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter(); r.Accumulate(SPP); ms.append((time.perf_counter() - t0) * 1e3)
    c = r.counters()
    out = {"ms": ms, "classes": {k: v["ms"] / args.steps for k, v in r.kernel_times().items() if v["launches"]},
           "rays_per_step": c["rays"] // (args.steps + 1), "shadow_rays_per_step": c["shadow_rays"] // (args.steps + 1)}
    r.close()
    print(json.dumps(out), flush=True)


def run_child(key, steps):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", key, "--steps", str(steps)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["build", "a", "b", "noise"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = ["table build: mirt_set_scene (default9, host-built tree) with the switch on minus the same call with it off, best of 3 after a first call, ms", ""]
    for k, v in run_child("build", args.steps).items():
        lines.append(f"  {k}: off {v['set_scene_off_ms']:.2f}  on {v['set_scene_on_ms']:.2f}  build {v['build_ms']:.2f}")
    res = {"a": [], "b": []}
    for _ in range(args.rounds):
        for key in res:
            res[key].append(run_child(key, args.steps))
    lines += ["", f"cfg2 shape under a 65 x 33 sun map, ambient 1: {args.rounds} rounds x {args.steps} timed steps per variant, alternating, a fresh process and one warm-up step each;",
              "shade / trace: HIP-event time per step (policy.profile), median over the rounds (min-max)", "",
              "| variant | shade ms per step | trace ms per step | host ms per step (profiled) | rays per step | shadow rays per step |", "|---|---|---|---|---|---|"]
    for key, label in (("a", "switch off"), ("b", "switch on")):
        sh = [r["classes"].get("shade", 0.0) for r in res[key]]
        tr = [r["classes"].get("trace", 0.0) for r in res[key]]
        ms = [m for r in res[key] for m in r["ms"]]
        lines.append(f"| ({key}) {label} | {statistics.median(sh):.3f} ({min(sh):.3f}-{max(sh):.3f}) | {statistics.median(tr):.3f} ({min(tr):.3f}-{max(tr):.3f}) | "
                     f"{statistics.median(ms):.2f} ({min(ms):.2f}-{max(ms):.2f}) | {res[key][-1]['rays_per_step']} | {res[key][-1]['shadow_rays_per_step']} |")
    nz = run_child("noise", args.steps)
    lines += ["", f"noise (ball on a ground ball under the sun map, 64 x 64 x 80, 16 buckets): mean of mirt_noise off {nz['off']:.4f}, on {nz['on']:.4f}, on / off {nz['ratio_on_over_off']:.3f}"]
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
