"""What the MIXED kernels of mirt_set_material_closures cost: BRDF_test and default9 at 1920 x 1088, 64 accumulations per step, max_bounces 16, three ways:
  (0) every material Lambertian   the kernels of policy.brdf = 0
  (1) every material GGX          the kernels of policy.brdf = 1
  (h) half the materials each     closure[m] = m % 2: the MIXED kernels — a wave with hits of both kinds runs both branches
No target is set: the divergence cost is a number nobody has measured.  Every measurement is a fresh child process: one warm-up step, then
--steps steps under policy.profile for the HIP-event time of the shade and trace classes per step, and the host clock around Accumulate(64);
Mray/s is rays per step over the host time.  The three ways trace different rays (another closure, other directions), so rays per second is what
is compared, beside k_shade's milliseconds.
    python profiles/experiments/mixed_closures_cost.py [--rounds 3] [--steps 3] [--out FILE]
    python profiles/experiments/mixed_closures_cost.py --child default9:h        (one measurement; prints a JSON line)"""
import argparse, importlib, json, os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
W, H, SPP = 1920, 1088, 64
SCENES = ("brdf_test", "default9")
WAYS = {"0": "every material Lambertian", "1": "every material GGX", "h": "half the materials each (MIXED)"}
DECAY = [0.0, 0.1, 0.3, 0.6, 1.0]


def child(args):
    sys.path.insert(0, ROOT)
    mirt = importlib.import_module("cpu-raytracing-experiments_amd")
    scene_name, way = args.child.split(":")
    sc = getattr(mirt.scene, scene_name)()
    n = len(sc.material)
    table = {"0": [0] * n, "1": [1] * n, "h": [m % 2 for m in range(n)]}[way]
    r = mirt.Renderer(sc, max_bounces=16, use_bvh=True, profile=True, gloss_decay=DECAY, material_closures=table)
    assert r.material_closures()[1] == (way == "h")
    r.Resize(W, H)
    r.Accumulate(SPP); r.kernel_times(reset=True)
    rays0 = r.counters()["rays"]
    ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter(); r.Accumulate(SPP); ms.append((time.perf_counter() - t0) * 1e3)
    out = {"ms": ms, "classes": {k: v["ms"] / args.steps for k, v in r.kernel_times().items() if v["launches"]}, "rays_per_step": (r.counters()["rays"] - rays0) // args.steps}
    r.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        return child(args)
    keys = [f"{s}:{w}" for s in SCENES for w in WAYS]
    res = {k: [] for k in keys}
    for rnd in range(args.rounds):
        for key in keys:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", key, "--steps", str(args.steps)]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
            res[key].append(json.loads(out.stdout.strip().splitlines()[-1]))
    lines = [f"{W} x {H}, max_bounces 16, {SPP} accumulations per step; {args.rounds} rounds x {args.steps} timed steps per variant, variants alternating, a fresh process and one",
             "warm-up step per measurement; shade / trace: HIP-event time per step (policy.profile), median over the rounds (min-max); Mray/s from the host clock", "",
             "| scene | closures | Mray/s | shade ms per step | trace ms per step | host ms per step (profiled) | rays per step |", "|---|---|---|---|---|---|---|"]
    for key in keys:
        scene_name, way = key.split(":")
        sh = [r["classes"].get("shade", 0.0) for r in res[key]]
        tr = [r["classes"].get("trace", 0.0) for r in res[key]]
        ms = [m for r in res[key] for m in r["ms"]]
        rays = res[key][-1]["rays_per_step"]
        rate = [r["rays_per_step"] / (m * 1e3) for r in res[key] for m in r["ms"]]
        lines.append(f"| {scene_name} | ({way}) {WAYS[way]} | {statistics.median(rate):.0f} ({min(rate):.0f}-{max(rate):.0f}) | {statistics.median(sh):.3f} ({min(sh):.3f}-{max(sh):.3f}) | "
                     f"{statistics.median(tr):.3f} ({min(tr):.3f}-{max(tr):.3f}) | {statistics.median(ms):.2f} ({min(ms):.2f}-{max(ms):.2f}) | {rays} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
