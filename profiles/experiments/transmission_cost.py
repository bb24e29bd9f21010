"""What mirt_set_transmission costs in k_shade at BASELINE cfg2's shape: 1024 x 1024, S(1000), max_bounces = 5, 64 accumulations per step, three ways:
  (a) switch off
  (b) switch on, no transmissive material        must launch the kernels of (a): equal within run-to-run noise
  (c) switch on, glass on 4 of the 17 materials   default9's two glass materials (transmission 0.95 / IOR - 1 = 0.44; 0.670, 0.764, 0.855 / 0.762), twice each
Every measurement is a fresh child process: one warm-up step, then --steps steps under policy.profile for the HIP-event time of the shade and
trace classes per step, and the host clock around Accumulate(64).
    python profiles/experiments/transmission_cost.py [--rounds 3] [--steps 3] [--out FILE]
    python profiles/experiments/transmission_cost.py --child a|b|c        (one measurement; prints a JSON line)"""
import argparse, importlib, json, os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SPP = 64
VARIANTS = {"a": "switch off", "b": "switch on, no transmissive material", "c": "switch on, 4 of 17 materials glass"}


def child(args):
    sys.path.insert(0, ROOT)
    mirt = importlib.import_module("cpu-raytracing-experiments_amd")
    cfg = mirt.scene.CONFIGS["cfg2"]
    sc = mirt.scene.synthetic(cfg["n"], ambient=cfg["ambient"])
    sc.material["transmission"] = 0
    if args.child == "c":
        for m, (t, ior) in zip((1, 5, 9, 13), (((0.95, 0.95, 0.95), 0.44), ((0.670, 0.764, 0.855), 0.762)) * 2):
            sc.material["transmission"][m] = t
            sc.material["IOR_minus_one"][m] = ior
    r = mirt.Renderer(sc, max_bounces=cfg["max_bounces"], buckets=cfg["buckets"], use_bvh=True, profile=True, transmission=args.child != "a")
    r.Resize(cfg["width"], cfg["height"])
    r.Accumulate(SPP); r.kernel_times(reset=True)
    ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter(); r.Accumulate(SPP); ms.append((time.perf_counter() - t0) * 1e3)
    out = {"ms": ms, "classes": {k: v["ms"] / args.steps for k, v in r.kernel_times().items() if v["launches"]}, "rays_per_step": r.counters()["rays"] // (args.steps + 1)}
    r.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=list(VARIANTS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = {k: [] for k in VARIANTS}
    for rnd in range(args.rounds):
        for key in VARIANTS:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", key, "--steps", str(args.steps)]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
            res[key].append(json.loads(out.stdout.strip().splitlines()[-1]))
    lines = [f"cfg2 shape: 1024 x 1024, S(1000), max_bounces 5, {SPP} accumulations per step; {args.rounds} rounds x {args.steps} timed steps per variant, variants alternating,",
             "a fresh process and one warm-up step per measurement; shade / trace: HIP-event time per step (policy.profile), median over the rounds (min-max)", "",
             "| variant | shade ms per step | trace ms per step | host ms per step (profiled) | rays per step |", "|---|---|---|---|---|"]
    for key, label in VARIANTS.items():
        sh = [r["classes"].get("shade", 0.0) for r in res[key]]
        tr = [r["classes"].get("trace", 0.0) for r in res[key]]
        ms = [m for r in res[key] for m in r["ms"]]
        lines.append(f"| ({key}) {label} | {statistics.median(sh):.3f} ({min(sh):.3f}-{max(sh):.3f}) | {statistics.median(tr):.3f} ({min(tr):.3f}-{max(tr):.3f}) | "
                     f"{statistics.median(ms):.2f} ({min(ms):.2f}-{max(ms):.2f}) | {res[key][-1]['rays_per_step']} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
