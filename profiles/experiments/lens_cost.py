"""What the thin lens costs at BASELINE cfg4's shape: 4096 x 4096, S(100 000), max_bounces = 9, one 63-accumulation batch per step
(streams = 1, max_batch = 63, as bench.py runs it), rendered four ways:
  (a) lens off                                   camera rays through the per-pixel candidate lists
  (b) lens off, trace_primary_rays = 1           every camera ray walks the tree: THE BASELINE FOR THE LENS (a lens takes this route)
  (c) lens on, focused at mid-field              A = 0.05, focus_depth = the pick at the image centre
  (d) lens on, strongly defocused                A = 0.5,  focus_depth = a tenth of that
Every measurement is a fresh child process: one warm-up step, --steps steps timed with a host clock around Accumulate(63) (which ends in a
device synchronise), then the same steps under policy.profile for the HIP-event time of the trace and shade classes (all bounces; only the
bounce-0 launches differ between the variants), then ONE accumulation with max_bounces = 1 under count_traffic: that batch is its camera rays
alone, so nodes / rays = boxes per camera ray ((a): the cone traversals and list tests of a one-accumulation batch, which builds no lists).
    python profiles/experiments/lens_cost.py [--rounds 2] [--steps 3] [--out profiles/lens_cost.txt]
    python profiles/experiments/lens_cost.py --child a|b|c|d        (one measurement; prints a JSON line)"""
import argparse, importlib, json, os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SPP = 63
VARIANTS = {"a": ("lens off", {}, None), "b": ("lens off, trace_primary_rays = 1", {"trace_primary_rays": True}, None),
            "c": ("lens on, focused at mid-field", {}, (0.05, 1.0)), "d": ("lens on, strongly defocused", {}, (0.5, 0.1))}


def renderer(mirt, key, **more):
    cfg = mirt.scene.CONFIGS["cfg4"]
    sc = mirt.scene.synthetic(cfg["n"], ambient=cfg["ambient"])
    kw = dict(max_bounces=cfg["max_bounces"], buckets=cfg["buckets"], use_bvh=True, streams=1, max_batch=SPP)
    kw.update(VARIANTS[key][1]); kw.update(more)
    r = mirt.Renderer(sc, **kw)
    r.Resize(cfg["width"], cfg["height"])
    lens = VARIANTS[key][2]
    if lens:
        _, depth = r.pick_focus(cfg["width"] // 2, cfg["height"] // 2)
        r.set_lens(lens[0], depth * lens[1])
    return r


def child(args):
    sys.path.insert(0, ROOT)
    mirt = importlib.import_module("cpu-raytracing-experiments_amd")
    r = renderer(mirt, args.child)
    r.Accumulate(SPP)
    ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter(); r.Accumulate(SPP); ms.append((time.perf_counter() - t0) * 1e3)
    out = {"ms": ms, "rays_per_step": r.counters()["rays"] // (args.steps + 1), "lens": r.lens()}
    r.close()
    r = renderer(mirt, args.child, profile=True)
    r.Accumulate(SPP); r.kernel_times(reset=True)
    for _ in range(args.steps): r.Accumulate(SPP)
    out["classes"] = {k: v["ms"] / args.steps for k, v in r.kernel_times().items() if v["launches"]}
    r.close()
    r = renderer(mirt, args.child, count_traffic=True, max_bounces=1)
    r.Accumulate(1)
    c = r.counters()
    out["boxes_per_camera_ray"] = c["nodes"] / c["rays"]; out["spheres_per_camera_ray"] = c["spheres"] / c["rays"]
    r.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=list(VARIANTS))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = {k: [] for k in VARIANTS}
    for rnd in range(args.rounds):
        for key in VARIANTS:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", key, "--steps", str(args.steps)]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
            res[key].append(json.loads(out.stdout.strip().splitlines()[-1]))
            print(f"round {rnd} ({key}): " + " ".join(f"{m:8.2f}" for m in res[key][-1]["ms"]), flush=True)
    lines = [f"cfg4 shape: 4096 x 4096, S(100000), max_bounces 9, streams 1, one batch of {SPP} accumulations per step; {args.rounds} rounds x {args.steps} timed steps per variant,",
             "variants alternating, a fresh process and one warm-up step per measurement; host clock around Accumulate(63)", "",
             "| variant | ms per step (min-max) | Mray/s | trace ms | shade ms | boxes / camera ray | spheres / camera ray |", "|---|---|---|---|---|---|---|"]
    med = {}
    for key, (label, _, _) in VARIANTS.items():
        ms = [m for r in res[key] for m in r["ms"]]
        last = res[key][-1]
        med[key] = statistics.median(ms)
        lines.append(f"| ({key}) {label} | {med[key]:.2f} ({min(ms):.2f}-{max(ms):.2f}) | {last['rays_per_step'] / med[key] / 1e3:.0f} | {last['classes'].get('trace', 0):.2f} | "
                     f"{last['classes'].get('shade', 0):.2f} | {last['boxes_per_camera_ray']:.1f} | {last['spheres_per_camera_ray']:.2f} |")
    lines += ["", f"(b) / (a) = {med['b'] / med['a']:.4f}   (c) / (b) = {med['c'] / med['b']:.4f}   (d) / (b) = {med['d'] / med['b']:.4f}"]
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
