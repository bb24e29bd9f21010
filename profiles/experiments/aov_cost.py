"""What the first-hit AOVs cost at BASELINE cfg4's shape: 4096 x 4096, S(100 000), max_bounces = 9, one 63-accumulation batch per step
(streams = 1, max_batch = 63, as bench.py runs it), rendered three ways:
  (a) the parent commit          --parent-root DIR: a built checkout of it (its libmirt.so in place); skipped when not given
  (b) this tree, AOVs off
  (c) this tree, AOVs on
Every measurement is a fresh child process (two builds of libmirt.so do not share one); the variants alternate a, b, c, a, b, c, ...
over --rounds rounds, each child warming up one step and timing --steps steps with a host clock around Accumulate(63), which ends in a
device synchronise.  A fourth child runs (b) and (c) under policy.profile for the HIP-event time of the MIRT_K_RESOLVE class: with AOVs
off it holds k_merge_contrib alone, with AOVs on k_merge_contrib + k_first_hit_aov.
    python profiles/experiments/aov_cost.py [--parent-root DIR] [--rounds 3] [--steps 3] [--out profiles/aov.txt]
    python profiles/experiments/aov_cost.py --child on|off|profile [--root DIR]     (one measurement; prints a JSON line)"""
import argparse, importlib, json, os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SPP = 63


def renderer(mirt, aov, profile=False):
    cfg = mirt.scene.CONFIGS["cfg4"]
    sc = mirt.scene.synthetic(cfg["n"], ambient=cfg["ambient"])
    kw = {"aov": True} if aov else {}                     # (the parent commit has no such argument)
    r = mirt.Renderer(sc, max_bounces=cfg["max_bounces"], buckets=cfg["buckets"], use_bvh=True, streams=1, max_batch=SPP, profile=profile, **kw)
    r.Resize(cfg["width"], cfg["height"])
    assert r.get_policy()["max_batch"] == SPP
    return r


def child(args):
    sys.path.insert(0, args.root)
    mirt = importlib.import_module("cpu-raytracing-experiments_amd")
    if args.child == "profile":
        out = {}
        for aov in (False, True):
            r = renderer(mirt, aov, profile=True)
            r.Accumulate(SPP); r.kernel_times(reset=True)
            for _ in range(args.steps): r.Accumulate(SPP)
            t = r.kernel_times()
            out["on" if aov else "off"] = {k: {"ms_per_step": v["ms"] / args.steps, "launches_per_step": v["launches"] / args.steps} for k, v in t.items()}
            r.close()
        print(json.dumps(out), flush=True)
        return
    r = renderer(mirt, args.child == "on")
    r.Accumulate(SPP)
    ms = []
    for _ in range(args.steps):
        t0 = time.perf_counter(); r.Accumulate(SPP); ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"ms": ms, "rays_per_step": r.counters()["rays"] // (args.steps + 1)}), flush=True)
    r.close()


def run_child(kind, root, steps):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--root", root, "--steps", str(steps)]
    res = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600)
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["on", "off", "profile"])
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        return child(args)
    variants = [("b", "this tree, AOVs off", "off", ROOT), ("c", "this tree, AOVs on", "on", ROOT)]
    if args.parent_root:
        variants.insert(0, ("a", "parent commit", "off", os.path.abspath(args.parent_root)))
    ms = {v[0]: [] for v in variants}
    rays = {}
    for rnd in range(args.rounds):
        for key, _, kind, root in variants:
            res = run_child(kind, root, args.steps)
            ms[key] += res["ms"]; rays[key] = res["rays_per_step"]
            print(f"round {rnd} ({key}): " + " ".join(f"{m:8.2f}" for m in res["ms"]), flush=True)
    lines = [f"cfg4 shape: 4096 x 4096, S(100000), max_bounces 9, streams 1, one batch of {SPP} accumulations per step; {args.rounds} rounds x {args.steps} timed steps per variant,",
             "variants alternating, a fresh process and one warm-up step per measurement; host clock around Accumulate(63), which ends in a device synchronise", ""]
    for key, label, _, _ in variants:
        v = ms[key]
        lines.append(f"({key}) {label:22s} median {statistics.median(v):8.2f} ms per step   min {min(v):8.2f}   max {max(v):8.2f}   stdev {statistics.pstdev(v):6.2f}   "
                     f"({rays[key] / statistics.median(v) / 1e3:6.0f} Mray/s, {rays[key]} rays per step)")
    med = {k: statistics.median(v) for k, v in ms.items()}
    if "a" in med:
        lines.append(f"(b) / (a) = {med['b'] / med['a']:.4f}")
    lines.append(f"(c) / (b) = {med['c'] / med['b']:.4f}   (c) - (b) = {med['c'] - med['b']:.2f} ms per step")
    prof = run_child("profile", ROOT, args.steps)
    lines += ["", "HIP-event time per kernel class and step under policy.profile (ms; launches per step):"]
    for key in ("off", "on"):
        lines.append(f"  AOVs {key:3s} " + "   ".join(f"{k} {v['ms_per_step']:.2f} ({v['launches_per_step']:.0f})" for k, v in prof[key].items() if v["launches_per_step"]))
    lines.append(f"  MIRT_K_RESOLVE on - off = k_first_hit_aov: {prof['on']['resolve']['ms_per_step'] - prof['off']['resolve']['ms_per_step']:.2f} ms per step "
                 f"(the class also holds k_merge_contrib: {prof['off']['resolve']['ms_per_step']:.2f} ms)")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
