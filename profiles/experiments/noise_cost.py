"""What the noise estimate costs at BASELINE cfg4's shape: 4096 x 4096, S(100 000), max_bounces = 9, 5 buckets, one 65-accumulation step
under policy.profile.  k_noise and k_resolve read the same accumulator slab (4096^2 x 5 buckets x 3 channels x 4 B = 1.0 GB), so the
HIP-event time of k_resolve in the same process is the yardstick: after the step the MIRT_K_RESOLVE timer is reset and each of
    Render()                       k_resolve: slab in, 16 B per pixel out
    noise()                        k_noise: slab in, 16 B per tile and the histogram out
    noise(want_map=True)           k_noise: + 4 B per pixel out
is run --repeats times, the timer read and reset after every call.  Bytes over time counts the slab and what the kernel stores.
    python profiles/experiments/noise_cost.py [--repeats 5] [--config cfg4] [--out profiles/noise.txt]"""
import argparse, importlib, json, os, statistics, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SPP = 65


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    mirt = importlib.import_module("cpu-raytracing-experiments_amd")
    cfg = mirt.scene.CONFIGS[args.config]
    r = mirt.Renderer(mirt.scene.synthetic(cfg["n"], ambient=cfg["ambient"]), max_bounces=cfg["max_bounces"], buckets=cfg["buckets"], use_bvh=True, profile=True)
    r.Resize(cfg["width"], cfg["height"])
    t0 = time.perf_counter(); r.Accumulate(SPP); step_ms = (time.perf_counter() - t0) * 1e3
    step = r.kernel_times(reset=True)
    pixels = (cfg["width"] // 16) * (cfg["height"] // 16) * 256
    slab = pixels * cfg["buckets"] * 3 * 4
    calls = {"k_resolve (Render)": (lambda: r.Render(), slab + pixels * 16),
             "k_noise (stats, tiles, histogram)": (lambda: r.noise(floor=0.01), slab + pixels // 16 + 8192),
             "k_noise + map": (lambda: r.noise(floor=0.01, want_map=True), slab + pixels * 4 + pixels // 16 + 8192)}
    ms, wall = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(args.repeats):
        for name, (call, _) in calls.items():
            t0 = time.perf_counter(); assert call(); wall[name].append((time.perf_counter() - t0) * 1e3)
            t = r.kernel_times(reset=True)["resolve"]
            assert t["launches"] == 1
            ms[name].append(t["ms"])
    res = r.noise(floor=0.01)
    lines = [f"{args.config} shape: {cfg['width']} x {cfg['height']}, S({cfg['n']}), max_bounces {cfg['max_bounces']}, {cfg['buckets']} buckets; one step of {SPP} accumulations under policy.profile:",
             f"  step {step_ms:.1f} ms on the host clock; HIP-event ms per class: " + "  ".join(f"{k} {v['ms']:.1f}" for k, v in step.items() if v["launches"]),
             f"accumulator slab {slab / 1e9:.3f} GB; {args.repeats} repeats, HIP-event time of the one launch (median, min .. max) and bytes moved over the median:", ""]
    for name, (_, nbytes) in calls.items():
        v = ms[name]
        lines.append(f"  {name:36s} {statistics.median(v):7.3f} ms  ({min(v):.3f} .. {max(v):.3f})   {nbytes / statistics.median(v) / 1e9:6.2f} TB/s   "
                     f"call on the host clock, with the copy back: {statistics.median(wall[name]):8.1f} ms")
    lines.append(f"  k_noise / k_resolve = {statistics.median(ms['k_noise (stats, tiles, histogram)']) / statistics.median(ms['k_resolve (Render)']):.3f}   "
                 f"k_noise / step = {statistics.median(ms['k_noise (stats, tiles, histogram)']) / step_ms:.5f}")
    lines.append(f"  after {SPP} accumulations: max {res['max']:.4f}, mean {res['mean']:.4f}, 0.95-quantile <= {mirt.noise_quantile(res['hist'], 0.95):.4f}, "
                 f"{res['nonfinite_pixels']} non-finite of {res['owned_pixels']} pixels, {int((res['hist'] > 0).sum())} bins in use")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    r.close()


if __name__ == "__main__":
    main()
