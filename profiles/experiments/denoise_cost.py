"""What the denoised resolve costs per à-trous pass: default9 at 1920 x 1088 and 4096 x 4096, 5 buckets, AOVs on, 5 accumulations, policy.profile.
render_denoised(iterations = i) is run for i = 0 .. 5, --repeats times each, the MIRT_K_RESOLVE timer read and reset after every call; the time of
pass i (step 2^(i-1)) is the median total at i minus the median total at i - 1, and i = 0 is k_denoise_prepare + k_denoise_finish.  A pass reads
32 B and writes 16 B of unique HBM traffic per pixel (x and v, the guides; x and v out); the fraction is of the 8 TB/s datasheet peak.
Both launch choices are measured in one process: MIRT_TUNE_DENOISE_STAGED = 2 (steps 1 and 2 stage block and halo in LDS; the default) and 0 (every
pass reads its taps straight from global memory) — read at mirt_create, so each gets a renderer of its own.
    python profiles/experiments/denoise_cost.py [--repeats 3] [--out FILE]"""
import argparse, importlib, os, statistics, sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    mirt = importlib.import_module("cpu-raytracing-experiments_amd")
    lines = []
    frames = {}
    for w, h in ((1920, 1088), (4096, 4096)):
        pixels = w * h
        for staged in (2, 0):
            os.environ["MIRT_TUNE_DENOISE_STAGED"] = str(staged)
            r = mirt.Renderer(mirt.scene.default9(), buckets=5, use_bvh=True, aov=True, profile=True)
            r.Resize(w, h)
            r.Accumulate(5)
            r.kernel_times(reset=True)
            total = []
            for i in range(6):
                ms = []
                for _ in range(args.repeats):
                    frame = r.render_denoised(iterations=i)
                    t = r.kernel_times(reset=True)["resolve"]
                    assert frame is not None and t["launches"] == i + 2
                    ms.append(t["ms"])
                total.append(statistics.median(ms))
            frames[(w, h, staged)] = frame
            r.close()
            lines.append(f"{w} x {h}, steps <= {staged} staged in LDS: prepare + finish {total[0]:.3f} ms; per pass (ms, unique bytes over time, fraction of 8 TB/s):")
            for i in range(1, 6):
                dt = total[i] - total[i - 1]
                lines.append(f"    step {1 << (i - 1):2d} ({'LDS' if (1 << (i - 1)) <= staged else 'direct'}): {dt:7.3f} ms   {pixels * 48 / dt / 1e9:7.2f} TB/s   {pixels * 48 / (dt * 1e-3) / HBM_PEAK:6.1%}")
            lines.append(f"    five passes with prepare and finish: {total[5]:.3f} ms")
        same = (frames[(w, h, 2)].view("uint32") == frames[(w, h, 0)].view("uint32")).all()
        lines.append(f"    the two launch choices give the same words: {bool(same)}")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
