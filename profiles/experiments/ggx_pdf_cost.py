"""mirt_set_ggx_pdf: what the switch costs in k_shade and what it buys in noise.  For each scene, 1920 x 1088 x 64 accumulations (8 buckets), the
switch off against on: k_shade milliseconds per launch from HIP events (policy.profile), the counters, and the 0.95 quantile of mirt_noise's
per-pixel relative standard error at equal accumulations.  Prints one line a run and one summary line a scene; profiles/ggx_pdf.txt keeps a copy.
    python profiles/experiments/ggx_pdf_cost.py [--size WxH] [--spp N]"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
mirt = importlib.import_module("cpu-raytracing-experiments_amd")

DECAY = [0.0, 0.1, 0.3, 0.6, 1.0]


def lit_default9():
    """default9 under a small environment map with one bright cell: a sun for sky sampling to find."""
    sc = mirt.scene.default9()
    hdri = np.full((5, 9, 4), 0.05, dtype=np.float32); hdri[..., 3] = 1.0
    hdri[1, 6, :3] = (40.0, 35.0, 30.0)
    sc.hdri, sc.ambient = hdri, np.full(3, 0.5, dtype=np.float32)
    return sc


SCENES = {
    "brdf_test, brdf 1": (mirt.scene.brdf_test, dict(brdf=1)),
    "default9, brdf 1": (mirt.scene.default9, dict(brdf=1)),
    "default9 + sun map, mixed closures, sky sampling": (lit_default9, dict(material_closures=[1, 0, 1, 0, 1, 0, 1, 0, 1], sky_sampling=True)),
}


def run(sc, w, h, spp, on, **kw):
    r = mirt.Renderer(sc, max_bounces=16, buckets=8, use_bvh=True, gloss_decay=DECAY, profile=True, ggx_pdf=on, **kw)
    r.Resize(w, h)
    r.Accumulate(8); r.ResetAccumulator(); r.kernel_times()                        # warm-up: allocations, candidate lists, first launches
    r.Accumulate(spp)
    t, c, n = r.kernel_times(), r.counters(), r.noise()
    out = dict(shade_ms=t["shade"]["ms"], shade_launches=t["shade"]["launches"], trace_ms=t["trace"]["ms"], q95=mirt.noise_quantile(n["hist"], 0.95), noise_mean=n["mean"],
               nonfinite=n["nonfinite_pixels"], rays=c["rays"], shadow_rays=c["shadow_rays"], terminated=c["terminated"], dropped=c["dropped"])
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1088"); ap.add_argument("--spp", type=int, default=64)
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    for name, (make, kw) in SCENES.items():
        res = {}
        for on in (False, True):
            res[on] = run(make(), w, h, a.spp, on, **kw)
            print(f"{name} | ggx_pdf {int(on)} | " + " ".join(f"{k}={v:.6g}" if isinstance(v, float) else f"{k}={v}" for k, v in res[on].items()), flush=True)
        off, on = res[False], res[True]
        same = all(off[k] == on[k] for k in ("rays", "terminated", "dropped"))
        print(f"{name} | k_shade ms/launch {off['shade_ms'] / off['shade_launches']:.4f} -> {on['shade_ms'] / on['shade_launches']:.4f} "
              f"(x{on['shade_ms'] / off['shade_ms']:.3f}) | noise q95 {off['q95']:.4g} -> {on['q95']:.4g} (x{on['q95'] / off['q95']:.3f}) | "
              f"rays/terminated/dropped equal: {same} | shadow_rays {off['shadow_rays']} -> {on['shadow_rays']}", flush=True)


if __name__ == "__main__":
    main()
