"""mirt_set_ggx_pdf on the GPU: the GGX closure's visible-normal pdf in the MIS weights.
 3  ggx_pdf at function level (debug_math fn 14);   4  the G1 frame — fails without the feature;   5  both weights at work: G2, and a low-roughness
 cap whose variance must fall;   6  the sampled sky;   7  exact invariants;   8  the interface.
The float64 side and the guards that make 4 - 6 tests are test_ggx_pdf_cpu.py's."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import ggx_pdf_definitions as gp
import test_definitions_cpu as cpu
import test_ggx_pdf_cpu as guards
from oracle_binding import bits
from test_definitions_cpu import (ggx_scene, g1_expectation, g_sampler, f_regions, region_stats, SIGMA, G1_ACC, G2_ACC, G2_REF, F_W, F_H, F_EYE, F_FOCAL,
                                  HIGH, DIFFUSE, G_DECAY, G_F0, GGX_EVAL_K, GGX_EVAL_REL, backend_image, guard_first_hits, report)
from test_definitions_gpu import GpuBackend

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
ERR_ARG, ERR_STATE = -1, -3
DECAY = [0.0, 0.1, 0.3, 0.6, 1.0]


class PdfBackend(GpuBackend):
    """GpuBackend whose renders run with the switch on (ggx_pdf=False: the plain backend's render, through the same code)."""
    name = "gpu_ggx_pdf"

    def render(self, sc, w, h, n_acc, max_bounces, buckets=5, mis=True, variant=0, ggx_pdf=True, **kw):
        r = self.mirt.Renderer(sc, max_bounces=max_bounces, buckets=buckets, mis=mis, ggx_pdf=ggx_pdf, **self.variants[variant][1], **kw)
        r.Resize(w, h); r.Accumulate(n_acc)
        frame = r.GetFrame().copy() if (n_acc % buckets == 0 and r.Render()) else None
        out = dict(acc=r.accumulator(), frame=frame, counters=r.counters())
        r.close()
        return out


@pytest.fixture(scope="module")
def be(mirt):
    b = PdfBackend(mirt)
    yield b
    b.close()


def same_words(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, what
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} words differ"


def gpu_run(mirt, sc, w, h, spp, keep=False, setup=None, accumulate=None, **kw):
    r = mirt.Renderer(sc, **{"max_bounces": 16, "use_bvh": True, "gloss_decay": DECAY, **kw})
    r.Resize(w, h)
    if setup:
        setup(r)
    (accumulate or (lambda q: q.Accumulate(spp)))(r)
    if keep:
        return r
    acc, c = r.accumulator(), r.counters()
    r.close()
    return acc, c


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def test_ggx_pdf_function(be):
    """debug_math fn 14 against definitions.ggx_vndf_pdf_of_direction in float64 on the same binary32 inputs (ggx_pdf_definitions.pdf_sweep): alpha
    from 0 to 1 with 0 and values whose square is below the 1e-5 floor, V and L from the normal down to cos = 1e-3, a quarter of the L inside the
    lobe.  L at or below the surface, V.z = 0 and V below it give exactly 0 — never NaN or inf — also at alpha = 0.  Bound per sample: the model
    check_ggx_eval applies to the D term of ggx_eval, GGX_EVAL_K / k + GGX_EVAL_REL with k the cancelling term of D from float64, carried over to
    G1 D / (4 V.z) (ggx_pdf_definitions: why it carries).  Measured: worst error / bound 0.37, at alpha = 3.5e-4 under the floor (k down to 1e-5)."""
    alpha, L, V, zero = gp.pdf_sweep()
    got = be.r.debug_math(14, be._rows(alpha, L, V), 1)[0].astype(f64)
    want, k = gp.pdf_reference(alpha, L, V)
    assert np.isfinite(got).all() and (got >= 0.0).all()
    assert (got[zero] == 0.0).all() and (want[zero] == 0.0).all()
    live = ~zero
    assert (want[live] > 0.0).all() and want.max() > 1e3 and (alpha[live] == 0.0).sum() >= 20 and ((alpha[live] > 0) & (alpha[live].astype(f64) ** 2 < 1e-5)).sum() >= 3
    rel = np.abs(got - want)[live] / want[live]
    bound = GGX_EVAL_K / k[live] + GGX_EVAL_REL
    ratio = rel / bound
    report("gpu/ggx_pdf_fn14", worst_over_bound=float(ratio.max()), at_alpha=float(alpha[live][ratio.argmax()]), smallest_k=float(k[live].min()), largest=float(want.max()))
    assert (rel <= bound).all(), f"ggx_pdf off by {ratio.max():.3g} x the bound"


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def g1_check(be, mirt, exp, variant, ggx_pdf):
    """check_ggx_direct with the expectation and the switch as arguments: regional means within SIGMA standard errors, shadow_rays = n exactly,
    rays and terminated within SIGMA of their Bernoulli sums."""
    regions = f_regions("F1_high")
    sc = ggx_scene(mirt, [HIGH])
    guard_first_hits(be, sc, 2)
    res = be.render(sc, F_W, F_H, G1_ACC, max_bounces=2, variant=variant, brdf=1, ggx_pdf=ggx_pdf)
    img = backend_image(res, G1_ACC)
    n, zs = F_W * F_H * G1_ACC, {}
    for label, mask in regions.items():
        want, se = region_stats(exp, mask, G1_ACC)
        assert (want > 0).all() and (se / want < 0.01).all(), (label, se / want)
        zs[label] = [float(v) for v in (img[mask].mean(axis=0) - want) / se]
    c = res["counters"]
    z_rays = (c["rays"] - n - G1_ACC * exp["survive"].sum()) / math.sqrt(G1_ACC * (exp["survive"] * (1 - exp["survive"])).sum())
    z_term = (c["terminated"] - n + G1_ACC * exp["drop"].sum()) / math.sqrt(G1_ACC * (exp["drop"] * (1 - exp["drop"])).sum())
    report(f"{be.name}/G1/variant{variant}/ggx_pdf={ggx_pdf}", **{f"z_{k}": "/".join(f"{v:+.2f}" for v in z) for k, z in zs.items()},
           z_rays=float(z_rays), z_terminated=float(z_term), shadow_rays=c["shadow_rays"])
    for label, z in zs.items():
        assert max(abs(v) for v in z) <= SIGMA, f"G1/{label}: {z} sigma from the expectation"
    assert c["shadow_rays"] == n and (exp["shadow"] == 1.0).all()
    assert abs(z_rays) <= SIGMA and abs(z_term) <= SIGMA, (z_rays, z_term)
    return res


@pytest.mark.parametrize("variant", [0, 1])
def test_g1_frame_with_the_pdf(be, mirt, variant):
    """FAILS WITHOUT THE FEATURE.  ggx_scene([HIGH]), max_bounces = 2, brdf = 1, G1_ACC accumulations, switch on: the regional means meet
    g1_expectation(closure_pdf="vndf"), which lies 101 standard errors from today's estimator (test_ggx_pdf_cpu.test_gpu_test_guards).  At
    max_bounces = 2 a ray the closure sampled is dropped where it hits (Q5), so this frame reads the light sample's weight alone.  The same
    render with the switch off still meets g1_expectation(); the counters of the two are equal except shadow_rays, which is n in both."""
    on = g1_check(be, mirt, g1_expectation(closure_pdf="vndf"), variant, True)
    off = g1_check(be, mirt, g1_expectation(), variant, False)
    for name in ("rays", "terminated", "dropped"):
        assert on["counters"][name] == off["counters"][name], name
    assert (bits(on["acc"]) != bits(off["acc"])).any()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_g2_frame_with_the_pdf(be, mirt, variant):
    """check_ggx_bounces at max_bounces = 4 with the switch on, against g_sampler(..., closure_pdf="vndf"): HIGH plus DIFFUSE's sphere as a second GGX
    surface under the gloss-decay table — from bounce 1 on the emitter hit's weight is read too, with the pdf the ray brought along."""
    diffuse = [(DIFFUSE[0], DIFFUSE[1], (cpu.G_DIFFUSE_F0, cpu.G_DIFFUSE_ROUGH))]
    sc = ggx_scene(mirt, [HIGH], diffuse)
    guard_first_hits(be, sc, 4)
    ref = g_sampler([HIGH], diffuse, 4, G2_REF, 4343, decay=G_DECAY, closure_pdf="vndf")
    res = be.render(sc, F_W, F_H, G2_ACC, max_bounces=4, variant=variant, brdf=1, gloss_decay=G_DECAY)
    img = backend_image(res, G2_ACC)
    zs = {}
    for label, mask in f_regions("F1_high").items():
        k = mask.reshape(-1)
        se = np.sqrt(ref["var"][k].sum(axis=0) * (1.0 / G2_ACC + 1.0 / G2_REF)) / k.sum()
        zs[label] = [float(v) for v in (img[mask].mean(axis=0) - ref["E"][k].mean(axis=0)) / se]
    n, q = F_W * F_H * G2_ACC, ref["dropped"]
    sigma_term = math.sqrt(n * q * (1 - q) * (1.0 + G2_ACC / G2_REF))
    z_term = (res["counters"]["terminated"] - n * (1 - q)) / sigma_term if sigma_term > 0 else float(res["counters"]["terminated"] - n)
    report(f"{be.name}/G2/bounces4/variant{variant}", **{f"z_{k}": "/".join(f"{v:+.2f}" for v in z) for k, z in zs.items()}, dropped_share=q, z_terminated=float(z_term))
    for label, z in zs.items():
        assert max(abs(v) for v in z) <= SIGMA, f"G2/{label}: {z} sigma from the sampler"
    assert abs(z_term) <= SIGMA, z_term


def test_low_roughness_cap(be, mirt):
    """The cap at roughness 0.3 (alpha = 0.09) under HIGH, max_bounces = 3, 200 accumulations.  Chosen so that the float64 sampler's per-path
    variance falls by 9.0 from "zero" to "vndf" (the issue asks for at least 4; test_ggx_pdf_cpu.test_gpu_test_guards).  Regional means within SIGMA
    of the "vndf" sampler (its variance, both counts).  The image's per-pixel variance across buckets, straight from the accumulator
    (ggx_pdf_definitions.bucket_variance), must fall by at least the square root of the sampler's ratio — halfway in log, which leaves the bucket
    estimate (4 degrees of freedom a pixel, heavy-tailed with the switch off) its own spread.  Measured: off 0.0814, on 0.00863, a ratio of 9.4
    against the sampler's 9.0 and the 3.0 asked."""
    n_acc, buckets = guards.LOW_ACC, 5
    low = guards.low_samplers()
    ratio = float(low["zero"]["var"].mean() / low["vndf"]["var"].mean())
    assert ratio >= guards.LOW_ROUGH_RATIO
    sc = ggx_scene(mirt, [HIGH], rough=guards.LOW_ROUGH)
    guard_first_hits(be, sc, guards.LOW_BOUNCES)
    res = {on: be.render(sc, F_W, F_H, n_acc, max_bounces=guards.LOW_BOUNCES, buckets=buckets, variant=1, brdf=1, ggx_pdf=on) for on in (False, True)}
    img, ref, zs = backend_image(res[True], n_acc), low["vndf"], {}
    for label, mask in f_regions("F1_high").items():
        k = mask.reshape(-1)
        se = np.sqrt(ref["var"][k].sum(axis=0) * (1.0 / n_acc + 1.0 / guards.LOW_REF)) / k.sum()
        zs[label] = [float(v) for v in (img[mask].mean(axis=0) - ref["E"][k].mean(axis=0)) / se]
    var = {on: gp.bucket_variance(res[on]["acc"], n_acc, buckets) for on in res}
    report(f"{be.name}/low_roughness", **{f"z_{k}": "/".join(f"{v:+.2f}" for v in z) for k, z in zs.items()}, sampler_ratio=ratio,
           bucket_variance_off=var[False], bucket_variance_on=var[True], gpu_ratio=var[False] / var[True], asked=math.sqrt(ratio))
    for label, z in zs.items():
        assert max(abs(v) for v in z) <= SIGMA, f"low roughness/{label}: {z} sigma from the sampler"
    for name in ("rays", "terminated", "dropped"):
        assert res[True]["counters"][name] == res[False]["counters"][name], name
    assert var[True] * math.sqrt(ratio) <= var[False], (var, ratio)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
def sky_ball(mirt, hdri):
    """One GGX sphere, F0 = 1, roughness 0.3, in the F frame's near-normal view under an environment map with ambient 1."""
    S = mirt.scene
    geo = np.array([S._sphere((0, 0, 0), 1.0, 0)], dtype=S.SPHERE)
    mats = np.array([S._material(albedo=(0, 0, 0), F0=(1, 1, 1), roughness=0.3)], dtype=S.MATERIAL)
    cam = S.Camera(eye=(0.0, 0.0, F_EYE), direction=(0.0, 0.0, -1.0), focal_length=F_FOCAL, exposure=1.0)
    return S.Scene(geometry=geo, material=mats, camera=cam, ambient=np.ones(3, dtype=f32), hdri=hdri, name="sky_ball")


def sky_maps():
    white = np.ones((1, 1, 4), dtype=f32)
    sun = np.full((8, 16, 4), 0.05, dtype=f32); sun[..., 3] = 1.0
    sun[1, 4, :3] = (60.0, 50.0, 40.0)                                             # one bright cell high in the +z half, which the cap faces
    return {"white_1x1": white, "one_bright_cell_16x8": sun}


@pytest.mark.parametrize("which", ["white_1x1", "one_bright_cell_16x8"])
def test_sky(mirt, which):
    """A GGX ball (F0 = 1, roughness 0.3) under a map with ambient 1, sky_sampling = True, max_bounces = 6, 200 accumulations of 64 x 64, three
    renders: the plain path (sky_sampling off), sky sampling with the switch off, sky sampling with it on.  The switch-on image against the plain
    path: means over the whole frame and over its four quadrants within SIGMA of each other, the standard error from the bucket means of both
    renders.  Its per-pixel bucket variance must be below that of sky sampling with the switch off, where a ray the closure sampled carries
    nothing into the sky and every photon comes through the light sample.  The near-normal view is chosen on purpose: the reference's sampler
    departs from the visible-normal density (D7: turned axes, a clamp) only away from it, and is not detectable here (DESIGN.md section 2, rows G1
    and G3) — so p~ is the sampler's density to within what these counts can see, and the comparison tests the weights, not D7.
    Measured, bucket variance plain / sky sampling / sky sampling with the switch: 2.4e-4 / 1.05 / 1.9e-3 under the white map, 6.1e-7 / 3.2e-2 /
    1.2e-6 under the bright cell; the largest |z| against the plain path 1.23."""
    W = H = 64; n_acc, buckets = 200, 5
    sc = sky_ball(mirt, sky_maps()[which])
    res = {}
    for label, kw in (("plain", dict(sky_sampling=False)), ("sky", dict(sky_sampling=True)), ("sky_pdf", dict(sky_sampling=True, ggx_pdf=True))):
        res[label] = gpu_run(mirt, sc, W, H, n_acc, max_bounces=6, buckets=buckets, brdf=1, gloss_decay=None, **kw)
    tiles = np.arange((W // 16) * (H // 16))
    quadrant = ((tiles // 4 >= 2).astype(int) * 2 + (tiles % 4 >= 2).astype(int))
    zs = {}
    for label, sel in [("frame", np.ones(16 * 256, dtype=bool))] + [(f"quadrant{q}", np.repeat(quadrant == q, 256)) for q in range(4)]:
        m_on, se_on = gp.bucket_mean_and_se(res["sky_pdf"][0], n_acc, buckets, sel)
        m_pl, se_pl = gp.bucket_mean_and_se(res["plain"][0], n_acc, buckets, sel)
        zs[label] = (m_on - m_pl) / np.sqrt(se_on ** 2 + se_pl ** 2)
        assert (m_pl > 0).all()
    var = {k: gp.bucket_variance(v[0], n_acc, buckets) for k, v in res.items()}
    report(f"gpu/ggx_pdf_sky/{which}", **{f"z_{k}": "/".join(f"{v:+.2f}" for v in z) for k, z in zs.items()}, **{f"bucket_variance_{k}": v for k, v in var.items()})
    for label, z in zs.items():
        assert np.abs(z).max() <= SIGMA, (label, z)
    assert var["sky_pdf"] < var["sky"], var
    for name in ("rays", "terminated", "dropped"):
        assert res["sky_pdf"][1][name] == res["sky"][1][name] == res["plain"][1][name], name


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def lit_default9(mirt):
    """default9 under a small environment map with one bright cell, so that sky sampling changes the launches."""
    sc = mirt.scene.default9()
    hdri = np.full((5, 9, 4), 0.05, dtype=f32); hdri[..., 3] = 1.0
    hdri[1, 6, :3] = (40.0, 35.0, 30.0)
    sc.hdri, sc.ambient = hdri, np.full(3, 0.5, dtype=f32)
    return sc


MIXED_TABLE = [1, 0, 1, 0, 1, 0, 1, 0, 1]


def test_counters_do_not_move(mirt):
    """The closure sample and the roulette read nothing new: rays, terminated and dropped are equal with the switch on and off — on brdf_test
    160 x 96 x 10 with brdf = 1, and on default9 64 x 64 x 10 with a mixed closure table, transmission, sky sampling and light_ris = 4 all on.  The
    accumulators differ (the switch does something)."""
    cases = {"brdf_test": (mirt.scene.brdf_test(), 160, 96, dict(brdf=1)),
             "default9_everything": (lit_default9(mirt), 64, 64, dict(material_closures=MIXED_TABLE, transmission=True, sky_sampling=True, light_ris=4))}
    for label, (sc, w, h, kw) in cases.items():
        (a0, c0), (a1, c1) = gpu_run(mirt, sc, w, h, 10, **kw), gpu_run(mirt, sc, w, h, 10, ggx_pdf=True, **kw)
        for name in ("rays", "terminated", "dropped"):
            assert c0[name] == c1[name], f"{label}: {name} {c0[name]} off, {c1[name]} on"
        assert c0["rays"] > w * h * 10 and np.isfinite(a1).all()
        assert (bits(a0) != bits(a1)).any(), label
        report(f"gpu/ggx_pdf_counters/{label}", rays=c1["rays"], terminated=c1["terminated"], dropped=c1["dropped"], shadow_off=c0["shadow_rays"], shadow_on=c1["shadow_rays"])


def test_all_lambertian_is_the_same_launch(mirt):
    """With every material Lambertian the switch changes no launch: the accumulator is bit-identical on and off and mirt_get_kernel_times shows the
    same launch counts — under policy.brdf = 0, and under brdf = 1 with a table that makes every material Lambertian."""
    sc = lit_default9(mirt)
    n = len(sc.material)
    for kw in (dict(brdf=0), dict(brdf=1, material_closures=[0] * n), dict(brdf=0, sky_sampling=True, transmission=True)):
        out = {}
        for on in (False, True):
            r = gpu_run(mirt, sc, 64, 64, 10, keep=True, profile=True, ggx_pdf=on, **kw)
            assert r.ggx_pdf() is on
            out[on] = (r.accumulator(), {k: v["launches"] for k, v in r.kernel_times().items()})
            r.close()
        same_words(out[True][0], out[False][0], f"all Lambertian, {sorted(kw)}")
        assert out[True][1] == out[False][1] and sum(out[True][1].values()) > 0


def test_all_ggx_table_equals_brdf_1(mirt):
    sc = lit_default9(mirt)
    want = gpu_run(mirt, sc, 64, 64, 10, brdf=1, ggx_pdf=True)[0]
    got = gpu_run(mirt, sc, 64, 64, 10, brdf=0, material_closures=[1] * len(sc.material), ggx_pdf=True)[0]
    same_words(got, want, "a table that makes every material GGX, switch on, against brdf = 1, switch on")
    assert (bits(want) != bits(gpu_run(mirt, sc, 64, 64, 10, brdf=1)[0])).any()


@pytest.mark.parametrize("closures", ["brdf_1", "mixed"])
def test_words_do_not_depend_on_the_route(mirt, closures):
    """Switch on: max_batch, streams, use_bvh, trace_primary_rays, Accumulate against AccumulateAsync under a deferred setting change, a lens (tree
    against brute force and batch sizes under it), and a group of two members on one device against one context."""
    W, H, N = 48, 32, 10
    sc = lit_default9(mirt)
    fixed = dict(brdf=1) if closures == "brdf_1" else dict(material_closures=MIXED_TABLE, sky_sampling=True, transmission=True, light_ris=2)

    def run(**kw):
        return gpu_run(mirt, sc, W, H, N, **{"max_batch": 3, "buckets": 5, "ggx_pdf": True, **fixed, **kw})[0]

    base = run()
    assert (bits(base) != bits(run(ggx_pdf=False))).any()
    routes = {
        "max_batch 1": dict(max_batch=1), "max_batch 5": dict(max_batch=5), "max_batch 0": dict(max_batch=0), "streams 1": dict(streams=1), "streams 3": dict(streams=3),
        "10 x async(1)": dict(accumulate=lambda r: [r.AccumulateAsync(1) for _ in range(N)]),
        "brute force": dict(use_bvh=False), "traced camera rays": dict(trace_primary_rays=True),
        "set after construction": dict(ggx_pdf=False, setup=lambda r: r.set_ggx_pdf(True)),
    }
    for label, kw in routes.items():
        same_words(run(**kw), base, label)
    # a deferred call keeps the setting it was issued under
    r = gpu_run(mirt, sc, W, H, 0, keep=True, accumulate=lambda q: None, max_batch=16, streams=1, buckets=5, ggx_pdf=True, **fixed)
    r.AccumulateAsync(3); r.set_ggx_pdf(False); assert r.accumulations == 3
    r.AccumulateAsync(2); r.Synchronize()
    q = gpu_run(mirt, sc, W, H, 3, keep=True, max_batch=16, streams=1, buckets=5, ggx_pdf=True, **fixed)
    q.set_ggx_pdf(False); q.Accumulate(2)
    same_words(r.accumulator(), q.accumulator(), "deferred calls under the setting they were issued under")
    assert (bits(q.accumulator()) != bits(run(ggx_pdf=False, max_batch=16, streams=1, accumulate=lambda z: z.Accumulate(5)))).any()
    r.close(); q.close()
    lens = dict(setup=lambda z: z.set_lens(0.05, 4.0))
    with_lens = run(**lens)
    assert (bits(with_lens) != bits(base)).any()
    same_words(run(use_bvh=False, **lens), with_lens, "lens on: tree against brute force")
    same_words(run(max_batch=1, **lens), with_lens, "lens on: batches of 1")
    g = mirt.GroupRenderer(sc, devices=[0, 0], max_bounces=16, buckets=5, use_bvh=True, max_batch=3, gloss_decay=DECAY, ggx_pdf=True, **fixed)
    assert g.ggx_pdf() is True
    g.Resize(W, H); g.Accumulate(N)
    same_words(g.accumulator(), base, "a group of the same device twice")
    g.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------
def test_interface(mirt):
    lib = mirt.load_library()
    W, H, N = 48, 32, 5
    sc = mirt.scene.default9()
    off = gpu_run(mirt, sc, W, H, N, brdf=1)[0]
    r = gpu_run(mirt, sc, W, H, 0, keep=True, accumulate=lambda q: None, brdf=1)
    assert r.ggx_pdf() is False
    assert lib.mirt_set_ggx_pdf(r._ctx, 2) == ERR_ARG and r.ggx_pdf() is False
    v = C.c_uint32(7)
    assert lib.mirt_get_ggx_pdf(r._ctx, None) == ERR_ARG and lib.mirt_get_ggx_pdf(None, C.byref(v)) == ERR_ARG
    r.set_ggx_pdf(True)
    assert r.ggx_pdf() is True and lib.mirt_get_ggx_pdf(r._ctx, C.byref(v)) == 0 and v.value == 1
    # exact stream order and the switch exclude each other, both ways
    assert lib.mirt_set_stream_order(r._ctx, 1) == ERR_STATE and r.stream_order == 0
    with pytest.raises(mirt.MirtError, match="mirt_set_ggx_pdf"):
        r.set_stream_order(True)
    r.set_ggx_pdf(False); r.set_stream_order(True)
    assert lib.mirt_set_ggx_pdf(r._ctx, 1) == ERR_STATE and r.ggx_pdf() is False
    with pytest.raises(mirt.MirtError, match="mirt_set_stream_order"):
        r.set_ggx_pdf(True)
    r.set_ggx_pdf(False)                                                               # switching off is always accepted
    r.set_stream_order(False)
    # on, then off again: the switch-off accumulator bit for bit after a reset; the accumulator is not reset by the switch itself
    r.set_ggx_pdf(True); r.Accumulate(N)
    on = r.accumulator()
    assert (bits(on) != bits(off)).any()
    r.set_ggx_pdf(False)
    assert r.accumulations == N
    same_words(r.accumulator(), on, "the switch does not reset the accumulator")
    r.ResetAccumulator(); r.Accumulate(N)
    same_words(r.accumulator(), off, "switched off again")
    r.close()


def test_headless_renders_the_python_frame(mirt, tmp_path):
    """mirt_headless --ggx-pdf (the C++ host over mirt_host.hpp, Renderer::SetGgxPdf) renders what the Python Renderer renders with ggx_pdf=True,
    and not what it renders without the flag."""
    exe = os.path.join(mirt.CSRC, "mirt_headless")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", mirt.CSRC, "mirt_headless"], check=True)
    frames = {}
    for on in (False, True):
        pfm = tmp_path / f"frame{int(on)}.pfm"
        subprocess.run([exe, "--scene", "brdf_test", "--brdf", "1", "--gloss-decay", ",".join(str(d) for d in DECAY), "--size", "160x96", "--spp", "10",
                        "--out", str(pfm)] + (["--ggx-pdf"] if on else []), check=True, timeout=120, capture_output=True, text=True)
        frames[on] = np.fromfile(pfm, dtype=np.float32, offset=len(b"PF\n160 96\n-1.0\n")).reshape(96, 160, 3)
    r = mirt.Renderer(mirt.scene.brdf_test(), max_bounces=16, use_bvh=True, brdf=1, gloss_decay=DECAY, ggx_pdf=True)
    r.Resize(160, 96); r.Accumulate(10); assert r.Render()
    same_words(frames[True], r.GetFrame()[:, :, :3], "mirt_headless --ggx-pdf against the Python frame")
    assert (bits(frames[True]) != bits(frames[False])).any()
    r.close()
