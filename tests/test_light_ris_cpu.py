"""Resampled importance sampling of the NEE light (mirt_set_light_ris), the side that needs no GPU: the float64 estimator of
tests/ris_definitions.py against the quadrature of definitions.direct_lambert on part F's frame-filling sphere, the guards that make the
GPU test a test, the figures it reads from tests/golden/light_ris_many.npz, and the C interface's symbols and refusals.  The oracle's
candidate loop (orc_set_light_ris, the reference every RIS kernel is held to word for word by tests/test_light_ris_gpu.py) is held here to
the same float64 estimator, to its own plain draw at one candidate, to a GGX expectation and to the reservoir draw that is exactly 1.0f.

MANY: HIGH and SIDE (F2) and fourteen further lights placed like BELOW - wholly below the horizon of every visible point, so a uniform
draw among the sixteen is wasted seven times out of eight.  Measured figures: DESIGN.md, "NEE light by resampled importance sampling"."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import definitions as df
import lens_twin as lt
import oracle_binding as ob
import ris_definitions as rd
import test_definitions_cpu as cpu
from test_definitions_cpu import (F_CASES, F_H, F_RHO, F_W, HIGH, SIDE, SIGMA, backend_image, df_lights, f_expectation, f_regions, footprint_points,
                                  guard_first_hits, lit_scene, report)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "light_ris_many.npz")


def below_lights():
    """Fourteen lights on two rings about -z, 128 and 137 degrees off the axis the camera looks along, of two sizes and changing colours."""
    out = []
    for i in range(14):
        polar, dist, radius = (math.radians(128.0), 2.75, 0.42) if i % 2 == 0 else (math.radians(137.0), 2.6, 0.30)
        az = 2.0 * math.pi * i / 14
        c = (dist * math.sin(polar) * math.cos(az), dist * math.sin(polar) * math.sin(az), dist * math.cos(polar))
        out.append((tuple(round(v, 3) for v in c), radius, (4.0 + (i % 3) * 3.0, 6.0, 10.0 - (i % 4) * 2.0)))
    return out


MANY = [HIGH, SIDE] + below_lights()
MANY_ACC = 120                                # accumulations of the GPU test on MANY: test_guards holds it to its rule
SOME = np.arange(0, F_W * F_H, 61)            # the pixels on which the quadrature runs over all sixteen lights (a minute for the whole image)
# the cases the GPU test renders: (case of F_CASES, candidates)
RIS_CASES = [("F1_high", 4), ("F2_two_lights", 4), ("MANY", 8)]
PER_SUB = 16                                  # paths per point of a pixel's 2 x 2 footprint: 64 per pixel
_cache = {}


def sampler(name, candidates, seed=2029, **switches):
    """ris_direct over every pixel's footprint for a case of F_CASES: per pixel E, var (h * w, 3), shadow (h * w,); once a process."""
    key = (name, candidates, seed, tuple(sorted(switches.items())))
    if key not in _cache:
        pts = footprint_points()
        _cache[key] = rd.ris_direct(pts, pts, F_RHO, df_lights(case_lights(name)), candidates, PER_SUB, np.random.default_rng(seed), **switches)
    return _cache[key]


def shadow_share(name, candidates):
    """Exact share of hits that cast a shadow ray, per pixel (h * w,): ris_definitions.shadow_share over the footprint.  The fourteen of MANY lie
    below every visible point's horizon (test_many_is_placed_as_stated), so a candidate of MANY casts with F2's probability times 2 / 16 -
    computed from F2's two cones, not sixteen."""
    key = ("share", name, candidates)
    if key not in _cache:
        pts = footprint_points()
        if name == "MANY":
            p1 = rd.shadow_share(pts.reshape(-1, 1, 3), pts.reshape(-1, 1, 3), df_lights(F_CASES["F2_two_lights"]["lights"]), 1, *cpu.F_QUAD) * 2.0 / len(MANY)
            _cache[key] = (1.0 - (1.0 - p1) ** candidates).reshape(pts.shape[:2]).mean(axis=1)
        else:
            _cache[key] = rd.shadow_share(pts, pts, df_lights(case_lights(name)), candidates, *cpu.F_QUAD)
    return _cache[key]


def case_lights(name):
    return MANY if name == "MANY" else F_CASES[name]["lights"]


def expectation(name):
    """f_expectation; for MANY, F2's with sixteen lights in both pdfs: the fourteen send nothing to a visible point and shadow nothing above its
    horizon, so they change the integrals only through the selection pdf (test_many_is_placed_as_stated compares with all sixteen on SOME).
    The shadow share is F2's times 2 / 16; the variance (of the plain draw) is not what F2's call gives and is left out."""
    if name != "MANY":
        return f_expectation(name)
    two = f_expectation("F2_two_lights", n_lights_in_light_pdf=len(MANY), n_lights_in_hit_weight=len(MANY))
    return dict(E=two["E"], shadow=f_expectation("F2_two_lights")["shadow"] * 2.0 / len(MANY))


def regions(name):
    return f_regions("F2_two_lights" if name == "MANY" else name)


def z_against_quadrature(name, got, n_eff, var=None):
    """Per region and channel: (mean of got["E"] - mean of the quadrature's E) in standard errors of the region's mean for n_eff samples a
    pixel, with the variance of `var` (default: got's own)."""
    exp = expectation(name)
    out = {}
    for label, mask in regions(name).items():
        k = mask.reshape(-1)
        se = np.sqrt((got if var is None else var)["var"][k].sum(axis=0) / n_eff) / k.sum()
        out[label] = (got["E"][k].mean(axis=0) - exp["E"][k].mean(axis=0)) / se
    return out


def test_many_is_placed_as_stated():
    """Each of the fourteen: wholly below the horizon of every visible point, hidden from the camera by the unit sphere, and disjoint from
    every other sphere of the scene - what F1 asserts for BELOW."""
    pts = footprint_points().reshape(-1, 3)
    eye = np.array([0.0, 0.0, cpu.F_EYE])
    spheres = [((0.0, 0.0, 0.0), 1.0)] + [(c, r) for c, r, _ in MANY]
    for c, r, _ in MANY[2:]:
        c = np.array(c)
        assert (((c[None, :] - pts * (1 + df.OFFSET)) * pts).sum(axis=1) + r < 0).all()                  # below the tangent plane of every visible point
        # hidden: the tangent cone of the unit sphere from the eye covers it (its angular extent from the eye's -z axis stays inside the cone,
        # and it lies beyond the circle of tangency)
        v = c - eye
        d = np.linalg.norm(v)
        off_axis = math.acos(-v[2] / d) + math.asin(r / d)
        assert off_axis < math.asin(1.0 / cpu.F_EYE) and c[2] + r < 1.0 / cpu.F_EYE
        for c2, r2 in spheres:
            if tuple(c2) != tuple(c):
                assert np.linalg.norm(c - np.array(c2)) > r + r2
    # the fourteen add nothing and cast nothing; they only dilute the draw
    q = many_quadrature()
    assert np.abs(q["E"] - expectation("MANY")["E"][SOME]).max() <= 1e-12 and np.abs(q["shadow"] - expectation("MANY")["shadow"][SOME]).max() <= 1e-12


def many_quadrature():
    """direct_lambert over all sixteen lights on the pixels SOME: E, var (k, 3), shadow (k,) of the mixture over the footprint."""
    if "quad" not in _cache:
        nrm = footprint_points()[SOME]
        k, sub = nrm.shape[:2]
        r = df.direct_lambert(nrm.reshape(-1, 3), nrm.reshape(-1, 3), F_RHO, df_lights(MANY), n_u=cpu.F_QUAD[0], n_phi=cpu.F_QUAD[1])
        E = r["E"].reshape(k, sub, 3).mean(axis=1)
        _cache["quad"] = dict(E=E, var=r["M2"].reshape(k, sub, 3).mean(axis=1) - E * E, shadow=r["shadow"].reshape(k, sub).mean(axis=1))
    return _cache["quad"]


@pytest.mark.parametrize("name", ["F2_two_lights", "MANY"])
@pytest.mark.parametrize("candidates", [1, 4, 8])
def test_sampler_meets_the_quadrature(name, candidates):
    got = sampler(name, candidates)
    z = z_against_quadrature(name, got, got["samples"])
    report(f"ris/{name}/M{candidates}", **{f"z_{k}": "/".join(f"{v:+.2f}" for v in zz) for k, zz in z.items()})
    for label, zz in z.items():
        assert np.abs(zz).max() <= SIGMA, (name, candidates, label, zz)


def test_one_candidate_has_the_plain_variance():
    """M = 1 is the plain light sample: the sampler's variance is direct_lambert's - on F2 the sums over each region, on MANY the sum over
    the pixels SOME, sampled 4096 times each.  Bound: a sample variance from n draws of a distribution with kurtosis k has relative
    standard error sqrt((k - 1) / n); n >= 64 x 256 pixels on F2 and 4096 x 68 on MANY, k below 60 (a sixteenth of MANY's draws carry anything), so
    SIGMA of them stay below 0.3 and 0.08: 0.15 and 0.1 taken (k is a figure of the definition, not of any backend)."""
    got, exp = sampler("F2_two_lights", 1), f_expectation("F2_two_lights")
    for label, mask in regions("F2_two_lights").items():
        k = mask.reshape(-1)
        ratio = got["var"][k].sum(axis=0) / exp["var"][k].sum(axis=0)
        report(f"ris/F2/M1/{label}", var_ratio="/".join(f"{v:.3f}" for v in ratio))
        assert np.abs(ratio - 1.0).max() <= 0.15, (label, ratio)
        sh = got["shadow"][k].mean(), exp["shadow"][k].mean()
        assert abs(sh[0] - sh[1]) <= SIGMA * math.sqrt(sh[1] * (1 - sh[1]) / (got["samples"] * k.sum()))
    pts = footprint_points()[SOME]
    got, exp = rd.ris_direct(pts, pts, F_RHO, df_lights(MANY), 1, 1024, np.random.default_rng(2031)), many_quadrature()
    ratio = got["var"].sum(axis=0) / exp["var"].sum(axis=0)
    report("ris/MANY/M1/some", var_ratio="/".join(f"{v:.3f}" for v in ratio))
    assert np.abs(ratio - 1.0).max() <= 0.1, ratio


@pytest.mark.parametrize("name,candidates", [("F1_high", 4), ("F2_two_lights", 1), ("F2_two_lights", 4), ("MANY", 1), ("MANY", 8)])
def test_shadow_share(name, candidates):
    """The exact share 1 - (1 - p)^M: with one candidate it is direct_lambert's `shadow`; the sampler's count of cast shadow rays is within
    SIGMA Bernoulli sigma of it (its own draws: 64 a pixel), over the image and over each region."""
    exact = shadow_share(name, candidates)
    if candidates == 1:
        assert np.abs(exact - expectation(name)["shadow"]).max() <= 1e-12
    if name == "MANY":
        q = rd.shadow_share(footprint_points()[SOME], footprint_points()[SOME], df_lights(MANY), candidates, *cpu.F_QUAD)      # all sixteen cones
        assert np.abs(q - exact[SOME]).max() <= 1e-12
    if name == "F1_high":
        assert (exact == 1.0).all()
        return
    got = sampler(name, candidates)
    for label, mask in [("image", np.ones((F_H, F_W), dtype=bool))] + list(regions(name).items()):
        k = mask.reshape(-1)
        diff, var = (got["shadow"][k].sum() - exact[k].sum()) * got["samples"], got["samples"] * (exact[k] * (1 - exact[k])).sum()
        if var == 0.0:                                                                    # every hit casts: so must every draw of the sampler
            assert diff == 0.0, (name, candidates, label)
            continue
        z = diff / math.sqrt(var)
        report(f"ris/{name}/M{candidates}/share/{label}", z=float(z), exact=float(exact[k].mean()))
        assert abs(z) <= SIGMA, (name, candidates, label, z)


MISREADINGS = ("no_one_over_m", "count_positive", "mean_of_candidates")


def many_guards(n_acc):
    """At n_acc accumulations on MANY with 8 candidates: the regional standard error over the expectation (check_direct wants it below 1 %),
    and for each misreading the largest distance from the quadrature, in standard errors of the true estimator."""
    exp, true = expectation("MANY"), sampler("MANY", 8)
    rel = max(float((np.sqrt(true["var"][m.reshape(-1)].sum(axis=0) / n_acc) / m.sum() / exp["E"][m.reshape(-1)].mean(axis=0)).max()) for m in regions("MANY").values())
    apart = {w: max(float(np.abs(z).max()) for z in z_against_quadrature("MANY", sampler("MANY", 8, **{w: True}), n_acc, var=true).values()) for w in MISREADINGS}
    return rel, apart


def test_guards():
    """What makes the GPU test a test.  Each misreading of the estimator misses the expectation by more than SIGMA standard errors at the GPU
    test's accumulation count, which is the smallest multiple of 5 at which that holds and the regional means are known to 1 %."""
    figures = {}
    for n_acc in range(5, MANY_ACC + 1, 5):
        rel, apart = many_guards(n_acc)
        holds = rel < 0.01 and min(apart.values()) > SIGMA
        assert holds == (n_acc == MANY_ACC), (n_acc, rel, apart)
    figures.update(rel_se=rel, **apart)
    # fewer wasted draws: the variance falls and the shadow ray is cast far more often
    one, eight = sampler("MANY", 1), sampler("MANY", 8)
    figures["var_ratio"] = float(eight["var"].sum() / one["var"].sum())
    figures["shadow_1"], figures["shadow_8"] = float(one["shadow"].mean()), float(eight["shadow"].mean())
    assert figures["var_ratio"] < 1.0
    for label, mask in regions("MANY").items():
        k = mask.reshape(-1)
        assert (eight["var"][k].sum(axis=0) < one["var"][k].sum(axis=0)).all(), label
    report("guards/ris", **figures)


def golden_figures():
    one, eight = sampler("MANY", 1), sampler("MANY", 8)
    return dict(var_ratio=np.float64(eight["var"].sum() / one["var"].sum()), shadow_probability=shadow_share("MANY", 8),
                candidates=np.int32(8), per_pixel=np.int32(eight["samples"]), seed=np.int32(2029))


def test_golden_figures_are_the_samplers():
    """tests/golden/light_ris_many.npz holds the sampler's variance ratio and the exact shadow share of MANY with eight candidates
    (python tests/test_light_ris_cpu.py writes it)."""
    g, want = np.load(GOLDEN), golden_figures()
    assert abs(float(g["var_ratio"]) / float(want["var_ratio"]) - 1.0) <= 1e-9
    assert g["shadow_probability"].dtype == np.float64 and np.abs(g["shadow_probability"] - want["shadow_probability"]).max() <= 1e-12
    assert int(g["candidates"]) == 8


# ---- the oracle's candidate loop ---------------------------------------------------------------------------------------------------
DECAY = [0.0, 0.3, 0.6, 0.8]
ANCHOR_CASES = {   # scene, width, height, oracle keywords
    "default9": (lambda m: m.scene.default9(), 96, 64, {}),
    "S1000": (lambda m: m.scene.synthetic(1000), 64, 64, {}),
    "brdf_test": (lambda m: m.scene.brdf_test(), 96, 64, {}),
    "default9_ggx": (lambda m: m.scene.default9(), 96, 64, dict(brdf=1, gloss_decay=DECAY)),
}


def oracle_state(sc, w, h, n_acc, **kw):
    o = ob.Oracle(sc, **{"max_bounces": 16, "buckets": 5, **kw})
    o.Resize(w, h); o.Accumulate(n_acc)
    out = dict(acc=o.accumulator(), frame=o.Render(), counters=o.counters())
    o.close()
    return out


def same_state(a, b, what):
    assert np.array_equal(ob.bits(a["acc"]), ob.bits(b["acc"])), f"{what}: accumulator"
    assert np.array_equal(ob.bits(a["frame"]), ob.bits(b["frame"])), f"{what}: frame"
    assert a["counters"] == b["counters"], f"{what}: counters"


@pytest.mark.parametrize("name", list(ANCHOR_CASES))
def test_oracle_one_candidate_is_the_plain_draw(mirt, name):
    """Anchor: the candidate loop with M = 1 leaves every word and every counter of the plain code path (M = 0, the text every golden file pins),
    in each of the oracle's three traversal modes.  Seven candidates do not: the loop is reached."""
    make, w, h, kw = ANCHOR_CASES[name]
    sc = make(mirt)
    for mode in (ob.TRAV_BRUTE, ob.TRAV_STREAM_BVH, ob.TRAV_PER_RAY_BVH):
        plain = oracle_state(sc, w, h, 5, trav_mode=mode, **kw)
        same_state(oracle_state(sc, w, h, 5, trav_mode=mode, light_ris=1, **kw), plain, f"{name}, mode {mode}: M = 1 against M = 0")
    seven = oracle_state(sc, w, h, 5, light_ris=7, **kw)
    assert (ob.bits(seven["acc"]) != ob.bits(plain["acc"])).any()
    # the twin's traversal returns the brute-force answer bit for bit, with candidates as without
    twin = oracle_state(sc, w, h, 5, light_ris=7, trav_mode=ob.TRAV_PER_RAY_BVH, **kw)
    assert np.array_equal(ob.bits(twin["acc"]), ob.bits(seven["acc"])) and np.array_equal(ob.bits(twin["frame"]), ob.bits(seven["frame"]))
    assert {k: twin["counters"][k] for k in ("rays", "terminated")} == {k: seven["counters"][k] for k in ("rays", "terminated")}
    assert twin["counters"]["shadow_rays"] <= seven["counters"]["shadow_rays"]         # Q5: the twin casts nothing for hits it then drops


@pytest.mark.parametrize("name,candidates", RIS_CASES)
def test_oracle_unbiased(mirt, name, candidates):
    """The oracle as a backend of the float64 estimator, with test_light_ris_gpu.py's test_unbiased's bounds: every regional mean within SIGMA
    standard errors of the quadrature (ris_definitions' variance), `shadow_rays` within SIGMA Bernoulli sigma of 1 - (1 - p)^M, `rays` and
    `terminated` the plain oracle's.  This is what keeps the oracle's loop from being a copy of the kernels' mistake."""
    n_acc = MANY_ACC if name == "MANY" else F_CASES[name]["n_acc"]
    sc = lit_scene(mirt, case_lights(name))
    exp, var = expectation(name), sampler(name, candidates)
    guard_first_hits(cpu.OracleBackend(mirt), sc, 3)
    res = oracle_state(sc, F_W, F_H, n_acc, max_bounces=3, trav_mode=ob.TRAV_PER_RAY_BVH, light_ris=candidates)
    plain = oracle_state(sc, F_W, F_H, n_acc, max_bounces=3, trav_mode=ob.TRAV_PER_RAY_BVH)
    img = backend_image(res, n_acc)
    zs = {}
    for label, mask in regions(name).items():
        k = mask.reshape(-1)
        want = exp["E"][k].mean(axis=0)
        se = np.sqrt(var["var"][k].sum(axis=0) / n_acc) / k.sum()
        assert mask.sum() >= 64 and (want > 0).all() and (se / want < 0.01).all(), (name, label, se / want)
        zs[label] = (img[mask].mean(axis=0) - want) / se
    c = res["counters"]
    share = np.load(GOLDEN)["shadow_probability"] if name == "MANY" else shadow_share(name, candidates)
    want_sh, sigma_sh = n_acc * share.sum(), math.sqrt(n_acc * (share * (1 - share)).sum())
    report(f"oracle/ris/{name}/M{candidates}", **{f"z_{k}": "/".join(f"{v:+.2f}" for v in z) for k, z in zs.items()},
           shadow_rays=c["shadow_rays"], shadow_expected=float(want_sh), shadow_sigma=float(sigma_sh), shadow_plain=plain["counters"]["shadow_rays"])
    for label, z in zs.items():
        assert np.abs(z).max() <= SIGMA, f"{name}/{label}: {z} sigma from the expectation"
    assert abs(c["shadow_rays"] - want_sh) <= SIGMA * sigma_sh, f"{name}: {c['shadow_rays']} shadow rays, expected {want_sh:.1f} +- {sigma_sh:.1f}"
    for k in ("rays", "terminated"):
        assert c[k] == plain["counters"][k], k


GGX_ACC, GGX_GRID = 256, 32          # accumulations (16 in each of 16 buckets); side of a region in pixels: 3 x 2 regions of the 96 x 64 image


def ggx_region_means(acc, w, h, n_acc):
    """[tile][16][3][256] -> per region and channel: the mean, and its standard error from the spread of the 16 independent bucket means."""
    img = np.zeros((16, h, w, 3))
    for t in range(acc.shape[0]):
        y0, x0 = 16 * (t // (w // 16)), 16 * (t % (w // 16))
        img[:, y0:y0 + 16, x0:x0 + 16, :] = np.moveaxis(acc[t].astype(np.float64), 1, 2).reshape(16, 16, 16, 3)
    r = img.reshape(16, h // GGX_GRID, GGX_GRID, w // GGX_GRID, GGX_GRID, 3).mean(axis=(2, 4)) / (n_acc / 16)
    return r.mean(axis=0), r.std(axis=0, ddof=1) / math.sqrt(16)


def test_oracle_ggx_expectation(mirt):
    """ris_definitions is Lambertian; for GGX the oracle's eight candidates are compared with its own plain draw on brdf_test (GGX, a decay
    table, 16 buckets): per 32 x 32 region and channel z = (mean_8 - mean_0) / sqrt(se_8^2 + se_0^2), each se from the spread of that run's 16
    independent bucket means, |z| <= SIGMA.  Condition: every region's relative se is below 1 % in both runs; GGX_ACC = 256 is the smallest multiple
    of 16 at which the plain oracle meets it here (0.0104 at 240, 0.0095 at 256).  Measured at 256: largest |z| 3.22.
    Not noise alone: |z| grows with the count (5.9 at 512, 8.1 at 2048) and stays below 1.2 through 2048 once the NEE stream is hashed apart from
    the camera sample's.  The reference draws the camera jitter and the bounce-0 light sample from ONE generator state (Renderer.hpp:117,255), so
    the plain draw's (u0, u1) ARE the pixel jitter; candidates 2..M are independent of it.  The expectations of M = 0 and M = 8 therefore differ by
    that correlation's share (about 0.5 % of a region's mean here), which 256 accumulations do not resolve and the 1 % condition allows."""
    w, h = 96, 64
    runs = {}
    for m in (0, 8):
        o = ob.Oracle(mirt.scene.brdf_test(), max_bounces=16, buckets=16, brdf=1, gloss_decay=DECAY, light_ris=m)
        o.Resize(w, h); o.Accumulate(GGX_ACC)
        runs[m] = ggx_region_means(o.accumulator(), w, h, GGX_ACC)
        o.close()
    (m0, s0), (m8, s8) = runs[0], runs[8]
    assert (m0 > 0).all() and (m8 > 0).all()
    assert (s0 / m0 < 0.01).all() and (s8 / m8 < 0.01).all(), (float((s0 / m0).max()), float((s8 / m8).max()))
    z = (m8 - m0) / np.sqrt(s8 * s8 + s0 * s0)
    report("oracle/ris/ggx", accumulations=GGX_ACC, rel_se_0=float((s0 / m0).max()), rel_se_8=float((s8 / m8).max()),
           z=" ".join("/".join(f"{v:+.2f}" for v in zz) for zz in z.reshape(-1, 3)))
    assert np.abs(z).max() <= SIGMA, z


# ---- the reservoir draw that is exactly 1.0f ----------------------------------------------------------------------------------------
ONE_W = ONE_H = 16                       # one tile of the F1_high scene (the unit sphere fills the frame and every hit casts), max_bounces = 3
ONE_BOUNCES = 3
ONE_ACC, ONE_PIXEL = 26873, 64           # search_unit_draw()[0]; its other two below 2^18: (65193, 104), (200960, 100)


def nee_draws(acc, pixels, bounce, count, max_bounces=ONE_BOUNCES):
    """The first `count` words of the NEE generator hash_2d(acc, seed[ID] + 2 * bounce) of tile 0's pixels, acc = the Accumulate() call's number
    (the first call is 1: Renderer.hpp:74 increments before it renders): (count, n) uint32."""
    seed = lt.seeds([0], max_bounces)[np.asarray(pixels)]
    state = lt.hash_2d(np.broadcast_to(np.asarray(acc, dtype=np.uint32), seed.shape), (seed.astype(np.uint64) + np.uint64(2 * bounce)) & lt.M32)
    out = []
    for _ in range(count):
        word, state = lt.pcg_generate(state)
        out.append(word)
    return np.stack(out)


def search_unit_draw(limit=1 << 18, chunk=1 << 12):
    """Every (accumulation number, pixel) below `limit` at which the reservoir draw of the FIRST candidate at bounce 0 - the 4th word of the NEE
    stream, after u0, u1 and the light - is at least 0xFFFFFF80, the words rand_unit_float turns into exactly 1.0f.  About 12 s; the test
    keeps its first result as ONE_ACC, ONE_PIXEL."""
    found = []
    for lo in range(1, limit, chunk):
        acc = np.arange(lo, min(limit, lo + chunk), dtype=np.uint32)
        words = nee_draws(np.repeat(acc, 256), np.tile(np.arange(256), len(acc)), 0, 4)[3]
        found += [(int(acc[i // 256]), int(i % 256)) for i in np.flatnonzero(words >= np.uint32(0xFFFFFF80))]
    return found


def one_scene(mirt):
    return lit_scene(mirt, F_CASES["F1_high"]["lights"])


def one_run(make_renderer, n_before=ONE_ACC - 1):
    """The accumulator after call number n_before + 1 alone: both sides are brought to the count by loading an empty slab, not by rendering up to it."""
    r = make_renderer()
    r.Resize(ONE_W, ONE_H)
    r.load_accumulator(np.zeros(ONE_W * ONE_H * 5 * 3, dtype=np.float32), n_before)
    r.Accumulate(1)
    assert r.accumulations == n_before + 1
    acc = r.accumulator().copy()
    r.close()
    return acc


def test_first_candidate_is_taken_when_the_draw_is_one(mirt):
    """`weight_sum == w` takes the first positive candidate whatever r; without it `r < w / weight_sum` is 1.0f < 1.0f and the hit casts nothing."""
    word = nee_draws(ONE_ACC, [ONE_PIXEL], 0, 4)[3]
    assert word[0] >= 0xFFFFFF80 and (word.astype(np.float32) * np.float32(2.0 ** -32))[0] == np.float32(1.0)
    sc = one_scene(mirt)
    o = ob.Oracle(sc, max_bounces=ONE_BOUNCES, light_ris=1); o.Resize(ONE_W, ONE_H)
    rec = o.debug_candidates(0, ONE_PIXEL, ONE_ACC)
    o.close()
    first = rec[(rec[:, 0] == 0) & (rec[:, 1] == 0)]
    assert len(first) == 1 and first[0, 2] == np.float32(1.0) and first[0, 3] > 0, rec      # the oracle drew 1.0f there, for a candidate that weighs something
    got = {m: one_run(lambda: ob.Oracle(sc, max_bounces=ONE_BOUNCES, light_ris=m)) for m in (0, 1)}
    assert got[0][0, ONE_ACC % 5, :, ONE_PIXEL].min() > 0                                   # the plain draw's light arrived in that pixel
    assert np.array_equal(ob.bits(got[1]), ob.bits(got[0]))
    assert not got[0][:, [b for b in range(5) if b != ONE_ACC % 5]].any()                   # one call, one bucket: the slab was loaded, not rendered up to


# ---- the oracle's interface ----------------------------------------------------------------------------------------------------------
def test_oracle_light_ris_interface(mirt, oracle_lib):
    assert oracle_lib.orc_set_light_ris(None, 4) == -1
    assert oracle_lib.orc_load_accumulator(None, None, 0) == -1
    o = ob.Oracle(mirt.scene.default9())
    assert o.light_ris == 0
    assert oracle_lib.orc_set_light_ris(o.h, 33) == -1 and oracle_lib.orc_set_light_ris(o.h, 32) == 0 and oracle_lib.orc_set_light_ris(o.h, 0) == 0
    with pytest.raises(ValueError, match="33 candidates"):
        o.set_light_ris(33)
    assert oracle_lib.orc_load_accumulator(o.h, None, 3) == -1
    o.close()


# ---- the C interface ---------------------------------------------------------------------------------------------------------------
def test_symbols_and_constants(mirt):
    lib = mirt.load_library()
    for name in ("mirt_set_light_ris", "mirt_get_light_ris", "mirt_group_set_light_ris"):
        assert name in lib._declared and getattr(lib, name)
    assert mirt.MAX_LIGHT_RIS == 32
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "mirt.h")).read()
    assert "#define MIRT_MAX_LIGHT_RIS 32u" in header
    for method in ("set_light_ris", "light_ris"):
        assert callable(getattr(mirt.Renderer, method)) and callable(getattr(mirt.GroupRenderer, method))


def test_null_arguments(mirt):
    """The checks that come before any context is touched: MIRT_ERR_ARG = -1.  (The setter's other refusals need a context: test_light_ris_gpu.py.)"""
    lib = mirt.load_library()
    v = C.c_uint32(7)
    assert lib.mirt_set_light_ris(None, 4) == -1
    assert lib.mirt_get_light_ris(None, C.byref(v)) == -1 and v.value == 7
    assert lib.mirt_group_set_light_ris(None, 4) == -1


if __name__ == "__main__":
    np.savez(GOLDEN, **golden_figures())
    print("wrote", GOLDEN)
