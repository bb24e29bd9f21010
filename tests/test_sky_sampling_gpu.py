"""Sky sampling (mirt_set_sky_sampling) on the device, against the float64 twin of tests/sky_definitions.py: the table the two HIP kernels
build, sky_sample and sky_pdf through mirt_debug_math fn 12 / 13, and the path — the same expectation with the switch on, less noise under a
sun, no effect where it must have none, and the statuses."""
import math

import numpy as np
import pytest

import definitions as df
import sky_definitions as sd
import test_definitions_cpu as cpu
from test_definitions_gpu import GpuBackend

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
W = H = 64
SUN_W, SUN_H = 65, 33
ATAN2_ABS, ASIN_ABS = 2e-3, 1e-3           # row D's asserted errors of fast_atan2 / fast_asin (test_definitions_cpu.check_sky)


def small_maps():
    rng = np.random.default_rng(4)
    maps = {}
    for w, h in ((1, 1), (2, 2), (2, 1), (1, 2), (9, 5)):
        m = rng.uniform(0.25, 2.0, (h, w, 4)).astype(f32)
        if (w, h) == (9, 5):
            m[1, 2, :3] = 0.0; m[3, :, :3] = 0.0                                   # a black cell and a black row: never drawn
        maps[(w, h)] = m
    maps[(SUN_W, SUN_H)] = sd.sun_map()
    return maps


MAPS = small_maps()
AMBIENT = (1.0, 0.5, 0.25)


def words(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def same_words(a, b, what):
    assert np.array_equal(words(a), words(b)), what


@pytest.fixture(scope="module")
def tables(mirt):
    """One context per map with the switch on: (renderer, the table read back, the twin's table)."""
    out = {}
    for key, m in MAPS.items():
        sc = cpu.one_sphere(mirt, hdri=m)
        sc.ambient = np.asarray(AMBIENT, dtype=f32)
        r = mirt.Renderer(sc, max_bounces=4, sky_sampling=True)
        out[key] = (r, r.debug_sky_table(), sd.table(m, AMBIENT))
    yield out
    for r, _, _ in out.values():
        r.close()


# ---- the table --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(MAPS))
def test_table_against_the_twin(tables, key):
    r, got, want = tables[key]
    w, h = key
    rows, cols = sd.cells(w, h)
    assert (got["rows"], got["cols"]) == (rows, cols) == (want["rows"], want["cols"])
    bound = sd.table_bounds(rows, cols)
    worst = {}
    for name in ("cond", "marg", "dens"):
        g, t = got[name].astype(f64), want[name]
        assert ((t == 0) <= (g == 0)).all(), name                                  # an exact zero stays one
        rel = np.abs(g - t) / np.where(t == 0, 1.0, t)
        worst[name] = float(rel.max())
        assert (rel <= bound[name]).all(), (name, worst[name], bound[name])
    cpu.report(f"gpu/sky_table/{w}x{h}", **{f"worst_{k}_over_bound": v / bound[k] for k, v in worst.items()}, **{f"worst_{k}": v for k, v in worst.items()})
    # the cell edges: 1 -+ sin el(k), each one rounding of the float64 value
    el = sd.elevation(np.arange(rows + 1), rows)
    for name, t in (("tn", 1.0 - np.sin(el)), ("ts", 1.0 + np.sin(el))):
        assert np.allclose(got[name].astype(f64), t, rtol=4 * sd.U32, atol=1e-30), name   # (float64's own 1 - sin near a pole costs ~1e-16 absolute: below the tolerance from |t| > 1e-9)
    assert got["tn"][0] == 0.0 and got["ts"][rows] == 0.0
    # monotone, and ending at the same total
    assert (np.diff(got["marg"]) >= 0).all() and (np.diff(got["cond"], axis=1) >= 0).all()
    assert words(got["marg"][-1:])[0] == words(np.array([got["total"]]))[0] and got["total"] > 0
    same_words(got["cond"][:, -1], got["rowsum"], "a row's running sums end at the row sum the marginal was made from")
    assert np.isfinite(got["words"]).all()


def test_two_builds_are_word_identical(mirt, tables):
    r, got, _ = tables[(SUN_W, SUN_H)]
    r.set_sky_sampling(False)
    with pytest.raises(mirt.MirtError, match="no sky sampling table"):
        r.debug_sky_table()
    r.set_sky_sampling(True)
    same_words(r.debug_sky_table()["words"], got["words"], "switch off and on again over the current scene")
    r.UpdateScene()
    same_words(r.debug_sky_table()["words"], got["words"], "mirt_set_scene with the switch on")
    sc = cpu.one_sphere(mirt, hdri=MAPS[(SUN_W, SUN_H)]); sc.ambient = np.asarray(AMBIENT, dtype=f32)
    q = mirt.Renderer(sc, sky_sampling=True)
    same_words(q.debug_sky_table()["words"], got["words"], "another context")
    q.close()


# ---- fn 12 / fn 13 ------------------------------------------------------------------------------------------------------------------
def draws(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.uniform(size=(2, n)).astype(f32)
    u[:, :8] = np.array([[0, 1, 0, 1, 0.5, 2.0 ** -32, 1 - 2.0 ** -24, 0.25], [0, 1, 1, 0, 0.5, 1 - 2.0 ** -24, 2.0 ** -32, 0.75]], dtype=f32)   # the ends of rand_unit_float's range
    return u


@pytest.mark.parametrize("key", list(MAPS))
def test_sky_sample_and_pdf(tables, key):
    r, got, want = tables[key]
    w, h = key
    rows, cols = got["rows"], got["cols"]
    n = 1 << 20 if key == (SUN_W, SUN_H) else 1 << 14
    u = draws(n, 7)
    out = r.debug_math(12, u, 6)
    d, q, row, col = out[:3].T.astype(f64), out[3], out[4].astype(np.int64), out[5].astype(np.int64)
    # a binary32 replay over the table read back names the same cell for every u
    d_twin, row32, col32, _, _ = sd.sample({"marg": got["marg"], "cond": got["cond"]}, u[0], u[1])
    assert np.array_equal(row, row32) and np.array_equal(col, col32)
    assert (want["prob"][row, col] > 0).all()                                      # a black cell is never drawn
    same_words(q, got["dens"][row, col], "q is the cell's word")
    # unit, within 1e-6 of the twin's direction, and in its cell (closed, widened by that 1e-6)
    assert (np.abs(np.linalg.norm(d, axis=1) - 1.0) <= 4 * sd.U32 * 2).all()
    err = np.linalg.norm(d - d_twin, axis=1)
    cpu.report(f"gpu/sky_sample/{w}x{h}", worst_distance_to_twin=float(err.max()))
    assert (err <= 1e-6).all(), float(err.max())
    el = sd.elevation(np.arange(rows + 1), rows)
    assert (d[:, 1] <= np.sin(el[row]) + 1e-6).all() and (d[:, 1] >= np.sin(el[row + 1]) - 1e-6).all()
    cos_el = np.hypot(d[:, 0], d[:, 2])
    wide = cos_el > 1e-3
    ex = cols * (0.5 + np.arctan2(d[:, 2], d[:, 0]) / (2 * np.pi))
    tol = 1e-6 / np.maximum(cos_el, 1e-3) * cols / (2 * np.pi)
    off = np.abs((ex - (col + 0.5) + cols / 2) % cols - cols / 2)                   # distance to the cell's middle, round the meridian
    assert (off[wide] <= 0.5 + tol[wide]).all()

    # fn 13 on those directions: the sampled cell, except within the lookup's asserted error of a cell edge
    out13 = r.debug_math(13, np.ascontiguousarray(out[:3]), 3)
    p, row13, col13 = out13[0], out13[1].astype(np.int64), out13[2].astype(np.int64)
    same_words(p, got["dens"][row13, col13], "p~ is the named cell's word")
    bw_phi = ATAN2_ABS + 1e-4 * 2 * math.pi / cols
    bw_lat = ASIN_ABS + 1e-4 * math.pi / rows
    phi = np.arctan2(d[:, 2], d[:, 0]); lat = np.arcsin(np.clip(d[:, 1], -1, 1))
    edge_phi = (np.arange(cols + 1) / cols - 0.5) * 2 * np.pi
    d_phi = np.abs((phi[:, None] - edge_phi[None, :] + np.pi) % (2 * np.pi) - np.pi).min(axis=1) if cols > 1 else np.full(n, np.inf)
    d_lat = np.abs(lat[:, None] - el[None, 1:-1]).min(axis=1) if rows > 1 else np.full(n, np.inf)
    aside = (d_phi <= bw_phi) | (d_lat <= bw_lat)
    wrong = (row13 != row) | (col13 != col)
    # a direction within the 1e-6 of a pole (u0 = 0 or 1 lands ON it: x = z = 0) lies that close to every column of its row: the azimuth says nothing there
    at_pole = cos_el <= 1e-6
    assert at_pole.sum() <= 8 and (row13[at_pole] == row[at_pole]).all()
    aside |= at_pole; col13 = np.where(at_pole, col, col13)
    assert not (wrong & ~aside).any(), int((wrong & ~aside).sum())
    assert (np.abs(row13 - row) <= 1).all() and (np.minimum(np.abs(col13 - col), cols - np.abs(col13 - col)) <= 1).all()
    if key == (SUN_W, SUN_H):
        share = sd.band_share(want, bw_phi, bw_lat)
        cpu.report("gpu/sky_pdf/65x33", set_aside=float(aside.mean()), band_share=share, wrong_inside_bands=int(wrong.sum()))
        assert aside.mean() <= 1.1 * share
        # chi-square of the 2^20 samples against the twin's cell probabilities
        pr = want["prob"].reshape(-1)
        counts = np.bincount(row * cols + col, minlength=pr.size).astype(f64)
        chi2 = ((counts - n * pr) ** 2 / (n * pr)).sum()
        cpu.report("gpu/sky_sample/65x33/chi2", chi2=float(chi2), dof=pr.size - 1, bound=df.chi2_upper(pr.size - 1, 1e-6))
        assert chi2 < df.chi2_upper(pr.size - 1, 1e-6)


# ---- the same expectation -----------------------------------------------------------------------------------------------------------
class SkyBackend(GpuBackend):
    """test_definitions_gpu's backend with the switch on for every render."""
    name = "gpu_sky"

    def render(self, sc, w, h, n_acc, max_bounces, buckets=5, mis=True, variant=0, **kw):
        r = self.mirt.Renderer(sc, max_bounces=max_bounces, buckets=buckets, mis=mis, sky_sampling=True, **self.variants[variant][1], **kw)
        r.Resize(w, h); r.Accumulate(n_acc)
        out = dict(acc=r.accumulator(), frame=None, counters=r.counters())
        r.close()
        return out


@pytest.fixture(scope="module")
def sky_be(mirt):
    b = SkyBackend(mirt)
    yield b
    b.close()


@pytest.mark.parametrize("variant", [0, 1])
def test_two_tone_sky_with_the_switch_on(sky_be, mirt, variant):
    """Part E's closed form 0.6 (1 + n.y) / 2 per pixel, its 5 sigma bounds unchanged (the analytic variance is the plain path's: an upper bound here)."""
    cpu.check_two_tone_sky(sky_be, mirt, variant=variant)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("w,h,n_acc", [(64, 64, 50), (256, 256, 20)])
def test_filling_sphere_with_the_switch_on(sky_be, mirt, w, h, n_acc, variant):
    """Part E's filling sphere (test_definitions_cpu.check_filling_sphere) with the switch on: the mean is albedo.r, `rays` = n (1 + p) and
    `terminated` = n as there, within the same 5 sigma of the plain path's Bernoulli variance; the three channels are the same words (Q10 carried
    into the sky's NEE); and now there ARE shadow rays: the scene has no sphere light, and the sky is one."""
    n = w * h * n_acc
    for albedo, label in cpu.FILLING:
        res = sky_be.render(cpu.one_sphere(mirt, albedo=albedo), w, h, n_acc, max_bounces=8, variant=variant)
        acc = res["acc"]
        same_words(acc[:, :, 0], acc[:, :, 1], "Q10"); same_words(acc[:, :, 0], acc[:, :, 2], "Q10")
        p = max(albedo)
        value = albedo[0] / p
        mean = acc[:, :, 0].astype(f64).sum() / n
        z_mean = (mean - p * value) / (value * math.sqrt(p * (1 - p) / n))
        c = res["counters"]
        z_rays = (c["rays"] - n * (1 + p)) / math.sqrt(n * p * (1 - p))
        cpu.report(f"gpu_sky/filling/{w}x{h}x{n_acc}/{label}", mean=float(mean), z_mean=float(z_mean), z_rays=float(z_rays), shadow_rays=c["shadow_rays"])
        assert c["terminated"] == n and c["shadow_rays"] > 0
        assert abs(z_mean) <= cpu.SIGMA and abs(z_rays) <= cpu.SIGMA, (label, z_mean, z_rays)


def sun_scene(mirt, kind):
    """A Lambert ball on a Lambert ground ball under the sun map; `kind` adds what the case is about."""
    S = mirt.scene
    cam = S.Camera(eye=(0.0, 1.2, 4.0), direction=(0.0, -0.2, -1.0), focal_length=35.0, exposure=1.0)
    geo = [S._sphere((0, -100.0, 0), 100.0 ** 2, 0), S._sphere((0, 0.5, 0), 0.25, 1)]
    mat = [S._material(albedo=(0.7, 0.7, 0.7), F0=(0.04, 0.04, 0.04), roughness=0.6), S._material(albedo=(0.8, 0.3, 0.2), F0=(0.9, 0.6, 0.3), roughness=0.4)]
    if kind == "light":
        geo.append(S._sphere((1.5, 1.5, 0.5), 0.09, 2)); mat.append(S._material(emission=(8.0, 8.0, 8.0)))
    if kind == "glass":
        geo.append(S._sphere((-1.1, 0.5, 0.6), 0.25, 2)); mat.append(S._material(albedo=(0.9, 0.9, 0.9), transmission=(0.9, 0.95, 1.0), IOR_minus_one=0.5))
    sc = S.Scene(np.array(geo, dtype=S.SPHERE), np.array(mat, dtype=S.MATERIAL), cam, np.ones(3, dtype=f32), name="sun_" + kind)
    sc.hdri = sd.sun_map(sun=(6, 40))                                              # elevation ~ 51 degrees, in front of the camera to its right
    return sc


SUN_CASES = {"lambert": ("plain", {}), "ggx": ("plain", dict(brdf=1)), "light_ris": ("light", dict(light_ris=4)), "glass": ("glass", dict(transmission=True))}
N_ACC, BUCKETS = 80, 16


@pytest.fixture(scope="module")
def sun_runs(mirt):
    """Each case rendered once with the switch off and once with it on: bucket means of the image, counters, mirt_noise's mean."""
    cache = {}

    def get(case):
        if case not in cache:
            kind, kw = SUN_CASES[case]
            sc = sun_scene(mirt, kind)
            res = {}
            for on in (False, True):
                r = mirt.Renderer(sc, max_bounces=6, buckets=BUCKETS, use_bvh=True, sky_sampling=on, **kw)
                r.Resize(W, H); r.Accumulate(N_ACC)
                acc = r.accumulator().astype(f64)                                  # [tile][bucket][rgb][256]
                res[on] = dict(bucket_means=acc.sum(axis=(0, 2, 3)) / (3 * W * H * (N_ACC // BUCKETS)), counters=r.counters(), noise=r.noise()["mean"])
                r.close()
            cache[case] = res
        return cache[case]
    return get


@pytest.mark.parametrize("case", list(SUN_CASES))
def test_sun_scene_has_the_same_expectation(sun_runs, case):
    res = sun_runs(case)
    off, on = res[False], res[True]
    sigma = math.sqrt(off["bucket_means"].var(ddof=1) / BUCKETS + on["bucket_means"].var(ddof=1) / BUCKETS)
    delta = on["bucket_means"].mean() - off["bucket_means"].mean()
    cpu.report(f"gpu/sky_sun/{case}", mean_off=float(off["bucket_means"].mean()), mean_on=float(on["bucket_means"].mean()), z=float(delta / sigma),
               shadow_rays_off=off["counters"]["shadow_rays"], shadow_rays_on=on["counters"]["shadow_rays"], noise_off=float(off["noise"]), noise_on=float(on["noise"]))
    assert abs(delta) <= 5.0 * sigma, (delta, sigma)
    for name in ("rays", "terminated"):
        assert on["counters"][name] == off["counters"][name], name
    assert on["counters"]["shadow_rays"] != off["counters"]["shadow_rays"]


def test_it_pays(sun_runs):
    """Equal samples on the sun scene: the mean of mirt_noise with the switch on is strictly below that with it off (measured ratio:
    profiles/sky_sampling.txt)."""
    res = sun_runs("lambert")
    assert res[True]["noise"] < res[False]["noise"], (res[True]["noise"], res[False]["noise"])


# ---- no effect where it must have none --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("why", ["no_ambient", "no_mis", "black_map"])
def test_no_effect(mirt, why):
    sc = mirt.scene.default9() if why != "black_map" else sun_scene(mirt, "light")
    if why == "no_ambient":
        sc.hdri = sd.sun_map(); assert not sc.ambient.any()
    elif why == "no_mis":
        sc.hdri = sd.sun_map(); sc.ambient = np.ones(3, dtype=f32)
    else:
        sc.hdri = np.zeros((5, 9, 4), dtype=f32)
    got = {}
    for on in (False, True):
        r = mirt.Renderer(sc, max_bounces=6, mis=why != "no_mis", sky_sampling=on)
        r.Resize(W, H); r.Accumulate(10)
        got[on] = (r.accumulator(), r.counters())
        r.close()
    same_words(got[True][0], got[False][0], why)
    assert got[True][1] == got[False][1]


# ---- statuses ---------------------------------------------------------------------------------------------------------------------------
def test_state_rules(mirt):
    lib = mirt.load_library()
    sc = sun_scene(mirt, "plain")
    r = mirt.Renderer(sc, max_bounces=4, buckets=1)
    assert r.sky_sampling() is False
    assert lib.mirt_set_sky_sampling(r._ctx, 2) == -1 and r.sky_sampling() is False   # MIRT_ERR_ARG
    r.Resize(W, H); r.Accumulate(2)
    before = r.accumulator()
    r.AccumulateAsync(1)                                                           # deferred: launched first, under the old setting
    r.set_sky_sampling(True)
    assert r.sky_sampling() is True and r.accumulations == 3
    q = mirt.Renderer(sc, max_bounces=4, buckets=1); q.Resize(W, H); q.Accumulate(3)
    same_words(r.accumulator(), q.accumulator(), "the switch neither resets the accumulator nor touches the deferred call")
    assert not np.array_equal(words(before), words(r.accumulator()))
    q.close()
    assert lib.mirt_set_stream_order(r._ctx, 1) == -3 and r.stream_order == 0       # MIRT_ERR_STATE
    with pytest.raises(mirt.MirtError, match="mirt_set_sky_sampling"):
        r.set_stream_order(True)
    r.set_sky_sampling(False); r.set_stream_order(True)
    assert lib.mirt_set_sky_sampling(r._ctx, 1) == -3 and r.sky_sampling() is False
    with pytest.raises(mirt.MirtError, match="mirt_set_stream_order"):
        r.set_sky_sampling(True)
    r.set_sky_sampling(False)                                                      # off is always accepted
    r.set_stream_order(False)
    r.close()
    for value in (-1.0, np.nan, np.inf):
        bad = sun_scene(mirt, "plain")
        bad.hdri[3, 5, :3] = value
        q = mirt.Renderer(bad, max_bounces=4)                                      # off: nothing is asked of the texels
        assert lib.mirt_set_sky_sampling(q._ctx, 1) == -1 and q.sky_sampling() is False
        with pytest.raises(mirt.MirtError, match="importance"):
            q.set_sky_sampling(True)
        with pytest.raises(mirt.MirtError, match="no sky sampling table"):
            q.debug_sky_table()
        q.scene = sc; q.UpdateScene(); q.set_sky_sampling(True)
        q.scene = bad
        with pytest.raises(mirt.MirtError, match="importance"):
            q.UpdateScene()                                                        # mirt_set_scene with the switch on
        q.close()
    # the last texel row and column own no cell: nothing is asked of them
    odd = sun_scene(mirt, "plain")
    odd.hdri[-1, :, :3] = -1.0; odd.hdri[:, -1, :3] = np.nan
    q = mirt.Renderer(odd, max_bounces=4, sky_sampling=True)
    q.close()


def test_group_twin(mirt):
    """mirt_group_set_sky_sampling on a group that names the one device twice: the single context's words, and every member's table is the same."""
    sc = sun_scene(mirt, "light")
    r = mirt.Renderer(sc, max_bounces=6, use_bvh=True, sky_sampling=True)
    r.Resize(W, H); r.Accumulate(10)
    g = mirt.GroupRenderer(sc, devices=(0, 0), max_bounces=6, sky_sampling=True)
    assert g.sky_sampling() is True
    g.Resize(W, H); g.Accumulate(10)
    same_words(g.accumulator(), r.accumulator(), "a group of the same device twice")
    g.set_sky_sampling(False)
    assert g.sky_sampling() is False
    g.close(); r.close()
