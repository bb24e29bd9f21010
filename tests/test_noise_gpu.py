"""The noise estimate on the GPU (mirt_noise, mirt_accumulate_until and their group twins; resolve.hpp k_noise) against the binary32 numpy
twin of noise_twin.py, which restates the quantity of include/mirt.h:

    y_j = scale * ((0.2126f * r_j + 0.7152f * g_j) + 0.0722f * b_j),  mean = (((y_0 + y_1) + ...) / (float)k,  d_j = y_j - mean,
    var = (((d_0 d_0 + d_1 d_1) + ...) / (float)(k - 1),  se = sqrt(var / (float)k),  e = (mean + floor == 0) ? 0 : se / (mean + floor)

Map, histogram, tile maximum and counts are compared on the raw words / as integers.  The tile mean is compared with the float64 mean of the
twin map's usable pixels within 255 u relative (u = 2^-24): a binary32 sum of 256 non-negative terms in ANY order is within 255 u of the
exact sum (Higham, gamma_255 to first order) — the kernel's fixed tree passes every term through 9 additions and one division, so it sits
near 10 u; the worst figure seen is printed."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import noise_twin as nt
from oracle_binding import bits

pytestmark = pytest.mark.gpu

f32 = np.float32
u = 2.0 ** -24
MIRT_OK, MIRT_NOT_READY, MIRT_NOT_CONVERGED, MIRT_ERR_ARG, MIRT_ERR_STATE = 0, 1, 2, -1, -3
SENTINEL = f32(-7.0)


def assert_same(got, want, what):
    got, want = bits(np.asarray(got)), bits(np.asarray(want))
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} words differ"


def check_against_twin(r, slab, accumulations, floor, tile_ids, what, exposure=1.0):
    """r.noise(floor) against the twin applied to `slab` (the context's accumulator, local tile order; tile_ids = their LaunchIndices)."""
    k = slab.shape[1]
    e = nt.noise_e(slab, nt.scale_of(exposure, accumulations, k), floor)
    buf = np.full((r.height, r.width), SENTINEL, dtype=f32)
    res = r.noise(floor=floor, map_out=buf)
    assert res is not None and res["map"] is buf
    assert_same(buf, nt.image(e, tile_ids, r.width, r.height, SENTINEL), f"{what}: map (pixels of no owned tile keep the sentinel)")
    assert np.array_equal(res["hist"], nt.histogram(e)), f"{what}: histogram"
    t_max, t_mean, n_ok, n_bad = nt.tile_records(e)
    tiles = res["tiles"]
    assert tiles.shape == (len(tile_ids), 4)
    assert_same(tiles[:, 0], t_max, f"{what}: tile maximum")
    assert np.array_equal(tiles[:, 2], n_ok.astype(f32)) and np.array_equal(tiles[:, 3], n_bad.astype(f32)), f"{what}: tile counts"
    err = np.abs(tiles[:, 1].astype(np.float64) - t_mean)
    worst = float((err / np.where(t_mean > 0, t_mean, 1.0)).max() / u) if len(tile_ids) else 0.0
    print(f"[noise] {what}: tile mean off by at most {worst:.2f} u (bound 255 u)")
    assert (err <= 255 * u * t_mean).all(), f"{what}: tile mean {worst:.1f} u off"
    want = nt.stats(e)
    for key in ("owned_pixels", "finite_pixels", "nonfinite_pixels"):
        assert res[key] == want[key], f"{what}: {key}"
    assert f32(res["max"]) == f32(want["max"]), f"{what}: max"
    total = 0.0
    for m, c in zip(tiles[:, 1], tiles[:, 2]):                                   # the documented double sum, ascending tile order
        total += float(m) * float(c)
    assert res["mean"] == (total / want["finite_pixels"] if want["finite_pixels"] else 0.0), f"{what}: mean is not the documented double sum"
    assert abs(res["mean"] - want["mean"]) <= 256 * u * want["mean"]
    return res, e


def make_renderer(mirt, w, h, k, **kw):
    r = mirt.Renderer(mirt.scene.default9(), buckets=k, **kw)
    r.Resize(w, h)
    return r


# ---- synthetic slabs -------------------------------------------------------------------------------------------------------------
def synthetic_slabs(rng, tiles, k):
    """name -> (slab, floor)"""
    pos = (10.0 ** rng.uniform(-2, 2, (tiles, 1, 3, 256)) * rng.uniform(0.2, 1.8, (tiles, k, 3, 256))).astype(f32)
    out = {"random positive": (pos, 0.0), "random positive, floor": (pos, 0.125)}
    out["all zero, floor 0"] = (np.zeros_like(pos), 0.0)
    fire = pos.copy(); fire[:, k - 1] *= f32(1e6)
    out["one bucket 1e6 times the others"] = (fire, 0.0)
    out["denormals"] = ((pos * f32(1e-41)).astype(f32), 0.0)
    equal = np.repeat(pos[:, :1], k, axis=1).copy()
    out["equal buckets"] = (equal, 0.0)
    bad = pos.copy(); bad[0, 0, 1, 3] = np.nan; bad[tiles - 1, k - 1, 2, 200] = np.inf
    out["one NaN and one inf word"] = (bad, 0.0)
    return out


@pytest.mark.parametrize("k", [2, 3, 5, 16])
@pytest.mark.parametrize("w,h", [(64, 48), (16, 16), (70, 50)])
def test_synthetic_slabs_equal_the_twin(mirt, w, h, k):
    tiles = (w // 16) * (h // 16)
    rng = np.random.default_rng(1000 * k + w)
    r = make_renderer(mirt, w, h, k)
    slabs = synthetic_slabs(rng, tiles, k)
    assert (slabs["denormals"][0] > 0).any() and (slabs["denormals"][0] < f32(1.2e-38)).all()
    acc = 3 * k                                                                   # scale = 1 / 3: not a power of two
    for name, (slab, floor) in slabs.items():
        r.load_accumulator(slab, acc)
        res, e = check_against_twin(r, slab, acc, floor, list(range(tiles)), f"{w}x{h}, k = {k}, {name}")
        if name == "all zero, floor 0" or (name == "equal buckets" and k == 2):
            assert not e.view(np.uint32).any() and res["max"] == 0.0 and res["hist"][0] == tiles * 256      # exactly 0 (the 0 / 0 rule; y + y and / 2 are exact: d_j = 0)
        if name == "equal buckets":
            # k equal y: the binary32 sum ((y + y) + y) + ... and its division by k round, so the mean may sit a few ulps off y for k > 2:
            # |mean - y| <= k u y, d_j = y - mean is exact (Sterbenz) and the same for every j, se = |d| / sqrt(k - 1) <= |d|: e <= (k + 1) u.
            # What the GPU gives is still the twin's word (checked above); "exactly 0" holds where the sums are exact.
            assert float(e.max()) <= (k + 1) * u and res["max"] <= (k + 1) * u and res["nonfinite_pixels"] == 0
        if name == "one NaN and one inf word":
            clean, _ = slabs["random positive"]
            r.load_accumulator(clean, acc)
            ref = r.noise(floor=floor)
            assert res["nonfinite_pixels"] == 2 and res["finite_pixels"] == tiles * 256 - 2
            e_clean = nt.noise_e(clean, nt.scale_of(1.0, acc, k), floor)
            gone = np.zeros(nt.BINS, dtype=np.int64)
            for t, px in ((0, 3), (tiles - 1, 200)):
                gone[e_clean[t, px].view(np.uint32) >> 20] += 1
            assert np.array_equal(ref["hist"].astype(np.int64) - gone, res["hist"]), "the histogram lost exactly the two unusable pixels"
            others = np.ones((tiles, 256), dtype=bool); others[0, 3] = others[tiles - 1, 200] = False
            assert f32(res["max"]) == e_clean[others].max(), "the maximum is that of the other pixels"
    r.close()


def test_status_codes(mirt):
    r = make_renderer(mirt, 64, 48, 1)
    lib, ctx = r._lib, r._ctx
    r.Accumulate(2)
    assert lib.mirt_noise(ctx, 0.0, None, None, None, None) == MIRT_ERR_STATE and b"buckets >= 2" in lib.mirt_last_error(ctx)
    rule = mirt.StopRule(0.5, 0.95, 0.0, 5, 100)
    assert lib.mirt_accumulate_until(ctx, C.byref(rule), None, None) == MIRT_ERR_STATE
    r.close()
    r = make_renderer(mirt, 64, 48, 5)
    lib, ctx = r._lib, r._ctx
    buf, tiles, hist = np.full((48, 64), SENTINEL, dtype=f32), np.full((12, 4), SENTINEL, dtype=f32), np.full(nt.BINS, 77, dtype=np.uint32)
    st = mirt.NoiseStats(); st.owned_pixels = 99
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda floor: lib.mirt_noise(ctx, floor, ptr(buf), ptr(tiles), ptr(hist), C.byref(st))
    untouched = lambda: (buf == SENTINEL).all() and (tiles == SENTINEL).all() and (hist == 77).all() and st.owned_pixels == 99
    assert call(0.0) == MIRT_NOT_READY and untouched() and r.noise() is None       # 0 accumulations
    r.Accumulate(7)
    assert call(0.0) == MIRT_NOT_READY and untouched()                              # 7 accumulations at k = 5
    assert lib.mirt_accumulate_until(ctx, C.byref(mirt.StopRule(0.5, 0.95, 0.0, 5, 100)), None, None) == MIRT_ERR_STATE and b"not a multiple" in lib.mirt_last_error(ctx)
    r.Accumulate(3)
    for bad in (-1.0, -1e-30, float("nan"), float("inf")):
        assert call(bad) == MIRT_ERR_ARG and untouched(), bad
    for rule in (mirt.StopRule(0.5, 0.95, 0.0, 7, 100), mirt.StopRule(0.5, 0.95, 0.0, 0, 100), mirt.StopRule(0.5, 0.0, 0.0, 5, 100), mirt.StopRule(0.5, 1.5, 0.0, 5, 100),
                 mirt.StopRule(-0.5, 0.95, 0.0, 5, 100), mirt.StopRule(0.5, 0.95, float("nan"), 5, 100)):
        assert lib.mirt_accumulate_until(ctx, C.byref(rule), None, None) == MIRT_ERR_ARG
    assert r.accumulations == 10
    assert call(0.0) == MIRT_OK and st.owned_pixels == 12 * 256 and not (buf == SENTINEL).any()
    assert lib.mirt_noise(ctx, 0.0, None, None, None, None) == MIRT_OK               # every output is optional
    r.SetTileRange(0, 0)                                                             # a context that owns no tile
    r.Accumulate(5)
    res = r.noise(want_map=True)
    assert res["owned_pixels"] == res["finite_pixels"] == res["nonfinite_pixels"] == 0 and not res["hist"].any() and res["tiles"].shape == (0, 4) and not res["map"].any()
    r.close()


# ---- rendered scenes ---------------------------------------------------------------------------------------------------------------
W, H, N_ACC = 64, 48, 10
ALL_TILES = list(range((W // 16) * (H // 16)))
SCENES = {"default9": lambda m: m.scene.default9(), "S1000": lambda m: m.scene.synthetic(1000, ambient=0.5)}
FLOOR = 0.01


def rendered(mirt, scene, asynchronous=False, **kw):
    r = mirt.Renderer(SCENES[scene](mirt), **kw)
    r.Resize(W, H)
    if asynchronous:
        r.AccumulateAsync(5); r.AccumulateAsync(5)
    else:
        r.Accumulate(N_ACC)
    return r


def same_result(a, b, what):
    assert_same(a["map"], b["map"], f"{what}: map")
    assert np.array_equal(a["hist"], b["hist"]), f"{what}: histogram"
    assert_same(a["tiles"], b["tiles"], f"{what}: tile records")
    for key in ("owned_pixels", "finite_pixels", "nonfinite_pixels", "max", "mean"):
        assert a[key] == b[key], f"{what}: {key}"


@pytest.mark.parametrize("scene", list(SCENES))
def test_rendered_scene_does_not_depend_on_launch_shape(mirt, scene):
    base_r = rendered(mirt, scene)
    exposure = float(base_r.scene.camera.exposure)
    base, _ = check_against_twin(base_r, base_r.accumulator(), N_ACC, FLOOR, ALL_TILES, f"{scene}", exposure)
    assert base["finite_pixels"] == W * H and base["max"] > 0
    base_r.close()
    same = {"max_batch=1": dict(max_batch=1), "max_batch=5": dict(max_batch=5), "max_batch=0": dict(max_batch=0), "streams=1": dict(streams=1), "streams=3": dict(streams=3),
            "2 x AccumulateAsync(5)": dict(asynchronous=True), "use_bvh": dict(use_bvh=True), "aov": dict(aov=True)}
    for label, kw in same.items():
        r = rendered(mirt, scene, **kw)
        same_result(r.noise(floor=FLOOR, want_map=True), base, f"{scene}, {label}")
        r.close()
    # modes that render another image: the twin applied to that mode's own accumulator
    for label, kw, after in (("brdf=1", dict(brdf=1), None), ("exact stream order", dict(exact_stream_order=True), None), ("lens", dict(), "lens")):
        r = mirt.Renderer(SCENES[scene](mirt), **kw)
        r.Resize(W, H)
        if after == "lens":
            r.set_lens(0.05, 3.0)
            assert r.lens()[0] > 0
        r.Accumulate(N_ACC)
        res, _ = check_against_twin(r, r.accumulator(), N_ACC, FLOOR, ALL_TILES, f"{scene}, {label}", exposure)
        if label != "exact stream order":                                          # (that mode's words differ from the wavefront's in a few pixels only)
            assert not np.array_equal(res["hist"], base["hist"]), f"{label} renders another image"
        r.close()


def test_partitions_and_group_equal_the_whole(mirt):
    single = rendered(mirt, "S1000", use_bvh=True)
    whole = single.noise(floor=FLOOR, want_map=True)
    h_tiles, v_tiles = W // 16, H // 16
    painted = np.full((H, W), SENTINEL, dtype=f32)
    hist = np.zeros(nt.BINS, dtype=np.uint32)
    tiles = np.zeros((v_tiles, h_tiles, 4), dtype=f32)
    counts = {"owned_pixels": 0, "finite_pixels": 0, "nonfinite_pixels": 0}
    for rank in range(2):
        r = mirt.Renderer(SCENES["S1000"](mirt), use_bvh=True)
        r.Resize(W, H); r.SetTileRows(rank, 2); r.Accumulate(N_ACC)
        ids = [row * h_tiles + x for row in range(rank, v_tiles, 2) for x in range(h_tiles)]
        part, _ = check_against_twin(r, r.accumulator(), N_ACC, FLOOR, ids, f"rank {rank} of 2")
        assert (r.noise(floor=FLOOR, map_out=painted))["map"] is painted          # only the context's own tiles are written
        hist += part["hist"]
        tiles[rank::2] = part["tiles"].reshape(-1, h_tiles, 4)
        for key in counts:
            counts[key] += part[key]
        r.close()
    assert_same(painted, whole["map"], "two contexts with interleaved tile rows: map")
    assert np.array_equal(hist, whole["hist"]) and all(counts[k] == whole[k] for k in counts)
    assert_same(tiles.reshape(-1, 4), whole["tiles"], "two contexts with interleaved tile rows: tile records")
    g = mirt.GroupRenderer(SCENES["S1000"](mirt), devices=[0, 0, 0], use_bvh=True)
    g.Resize(W, H)
    assert g.noise() is None
    g.Accumulate(N_ACC)
    same_result(g.noise(floor=FLOOR, want_map=True), whole, "GroupRenderer(devices=[0, 0, 0])")
    g.close()
    single.close()


def test_noise_changes_no_state(mirt):
    r = rendered(mirt, "default9", count_traffic=True)
    assert r.Render()
    before = (r.accumulator().copy(), r.GetFrame().copy(), r.counters(), r.accumulations)
    for floor in (0.0, 0.5):
        assert r.noise(floor=floor, want_map=True) is not None
    assert r.Render()
    assert_same(r.accumulator(), before[0], "accumulator after mirt_noise")
    assert_same(r.GetFrame(), before[1], "frame after mirt_noise")
    assert r.counters() == before[2] and r.accumulations == before[3]
    r.close()


# ---- statistical soundness ---------------------------------------------------------------------------------------------------------
def test_statistical_soundness_on_the_filling_sphere(mirt):
    """The filling-sphere scene of DESIGN.md §2 part E (grey albedo 0.6): every sample of every pixel is v = 1 with probability p = 0.6 and
    0 otherwise, independently, in all three channels, so the luminance sample is v (the three weights sum to 1 within 1 u).  With k = 5
    buckets and n accumulations a bucket mean is X_j = v B_j / m, B_j ~ Binomial(m = n / k, p), variance s_b^2 = v^2 p q / m (q = 1 - p).

    (a) se^2 = s^2 / k with s^2 the unbiased sample variance of the k bucket means, so E[se^2] = v^2 p q / n EXACTLY.  Read with
        floor F = 1000 >> v the denominator is F + mean, within [F, F + v]: E[e^2] (F + p v)^2 = v^2 p q / n within 2 v / F = 0.2 %.
        Var(s^2) = mu4 / k - s_b^4 (k - 3) / (k (k - 1)) with the binomial's mu4 = (v / m)^4 m p q (1 + 3 (m - 2) p q); pixels are
        independent, so sigma of the image mean of se^2 over P = 64^2 pixels is sqrt(Var(s^2) / k^2 / P): 1.1 % of the expectation.
    (b) se is proportional to 1 / sqrt(m): the median of e over the pixels at n and at 4 n differ by a factor 2.  For bucket means close to
        normal (m = 20 and 80) (k - 1) s^2 / s_b^2 is chi-square with nu = k - 1 = 4 degrees of freedom; L = log e = log(chi^2) / 2 + const
        has density f_L = 2 x f_chi2(x) at chi^2 = x; at the median x = 3.3567 that is 2 * 3.3567 * (x / 4) exp(-x / 2) = 1.052.  A sample
        median of P values has standard error 1 / (2 f_L sqrt(P)) = 0.00743 in L; the log of the ratio of two independent medians has
        sigma = sqrt(2) * 0.00743 = 0.0105.  (The binomial's skew and the noise of the denominator at floor 0 move the population ratio
        to 2.006 — a third of one sigma.)
    Both within 5 sigma; the z-scores are printed."""
    import test_definitions_cpu as cpu
    p, v, k, P = 0.6, 1.0, 5, 64 * 64
    q = 1.0 - p
    F = 1000.0
    med, z_e2 = {}, {}
    for n in (100, 400):
        r = mirt.Renderer(cpu.one_sphere(mirt, albedo=(0.6, 0.6, 0.6)), max_bounces=8, buckets=k)
        r.Resize(64, 64)
        r.Accumulate(n)
        rel = r.noise(floor=0.0, want_map=True)
        far = r.noise(floor=F, want_map=True)
        r.close()
        assert rel["finite_pixels"] == far["finite_pixels"] == P
        med[n] = float(np.median(rel["map"].astype(np.float64)))
        m = n // k
        s_b2 = v * v * p * q / m
        mu4 = (v / m) ** 4 * m * p * q * (1 + 3 * (m - 2) * p * q)
        var_s2 = mu4 / k - s_b2 ** 2 * (k - 3) / (k * (k - 1))
        sigma = math.sqrt(var_s2 / k ** 2 / P)
        want = v * v * p * q / n
        got = float((far["map"].astype(np.float64) ** 2).mean()) * (F + p * v) ** 2
        z_e2[n] = (got - want) / sigma
        assert abs(got - want) <= 5 * sigma + (2 * v / F) * want, f"n = {n}: image mean of se^2 {got:.6g} vs {want:.6g}, z = {z_e2[n]:+.2f}"
    sigma_log = math.sqrt(2.0) / (2.0 * 1.052 * math.sqrt(P))
    z_med = (math.log(med[100] / med[400]) - math.log(2.0)) / sigma_log
    print(f"[noise] filling sphere: median ratio {med[100] / med[400]:.4f} (z = {z_med:+.2f}), image mean of e^2: z = {z_e2[100]:+.2f} at n = 100, {z_e2[400]:+.2f} at n = 400")
    assert abs(z_med) <= 5, f"median of e fell by {med[100] / med[400]:.4f} from n = 100 to 400, z = {z_med:+.2f}"


# ---- accumulate_until --------------------------------------------------------------------------------------------------------------
RULE = dict(target=0.3, quantile=0.9, floor=0.05, check_every=5, max_accumulations=400)


def test_accumulate_until(mirt):
    r = make_renderer(mirt, W, H, 5)
    out = r.accumulate_until(**RULE)
    print(f"[noise] accumulate_until on default9 {W}x{H}: {out}")
    assert out["converged"] and 0 < out["issued"] < RULE["max_accumulations"] and out["issued"] % 5 == 0 and r.accumulations == out["issued"]
    res = r.noise(floor=RULE["floor"])
    assert out["nonfinite_pixels"] == 0 and {k: res[k] for k in ("max", "mean", "finite_pixels")} == {k: out[k] for k in ("max", "mean", "finite_pixels")}
    assert mirt.noise_quantile(res["hist"], float(f32(RULE["quantile"]))) <= f32(RULE["target"])
    if out["issued"] > 5:                                                           # one check earlier it had not converged yet
        e = mirt.Renderer(mirt.scene.default9(), buckets=5); e.Resize(W, H); e.Accumulate(out["issued"] - 5)
        assert mirt.noise_quantile(e.noise(floor=RULE["floor"])["hist"], float(f32(RULE["quantile"]))) > f32(RULE["target"])
        e.close()
    fresh = make_renderer(mirt, W, H, 5)
    fresh.Accumulate(out["issued"])
    assert_same(r.accumulator(), fresh.accumulator(), "accumulator after accumulate_until vs the same number of plain accumulations")
    fresh.close()
    # an unreachable target: MIRT_NOT_CONVERGED at exactly max_accumulations (the last step is shortened: 10 + 5)
    r.ResetAccumulator()
    st, issued = mirt.NoiseStats(), C.c_uint32(0)
    rule = mirt.StopRule(0.0, 0.9, 0.05, 10, 17)
    assert r._lib.mirt_accumulate_until(r._ctx, C.byref(rule), C.byref(st), C.byref(issued)) == MIRT_NOT_CONVERGED
    assert issued.value == 15 and r.accumulations == 15 and st.finite_pixels == W * H
    again = r.accumulate_until(target=0.0, quantile=0.9, floor=0.05, check_every=10, max_accumulations=15)
    assert not again["converged"] and again["issued"] == 0 and r.accumulations == 15
    with pytest.raises(mirt.MirtError, match="multiple of buckets"):
        r.accumulate_until(target=0.3, check_every=7)
    r.close()
    g = mirt.GroupRenderer(mirt.scene.default9(), devices=[0, 0, 0], buckets=5, use_bvh=False)
    g.Resize(W, H)
    got = g.accumulate_until(**RULE)
    assert got == out, "the group twin stops where the single context does, with the same stats"
    with pytest.raises(mirt.MirtError, match="multiple of buckets"):
        g.accumulate_until(target=0.3, check_every=7)
    g.close()


# ---- headless host -----------------------------------------------------------------------------------------------------------------
def test_headless_until_noise_writes_the_map(mirt, tmp_path):
    exe = os.path.join(mirt.CSRC, "mirt_headless")
    path = str(tmp_path / "noise.pfm")
    run = subprocess.run([exe, "--scene", "default9", "--size", f"{W}x{H}", "--until-noise", str(RULE["target"]), "--noise-quantile", str(RULE["quantile"]),
                          "--noise-floor", str(RULE["floor"]), "--check-every", str(RULE["check_every"]), "--max-accumulations", str(RULE["max_accumulations"]),
                          "--noise-out", path], check=True, capture_output=True, text=True)
    lines = run.stdout.strip().splitlines()
    report, stats = json.loads(lines[-2]), json.loads(lines[-1])["noise"]
    r = mirt.Renderer(mirt.scene.default9(), use_bvh=True)
    r.Resize(W, H)
    out = r.accumulate_until(**RULE)
    res = r.noise(floor=RULE["floor"], want_map=True)
    assert stats["converged"] is True and stats["issued"] == out["issued"] == report["accumulations"] and report["frame_ready"] is True
    assert stats["finite_pixels"] == W * H and stats["nonfinite_pixels"] == 0 and stats["mean"] == res["mean"] and f32(stats["max"]) == f32(res["max"])
    assert f32(stats["quantile_value"]) == f32(mirt.noise_quantile(res["hist"], float(f32(RULE["quantile"])))) and stats["quantile_value"] <= RULE["target"]
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        assert [int(x) for x in f.readline().split()] == [W, H]
        assert float(f.readline()) < 0
        data = np.frombuffer(f.read(), dtype="<f4").reshape(H, W)
    assert_same(data, res["map"], "noise.pfm vs Renderer.noise()")
    r.close()


def test_headless_noise_without_the_stopping_loop(mirt, tmp_path):
    """--noise-out after a fixed --spp: no stopping loop ran, so "converged" and "issued" are null; a sample count that gives no estimate
    fails the run before anything is printed or written."""
    exe = os.path.join(mirt.CSRC, "mirt_headless")
    path, frame = str(tmp_path / "noise.pfm"), str(tmp_path / "frame.pfm")
    run = subprocess.run([exe, "--scene", "default9", "--size", f"{W}x{H}", "--spp", "10", "--noise-floor", "0.05", "--noise-out", path], check=True, capture_output=True, text=True)
    stats = json.loads(run.stdout.strip().splitlines()[-1])["noise"]
    assert stats["converged"] is None and stats["issued"] is None and stats["finite_pixels"] == W * H and os.path.getsize(path) > W * H * 4
    bad = subprocess.run([exe, "--scene", "default9", "--size", f"{W}x{H}", "--spp", "7", "--noise-out", path + "2", "--out", frame], capture_output=True, text=True)
    assert bad.returncode == 1 and "no noise estimate" in bad.stderr and bad.stdout == "" and not os.path.exists(path + "2") and not os.path.exists(frame)
