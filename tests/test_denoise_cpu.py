"""The variance-guided à-trous denoised resolve without a GPU: the interface at every layer, mirt_atrous_defaults (host code), and the
properties of the binary32 twin (denoise_twin.py) — the definition's own sanity, checked where no kernel is involved."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import denoise_twin as dt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
u = 2.0 ** -24
MIRT_ERR_ARG = -1
NEW_NAMES = ("mirt_atrous_defaults", "mirt_render_atrous", "mirt_group_render_atrous")


def words(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ---- interface -----------------------------------------------------------------------------------------------------------------------------------
def test_denoise_interface_is_declared_at_every_layer(mirt):
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    declared = set(re.findall(r"^int\s+(mirt_\w+)\s*\(", header, flags=re.M))
    lib = mirt.load_library()
    raw = C.CDLL(mirt.LIB_PATH)
    for n in NEW_NAMES:
        assert n in declared, f"{n} is not declared (on one line) in include/mirt.h"
        assert hasattr(raw, n), f"{n} is not exported by libmirt.so"
        assert n in lib._declared, f"{n} is not bound in Python"
    assert {n for n in declared if "atrous" in n} == set(NEW_NAMES)
    assert "typedef struct mirt_denoise_params {" in header
    for text in ("THE DEFINITION", "1.0f / (1.0f + tz * tz)", "W >= 9/64", "writes mirt_render's frame word for word", "a function of the two slabs and the counts alone"):
        assert text in header, text
    assert C.sizeof(mirt.DenoiseParams) == 28 and mirt.DenoiseParams.sigma_lum.offset == 12 and mirt.DenoiseParams.albedo_floor.offset == 24
    for cls in (mirt.Renderer, mirt.GroupRenderer):
        assert callable(cls.render_denoised) and callable(cls.denoise_defaults)
        assert list(inspect.signature(cls.render_denoised).parameters)[1] == "out"
    host = open(os.path.join(mirt.CSRC, "mirt_host.hpp")).read()
    for member in ("RenderDenoised(", "static mirt_denoise_params DenoiseDefaults("):
        assert member in host
    headless = open(os.path.join(mirt.CSRC, "mirt_headless.cpp")).read()
    for option in ("--denoise", "--denoise-plain-out"):
        assert f'"{option}"' in headless
    makefile = open(os.path.join(mirt.CSRC, "Makefile")).read()
    assert re.search(r"^KERNEL_DEPS = .*\bdenoise\.hpp\b", makefile, flags=re.M)


def test_defaults_are_the_documented_values(mirt):
    lib = mirt.load_library()
    assert lib.mirt_atrous_defaults(None) == MIRT_ERR_ARG
    p = mirt.DenoiseParams(9, 9, 9, -1.0, -1.0, -1.0, -1.0)
    assert lib.mirt_atrous_defaults(C.byref(p)) == 0
    want = {"iterations": 5, "normal_squarings": 5, "demodulate": 1, "sigma_lum": float(f32(4.0)), "sigma_depth": float(f32(0.05)), "lum_floor": float(f32(1e-4)),
            "albedo_floor": 1.0 / 256.0}
    assert p.as_dict() == want and mirt.denoise_defaults() == want
    assert {k: float(f32(v)) if isinstance(v, float) else v for k, v in dt.DEFAULTS.items()} == want, "the twin starts from the same values"
    assert lib.mirt_render_atrous(None, C.byref(p), None) == MIRT_ERR_ARG and lib.mirt_group_render_atrous(None, C.byref(p), None) == MIRT_ERR_ARG


# ---- the twin's properties -------------------------------------------------------------------------------------------------------------------------
W, H, K, ACC = 48, 32, 5, 15
TILES = (W // 16) * (H // 16)
COUNTS = np.full(TILES, ACC, dtype=np.uint32)


def from_images(rgb_buckets, depth, normal, albedo):
    """Images -> slabs.  rgb_buckets (K, 3, H, W) per-bucket radiance sums; depth (H, W), normal (3, H, W), albedo (3, H, W) per-sample values."""
    def tiled(img):                                                             # (..., H, W) -> (TILES, ..., 256)
        lead = img.shape[:-2]
        a = img.reshape(lead + (H // 16, 16, W // 16, 16))
        a = np.moveaxis(a, (-4, -2), (0, 1)).reshape((TILES,) + lead + (256,))
        return a
    acc = tiled(np.asarray(rgb_buckets, dtype=f32))
    aov = np.concatenate([tiled(np.asarray(depth, dtype=f32)[None]), tiled(np.asarray(normal, dtype=f32)), tiled(np.asarray(albedo, dtype=f32))], axis=1) * f32(ACC)
    return np.ascontiguousarray(acc, dtype=f32), np.ascontiguousarray(aov, dtype=f32)


def noisy_radiance(rng, level=1.0):
    return (level * rng.uniform(0.5, 1.5, (K, 3, H, W))).astype(f32)


def flat_guides(depth=4.0, normal=(0.0, 0.0, 1.0), albedo=0.5):
    n = np.broadcast_to(np.asarray(normal, dtype=f32)[:, None, None], (3, H, W))
    return np.full((H, W), depth, dtype=f32), n.copy(), np.full((3, H, W), albedo, dtype=f32)


def test_layout_helper_round_trips():
    img = np.arange(H * W, dtype=f32).reshape(H, W)
    acc, _ = from_images(np.broadcast_to(img, (K, 3, H, W)), *flat_guides())
    assert np.array_equal(dt.to_image(acc[:, 0, 0], W, H), img)


def test_zero_iterations_without_demodulation_is_the_twin_of_render():
    rng = np.random.default_rng(1)
    rgb = noisy_radiance(rng)
    rgb[0, 1, 5, 7] = np.nan
    rgb[4, 2, 20, 40] = np.inf
    for k in (2, 4, 5, 16):
        acc, aov = from_images(np.broadcast_to(rgb[:1], (k, 3, H, W)) * rng.uniform(0.5, 1.5, (k, 3, H, W)).astype(f32), *flat_guides())
        counts = np.full(TILES, 3 * k, dtype=np.uint32)
        assert np.array_equal(words(dt.denoise(acc, aov, counts, 0.7, {"iterations": 0, "demodulate": 0}, W, H)), words(dt.render_frame(acc, counts, 0.7, W, H))), k
    acc, aov = from_images(rgb, *flat_guides())
    a, b = dt.denoise(acc, aov, COUNTS, 1.0, {"iterations": 0, "demodulate": 0}, W, H), dt.render_frame(acc, COUNTS, 1.0, W, H)
    assert np.array_equal(words(a), words(b))
    # the twin of render against float64: median of the bucket means, exposure, the ACES fit — a few ulps of a value in [0, 1]
    mean = np.median(rgb.astype(np.float64), axis=0) / (ACC // K)
    import definitions as df
    want = df.aces_fitted(np.moveaxis(mean, 0, -1).reshape(-1, 3)).reshape(H, W, 3)
    ok = np.isfinite(want).all(axis=-1)
    assert ok.sum() == H * W - 1                                                # the NaN pixel; an inf word never is the median of five
    assert np.abs(b[..., :3][ok] - want[ok]).max() < 64 * u


def test_a_constant_image_stays_constant():
    """Every x_q equals x_p, so X / W is x up to the rounding of the 25-term sums: |X / W - x| <= (25 + 1) u x to first order."""
    rgb = np.broadcast_to(np.array([0.3, 0.6, 0.2], dtype=f32)[None, :, None, None], (K, 3, H, W)).copy()
    rgb *= np.linspace(0.8, 1.2, K, dtype=f32)[:, None, None, None]             # the buckets differ, every pixel alike: v > 0 everywhere
    acc, aov = from_images(rgb, *flat_guides())
    for demodulate in (0, 1):
        st0 = dt.run(acc, aov, COUNTS, 1.0, {"iterations": 0, "demodulate": demodulate}, W, H)
        st5 = dt.run(acc, aov, COUNTS, 1.0, {"iterations": 5, "demodulate": demodulate}, W, H)
        assert st0["usable"].all() and float(st0["v"].min()) > 0
        for c in range(3):
            x0 = st0["x"][c].astype(np.float64)
            rel = np.abs(st5["x"][c].astype(np.float64) - x0) / x0
            print(f"[denoise] constant image, demodulate = {demodulate}, channel {c}: off by at most {rel.max() / u:.2f} u after five passes (bound {5 * 26} u)")
            assert rel.max() <= 5 * 26 * u


def halves(rng, depth=(4.0, 4.0), normal=((0.0, 0.0, 1.0), (0.0, 0.0, 1.0)), level=(1.0, 1.0)):
    rgb = noisy_radiance(rng)
    rgb[..., W // 2:] *= f32(level[1] / level[0])
    d, n, a = flat_guides()
    d[:, :W // 2], d[:, W // 2:] = depth
    for c in range(3):
        n[c, :, :W // 2], n[c, :, W // 2:] = normal[0][c], normal[1][c]
    return from_images(rgb, d, n, a)


def test_orthogonal_normals_never_mix():
    """nn = 0 across the border: the smoothed variance leaves such neighbours out, and a tap there has wn = 0, so w = 0 exactly and W + 0 = W,
    X + 0 * x = X, V + 0 = V word for word (finite x).  The other half might as well be absent."""
    acc, aov = halves(np.random.default_rng(2), normal=((0.0, 0.0, 1.0), (1.0, 0.0, 0.0)), level=(1.0, 8.0))
    whole = dt.run(acc, aov, COUNTS, 1.0, {}, W, H)
    left = np.zeros((H, W), dtype=bool); left[:, :W // 2] = True
    for side, mask in (("left", left), ("right", ~left)):
        alone = dt.run(acc, aov, COUNTS, 1.0, {}, W, H, force_unusable=~mask)
        for c in range(3):
            assert np.array_equal(words(whole["x"][c][mask]), words(alone["x"][c][mask])), side
        assert np.array_equal(words(whole["v"][mask]), words(alone["v"][mask])), side


def test_hit_against_miss_mixes_less_than_the_cauchy_bound():
    """Depths 1 and 1e4, the same normal, sigma_lum huge (the luminance stop open): a tap across the border at distance d = step * max(|dx|, |dy|)
    weighs at most h h / (1 + tz^2) with tz = 9999 / (0.05 * 1e4 * d) ~ 20 / d — so after one pass at step 1 a border pixel moves towards the
    other side by at most the summed bound over its cross-border taps, relative to W >= 9/64."""
    rng = np.random.default_rng(3)
    acc, aov = halves(rng, depth=(1.0, 1e4), level=(1.0, 16.0))
    params = {"iterations": 1, "sigma_lum": 1e6, "demodulate": 0}
    whole = dt.run(acc, aov, COUNTS, 1.0, params, W, H)
    left = np.zeros((H, W), dtype=bool); left[:, :W // 2] = True
    worst = 0.0
    for mask in (left, ~left):
        alone = dt.run(acc, aov, COUNTS, 1.0, params, W, H, force_unusable=~mask)
        for c in range(3):
            worst = max(worst, float(np.abs(whole["x"][c][mask].astype(np.float64) - alone["x"][c][mask]).max()))
    h5 = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16]
    tz = lambda d: 9999.0 / (0.05 * (1e4 * d) + 1.2e-38)
    cross = sum(h5[dy + 2] * h5[dx + 2] / (1.0 + tz(max(abs(dx), abs(dy))) ** 2) for dy in range(-2, 3) for dx in (1, 2))      # a pixel at the border: the taps on the far side
    bound = cross / (9 / 64) * 16.0 * 1.5 * 2                                   # weight share x the largest radiance there, both ways of (X + dX) / (W + dW)
    print(f"[denoise] hit against miss: a border pixel moves by at most {worst:.3e} (bound {bound:.3e})")
    assert 0 < worst < bound


def test_a_nan_centre_passes_through_and_is_absent_for_its_neighbours():
    rng = np.random.default_rng(4)
    rgb = noisy_radiance(rng)
    rgb[2, 1, 10, 20] = np.nan
    acc, aov = from_images(rgb, *flat_guides())
    out = dt.denoise(acc, aov, COUNTS, 1.0, {}, W, H)
    plain = dt.render_frame(acc, COUNTS, 1.0, W, H)
    assert np.array_equal(words(out[10, 20]), words(plain[10, 20])), "the word mirt_render writes"
    st = dt.run(acc, aov, COUNTS, 1.0, {}, W, H)
    assert not st["usable"][10, 20] and st["usable"].sum() == H * W - 1
    rgb[2, 1, 10, 20] = 1.0                                                     # the same image with a finite word there, and the pixel masked out
    acc2, aov2 = from_images(rgb, *flat_guides())
    gone = np.zeros((H, W), dtype=bool); gone[10, 20] = True
    masked = dt.denoise(acc2, aov2, COUNTS, 1.0, {}, W, H, force_unusable=gone)
    others = ~gone
    assert np.array_equal(words(out[others]), words(masked[others]))
    assert np.isfinite(out[others]).all()


def test_filtered_variance_never_exceeds_the_largest_input_variance():
    """v' = sum(w^2 v) / (sum w)^2 <= max v, since sum(w^2) <= (sum w)^2 for w >= 0; the roundings of up to 25 terms allow a few u."""
    rng = np.random.default_rng(5)
    rgb = noisy_radiance(rng) * (10.0 ** rng.uniform(-1, 1, (1, 1, H, W))).astype(f32)
    d, n, a = flat_guides()
    d[:] = rng.uniform(0.5, 50, (H, W))
    acc, aov = from_images(rgb, d, n, a)
    st = dt.prepare(acc, aov, COUNTS, 1.0, dict(dt.DEFAULTS), W, H)
    top = float(st["v"].max())
    for i in range(5):
        st["x"], st["v"] = dt.atrous_pass(st, 1 << i, dt.DEFAULTS)
        assert float(st["v"].max()) <= top * (1 + 64 * u), i
        assert float(st["v"].min()) >= 0
    assert float(st["v"].mean()) < 0.5 * top
