"""The variance-guided à-trous denoised resolve on the GPU (mirt_render_atrous / mirt_group_render_atrous; csrc/denoise.hpp) against the binary32
numpy twin of denoise_twin.py, which restates THE DEFINITION of include/mirt.h operation for operation: frames are compared on their raw
words.  Then what the definition promises — iterations = 0 with demodulate = 0 is mirt_render's frame, no state changes, the result is a function
of the slabs and the counts alone (batching, streams, a group's gather) — the refusals, and the direction of the claim: a noisy frame gets closer
to a converged reference, a converged frame stays where it is.

RMSE figures of the last two tests are printed, never bounded by a ratio: none has been promised (profiles/denoise.txt records them)."""
import ctypes as C

import numpy as np
import pytest

import denoise_twin as dt
from oracle_binding import bits

pytestmark = pytest.mark.gpu

f32 = np.float32
MIRT_OK, MIRT_NOT_READY, MIRT_ERR_ARG, MIRT_ERR_STATE = 0, 1, -1, -3
SENTINEL = f32(-7.0)


def assert_same(got, want, what):
    got, want = bits(np.asarray(got)), bits(np.asarray(want))
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    bad = got != want
    n = int(bad.sum())
    where = np.argwhere(bad)[:4].tolist() if n else []
    assert n == 0, f"{what}: {n} of {got.size} words differ, first at {where}: got {[hex(int(got[tuple(i)])) for i in where]}, want {[hex(int(want[tuple(i)])) for i in where]}"


# ---- synthetic slabs ---------------------------------------------------------------------------------------------------------------------------
def synthetic(w, h, k, seed):
    """-> (accumulator slab, AOV slab, accumulations).  Random positive radiance with a few 1e6 fireflies, a block of denormals, one NaN and one
    inf bucket word; guides mix hit pixels (unit normals in several directions, depths 0.5 .. 50, albedo channels on both sides of 1/256) with
    miss pixels (zero normal, depth 1e4, no albedo).  The AOV slab holds sums over `accumulations` samples, as the library's does."""
    rng = np.random.default_rng(seed)
    tiles = (w // 16) * (h // 16)
    acc_n = 3 * k                                                                 # scale = 1 / 3: not a power of two
    slab = (10.0 ** rng.uniform(-2, 1, (tiles, 1, 3, 256)) * rng.uniform(0.2, 1.8, (tiles, k, 3, 256))).astype(f32)
    for _ in range(6):                                                            # fireflies: one bucket of a pixel, all three channels
        slab[rng.integers(tiles), rng.integers(k), :, rng.integers(96, 256)] *= f32(1e6)     # (not in the denormal row below)
    slab[tiles - 1, :, :, 64:80] *= f32(1e-41)                                    # a row of denormal pixels
    assert (slab[tiles - 1, :, :, 64:80] < f32(1.2e-38)).all()
    slab[0, 0, 1, 3] = np.nan
    slab[tiles - 1, k - 1, 2, 200] = np.inf
    aov = np.zeros((tiles, 7, 256), dtype=f32)
    hit = rng.uniform(size=(tiles, 256)) < 0.7
    axes = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0.6, 0.0, 0.8], [-0.36, 0.48, 0.8]])
    n = axes[rng.integers(len(axes), size=(tiles, 256))] + rng.normal(scale=0.05, size=(tiles, 256, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    aov[:, 0] = np.where(hit, rng.uniform(0.5, 50.0, (tiles, 256)), 1e4) * acc_n
    aov[:, 1:4] = np.where(hit[:, None, :], np.moveaxis(n, 2, 1), 0.0) * acc_n
    alb = np.where(rng.uniform(size=(tiles, 3, 256)) < 0.25, rng.uniform(0.0, 1.0 / 256.0, (tiles, 3, 256)), rng.uniform(0.05, 1.0, (tiles, 3, 256)))
    aov[:, 4:7] = np.where(hit[:, None, :], alb, 0.0) * acc_n
    return slab, aov.astype(f32), acc_n


def loaded(mirt, w, h, k, slab, aov, acc_n, counts=None):
    r = mirt.Renderer(mirt.scene.default9(), buckets=k, aov=True)
    r.Resize(w, h)
    r.load_accumulator(slab, acc_n)
    r.load_aov(aov)
    if counts is not None:
        r.load_tile_counts(counts)
    return r


PARAM_SETS = [{"iterations": i, "demodulate": d} for i in (0, 1, 2, 3, 5) for d in (0, 1)]


@pytest.mark.parametrize("k", [2, 5, 16])
@pytest.mark.parametrize("w,h", [(48, 32), (16, 16)])
def test_synthetic_slabs_equal_the_twin(mirt, w, h, k):
    """48 x 32: 3 x 2 tiles — every pixel has taps that leave the image at step 16, taps cross tile borders both ways; 16 x 16: one tile.
    Iterations 0 .. 5 cover both k_atrous variants (staged for steps 1 and 2, direct from step 4) and the hand-over between them."""
    slab, aov, acc_n = synthetic(w, h, k, 100 * k + w)
    tiles = slab.shape[0]
    counts = np.full(tiles, acc_n, dtype=np.uint32)
    r = loaded(mirt, w, h, k, slab, aov, acc_n)
    st = dt.prepare(slab, aov, counts, 1.0, dict(dt.DEFAULTS), w, h)
    assert 2 <= int((~st["usable"]).sum()) <= 8 and st["usable"].sum() > 200, "the NaN and the inf pixel are unusable, and few others"
    st0 = dt.prepare(slab, aov, counts, 1.0, dict(dt.DEFAULTS, demodulate=1), w, h)
    assert any((m == 1).any() and (m != 1).any() for m in st0["m"]), "albedo channels on both sides of albedo_floor"
    for params in PARAM_SETS:
        got = r.render_denoised(**params)
        assert got is not None
        assert_same(got, dt.denoise(slab, aov, counts, 1.0, params, w, h), f"{w}x{h}, k = {k}, {params}")
    wide = {"iterations": 5, "sigma_lum": 64.0, "sigma_depth": 4.0, "normal_squarings": 0, "albedo_floor": 0.5}       # every weight far from 0: the sums matter
    assert_same(r.render_denoised(**wide), dt.denoise(slab, aov, counts, 1.0, wide, w, h), f"{w}x{h}, k = {k}, wide stops")
    r.close()


def test_unequal_tile_counts_equal_the_twin(mirt):
    """Two tiles frozen at a lower multiple of `buckets`: every tile resolves at its own count, signal, variance and guides alike."""
    w, h, k = 48, 32, 5
    slab, aov, acc_n = synthetic(w, h, k, 77)
    counts = np.full(6, acc_n, dtype=np.uint32)
    counts[1] = counts[4] = 2 * k
    r = loaded(mirt, w, h, k, slab, aov, acc_n, counts)
    assert np.array_equal(r.tile_counts(), counts)
    for params in ({"iterations": 0, "demodulate": 0}, {"iterations": 3}, {}):
        assert_same(r.render_denoised(**params), dt.denoise(slab, aov, counts, 1.0, params, w, h), f"unequal counts, {params}")
    even = dt.denoise(slab, aov, np.full(6, acc_n, dtype=np.uint32), 1.0, {}, w, h)
    assert not np.array_equal(bits(even), bits(r.render_denoised())), "the counts matter"
    r.close()


def test_odd_image_size_writes_only_the_tiled_pixels(mirt):
    """70 x 50: the tiles cover 64 x 48; "the image" of the definition is that part, the caller's other pixels are left alone."""
    w, h, k = 70, 50, 5
    slab, aov, acc_n = synthetic(w, h, k, 5)
    r = loaded(mirt, w, h, k, slab, aov, acc_n)
    buf = np.full((h, w, 4), SENTINEL, dtype=f32)
    assert r.render_denoised(out=buf, iterations=3) is buf
    want = dt.denoise(slab, aov, np.full(12, acc_n, dtype=np.uint32), 1.0, {"iterations": 3}, w, h)
    want[48:, :, :] = SENTINEL
    want[:, 64:, :] = SENTINEL
    assert_same(buf, want, "70x50")
    r.close()


# ---- rendered scenes ---------------------------------------------------------------------------------------------------------------------------
W = H = 64


def rendered(mirt, n_acc=10, sc=None, **kw):
    r = mirt.Renderer(sc if sc is not None else mirt.scene.synthetic(8), buckets=5, max_bounces=5, use_bvh=True, aov=True, **kw)
    r.Resize(W, H)
    r.Accumulate(n_acc)
    return r


def test_zero_iterations_without_demodulation_is_render(mirt):
    r = rendered(mirt)
    assert r.Render()
    plain = r.GetFrame().copy()
    assert_same(r.render_denoised(iterations=0, demodulate=0), plain, "iterations = 0, demodulate = 0 against Render()")
    assert not np.array_equal(bits(r.render_denoised()), bits(plain)), "the defaults do filter"
    r.close()


def test_no_state_is_changed(mirt):
    r = rendered(mirt)
    assert r.Render()
    before = (r.accumulator().copy(), r.aov().copy(), r.counters(), r.GetFrame().copy(), r.accumulations, r.tile_counts().copy())
    for params in ({}, {"iterations": 2, "demodulate": 0}):
        assert r.render_denoised(**params) is not None
    assert r.Render()
    after = (r.accumulator(), r.aov(), r.counters(), r.GetFrame(), r.accumulations, r.tile_counts())
    assert_same(after[0], before[0], "accumulator")
    assert_same(after[1], before[1], "AOV slab")
    assert after[2] == before[2] and after[4] == before[4] and np.array_equal(after[5], before[5])
    assert_same(after[3], before[3], "Render() afterwards")
    r.Accumulate(5)                                                              # and the context goes on as one that never denoised
    other = rendered(mirt, 15)
    assert_same(r.accumulator(), other.accumulator(), "accumulator after five more accumulations")
    r.close(); other.close()


def test_result_does_not_depend_on_batching_or_streams(mirt):
    frames = []
    for kw in ({"max_batch": 1, "streams": 1}, {"max_batch": 8, "streams": 3}, {"max_batch": 8, "streams": 1, "use_bvh": False}):
        r = mirt.Renderer(mirt.scene.synthetic(8), buckets=5, max_bounces=5, aov=True, **{"use_bvh": True, **kw})
        r.Resize(W, H)
        r.Accumulate(10)
        frames.append(r.render_denoised())
        r.close()
    assert_same(frames[1], frames[0], "max_batch 8 / streams 3 against 1 / 1")
    assert_same(frames[2], frames[0], "brute force against the tree")
    # ... and on nothing but the slabs: the twin from the read-back slabs gives the same words
    r = rendered(mirt)
    assert_same(frames[0], dt.denoise(r.accumulator(), r.aov(), r.tile_counts(), r.scene.camera.exposure, {}, W, H), "rendered slabs through the twin")
    r.close()


def test_group_split_by_tile_rows_gives_the_single_context_words(mirt):
    single = rendered(mirt)
    want = single.render_denoised()
    g = mirt.GroupRenderer(mirt.scene.synthetic(8), devices=[0, 0], buckets=5, max_bounces=5, use_bvh=True, aov=True)
    g.Resize(W, H)
    buf = np.full((H, W, 4), SENTINEL, dtype=f32)
    assert g.render_denoised(out=buf) is None and (buf == SENTINEL).all()
    g.Accumulate(10)
    assert_same(g.render_denoised(), want, "GroupRenderer(devices=[0, 0]).render_denoised()")
    assert_same(g.render_denoised(iterations=2, sigma_lum=1.0), single.render_denoised(iterations=2, sigma_lum=1.0), "other parameters")
    g.close(); single.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def raw_call(mirt, r, buf, **params):
    d = mirt.denoise_defaults()
    d.update(params)
    p = mirt.DenoiseParams(*(d[n] for n, _ in mirt.DenoiseParams._fields_))
    return r._lib.mirt_render_atrous(r._ctx, C.byref(p), buf.ctypes.data_as(C.c_void_p))


def test_refusals(mirt):
    sc = mirt.scene.default9()
    buf = np.full((32, 48, 4), SENTINEL, dtype=f32)

    r = mirt.Renderer(sc, buckets=5)                                             # AOVs off
    r.Resize(48, 32); r.Accumulate(5)
    assert raw_call(mirt, r, buf) == MIRT_ERR_STATE and b"AOVs are off" in r._lib.mirt_last_error(r._ctx)
    with pytest.raises(mirt.MirtError):
        r.render_denoised()
    r.close()

    r = mirt.Renderer(sc, buckets=1, aov=True)                                   # no spread to read a variance from
    r.Resize(48, 32); r.Accumulate(2)
    assert raw_call(mirt, r, buf) == MIRT_ERR_STATE and b"buckets >= 2" in r._lib.mirt_last_error(r._ctx)
    r.close()

    r = mirt.Renderer(sc, buckets=5, aov=True)                                   # part of the image
    r.Resize(48, 32)
    r.SetTileRange(0, 3); r.Accumulate(5)
    assert raw_call(mirt, r, buf) == MIRT_ERR_STATE and b"owns 3 of the image's 6 tiles" in r._lib.mirt_last_error(r._ctx)
    r.SetTileRange(3, 3); r.Accumulate(5)
    assert raw_call(mirt, r, buf) == MIRT_ERR_STATE
    r.SetTileRows(1, 2); r.Accumulate(5)
    assert raw_call(mirt, r, buf) == MIRT_ERR_STATE
    r.SetTileRange(0, 6); r.Accumulate(7)                                        # the whole image again; 7 is not a multiple of 5
    assert raw_call(mirt, r, buf) == MIRT_NOT_READY and r.render_denoised(out=buf) is None
    r.Accumulate(3)
    for bad in ({"iterations": 9}, {"normal_squarings": 9}, {"demodulate": 2}, {"sigma_lum": -1.0}, {"sigma_lum": float("nan")}, {"sigma_depth": float("inf")},
                {"sigma_depth": -0.5}, {"lum_floor": 0.0}, {"lum_floor": -1e-4}, {"lum_floor": float("inf")}, {"albedo_floor": float("nan")}):
        assert raw_call(mirt, r, buf, **bad) == MIRT_ERR_ARG, bad
    p = mirt.DenoiseParams(*mirt.denoise_defaults().values())
    assert r._lib.mirt_render_atrous(r._ctx, None, buf.ctypes.data_as(C.c_void_p)) == MIRT_ERR_ARG
    assert r._lib.mirt_render_atrous(r._ctx, C.byref(p), None) == MIRT_ERR_ARG
    assert r._lib.mirt_render_atrous(None, C.byref(p), buf.ctypes.data_as(C.c_void_p)) == MIRT_ERR_ARG
    assert (buf == SENTINEL).all(), "no refusal wrote a word"
    assert raw_call(mirt, r, buf) == MIRT_OK and (buf[..., 3] == 1).all()
    with pytest.raises(TypeError):
        r.render_denoised(sigma=1.0)
    r.close()

    r = mirt.Renderer(sc, buckets=5, exact_stream_order=True)                    # exact stream order has no AOVs: refused through the AOV rule
    r.Resize(48, 32); r.Accumulate(5)
    assert raw_call(mirt, r, buf) == MIRT_ERR_STATE
    r.close()


# ---- the direction of the claim ------------------------------------------------------------------------------------------------------------------
N_REF, N_NOISY, SEED_BASE = 4095, 20, 5000      # 4095: the multiple of 5 buckets next to 4096 (Render() resolves multiples of `buckets` only)


def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


@pytest.fixture(scope="module", params=[0, 1], ids=["lambertian", "ggx"])
def quality(request, mirt):
    """default9 at 64 x 64, buckets 5: the plain frame at 4095 accumulations, and the plain and the denoised (defaults) frame of 20 accumulations
    numbered 5001 .. 5020 — other seeds than the reference's — moved into a context that counts them as 20."""
    brdf = request.param
    make = lambda: mirt.Renderer(mirt.scene.default9(), buckets=5, use_bvh=True, aov=True, brdf=brdf)
    ref = make(); ref.Resize(W, H); ref.Accumulate(N_REF)
    assert ref.Render()
    out = {"brdf": brdf, "reference": ref.GetFrame().copy(), "reference_denoised": ref.render_denoised()}
    ref.close()
    src = make(); src.Resize(W, H)
    src.load_accumulator(np.zeros_like(src.accumulator()), SEED_BASE)
    src.Accumulate(N_NOISY)
    slab, aov = src.accumulator(), src.aov()
    src.close()
    noisy = make(); noisy.Resize(W, H)
    noisy.load_accumulator(slab, N_NOISY); noisy.load_aov(aov)
    assert noisy.Render()
    out["noisy"], out["noisy_denoised"] = noisy.GetFrame().copy(), noisy.render_denoised()
    noisy.close()
    return out


def test_it_denoises(quality):
    plain, filtered = rmse(quality["noisy"], quality["reference"]), rmse(quality["noisy_denoised"], quality["reference"])
    print(f"[denoise] brdf = {quality['brdf']}: RMSE to the {N_REF}-accumulation frame, {N_NOISY} accumulations: plain {plain:.5f}, denoised {filtered:.5f}, ratio {filtered / plain:.3f}")
    assert filtered < plain


def test_converged_input_is_left_alone(quality):
    moved, noise = rmse(quality["reference_denoised"], quality["reference"]), rmse(quality["noisy"], quality["reference"])
    print(f"[denoise] brdf = {quality['brdf']}: the {N_REF}-accumulation frame moves by RMSE {moved:.5f} when denoised; the plain {N_NOISY}-accumulation frame is {noise:.5f} away")
    assert moved < noise
