"""The full-image kernels and host paths at image sizes that are no whole number of 16 x 16 tiles (ragged_sizes.py: 70 x 40, 40 x 70, 17 x 16,
16 x 31, 79 x 33), where `width`, `w_img = 16 (width // 16)` and `256 x tiles` against `width x height` come apart: k_resolve, k_resolve_aov,
k_noise's map, k_denoise_prepare / k_atrous<STAGED> / k_atrous<!STAGED> / k_denoise_finish, k_reproject<MOTION>, k_id_map, copy_owned_tiles, the
`whole` branch of filtered_resolve and a group's gather.  Every feature is held to the yardstick and the bound of its own whole-tile test, unchanged
(word for word everywhere but the float64 resolve, RESOLVE_ABS, and the noise tile mean, 255 u): the oracle, definitions.py, test_aov.py's twin,
noise_twin.py, denoise_twin.py, temporal_twin.py, temporal_motion_twin.py, lens_twin.py.  test_ragged_sizes_cpu.py shows on the twins alone that these
inputs tell `width` from `w_img`.

THE REMAINDER (pixels no tile owns; include/mirt.h says it per entry point): every mirt_* resolve leaves them as the caller handed them; the Python
methods hand over zeros, so theirs are 0; mirt_id_map covers all width x height pixels."""
import ctypes as C

import numpy as np
import pytest

import definitions as df
import denoise_twin as dt
import lens_twin as lt
import noise_twin as nt
import oracle_binding as ob
import ragged_sizes as rs
import temporal_motion_twin as mt
import temporal_twin as tt
import test_aov as ta
import test_history_motion_gpu as hm
import test_noise_gpu as ng
from oracle_binding import bits
from test_definitions_cpu import RESOLVE_ABS
from test_denoise_gpu import assert_same

pytestmark = pytest.mark.gpu

f32 = np.float32
MIRT_OK = 0
SENTINEL = f32(-7.0)
SENTINEL_WORD = int(np.array([SENTINEL]).view(np.uint32)[0])


def scene_of(mirt, name):
    return mirt.scene.default9() if name == "default9" else mirt.scene.synthetic(200)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def sentinel_image(*shape):
    return np.full(shape, SENTINEL, dtype=f32)


def check_remainder(image, w, h, what, value=SENTINEL):
    """Every word of the rows [h_img, height) and the columns [w_img, width) holds `value`."""
    wi, hi = rs.img(w, h)
    rest = np.concatenate([bits(image[hi:]).reshape(-1), bits(image[:hi, wi:]).reshape(-1)])
    word = int(np.array([value], dtype=f32).view(np.uint32)[0])
    assert (rest == word).all(), f"{what}: {int((rest != word).sum())} of {rest.size} remainder words are not {value}"


def owned(image, w, h):
    wi, hi = rs.img(w, h)
    return image[:hi, :wi]


# ---- 1. the frame ---------------------------------------------------------------------------------------------------------------------------------------
CONFIGS = {"brute": dict(use_bvh=False), "lists": dict(use_bvh=True), "trace_primary_rays": dict(use_bvh=True, trace_primary_rays=True)}
_oracle_cache = {}


def oracle_state(mirt, name, w, h, k, n, lens=None):
    key = (name, w, h, k, n, lens)
    if key not in _oracle_cache:
        o = ob.Oracle(scene_of(mirt, name), max_bounces=4, buckets=k, trav_mode=ob.TRAV_BRUTE, lens=lens); o.Resize(w, h); o.Accumulate(n)
        _oracle_cache[key] = (o.accumulator().copy(), o.Render().copy(), o.counters())
        o.close()
    return _oracle_cache[key]


@pytest.mark.parametrize("k", [1, 4, 5])
@pytest.mark.parametrize("w,h", rs.SIZES)
def test_frame_accumulator_and_counters_equal_the_oracle(mirt, w, h, k):
    for name in ("default9", "S200"):
        n = 2 * k
        want_acc, want_frame, want_counters = oracle_state(mirt, name, w, h, k, n)
        resolve64 = df.resolve(want_acc, n, 1.0, w, h)
        for config, kw in CONFIGS.items():
            if name == "S200" and config == "brute":
                continue
            what = f"{name} {w}x{h} k={k} {config}"
            r = mirt.Renderer(scene_of(mirt, name), max_bounces=4, buckets=k, **kw); r.Resize(w, h)
            r.Accumulate(n)
            assert r.Render()
            frame = r.GetFrame()
            assert_same(r.accumulator(), want_acc, f"{what}: accumulator")
            assert r.counters()["rays"] == want_counters["rays"] and r.counters()["terminated"] == want_counters["terminated"], f"{what}: counters"
            assert_same(owned(frame, w, h), owned(want_frame, w, h), f"{what}: frame on [:h_img, :w_img]")
            check_remainder(frame, w, h, f"{what}: Render()", 0.0)
            err = float(np.abs(frame.astype(np.float64) - resolve64).max())
            print(f"[ragged] {what}: frame against the float64 median of means {err:.3g} ({err / RESOLVE_ABS:.3f} of RESOLVE_ABS)")
            assert err <= RESOLVE_ABS
            r.close()


# ---- 2. the lens: half_width comes from width, not w_img ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", rs.TEMPORAL_SIZES)
def test_lens_equals_the_oracle_and_the_twin(mirt, w, h):
    A, fd, k, n = 0.03, 1.1, 5, 5                                                  # default9's lens of test_lens_gpu.py
    want_acc, want_frame, _ = oracle_state(mirt, "default9", w, h, k, n, lens=(A, fd))
    o = ob.Oracle(mirt.scene.default9(), max_bounces=4); o.Resize(w, h)
    r = mirt.Renderer(mirt.scene.default9(), max_bounces=4, buckets=k, use_bvh=True); r.Resize(w, h)
    assert float(r.scene.camera.half_width) == w / 2 and float(r.scene.camera.half_height) == h / 2
    r.set_lens(A, fd)
    for acc in (1, 2, 9):
        p, d = r.debug_raygen(acc)
        O, D = lt.oracle_lens_rays(o, acc, A, fd)
        assert_same(p, O, f"{w}x{h}: lens origins, accumulation {acc}")
        assert_same(d, D, f"{w}x{h}: lens directions, accumulation {acc}")
    r.Accumulate(n)
    assert r.Render()
    assert_same(r.accumulator(), want_acc, f"{w}x{h}: accumulator under a lens")
    assert_same(owned(r.GetFrame(), w, h), owned(want_frame, w, h), f"{w}x{h}: frame under a lens")
    r.close(); o.close()


# ---- 3. AOVs, 4. noise ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", rs.SIZES)
def test_aovs_equal_the_twin(mirt, w, h):
    n = 3
    want, counts = ta.cached_twin(("ragged", w, h), lambda: ta.twin(mirt.scene.default9(), w, h, n, 4))
    assert counts["hit"] > 0
    r = mirt.Renderer(mirt.scene.default9(), max_bounces=4, use_bvh=True, aov=True); r.Resize(w, h)
    r.Accumulate(n)
    assert_same(r.aov(), want, f"{w}x{h}: AOV sums")
    for which, image in zip((mirt.AOV_DEPTH, mirt.AOV_NORMAL, mirt.AOV_ALBEDO), ta.twin_resolve(want, w, h, n)):
        assert_same(r.render_aov(which), image, f"{w}x{h}: render_aov({which}), remainder 0")
        buf = sentinel_image(*image.shape)
        assert r._lib.mirt_render_aov(r._ctx, which, ptr(buf)) == MIRT_OK
        assert_same(owned(buf, w, h), owned(image, w, h), f"{w}x{h}: mirt_render_aov({which})")
        check_remainder(buf, w, h, f"{w}x{h}: mirt_render_aov({which})")
    r.close()


@pytest.mark.parametrize("k", [2, 5])
@pytest.mark.parametrize("w,h", rs.SIZES)
def test_noise_equals_the_twin(mirt, w, h, k):
    n_tiles = rs.tiles(w, h)
    r = ng.make_renderer(mirt, w, h, k, use_bvh=True, max_bounces=4)
    r.Accumulate(2 * k)
    slab = r.accumulator()
    res, e = ng.check_against_twin(r, slab, 2 * k, 0.01, list(range(n_tiles)), f"ragged {w}x{h}, k = {k}, rendered")      # map (remainder: sentinel), records, histogram, stats
    above = r.noise_above(0.05, 0.01)
    ok = nt.usable(e)
    assert np.array_equal(above, (ok & (e > f32(0.05))).sum(axis=1).astype(np.uint32)), "tile_above"
    assert_same(r.noise(floor=0.01, want_map=True)["map"], nt.image(e, range(n_tiles), w, h, f32(0.0)), "noise(want_map=True): remainder 0")
    synthetic, _, acc_n = rs.synthetic(w, h, k, 11 * w + h + k)
    r.load_accumulator(synthetic, acc_n)
    ng.check_against_twin(r, synthetic, acc_n, 0.0, list(range(n_tiles)), f"ragged {w}x{h}, k = {k}, synthetic with NaN in the last owned column and row")
    r.close()


# ---- 5. the à-trous resolve -------------------------------------------------------------------------------------------------------------------------------
def loaded(mirt, w, h, k, slab, aov, acc_n):
    r = mirt.Renderer(mirt.scene.default9(), buckets=k, aov=True)
    r.Resize(w, h)
    r.load_accumulator(slab, acc_n)
    r.load_aov(aov)
    return r


@pytest.mark.parametrize("staged", [None, "0"], ids=["staged steps 1-2", "no step staged"])
@pytest.mark.parametrize("w,h", rs.SIZES)
def test_denoised_equals_the_twin(mirt, monkeypatch, w, h, staged):
    """Inputs of ragged_sizes.synthetic: smooth guides, so a tap at x >= w_img or y >= h_img that was read would show (CPU condition (a)), and a NaN
    word in the last owned column and in the last owned row.  iterations 0, 1, 3, 5: k_atrous<STAGED> at steps 1 and 2, k_atrous<!STAGED> from 4 on;
    with MIRT_TUNE_DENOISE_STAGED = 0 the unstaged form runs every step."""
    if staged is not None:
        monkeypatch.setenv("MIRT_TUNE_DENOISE_STAGED", staged)
    for k in (2, 5):
        slab, aov, acc_n = rs.synthetic(w, h, k, 7 * w + h)
        counts = np.full(rs.tiles(w, h), acc_n, dtype=np.uint32)
        r = loaded(mirt, w, h, k, slab, aov, acc_n)
        for it in (0, 1, 3, 5):
            for demodulate in (0, 1):
                params = {"iterations": it, "demodulate": demodulate}
                want = dt.denoise(slab, aov, counts, 1.0, params, w, h)
                assert_same(r.render_denoised(**params), want, f"{w}x{h}, k = {k}, {params}: render_denoised, remainder 0")
        buf = sentinel_image(h, w, 4)
        assert r.render_denoised(out=buf, iterations=3) is buf
        assert_same(owned(buf, w, h), owned(dt.denoise(slab, aov, counts, 1.0, {"iterations": 3}, w, h), w, h), f"{w}x{h}, k = {k}: mirt_render_atrous")
        check_remainder(buf, w, h, f"{w}x{h}: mirt_render_atrous")
        r.close()


# ---- 6. the temporal history ------------------------------------------------------------------------------------------------------------------------------
def move_renderer(r, name):
    rs.MOVES[name](r.scene.camera)
    r.UpdateCamera()


def next_frame(r, k):
    r.ResetAccumulator()
    r.Accumulate(k)


def check_temporal(r, want_frame, want_len, want_st, w, h, what, **params):
    frame, got_len, st = r.render_temporal(want_len=True, want_stats=True, **params)
    print(f"[ragged] temporal {what}: {st}")
    assert st == want_st, f"{what}: class counts, twin {want_st}"
    assert_same(owned(got_len, w, h), want_len, f"{what}: history_len")
    assert_same(frame, want_frame, f"{what}: frame, remainder 0")
    check_remainder(got_len, w, h, f"{what}: render_temporal's history_len", 0.0)


@pytest.mark.parametrize("k", [2, 5])
@pytest.mark.parametrize("w,h", rs.TEMPORAL_SIZES)
def test_temporal_sequence_equals_the_twin(mirt, w, h, k):
    params = {"iterations": 2}
    r = mirt.Renderer(mirt.scene.default9(), buckets=k, max_bounces=4, aov=True, use_bvh=True); r.Resize(w, h)
    hist, prev = None, None
    for i, name in enumerate((None,) + tuple(rs.MOVES)):
        if name:
            move_renderer(r, name)
        next_frame(r, k)
        acc, aov, counts = r.accumulator().copy(), r.aov().copy(), r.tile_counts().copy()
        cam = rs.twin_camera(r.scene.camera)
        if prev is not None:
            lands = rs.landers(dt.prepare(acc, aov, counts, 1.0, dict(dt.DEFAULTS), w, h), cam, prev, w, h)
            assert lands.sum() >= 16, f"{name}: {int(lands.sum())} pixels' points land in columns [w_img, width) or rows [h_img, height) of the history"
        want_frame, want_len, want_st, new_hist = tt.render(acc, aov, counts, 1.0, params, {}, w, h, cam, hist)
        if prev is not None:
            cls = tt.reproject_blend(dt.prepare(acc, aov, counts, 1.0, dict(dt.DEFAULTS), w, h), owned(np.full((h, w), f32(k)), w, h), cam, hist, dict(dt.DEFAULTS), dict(tt.DEFAULTS))[3]
            assert (cls[lands] == tt.OUTSIDE).all(), "the twin classes them outside"
        # the raw entry point into sentinel-filled buffers, update = 0: the same words on the owned pixels, the remainder as handed over
        buf, length = sentinel_image(h, w, 4), sentinel_image(h, w)
        got = r.render_temporal(out=buf, want_len=False, update=0, **params)
        assert got is buf
        assert_same(owned(buf, w, h), owned(want_frame, w, h), f"frame {i + 1}: mirt_render_temporal, update = 0")
        check_remainder(buf, w, h, f"frame {i + 1}: mirt_render_temporal's frame")
        dp, tp = mirt._split_temporal_params(dict(params, update=0))
        assert r._lib.mirt_render_temporal(r._ctx, C.byref(dp), C.byref(tp), ptr(buf), ptr(length), None) == MIRT_OK
        assert_same(owned(length, w, h), want_len, f"frame {i + 1}: mirt_render_temporal's history_len")
        check_remainder(length, w, h, f"frame {i + 1}: mirt_render_temporal's history_len")
        check_temporal(r, want_frame, want_len, want_st, w, h, f"{w}x{h} k={k} frame {i + 1} ({name})", **params)
        assert sum(want_st.values()) == rs.img(w, h)[0] * rs.img(w, h)[1]
        hist, prev = new_hist, cam
    # a Resize between two ragged sizes of the same tile counts drops the history
    assert r.history_info()["valid"]
    r.Resize(w + 3, h + 5)
    assert rs.tiles(w + 3, h + 5) == rs.tiles(w, h) and r.history_info() == {"valid": False, "bytes": 0}
    next_frame(r, k)
    frame, st = r.render_temporal(want_stats=True, **params)
    assert st["reprojected"] == st["outside"] == st["rejected"] == 0
    assert_same(frame, r.render_denoised(**params), "after the Resize: no history, the à-trous resolve")
    r.close()


# ---- 7. id map and sphere motion ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["host_sah", "brute", "gpu_build"])
@pytest.mark.parametrize("w,h", rs.SIZES)
def test_id_map_covers_the_whole_image(mirt, w, h, config):
    wi, hi = rs.img(w, h)
    for name in ("default9", "S200"):
        r = mirt.Renderer(scene_of(mirt, name), buckets=2, max_bounces=4, aov=True, **hm.CONFIGS[config]); r.Resize(w, h)
        prim, dist = r.id_map()
        p, d = hm.centre_rays(r)                                                  # all width x height pixel centres, rows of `width`
        tfar, want_prim = r.debug_trace_closest(p, d)
        want_prim, tfar = want_prim.reshape(h, w), tfar.reshape(h, w)
        hit = want_prim >= 0
        assert np.array_equal(prim, want_prim), f"{name} {w}x{h} {config}: prim over width x height"
        assert_same(dist[hit], tfar[hit], f"{name} {w}x{h} {config}: distance")
        assert np.isposinf(dist[~hit]).all()
        if name == "default9":                                                    # (the top rows of default9 are sky: there the map's inf against the buffer's 0 shows the write)
            assert hit.any() and (w == wi or hit[:, wi:].any()) and (h == hi or hit[hi:].any() or h > w), "the remainder shows spheres"
        for x, y in {(w - 1, 0), (0, h - 1), (wi - 1, hi - 1), (w - 1, h - 1)}:      # column remainder, row remainder, the last owned pixel, the last pixel
            got, _ = r.pick_focus(x, y)
            assert bits(f32(got)) == bits(dist[y, x]), f"pick_focus({x}, {y})"
        r.close()


def test_moved_sphere_history_equals_the_twin(mirt):
    """test_history_motion_gpu's moved ball at 70 x 40."""
    w, h = 70, 40
    r = mirt.Renderer(mirt.scene.default9(), buckets=hm.K, max_bounces=4, aov=True, use_bvh=True)
    r.set_history_motion(True)
    r.Resize(w, h)
    hm.move_ball(r, radius_scale=1.6)
    hist = None
    for i, step in enumerate((None, -5.0, 3.0)):
        if step is not None:
            hm.move_ball(r, hm.pixel_step(r, step))
            assert r.history_info()["valid"]
        next_frame(r, hm.K)
        acc, aov, counts = r.accumulator().copy(), r.aov().copy(), r.tile_counts().copy()
        ids, _ = r.id_map()
        assert ids.shape == (h, w)
        want_frame, want_len, want_st, hist, cls = mt.render(acc, aov, counts, 1.0, hm.PARAMS, {}, w, h, rs.twin_camera(r.scene.camera), hist, ids, hm.table(r))
        check_temporal(r, want_frame, want_len, want_st, w, h, f"moved ball, frame {i + 1}", **hm.PARAMS)
        if step is not None:
            assert want_st["reprojected"] > 0 and (cls[owned(ids, w, h) == int(r._bvh_of_geometry[hm.BALL])] == mt.REPROJECTED).any(), "the ball's pixels follow it"
    r.close()


# ---- 8. a group ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", rs.TEMPORAL_SIZES)
def test_group_of_three_equals_the_single_context(mirt, w, h):
    """70 x 40 has two tile rows: the third member owns nothing."""
    k, params = 5, {"iterations": 2}
    kw = dict(buckets=k, max_bounces=4, use_bvh=True, aov=True)
    single = mirt.Renderer(mirt.scene.default9(), **kw); single.Resize(w, h)
    g = mirt.GroupRenderer(mirt.scene.default9(), devices=[0, 0, 0], **kw); g.Resize(w, h)
    for i, name in enumerate((None, "strafe")):
        for r in (single, g):
            if name:
                move_renderer(r, name)
            next_frame(r, k)
        assert single.Render() and g.Render()
        assert_same(g.accumulator(), single.accumulator(), f"group {w}x{h}: accumulator")
        assert_same(g.GetFrame(), single.GetFrame(), f"group {w}x{h}: frame")
        assert_same(g.read_aov(), single.aov(), f"group {w}x{h}: read_aov")
        for which in range(3):
            assert_same(g.render_aov(which), single.render_aov(which), f"group {w}x{h}: render_aov({which})")
        gn, sn = g.noise(floor=0.01, want_map=True), single.noise(floor=0.01, want_map=True)
        assert_same(gn["map"], sn["map"], f"group {w}x{h}: noise map")
        assert_same(gn["tiles"][:, [0, 2, 3]], sn["tiles"][:, [0, 2, 3]], f"group {w}x{h}: tile records")
        assert_same(gn["tiles"][:, 1], sn["tiles"][:, 1], f"group {w}x{h}: tile means")
        assert np.array_equal(gn["hist"], sn["hist"])
        assert_same(g.render_denoised(**params), single.render_denoised(**params), f"group {w}x{h}: render_denoised")
        got, want = g.render_temporal(want_len=True, want_stats=True, **params), single.render_temporal(want_len=True, want_stats=True, **params)
        assert got[2] == want[2] and (i == 0 or want[2]["reprojected"] > 0)
        assert_same(got[1], want[1], f"group {w}x{h}, frame {i + 1}: history_len")
        assert_same(got[0], want[0], f"group {w}x{h}, frame {i + 1}: temporal frame")
        gi, si = g.id_map(), single.id_map()
        assert np.array_equal(gi[0], si[0])
        assert_same(gi[1], si[1], f"group {w}x{h}: id map distances")
        buf = sentinel_image(h, w, 4)
        assert g._lib.mirt_group_render(g._g, ptr(buf)) == MIRT_OK
        assert_same(owned(buf, w, h), owned(single.GetFrame(), w, h), f"group {w}x{h}: mirt_group_render")
        check_remainder(buf, w, h, f"group {w}x{h}: mirt_group_render")
    g.close(); single.close()


# ---- 9. the remainder through the C entry points (the others above, next to their comparisons) ----------------------------------------------------------------
@pytest.mark.parametrize("w,h", rs.SIZES)
def test_mirt_render_leaves_the_remainder_as_handed_over(mirt, w, h):
    r = mirt.Renderer(mirt.scene.default9(), max_bounces=4, buckets=5, use_bvh=True); r.Resize(w, h)
    r.Accumulate(5)
    assert r.Render()
    buf = sentinel_image(h, w, 4)
    assert r._lib.mirt_render(r._ctx, ptr(buf)) == MIRT_OK
    assert_same(owned(buf, w, h), owned(r.GetFrame(), w, h), f"{w}x{h}: mirt_render into a sentinel-filled buffer")
    check_remainder(buf, w, h, f"{w}x{h}: mirt_render")
    check_remainder(r.GetFrame(), w, h, f"{w}x{h}: Render()", 0.0)
    r.close()


# ---- 10. frozen tiles -----------------------------------------------------------------------------------------------------------------------------------------
def test_frozen_tiles_resolve_at_their_own_counts(mirt):
    w, h, k = 70, 40, 5
    n_tiles = rs.tiles(w, h)
    frozen = np.array([1 if t % 3 == 0 else 0 for t in range(n_tiles)], dtype=np.uint8)
    counts = np.where(frozen, 5, 10).astype(np.uint32)
    r = mirt.Renderer(mirt.scene.default9(), max_bounces=4, buckets=k, use_bvh=True, aov=True); r.Resize(w, h)
    r.Accumulate(5); r.freeze_tiles(frozen); r.Accumulate(5)
    assert np.array_equal(r.tile_counts(), counts)
    acc, aov = r.accumulator(), r.aov()
    at5, at10 = oracle_state(mirt, "default9", w, h, k, 5)[0], oracle_state(mirt, "default9", w, h, k, 10)[0]
    aov5, aov10 = (ta.twin(mirt.scene.default9(), w, h, n, 4)[0] for n in (5, 10))
    for t in range(n_tiles):
        assert_same(acc[t], (at5 if frozen[t] else at10)[t], f"tile {t} at count {counts[t]}: accumulator against the oracle")
        assert_same(aov[t], (aov5 if frozen[t] else aov10)[t], f"tile {t} at count {counts[t]}: AOV sums against the twin")
    assert r.Render()
    assert_same(r.GetFrame(), dt.render_frame(acc, counts, 1.0, w, h), "frame: every tile at its own count")
    e = np.concatenate([nt.noise_e(acc[t:t + 1], nt.scale_of(1.0, int(counts[t]), k), 0.01) for t in range(n_tiles)])
    noise = r.noise(floor=0.01, map_out=sentinel_image(h, w))
    assert_same(noise["map"], nt.image(e, range(n_tiles), w, h, SENTINEL), "noise map: per-tile scales, the remainder as handed over")
    assert np.array_equal(noise["hist"], nt.histogram(e))
    for params in ({"iterations": 0, "demodulate": 0}, {"iterations": 3}):
        assert_same(r.render_denoised(**params), dt.denoise(acc, aov, counts, 1.0, params, w, h), f"denoised with per-tile counts, {params}")
    r.close()
