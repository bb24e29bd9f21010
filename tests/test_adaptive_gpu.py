"""Per-tile adaptive sampling on the GPU (mirt_freeze_tiles, mirt_tile_counts, mirt_load_tile_counts, mirt_tile_above,
mirt_accumulate_adaptive; the sparse twins of the bounce-0 kernels and of the merge in kernels.hpp).

The contract has no tolerance: a tile whose count is n holds, word for word, what n plain accumulations leave in that tile.  So everything
here is compared on the raw words — with a plain context (one that never freezes a tile) after n accumulations, and with the brute-force CPU
oracle.  Image 80 x 48: 15 tiles, an odd count, so the last 512-pixel chunk of k_shade<FIRST> holds one tile."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import adaptive_twin as at
import noise_twin as nt
import oracle_binding as ob
import test_light_ris_gpu as rg
from oracle_binding import bits

pytestmark = pytest.mark.gpu

f32 = np.float32
MIRT_OK, MIRT_NOT_READY, MIRT_ERR_ARG, MIRT_ERR_STATE = 0, 1, -1, -3
W, H, TILES = 80, 48, 15
A = (0, 3, 4, 14)                                    # first and last tile, both tiles of one chunk; with tile 5 one tile of a chunk
B = tuple(t for t in range(TILES) if t != 7)         # all but one
COUNTS = np.array([5 if t in A else 10 if t in B else 15 for t in range(TILES)], dtype=np.uint32)


def assert_same(got, want, what):
    got, want = bits(np.asarray(got)), bits(np.asarray(want))
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} words differ"


def scene_of(mirt, name):
    return mirt.scene.default9() if name == "default9" else mirt.scene.synthetic(1000, ambient=0.5)


def mask_of(gids, frozen_gids):
    return np.array([1 if g in frozen_gids else 0 for g in gids], dtype=np.uint8)


def plain_slabs(mirt, sc, steps, aov=False, **kw):
    """{n: accumulator (and AOV slab) of a context that never freezes a tile, after n accumulations}, whole image."""
    r = mirt.Renderer(sc, max_bounces=5, buckets=5, aov=aov, **kw)
    r.Resize(W, H)
    out, n = {}, 0
    for step in steps:
        r.Accumulate(step); n += step
        out[n] = (r.accumulator(), r.aov() if aov else None, r.counters())
    r.close()
    return out


def run_schedule(r, ref, gids, step=5, accumulate=None, aov=False, what=""):
    """accumulate step, freeze A, accumulate step, freeze B, accumulate step; every tile equals the plain context's at its count.  Then
    freeze everything and accumulate once more: no word changes, `accumulations` still counts the calls."""
    accumulate = accumulate or r.Accumulate
    accumulate(step); r.freeze_tiles(mask_of(gids, A))
    accumulate(step); r.freeze_tiles(mask_of(gids, B))
    accumulate(step)
    counts = np.array([step if g in A else 2 * step if g in B else 3 * step for g in gids], dtype=np.uint32)
    assert np.array_equal(r.tile_counts(), counts), what
    got, got_aov = r.accumulator(), r.aov() if aov else None
    for local, g in enumerate(gids):
        assert_same(got[local], ref[int(counts[local])][0][g], f"{what}: tile {g} at count {counts[local]}")
        if aov:
            assert_same(got_aov[local], ref[int(counts[local])][1][g], f"{what}: AOV slab of tile {g} at count {counts[local]}")
    assert not np.isnan(got).any()
    r.freeze_tiles(np.ones(len(gids), dtype=np.uint8))
    accumulate(step)
    assert r.accumulations == 4 * step
    assert_same(r.accumulator(), got, f"{what}: every tile frozen, nothing changes")
    assert np.array_equal(r.tile_counts(), counts)
    return got, counts


@pytest.fixture(scope="module")
def plain(mirt):
    cache = {}

    def get(scene_name, steps=(5, 5, 5), aov=False, **kw):
        key = (scene_name, steps, aov, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = plain_slabs(mirt, scene_of(mirt, scene_name), steps, aov=aov, use_bvh=True, **kw)
        return cache[key]
    return get


# ---- 1. frozen tiles are exact -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene_name", ["default9", "S1000"])
def test_frozen_tiles_equal_plain_context_and_oracle(mirt, plain, scene_name):
    ref = plain(scene_name)
    r = mirt.Renderer(scene_of(mirt, scene_name), max_bounces=5, buckets=5, use_bvh=True)
    r.Resize(W, H)
    got, counts = run_schedule(r, ref, list(range(TILES)), what=scene_name)
    r.close()
    o = ob.Oracle(scene_of(mirt, scene_name), max_bounces=5, buckets=5, trav_mode=ob.TRAV_BRUTE); o.Resize(W, H)
    for n in (5, 10, 15):
        o.Accumulate(5)
        slab = o.accumulator()
        for t in np.nonzero(counts == n)[0]:
            assert_same(got[t], slab[t], f"{scene_name}: tile {t} against the oracle after {n} accumulations")
    o.close()


CONFIGS = {
    "trace_primary_rays": dict(trace_primary_rays=True),
    "no tree": dict(use_bvh=False),
    "gpu_build": dict(gpu_build=True),
    "max_batch 1": dict(max_batch=1),
    "max_batch 5": dict(max_batch=5),
    "streams 1": dict(streams=1),
    "streams 3, max_batch 2": dict(streams=3, max_batch=2),
    "ggx with decay": dict(brdf=1, gloss_decay=[0.0, 0.3, 0.6]),
    "count_traffic, trace_primary_rays": dict(count_traffic=True, trace_primary_rays=True),      # k_trace<COUNT = true, kPrimaryActive>, tree walk
    "count_traffic, no tree": dict(count_traffic=True, use_bvh=False),                           # the same, brute-force loop
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_frozen_tiles_in_every_mode(mirt, plain, name):
    """The plain reference is the DEFAULT configuration's wherever the mode does not change results (every mode but the closure)."""
    kw = dict(CONFIGS[name])
    ref = plain_slabs(mirt, scene_of(mirt, "default9"), (5, 5, 5), use_bvh=True, **kw) if "brdf" in kw else plain("default9")
    kw.setdefault("use_bvh", True)
    r = mirt.Renderer(scene_of(mirt, "default9"), max_bounces=5, buckets=5, **kw)
    r.Resize(W, H)
    run_schedule(r, ref, list(range(TILES)), what=name)
    r.close()


@pytest.mark.parametrize("max_batch", [1, 5])
@pytest.mark.parametrize("lens", [None, (0.05, 4.0)], ids=["pinhole", "lens"])
@pytest.mark.parametrize("w,h", [(W, H), (32, 16)])
def test_counting_camera_rays_of_the_active_tiles(mirt, w, h, lens, max_batch):
    """k_trace<COUNT = true, kPrimaryActive, LENS>, tree walk and brute-force loop: camera rays only (max_bounces = 1), 5 accumulations, every third
    tile frozen, 5 more; words, frame, `rays` and `terminated` are the oracle's.  `rays` is then active tiles x 256 x the accumulations issued while
    they were active.  32 x 16 is two tiles, one of them frozen: with max_batch = 1 a launch is 256 rays — less than a workgroup, every ray in
    slot 0 of its batch —, with max_batch = 5 it is five slots of one list."""
    sc, tiles = scene_of(mirt, "default9"), (w // 16) * (h // 16)
    active = tiles - len(range(0, tiles, 3))
    kw = dict(lens=lens) if lens else {}
    route = dict(count_traffic=True, max_batch=max_batch)
    rg.check_frozen_against_oracle(mirt, sc, ("default9", "camera rays", lens), w, h,
                                   (("tree", dict(route, use_bvh=True, trace_primary_rays=True)), ("brute", dict(route, use_bvh=False))), max_bounces=1, **kw)
    want = rg.oracle_states(sc, ("default9", "camera rays", lens), w, h, (5, 10), max_bounces=1, tiles_after=(5, np.flatnonzero(np.arange(tiles) % 3 != 0)), **kw)
    assert want[5]["counters"]["rays"] + want["active"][ob.TRAV_BRUTE]["rays"] == (tiles * 5 + active * 5) * 256      # what the contexts' `rays` were just compared with


def test_frozen_tiles_async_lens_aov_and_wave_kernel(mirt, plain):
    sc = scene_of(mirt, "default9")
    # mirt_accumulate_async(1) x n: deferred calls are launched under the mask they were issued under
    r = mirt.Renderer(sc, max_bounces=5, buckets=5, use_bvh=True); r.Resize(W, H)
    run_schedule(r, plain("default9"), list(range(TILES)), accumulate=lambda n: [r.AccumulateAsync(1) for _ in range(n)], what="async")
    r.close()
    # a thin lens (the LENS twins), with the first-hit AOVs on
    lens_ref = {}
    p = mirt.Renderer(sc, max_bounces=5, buckets=5, use_bvh=True, aov=True); p.Resize(W, H); p.set_lens(0.05, 4.0)
    for n in (5, 10, 15):
        p.Accumulate(5); lens_ref[n] = (p.accumulator(), p.aov(), None)
    p.close()
    r = mirt.Renderer(sc, max_bounces=5, buckets=5, use_bvh=True, aov=True); r.Resize(W, H); r.set_lens(0.05, 4.0)
    run_schedule(r, lens_ref, list(range(TILES)), aov=True, what="lens + aov")
    r.close()
    # pinhole with AOVs (candidate lists + k_first_hit_aov's twin)
    r = mirt.Renderer(sc, max_bounces=5, buckets=5, use_bvh=True, aov=True); r.Resize(W, H)
    run_schedule(r, plain("default9", aov=True), list(range(TILES)), aov=True, what="aov")
    r.close()
    # batches of 35: k_primary_hits_wave's twin (batches of 32 and more)
    r = mirt.Renderer(sc, max_bounces=5, buckets=5, use_bvh=True); r.Resize(W, H)
    assert r.get_policy()["max_batch"] >= 35
    run_schedule(r, plain("default9", steps=(35, 35, 35)), list(range(TILES)), step=35, what="batches of 35")
    r.close()


def test_frozen_tiles_with_interleaved_tile_rows(mirt, plain):
    ref = plain("default9")
    for first, gids in ((0, [0, 1, 2, 3, 4, 10, 11, 12, 13, 14]), (1, [5, 6, 7, 8, 9])):
        r = mirt.Renderer(scene_of(mirt, "default9"), max_bounces=5, buckets=5, use_bvh=True); r.Resize(W, H)
        r.SetTileRows(first, 2)
        run_schedule(r, ref, gids, what=f"tile rows {first}, {first} + 2, ...")
        r.close()


def test_poisoned_contribution_buffer(mirt, plain, monkeypatch):
    """MIRT_DEBUG_POISON_CONTRIB=1 fills every contribution buffer with NaN before each batch: the merge must not touch a frozen tile, whose
    words nobody stores any more (run_schedule asserts that no NaN arrives and that frozen tiles keep their words)."""
    monkeypatch.setenv("MIRT_DEBUG_POISON_CONTRIB", "1")
    r = mirt.Renderer(scene_of(mirt, "default9"), max_bounces=5, buckets=5, use_bvh=True); r.Resize(W, H)
    run_schedule(r, plain("default9"), list(range(TILES)), what="poisoned contribution buffer")
    r.close()


# ---- 2. counters ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(trace_primary_rays=True)], ids=["lists", "tree walk"])
def test_counters_are_the_sum_over_runs_of_equal_count(mirt, kw):
    """Freeze patterns of contiguous runs: rays, shadow_rays, terminated and dropped equal the sum over the runs of a plain context on
    mirt_set_tile_range(run) after the run's count — integer sums, and any partition of the tiles reproduces the counters."""
    sc = scene_of(mirt, "default9")
    runs = [(0, 4, 5), (4, 6, 15), (10, 5, 10)]                                  # (first tile, tiles, count)
    r = mirt.Renderer(sc, max_bounces=5, buckets=5, use_bvh=True, **kw); r.Resize(W, H)
    r.Accumulate(5); r.freeze_tiles([1] * 4 + [0] * 11)
    r.Accumulate(5); r.freeze_tiles([0] * 10 + [1] * 5)
    r.Accumulate(5)
    got = r.counters(); r.close()
    want = dict.fromkeys(("rays", "shadow_rays", "terminated", "dropped"), 0)
    for first, n, count in runs:
        p = mirt.Renderer(sc, max_bounces=5, buckets=5, use_bvh=True, **kw); p.Resize(W, H); p.SetTileRange(first, n); p.Accumulate(count)
        c = p.counters(); p.close()
        for k in want:
            want[k] += c[k]
    assert {k: got[k] for k in want} == want
    assert got["rays"] > 0


# ---- 3. resolves, checkpoint ---------------------------------------------------------------------------------------------------
def tile_pixels(img, t):
    x0, y0 = 16 * (t % (W // 16)), 16 * (t // (W // 16))
    return img[y0:y0 + 16, x0:x0 + 16]


def test_resolves_use_each_tiles_own_count_and_checkpoint_resumes(mirt, plain):
    sc = scene_of(mirt, "default9")
    ref = plain("default9", aov=True)
    frames = {}
    for n in (5, 10, 15):                                                           # the plain context's resolves at every count, from its slabs
        p = mirt.Renderer(sc, max_bounces=5, buckets=5, use_bvh=True, aov=True); p.Resize(W, H)
        p.load_accumulator(ref[n][0], n); p.load_aov(ref[n][1])
        assert p.Render()
        frames[n] = (p.GetFrame().copy(), [p.render_aov(w) for w in (mirt.AOV_DEPTH, mirt.AOV_NORMAL, mirt.AOV_ALBEDO)], p.noise(floor=0.01, want_map=True))
        p.close()
    r = mirt.Renderer(sc, max_bounces=5, buckets=5, use_bvh=True, aov=True); r.Resize(W, H)
    r.Accumulate(5); r.freeze_tiles(mask_of(range(TILES), A)); r.Accumulate(5); r.freeze_tiles(mask_of(range(TILES), B)); r.Accumulate(5)
    assert np.array_equal(r.tile_counts(), COUNTS) and r.Render()
    frame, aovs, noise = r.GetFrame().copy(), [r.render_aov(w) for w in (mirt.AOV_DEPTH, mirt.AOV_NORMAL, mirt.AOV_ALBEDO)], r.noise(floor=0.01, want_map=True)
    for t in range(TILES):
        want = frames[int(COUNTS[t])]
        assert_same(tile_pixels(frame, t), tile_pixels(want[0], t), f"mirt_render, tile {t}")
        for k in range(3):
            assert_same(tile_pixels(aovs[k], t), tile_pixels(want[1][k], t), f"mirt_render_aov {k}, tile {t}")
        assert_same(tile_pixels(noise["map"], t), tile_pixels(want[2]["map"], t), f"mirt_noise map, tile {t}")
        assert_same(noise["tiles"][t], want[2]["tiles"][t], f"mirt_noise record, tile {t}")
    # histogram and stats: the twin fed with per-tile scales
    slab = r.accumulator()
    e = np.concatenate([nt.noise_e(slab[t:t + 1], nt.scale_of(sc.camera.exposure, int(COUNTS[t]), 5), 0.01) for t in range(TILES)])
    assert np.array_equal(noise["hist"], nt.histogram(e))
    want = nt.stats(e)
    assert all(noise[k] == want[k] for k in ("owned_pixels", "finite_pixels", "nonfinite_pixels")) and f32(noise["max"]) == f32(want["max"])
    total = 0.0
    for m, c in zip(noise["tiles"][:, 1], noise["tiles"][:, 2]):                   # the documented double sum, ascending tile order (as test_noise_gpu.py)
        total += float(m) * float(c)
    assert noise["mean"] == total / want["finite_pixels"], "mean is not the documented double sum"
    assert abs(noise["mean"] - want["mean"]) <= 256 * 2.0 ** -24 * want["mean"]
    # mirt_tile_above against the count taken from the map: a target below every pixel, above every pixel, in between
    e_map = np.stack([tile_pixels(noise["map"], t).reshape(-1) for t in range(TILES)])
    usable = nt.usable(e_map)
    middle = float(np.median(e_map[usable]))
    for target in (0.0, float(e_map[usable].max()), middle):
        above = r.noise_above(target, floor=0.01)
        assert np.array_equal(above, at.above_of(e_map, target)), f"noise_above, target {target}"
    assert r.noise_above(middle, floor=0.01).sum() not in (0, int(usable.sum()))
    # checkpoint: accumulator + counts into a fresh context give the same frame, and both continue to the same words
    q = mirt.Renderer(sc, max_bounces=5, buckets=5, use_bvh=True); q.Resize(W, H)
    q.load_accumulator(slab, 15); q.load_tile_counts(COUNTS)
    assert np.array_equal(q.tile_counts(), COUNTS) and q.Render()
    assert_same(q.GetFrame(), frame, "frame of the resumed context")
    q.Accumulate(5); r.Accumulate(5)
    assert_same(q.accumulator(), r.accumulator(), "resumed context after 5 more accumulations")
    full = plain("default9", steps=(5, 5, 5, 5))
    assert_same(q.accumulator()[7], full[20][0][7], "the one active tile went on to 20 accumulations")
    q.close(); r.close()


# ---- 4. status codes -----------------------------------------------------------------------------------------------------------
def test_status_codes(mirt):
    sc = scene_of(mirt, "default9")
    r = mirt.Renderer(sc, max_bounces=5, buckets=5, use_bvh=True); r.Resize(W, H)
    lib, ctx = r._lib, r._ctx
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ones, counts = np.ones(TILES, dtype=np.uint8), np.zeros(TILES, dtype=np.uint32)
    assert lib.mirt_freeze_tiles(ctx, ptr(ones), TILES) == MIRT_ERR_STATE and b"nothing accumulated" in lib.mirt_last_error(ctx)      # 0 accumulations
    assert lib.mirt_tile_above(ctx, 0.0, 0.5, ptr(counts), TILES) == MIRT_NOT_READY
    r.Accumulate(7)
    assert lib.mirt_freeze_tiles(ctx, ptr(ones), TILES) == MIRT_ERR_STATE and b"not a multiple" in lib.mirt_last_error(ctx)           # off a bucket multiple
    r.Accumulate(3)
    assert lib.mirt_freeze_tiles(ctx, ptr(ones), TILES - 1) == MIRT_ERR_ARG and lib.mirt_freeze_tiles(ctx, ptr(ones), TILES + 1) == MIRT_ERR_ARG
    assert lib.mirt_tile_counts(ctx, ptr(counts), TILES - 1) == MIRT_ERR_ARG and lib.mirt_tile_above(ctx, 0.0, 0.5, ptr(counts), TILES - 1) == MIRT_ERR_ARG
    for bad in (-1.0, float("nan"), float("inf")):
        assert lib.mirt_tile_above(ctx, 0.0, bad, ptr(counts), TILES) == MIRT_ERR_ARG and lib.mirt_tile_above(ctx, bad, 0.5, ptr(counts), TILES) == MIRT_ERR_ARG
    assert (r.tile_counts() == 10).all()
    r.set_stream_order(True)
    assert lib.mirt_freeze_tiles(ctx, ptr(ones), TILES) == MIRT_ERR_STATE and b"exact stream order" in lib.mirt_last_error(ctx)
    assert lib.mirt_accumulate_adaptive(ctx, C.byref(mirt.StopRule(0.5, 0.95, 0.0, 5, 100)), 0, None) == MIRT_ERR_STATE
    r.set_stream_order(False)
    one = np.zeros(TILES, dtype=np.uint8); one[2] = 1
    r.freeze_tiles(one)
    assert lib.mirt_set_stream_order(ctx, 1) == MIRT_ERR_STATE and b"frozen" in lib.mirt_last_error(ctx)
    r.Accumulate(5)
    want = np.full(TILES, 15, dtype=np.uint32); want[2] = 10
    assert np.array_equal(r.tile_counts(), want)
    for bad_count in (7, 0, 20):                                                   # not a multiple of buckets, zero, above accumulations
        c = want.copy(); c[5] = bad_count
        assert lib.mirt_load_tile_counts(ctx, ptr(c), TILES) == MIRT_ERR_ARG and np.array_equal(r.tile_counts(), want)
    assert lib.mirt_load_tile_counts(ctx, ptr(want), TILES - 1) == MIRT_ERR_ARG
    for rule in (mirt.StopRule(0.5, 0.95, 0.0, 7, 100), mirt.StopRule(0.5, 0.0, 0.0, 5, 100), mirt.StopRule(-0.5, 0.95, 0.0, 5, 100)):
        assert lib.mirt_accumulate_adaptive(ctx, C.byref(rule), 0, None) == MIRT_ERR_ARG
    r.ResetAccumulator()                                                           # clears every freeze and count
    assert (r.tile_counts() == 0).all() and not r.frozen_tiles().any() and lib.mirt_set_stream_order(ctx, 1) == MIRT_OK
    r.set_stream_order(False)
    # ... and so do mirt_resize, mirt_set_tile_range, mirt_set_tile_rows and a change of `buckets`
    for name, change, tiles in (("resize", lambda: r.Resize(W, H), TILES), ("tile range", lambda: r.SetTileRange(5, 6), 6), ("tile rows", lambda: r.SetTileRows(1, 2), 5),
                                ("buckets", lambda: r.set_policy(buckets=2), 5)):
        n = len(r.tile_counts())
        r.Accumulate(10); r.freeze_tiles([1] + [0] * (n - 1))
        assert r.frozen_tiles().sum() == 1, name
        change()
        assert len(r.tile_counts()) == tiles and (r.tile_counts() == 0).all() and not r.frozen_tiles().any() and r.accumulations == 0, name
    r.close()


# ---- 5. the adaptive loop ------------------------------------------------------------------------------------------------------
def test_adaptive_loop_equals_the_replay(mirt):
    S = at.SCENE
    sc = scene_of(mirt, "default9")
    w, h, k, every, top = S["width"], S["height"], S["buckets"], S["check_every"], S["max_accumulations"]
    tiles = (w // 16) * (h // 16)
    make = lambda: mirt.Renderer(sc, max_bounces=S["max_bounces"], buckets=k, use_bvh=True)
    p = make(); p.Resize(w, h)
    slabs = {}
    for n in range(every, top + 1, every):
        p.Accumulate(every); slabs[n] = p.accumulator()
    plain_rays = p.counters()["rays"]; p.close()
    want = at.replay(lambda n: slabs[n], tiles, sc.camera.exposure, at.TARGET, S["quantile"], S["floor"], k, every, 0, top)
    assert want["masks"][0].sum() >= 1 and want["masks"][-1].sum() < tiles           # (asserted on the CPU too: the test is not vacuous)
    # step by step from noise() and adaptive_select
    r = make(); r.Resize(w, h)
    frozen = np.zeros(tiles, dtype=np.uint8)
    for i in range(top // every):
        r.Accumulate(every)
        frozen = mirt.adaptive_select(r.noise(floor=S["floor"])["tiles"], r.noise_above(at.TARGET, floor=S["floor"]), frozen, S["quantile"])
        assert np.array_equal(frozen, want["masks"][i]), f"freeze set after check {i + 1}"
        r.freeze_tiles(frozen)
    assert np.array_equal(r.tile_counts(), want["counts"])
    r.close()
    # the loop itself
    r = make(); r.Resize(w, h)
    res = r.accumulate_adaptive(at.TARGET, quantile=S["quantile"], floor=S["floor"], check_every=every, max_accumulations=top)
    counts = r.tile_counts()
    assert not res["converged"] and res["issued"] == top and res["checks"] == want["checks"] and res["owned_tiles"] == tiles
    assert np.array_equal(counts, want["counts"]) and res["frozen_tiles"] == int(want["masks"][-1].sum())
    assert res["tile_accumulations"] == int(counts.sum()) < tiles * res["issued"]
    got = r.accumulator()
    for t in range(tiles):
        assert_same(got[t], slabs[int(counts[t])][t], f"tile {t} at count {counts[t]}")
    assert r.counters()["rays"] < plain_rays
    r.close()
    # min_accumulations: nothing freezes before it
    r = make(); r.Resize(w, h)
    res = r.accumulate_adaptive(at.TARGET, quantile=S["quantile"], floor=S["floor"], check_every=every, min_accumulations=20, max_accumulations=20)
    assert not res["converged"] and res["issued"] == 20 and (r.tile_counts() == 20).all() and res["frozen_tiles"] > 0
    r.close()
    # MIRT_OK: every tile freezes at the first check
    r = make(); r.Resize(w, h)
    res = r.accumulate_adaptive(at.TARGET_ALL_FREEZE, quantile=S["quantile"], floor=S["floor"], check_every=every, max_accumulations=top)
    assert res["converged"] and res["issued"] == every and res["checks"] == 1 and res["frozen_tiles"] == tiles and (r.tile_counts() == every).all()
    r.close()


# ---- listed pixels (no candidate list) in frozen tiles -------------------------------------------------------------------------------
def test_listed_pixels_of_frozen_tiles_are_not_traced(mirt):
    """A scene whose silhouettes overflow the candidate lists: the pixels without a list are traced by k_trace<kPrimaryList>, once a tile is
    frozen over cand_listed ∩ active (k_listed_active).  Every run of tiles needs such pixels.  Words equal the plain contexts' on those tiles;
    `rays`, `shadow_rays`, `terminated`, `dropped` and the shadow rays' box and sphere tests equal their sum over the runs of equal count.  (The
    camera rays' own box counts include the lists' build, which a counting context repeats per batch over every owned pixel: no partition sum.)"""
    sc = mirt.scene.synthetic(20000, ambient=0.5)
    kw = dict(max_bounces=5, buckets=5, use_bvh=True, count_traffic=True)
    r = mirt.Renderer(sc, **kw); r.Resize(W, H)
    listed = (r.debug_primary_counts() == 0xFFFFFFFF).sum(axis=1)
    print(f"[adaptive] pixels without a list per tile: {listed.tolist()}")
    runs = [(0, 7, 15), (7, 4, 5), (11, 4, 10)]                                  # (first tile, tiles, count); the top tile row of this view has no such pixel
    assert all(listed[a:a + n].sum() > 0 for a, n, _ in runs), "every run needs pixels without a list"
    r.Accumulate(5); r.freeze_tiles([0] * 7 + [1] * 4 + [0] * 4)
    r.Accumulate(5); r.freeze_tiles([0] * 11 + [1] * 4)
    r.Accumulate(5)
    got, slab = r.counters(), r.accumulator(); r.close()
    keys = ("rays", "shadow_rays", "terminated", "dropped", "shadow_nodes", "shadow_spheres")
    want = dict.fromkeys(keys, 0)
    for first, n, count in runs:
        p = mirt.Renderer(sc, **kw); p.Resize(W, H); p.SetTileRange(first, n); p.Accumulate(count)
        c = p.counters()
        assert_same(slab[first:first + n], p.accumulator(), f"tiles {first} .. {first + n - 1} at count {count}")
        p.close()
        for k in keys:
            want[k] += c[k]
    assert {k: got[k] for k in keys} == want
    # Are the listed pixels of FROZEN tiles still traced?  Words and the counters above cannot tell (nobody reads those hit records, and `rays` comes
    # from k_primary_hits<COUNT, SPARSE = true>), the camera rays' box tests can: a counting context adds, per batch, the lists' build — the same cones over every
    # owned pixel, the same number each batch — plus the tree walk of the listed pixels' samples, whose rays differ from batch to batch.  With every
    # tile that holds a listed pixel frozen, nothing is left to walk: `nodes` grows by the same amount in every batch, and by less than in a plain
    # context, whose amounts differ.
    # (max_bounces = 1: camera rays only — the later bounces' closest-hit rays count into `nodes` as well.)
    def node_steps(freeze):
        x = mirt.Renderer(sc, **dict(kw, max_bounces=1)); x.Resize(W, H)
        x.Accumulate(5)
        if freeze is not None:
            x.freeze_tiles(freeze)
        steps, last = [], x.counters()["nodes"]
        for _ in range(3):
            x.Accumulate(5); now = x.counters()["nodes"]; steps.append(now - last); last = now
        x.close()
        return steps
    plain_steps, sparse_steps = node_steps(None), node_steps(listed > 0)
    print(f"[adaptive] box tests per batch: plain {plain_steps}, every tile with listed pixels frozen {sparse_steps}")
    assert (listed == 0).sum() >= 1 and len(set(plain_steps)) > 1
    assert len(set(sparse_steps)) == 1 and sparse_steps[0] > 0 and sparse_steps[0] < min(plain_steps)


# ---- 6. group ------------------------------------------------------------------------------------------------------------------------
def test_group_of_three_equals_the_single_context(mirt):
    S = at.SCENE
    sc = scene_of(mirt, "default9")
    w, h, k, every, top = S["width"], S["height"], S["buckets"], S["check_every"], S["max_accumulations"]
    kw = dict(max_bounces=S["max_bounces"], buckets=k, use_bvh=True, aov=True)
    r = mirt.Renderer(sc, **kw); r.Resize(w, h)
    g = mirt.GroupRenderer(sc, devices=(0, 0, 0), **kw); g.Resize(w, h)
    tiles = (w // 16) * (h // 16)
    mask = np.zeros(tiles, dtype=np.uint8); mask[[0, 5, 6, 15]] = 1                 # tiles of all three members (tile rows 0, 1, 3)
    for x in (r, g):
        x.Accumulate(every); x.freeze_tiles(mask); x.Accumulate(every)
    assert np.array_equal(g.tile_counts(), r.tile_counts()) and np.array_equal(g.frozen_tiles(), r.frozen_tiles()) and np.array_equal(g.frozen_tiles(), mask)
    assert set(r.tile_counts().tolist()) == {every, 2 * every}
    for target in (0.0, at.TARGET, 1e30):
        assert np.array_equal(g.noise_above(target), r.noise_above(target)), target
    assert r.Render() and g.Render()
    assert_same(g.GetFrame(), r.GetFrame(), "gathered frame, every tile at its own count")
    assert_same(g.accumulator(), r.accumulator(), "gathered accumulator")
    for which in (mirt.AOV_DEPTH, mirt.AOV_NORMAL, mirt.AOV_ALBEDO):
        assert_same(g.render_aov(which), r.render_aov(which), f"gathered AOV {which}")
    rep_r = r.accumulate_adaptive(at.TARGET, quantile=S["quantile"], floor=S["floor"], check_every=every, max_accumulations=top)
    rep_g = g.accumulate_adaptive(at.TARGET, quantile=S["quantile"], floor=S["floor"], check_every=every, max_accumulations=top)
    assert rep_g == rep_r and not rep_r["converged"] and 0 < rep_r["frozen_tiles"] < tiles
    assert np.array_equal(g.tile_counts(), r.tile_counts()) and g.counters()["rays"] == r.counters()["rays"]
    assert r.Render() and g.Render()
    assert_same(g.GetFrame(), r.GetFrame(), "gathered frame after the loop")
    bad = np.zeros(tiles + 1, dtype=np.uint8)
    assert g._lib.mirt_group_freeze_tiles(g._g, bad.ctypes.data_as(C.c_void_p), tiles + 1) == MIRT_ERR_ARG
    g.Accumulate(1)
    assert g._lib.mirt_group_freeze_tiles(g._g, bad.ctypes.data_as(C.c_void_p), tiles) == MIRT_ERR_STATE
    r.close(); g.close()


# ---- 7. headless ---------------------------------------------------------------------------------------------------------------------
def test_headless_adaptive_writes_the_counts(mirt, tmp_path):
    S = at.SCENE
    w, h = S["width"], S["height"]
    exe = os.path.join(mirt.CSRC, "mirt_headless")
    path = str(tmp_path / "counts.pfm")
    run = subprocess.run([exe, "--scene", "default9", "--size", f"{w}x{h}", "--bounces", str(S["max_bounces"]), "--buckets", str(S["buckets"]), "--adaptive", str(at.TARGET),
                          "--noise-quantile", str(S["quantile"]), "--noise-floor", str(S["floor"]), "--check-every", str(S["check_every"]),
                          "--max-accumulations", str(S["max_accumulations"]), "--counts-out", path], check=True, capture_output=True, text=True)
    lines = [json.loads(line) for line in run.stdout.strip().splitlines() if line.startswith("{")]
    report = next(d["adaptive"] for d in lines if "adaptive" in d)
    r = mirt.Renderer(scene_of(mirt, "default9"), max_bounces=S["max_bounces"], buckets=S["buckets"], use_bvh=True); r.Resize(w, h)
    res = r.accumulate_adaptive(at.TARGET, quantile=S["quantile"], floor=S["floor"], check_every=S["check_every"], max_accumulations=S["max_accumulations"])
    counts = r.tile_counts()
    for key in ("converged", "issued", "checks", "frozen_tiles", "owned_tiles", "tile_accumulations"):
        assert report[key] == res[key], key
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        assert [int(x) for x in f.readline().split()] == [w, h]
        assert float(f.readline()) < 0
        data = np.frombuffer(f.read(), dtype="<f4").reshape(h, w)
    painted = np.repeat(np.repeat(counts.reshape(h // 16, w // 16), 16, axis=0), 16, axis=1).astype(f32)
    assert np.array_equal(data, painted) and len(set(counts.tolist())) > 2
    assert lines[0]["accumulator_fnv1a"] == ob.fnv1a(r.accumulator())
    r.close()
