"""The camera rays' candidate lists live as long as the view (-m gpu).  k_primary_cand's output — a list of spheres per local pixel and
the pixels whose list overflowed — depends on the scene and its tree, the camera, the image size and the tiles a context owns, and on
nothing a batch brings along.  The first batch that wants lists builds them; later batches of any size, on any pipeline slot, read them;
every call that changes one of their inputs makes the next batch build them again; ResetAccumulator does not.

Yardsticks: a context with trace_primary_rays=1 (no lists at all: every camera ray walks the tree) run through the same calls, and, after
an invalidating call, a fresh context created in the new state.  Everything is compared on the raw words.  MIRT_DEBUG_POISON_CONTRIB=1
is set for every context, so a path that no kernel served reaches the accumulator as a NaN."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

f32 = np.float32
COUNTERS = ("rays", "shadow_rays", "terminated", "dropped")
W, H, MB = 128, 128, 5


@pytest.fixture(autouse=True)
def poisoned(monkeypatch):
    monkeypatch.setenv("MIRT_DEBUG_POISON_CONTRIB", "1")      # read at mirt_create


def same_bits(got, want, what):
    got = np.ascontiguousarray(got, dtype=f32); want = np.ascontiguousarray(want, dtype=f32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} words differ"


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def steep(mirt, n=1000):
    """S(n) seen from its usual eye, looking down 31 degrees: every pixel sees the ground sphere or something in front of it."""
    sc = mirt.scene.synthetic(n, ambient=0.5)
    sc.camera = mirt.scene.Camera(eye=tuple(float(v) for v in sc.camera.pos), direction=(0.0, -0.6, -1.0), focal_length=40.0, exposure=1.0)
    return sc


def crowded(mirt):
    """steep S(1000) + 600 spheres of radius 0.004 in a cube of side 0.15 on the view axis, 10 units from the eye.  At 128 rows a pixel
    is 0.047 wide there (|z| = 213): the cones of the pixels around the image centre touch far more than kCandMax = 31 of them and none
    is large enough to end the search, so those pixels get no list and k_trace<kPrimaryList> serves them."""
    sc = steep(mirt)
    s = mirt.scene
    d = np.array([0.0, -0.6, -1.0]); d /= np.sqrt((d * d).sum())
    centre = np.asarray(sc.camera.pos, dtype=np.float64) + 10.0 * d
    rng = np.random.default_rng(7)
    dust = np.zeros(600, dtype=s.SPHERE)
    dust["position"] = (centre + rng.uniform(-0.075, 0.075, size=(600, 3))).astype(f32)
    dust["radius_sq"] = f32(0.004) * f32(0.004)
    dust["material_ID"] = (np.arange(600) % 16).astype(np.int32)
    sc.geometry = np.concatenate([np.asarray(sc.geometry, dtype=s.SPHERE), dust])
    sc.name = "S(1000) + dust"
    return sc


def look_up(mirt, sc):
    """The same eye, looking up 5.7 degrees: the horizon of the ground sphere lies 8 degrees below the horizontal, so most pixels see sky only."""
    sc.camera = mirt.scene.Camera(eye=tuple(float(v) for v in sc.camera.pos), direction=(0.0, 0.1, -1.0), focal_length=40.0, exposure=1.0)


def snapshot(r, what):
    acc = r.accumulator().copy()
    assert not np.isnan(acc).any(), f"{what}: a contribution word was never written"
    out = {"acc": acc, "counters": {k: r.counters()[k] for k in COUNTERS}}
    if r.accumulations and r.accumulations % 5 == 0:                               # (Render() is not ready before the first accumulation)
        assert r.Render()
        out["frame"] = r.GetFrame().copy()
        assert not np.isnan(out["frame"]).any(), what
    if r.aov_enabled:
        out["aov"] = r.aov().copy()
    return out


def same_snapshot(got, want, what):
    assert got.keys() == want.keys(), what
    for k in got:
        if k == "counters":
            assert got[k] == want[k], f"{what}: counters {got[k]} vs {want[k]}"
        else:
            same_bits(got[k], want[k], f"{what}: {k}")


# ---- cached lists against no lists ------------------------------------------------------------------------------------------
def test_scene_has_pixels_with_and_without_a_list(mirt):
    r = mirt.Renderer(crowded(mirt), max_bounces=MB, use_bvh=True)
    r.Resize(W, H)
    hist = r.debug_primary_lists()
    print("crowded: candidate list lengths 0..8+ and pixels without a list:", hist)
    assert sum(hist) == W * H
    assert hist[9] > 0, "no pixel overflows its list: k_trace<kPrimaryList> is not exercised"
    assert sum(hist[1:9]) > W * H // 2
    assert r.debug_primary_lists() == hist                                            # the second call reads the lists of the first
    r.Accumulate(5)
    assert r.debug_primary_lists() == hist
    r.close()


@pytest.mark.parametrize("streams", [1, 3])
@pytest.mark.parametrize("max_batch", [1, 5, 0])
def test_cached_lists_equal_walking_the_tree(mirt, max_batch, streams):
    """Several consecutive batches, AOVs on: one call, N asynchronous calls of one accumulation, a remainder, and the same again after
    ResetAccumulator — which must give the first round's words once more, from lists that were not rebuilt."""
    rs = {}
    for walk in (False, True):
        r = mirt.Renderer(crowded(mirt), max_bounces=MB, use_bvh=True, max_batch=max_batch, streams=streams, trace_primary_rays=walk, aov=True)
        r.Resize(W, H)
        rs[walk] = r
    lists, walk = rs[False], rs[True]
    what = f"max_batch={max_batch} streams={streams}"

    def both(step, label):
        snaps = []
        for r in (lists, walk):
            step(r)
            snaps.append(snapshot(r, f"{what}, {label}"))
        same_snapshot(snaps[0], snaps[1], f"{what}, {label}: lists vs trace_primary_rays=1")
        return snaps[0]

    def one_by_one(r):
        for _ in range(13):
            r.AccumulateAsync(1)
        r.Synchronize()

    first = both(lambda r: r.Accumulate(13), "Accumulate(13)")
    both(one_by_one, "+ 13 x AccumulateAsync(1)")
    both(lambda r: r.Accumulate(4), "+ Accumulate(4)")
    assert lists.accumulations == 30
    both(lambda r: r.ResetAccumulator(), "ResetAccumulator")
    again = both(one_by_one, "13 x AccumulateAsync(1) after the reset")
    same_snapshot(again, first, f"{what}: 13 asynchronous calls after a reset vs Accumulate(13) on the new context")
    both(lambda r: r.Accumulate(12), "+ Accumulate(12)")
    plan = lists.get_policy()
    assert plan["streams"] == streams and plan["max_batch"] == (max_batch if max_batch else 256)
    for r in rs.values():
        r.close()


def test_two_contexts_with_interleaved_tile_rows(mirt):
    """Each context keeps the lists of its own rows; together they give the words of one context that walks the tree."""
    whole = mirt.Renderer(crowded(mirt), max_bounces=MB, use_bvh=True, trace_primary_rays=True, aov=True)
    whole.Resize(W, H)
    parts = []
    for rank in range(2):
        r = mirt.Renderer(crowded(mirt), max_bounces=MB, use_bvh=True, max_batch=5, aov=True)
        r.Resize(W, H); r.SetTileRows(rank, 2)
        parts.append(r)
    h_tiles, v_tiles = W // 16, H // 16
    for round_ in range(2):
        for n in (10, 7):
            for r in [whole] + parts:
                r.Accumulate(n)
            for name, planes in (("accumulator", 5 * 3), ("aov", 7)):
                get = (lambda r: r.accumulator()) if name == "accumulator" else (lambda r: r.aov())
                merged = np.zeros((v_tiles, h_tiles, planes * 256), dtype=f32)
                for rank, r in enumerate(parts):
                    part = get(r)
                    assert not np.isnan(part).any()
                    merged[rank::2] = part.reshape(v_tiles // 2, h_tiles, planes * 256)
                same_bits(merged.reshape(-1), get(whole).reshape(-1), f"round {round_}, +{n}: {name} of two contexts")
            total = {k: sum(r.counters()[k] for r in parts) for k in COUNTERS}
            assert total == {k: whole.counters()[k] for k in COUNTERS}
        for r in [whole] + parts:
            r.ResetAccumulator()
    for r in [whole] + parts:
        r.close()


# ---- when the lists are built ---------------------------------------------------------------------------------------------------
def test_lists_are_built_once_per_view(mirt):
    """policy.profile brackets every launch of the trace stage: a batch has max_bounces of them, and one more when it builds the lists."""
    sc = crowded(mirt)
    r = mirt.Renderer(sc, max_bounces=MB, use_bvh=True, max_batch=5, streams=1, profile=True)
    r.Resize(W, H)
    r.kernel_times()

    def batch_launches(n=5):
        r.Accumulate(n)
        return r.kernel_times()["trace"]["launches"]

    assert batch_launches() == MB + 1, "the first batch builds the lists"
    assert batch_launches() == MB
    assert batch_launches(4) == MB, "a smaller batch (>= 3 accumulations) reads the same lists"
    r.ResetAccumulator()
    assert batch_launches() == MB, "ResetAccumulator alone must not rebuild the lists"
    r.UpdateCamera()                                                                # the same camera again: nothing changed
    assert batch_launches() == MB
    look_up(mirt, sc); sc.camera.resize(W, H); r.UpdateCamera()
    assert batch_launches() == MB + 1, "camera moved"
    assert batch_launches() == MB
    r.Resize(W, H)
    assert batch_launches() == MB + 1, "Resize"
    r.UpdateScene()
    assert batch_launches() == MB + 1, "UpdateScene"
    r.SetTileRows(0, 2)
    assert batch_launches() == MB + 1, "SetTileRows"
    r.SetTileRange(0, 16)
    assert batch_launches() == MB + 1, "SetTileRange"
    assert batch_launches() == MB
    r.set_policy(trace_primary_rays=1)
    assert batch_launches() == MB
    r.set_policy(trace_primary_rays=0)
    assert batch_launches() == MB + 1, "trace_primary_rays toggled"
    r.set_policy(use_bvh=0)
    assert batch_launches() == MB
    r.set_policy(use_bvh=1)
    assert batch_launches() == MB + 1, "use_bvh toggled"
    r.set_policy(count_traffic=1)
    assert batch_launches() == MB + 1 and batch_launches() == MB + 1, "a counting pass builds the lists in every batch"
    r.set_policy(count_traffic=0)
    assert batch_launches() == MB
    r.close()


def test_counting_pass_counts_the_build_in_every_batch(mirt):
    """count_traffic=1: the box and sphere tests of k_primary_cand are part of every batch's counts, as they were when every batch built its lists."""
    r = mirt.Renderer(crowded(mirt), max_bounces=MB, use_bvh=True, max_batch=5, count_traffic=True)
    r.Resize(W, H)
    r.Accumulate(5)
    one = r.counters()
    r.ResetAccumulator()
    r.Accumulate(5)
    assert r.counters() == one and one["nodes"] > 0 and one["spheres"] > 0
    r.close()


# ---- invalidation: the next batch equals a fresh context's ----------------------------------------------------------------------------
def move_spheres(mirt, sc):
    geo = np.array(sc.geometry, dtype=mirt.scene.SPHERE)
    geo["position"][1:1000, 0] = -geo["position"][1:1000, 0]                        # mirrored in x: the builder sorts the prims anew
    geo["position"][1:1000, 2] += f32(3.0)
    sc.geometry = geo


# name -> (scene factory, Renderer kwargs at the start, change(mirt, r, sc), Renderer kwargs and set-up of the fresh context)
INVALIDATIONS = {
    "camera": (crowded, {}, lambda m, r, sc: (look_up(m, sc), sc.camera.resize(W, H), r.UpdateCamera()), {}, None),
    "resize": (crowded, {}, lambda m, r, sc: r.Resize(192, 96), {}, lambda r: r.Resize(192, 96)),
    "scene": (crowded, {}, lambda m, r, sc: (move_spheres(m, sc), r.UpdateScene()), {}, None),
    "tile_rows": (crowded, {}, lambda m, r, sc: r.SetTileRows(1, 2), {}, lambda r: r.SetTileRows(1, 2)),
    "use_bvh": (crowded, {"use_bvh": False}, lambda m, r, sc: r.set_policy(use_bvh=1), {}, None),
    "use_bvh_off_and_on": (crowded, {}, lambda m, r, sc: (r.set_policy(use_bvh=0), r.Accumulate(5), r.set_policy(use_bvh=1)), {}, None),
    "gpu_build": (steep, {}, lambda m, r, sc: (r.set_policy(gpu_build=1), r.UpdateScene()), {"gpu_build": True}, None),
    "reference_tree": (steep, {}, lambda m, r, sc: (r.set_policy(reference_tree=1), r.UpdateScene()), {"reference_tree": True}, None),
    "trace_primary_rays": (crowded, {"trace_primary_rays": True}, lambda m, r, sc: r.set_policy(trace_primary_rays=0), {}, None),
}


@pytest.mark.parametrize("streams", [1, 3])
@pytest.mark.parametrize("name", list(INVALIDATIONS))
def test_after_an_invalidating_call_the_next_batch_is_a_fresh_contexts(mirt, name, streams):
    make, kw0, change, kw1, setup = INVALIDATIONS[name]
    sc = make(mirt)
    base = dict(max_bounces=MB, use_bvh=True, max_batch=5, streams=streams)
    r = mirt.Renderer(sc, **{**base, **kw0})
    r.Resize(W, H)
    r.Accumulate(10)                                                                # two batches: the lists of the old state are in place
    before = r.debug_primary_lists() if r.get_policy()["use_bvh"] else None
    change(mirt, r, sc)
    r.ResetAccumulator()
    r.Accumulate(10)
    got = snapshot(r, name)
    after = r.debug_primary_lists()
    fresh = mirt.Renderer(copy.deepcopy(sc), **{**base, **kw1})
    fresh.Resize(W, H)
    if setup:
        setup(fresh)
    assert fresh.debug_primary_lists() == after, f"{name}: the lists in use are not those of a fresh context"
    fresh.Accumulate(10)
    same_snapshot(got, snapshot(fresh, name + " (fresh)"), f"{name}, streams={streams}: after the change vs a fresh context")
    if name == "camera":
        # a pixel whose list held something before and holds nothing now had a wrong list: that must be most pixels, or stale lists could pass
        n = W * H
        print("camera: list lengths before", before, "after", after)
        assert before[0] < n // 20 and after[0] > n // 2, (before, after)
        assert after[0] < n * 9 // 10, "the new view must still show something"
    r.close(); fresh.close()
