"""Store-once contribution buffer (-m gpu).  A batch of more accumulations than buckets (or one of several batches in flight)
writes each path's final radiance into its own word of the batch's contribution buffer with a single store, and the buffer
is never cleared.  MIRT_DEBUG_POISON_CONTRIB=1 fills it with a NaN pattern before every batch, so a word that no path
wrote reaches the accumulator as a NaN.  Each case reaches the endings a path can have (miss, Russian roulette with and
without a pending shadow ray, emissive hit, dropped after the last bounce) and is compared bit for bit with the
brute-force oracle."""
import numpy as np
import pytest

import oracle_binding as ob

pytestmark = pytest.mark.gpu


def same_bits(got, want, what):
    got = np.ascontiguousarray(got, dtype=np.float32); want = np.ascontiguousarray(want, dtype=np.float32)
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} words differ"


@pytest.fixture
def poisoned(monkeypatch):
    monkeypatch.setenv("MIRT_DEBUG_POISON_CONTRIB", "1")      # read at mirt_create


def run_case(mirt, sc, w, h, calls, mb, use_bvh=True, streams=1, max_batch=0, expect_contrib=True):
    spp = sum(calls)
    o = ob.Oracle(sc, max_bounces=mb, trav_mode=ob.TRAV_BRUTE); o.Resize(w, h); o.Accumulate(spp)
    r = mirt.Renderer(sc, max_bounces=mb, use_bvh=use_bvh, streams=streams, max_batch=max_batch); r.Resize(w, h)
    pol = r.get_policy()
    assert (pol["streams"] > 1 or pol["max_batch"] > 5) == expect_contrib     # uses_contrib(): more than one batch in flight, or batches > buckets
    for n in calls:
        r.AccumulateAsync(n)
    r.Synchronize()
    acc = r.accumulator()
    assert not np.isnan(acc).any(), "a contribution word was never written"
    same_bits(acc, o.accumulator(), "accumulator")
    if spp % 5 == 0:
        assert r.Render()
        frame = r.GetFrame()
        assert not np.isnan(frame).any()
        same_bits(frame, o.Render(), "frame")
    cg, co = r.counters(), o.counters()
    assert cg["rays"] == co["rays"] and cg["terminated"] == co["terminated"]
    assert cg["terminated"] + cg["dropped"] == spp * w * h                 # every path ended exactly once
    r.close()
    return cg


@pytest.mark.parametrize("use_bvh", [True, False])
def test_misses_and_roulette_endings(mirt, poisoned, use_bvh):
    """Sky misses (ambient 0.5), Russian roulette with and without a pending shadow ray; the BVH trace loop and the brute-force one."""
    c = run_case(mirt, mirt.scene.synthetic(1000, ambient=0.5), 192, 96, [12], mb=6, use_bvh=use_bvh)
    assert c["shadow_rays"] > 0 and c["terminated"] > 0


def test_emissive_hits(mirt, poisoned):
    """default9: three emissive spheres, so records carry the emissive term (kDestFull) for surviving and ending paths."""
    run_case(mirt, mirt.scene.default9(), 128, 64, [10], mb=16)


def test_paths_dropped_after_the_last_bounce(mirt, poisoned):
    """max_bounces = 2 and 1: many paths are still alive after the last bounce (Q5) and their words must still be written (+0)."""
    for mb in (2, 1):
        c = run_case(mirt, mirt.scene.synthetic(1000, ambient=0.5), 128, 96, [10], mb=mb)
        assert c["dropped"] > 0


def test_two_streams_and_a_partial_last_batch(mirt, poisoned):
    """Two batches in flight (each its own contribution buffer), batches of 4 with a last batch of 1 accumulation."""
    run_case(mirt, mirt.scene.synthetic(1000, ambient=0.5), 160, 96, [7, 6], mb=5, streams=2, max_batch=4)
    run_case(mirt, mirt.scene.default9(), 96, 64, [9, 6], mb=16, streams=2, max_batch=7)


def test_direct_mode_is_unchanged(mirt, poisoned):
    """One stream and batches no larger than the bucket count: paths add straight into the accumulator (no contribution buffer)."""
    run_case(mirt, mirt.scene.default9(), 128, 64, [5, 3, 2], mb=16, streams=1, max_batch=5, expect_contrib=False)
    run_case(mirt, mirt.scene.synthetic(1000, ambient=0.5), 128, 96, [5, 5], mb=2, streams=1, max_batch=3, expect_contrib=False)
