"""A path's radiance lives in its word of the batch's contribution buffer (-m gpu).  k_shade<FIRST> stores the word for every
path of the batch (+0 and what bounce 0 adds at once); every later `R += ...` of the reference is a read-modify-write of that
word, in the reference's order: k_trace's shadow_finish adds an unoccluded NEE term (and the emissive term that waited for
it), k_shade the emissive term of a hit without a pending light record and the sky term of a miss; a path still alive after
the last bounce gets its word overwritten with +0.  No stream carries radiance any more, and every batch — however small —
has a contribution buffer.  MIRT_DEBUG_POISON_CONTRIB=1 fills the buffer with a NaN pattern before every batch, so a word
that bounce 0 did not store reaches the accumulator as a NaN.  Every case is compared bit for bit with the brute-force oracle:
accumulator, frame, the rays / terminated counters, and `dropped` as the paths the oracle did not terminate."""
import numpy as np
import pytest

import oracle_binding as ob

pytestmark = pytest.mark.gpu


def same_bits(got, want, what):
    got = np.ascontiguousarray(got, dtype=np.float32); want = np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, what
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} words differ"


@pytest.fixture(autouse=True)
def poisoned(monkeypatch):
    monkeypatch.setenv("MIRT_DEBUG_POISON_CONTRIB", "1")      # read at mirt_create


def check(r, o, what, n_paths):
    acc = r.accumulator()
    assert not np.isnan(acc).any(), f"{what}: a contribution word was never written"
    same_bits(acc, o.accumulator(), f"{what}: accumulator")
    if r.accumulations % 5 == 0:
        assert r.Render()
        frame = r.GetFrame()
        assert not np.isnan(frame).any()
        same_bits(frame, o.Render(), f"{what}: frame")
    cg, co = r.counters(), o.counters()
    for k in ("rays", "terminated"):
        assert cg[k] == co[k], f"{what}: counter {k} {cg[k]} vs oracle {co[k]}"
    assert cg["shadow_rays"] <= co["shadow_rays"], what                # the reference also traces NEE rays of last-bounce hits, whose paths it then drops (Q5)
    assert cg["dropped"] == n_paths - co["terminated"], what           # the oracle does not count them: every path ends exactly once
    return cg


def run_case(mirt, sc, w, h, calls, mb, what, use_bvh=True, streams=1, max_batch=0, mis=True, brdf=0, decay=None):
    spp = sum(calls)
    o = ob.Oracle(sc, max_bounces=mb, mis=mis, trav_mode=ob.TRAV_BRUTE, brdf=brdf, gloss_decay=decay); o.Resize(w, h); o.Accumulate(spp)
    r = mirt.Renderer(sc, max_bounces=mb, mis=mis, use_bvh=use_bvh, streams=streams, max_batch=max_batch, brdf=brdf, gloss_decay=decay); r.Resize(w, h)
    for n in calls:
        r.AccumulateAsync(n)
    r.Synchronize()
    c = check(r, o, what, spp * w * h)
    r.close(); o.close()
    return c


@pytest.mark.parametrize("mb", [6, 9])
def test_sky_added_at_later_bounces(mirt, mb):
    """ambient > 0: a miss at bounce b > 0 adds thr.r * sky to a word that already holds the NEE terms of the earlier bounces."""
    c = run_case(mirt, mirt.scene.synthetic(1000, ambient=0.5), 192, 96, [12], mb, f"S(1000) ambient mb={mb}")
    assert c["shadow_rays"] > 0 and c["terminated"] > 0


def test_emissive_hits_with_and_without_a_light_record(mirt):
    """default9, 16 bounces: emissive hits whose light record is pending (E travels in the record: (w + S) + E, or w + E behind an
    occluder) and emissive hits without one (k_shade adds E), on paths that survive and on paths Russian roulette ends."""
    c = run_case(mirt, mirt.scene.default9(), 128, 64, [10], 16, "default9 mb=16")
    assert c["shadow_rays"] > 0
    run_case(mirt, mirt.scene.default9(), 128, 64, [10], 16, "default9 mb=16 without MIS", mis=False)     # no light records at all: every E is k_shade's


@pytest.mark.parametrize("mb", [3, 2])
def test_nee_add_then_dropped(mirt, mb):
    """MIS, few bounces: a path receives an unoccluded NEE add in the last k_trace launch and is then dropped after the last bounce
    (Q5) — its word must end as +0, as in the reference, which never accumulates such a path."""
    for sc, w, h, what in ((mirt.scene.synthetic(1000, ambient=0.5), 128, 96, "S(1000)"), (mirt.scene.default9(), 128, 64, "default9")):
        c = run_case(mirt, sc, w, h, [10], mb, f"{what} mb={mb}")
        assert c["dropped"] > 0 and c["shadow_rays"] > 0


def test_brute_force_loops(mirt):
    """use_bvh=False: the brute-force loops of k_trace call shadow_finish too."""
    c = run_case(mirt, mirt.scene.synthetic(1000, ambient=0.5), 128, 96, [7], 6, "S(1000) brute force", use_bvh=False)
    assert c["shadow_rays"] > 0
    run_case(mirt, mirt.scene.default9(), 96, 64, [10], 16, "default9 brute force", use_bvh=False)


def test_scene_with_fat_rays(mirt):
    """The scene and bounce count of cfg2 (S(1000), ambient 0.5, 5 bounces): its tangent frames stretch a few directions per million
    past the limit of the tree walk, and those rays take the one-workgroup-per-ray detour (k_trace_fat), whose thread 0 calls
    shadow_finish for a shadow ray.  (The detour has no counter of its own; 3.9 M paths make some tens of such rays.)"""
    c = run_case(mirt, mirt.scene.synthetic(1000, ambient=0.5), 512, 384, [20], 5, "S(1000) 512x384x20")
    assert c["shadow_rays"] > 0


@pytest.mark.parametrize("calls", [[5, 3, 2], [1, 1, 1, 1, 1]])
def test_small_batches_on_a_loaded_accumulator(mirt, calls):
    """One stream, batches no larger than the bucket count, and an accumulator loaded before the first call: the accumulator words
    hold earlier samples, so a path's running sum must not be formed in them — every batch has a contribution buffer and is merged."""
    sc = mirt.scene.default9()
    w, h, mb, before = 128, 64, 16, 5
    o = ob.Oracle(sc, max_bounces=mb, trav_mode=ob.TRAV_BRUTE); o.Resize(w, h); o.Accumulate(before)
    r = mirt.Renderer(sc, max_bounces=mb, use_bvh=True, streams=1, max_batch=5); r.Resize(w, h)
    pol = r.get_policy()
    assert pol["streams"] == 1 and pol["max_batch"] == 5
    r.load_accumulator(o.accumulator(), before)                                # resume: the oracle's first five samples
    assert r.accumulations == before
    done = before
    for n in calls:
        r.Accumulate(n); o.Accumulate(n); done += n
        acc = r.accumulator()
        assert not np.isnan(acc).any()
        same_bits(acc, o.accumulator(), f"resume + {calls}: accumulator after {done} accumulations")
    assert r.Render(); same_bits(r.GetFrame(), o.Render(), f"resume + {calls}: frame")
    cg, co = r.counters(), o.counters()                                        # the oracle counted the five loaded samples too
    o5 = ob.Oracle(sc, max_bounces=mb, trav_mode=ob.TRAV_BRUTE); o5.Resize(w, h); o5.Accumulate(before)
    c5 = o5.counters()
    for k in ("rays", "terminated"):
        assert cg[k] == co[k] - c5[k], k
    assert cg["dropped"] == sum(calls) * w * h - (co["terminated"] - c5["terminated"])
    r.close(); o.close(); o5.close()


def test_small_batches_from_an_empty_accumulator(mirt):
    run_case(mirt, mirt.scene.default9(), 128, 64, [5, 3, 2], 16, "[5, 3, 2] max_batch=5", streams=1, max_batch=5)
    run_case(mirt, mirt.scene.synthetic(1000, ambient=0.5), 128, 96, [1, 1, 1, 1, 1], 6, "[1] x 5 max_batch=5", streams=1, max_batch=5)


def test_two_streams_and_a_partial_last_batch(mirt):
    """Two batches in flight, each with its own buffer; batches of 4 with a last batch of 1 accumulation (the buffer's slot pitch
    is the batch's own accumulation count)."""
    run_case(mirt, mirt.scene.synthetic(1000, ambient=0.5), 160, 96, [7, 6], 5, "two streams S(1000)", streams=2, max_batch=4)
    run_case(mirt, mirt.scene.default9(), 96, 64, [9, 6], 16, "two streams default9", streams=2, max_batch=7)


def test_ggx_closure(mirt):
    """brdf=1: the second pair of k_shade instantiations."""
    decay = [0.0, 0.1, 0.3, 0.6, 1.0]
    run_case(mirt, mirt.scene.brdf_test(), 160, 96, [10], 16, "brdf_test GGX", brdf=1, decay=decay)
    run_case(mirt, mirt.scene.default9(), 64, 64, [10], 16, "default9 GGX", brdf=1, decay=decay)


def test_group_of_two_members_on_one_device(mirt):
    sc = mirt.scene.default9()
    w, h, mb, spp = 160, 96, 16, 10
    o = ob.Oracle(sc, max_bounces=mb, trav_mode=ob.TRAV_BRUTE); o.Resize(w, h); o.Accumulate(spp)
    g = mirt.GroupRenderer(sc, devices=[0, 0], max_bounces=mb, use_bvh=True); g.Resize(w, h)
    g.Accumulate(spp - 3); g.Accumulate(3)
    acc = g.accumulator()
    assert not np.isnan(acc).any()
    same_bits(acc, o.accumulator(), "group of 2: accumulator")
    assert g.Render(); same_bits(g.GetFrame(), o.Render(), "group of 2: frame")
    cg, co = g.counters(), o.counters()
    for k in ("rays", "terminated"):
        assert cg[k] == co[k], k
    assert cg["dropped"] == spp * w * h - co["terminated"]
    g.close(); o.close()
