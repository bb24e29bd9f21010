"""mirt_set_environment and mirt_set_sun_sky on the GPU: the baked map against the float64 definition within the derived bound, and the property of
the Ambient update — after it, everything equals a fresh mirt_set_scene with that environment, word for word — with its lifetime rules."""
import numpy as np
import pytest

import sky_definitions as sd
import sun_sky_definitions as ss
from test_sky_sampling_gpu import sun_scene
from test_sun_sky_cpu import SWEEP, check_against_definition, disc_case, report, sweep_params

pytestmark = pytest.mark.gpu
f32 = np.float32
W = H = 32
N_ACC, BUCKETS = 10, 5


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_words(a, b, what):
    assert a.shape == b.shape and np.array_equal(words(a), words(b)), what


def lit_scene(mirt, hdri=None, ambient=(1.0, 0.9, 0.8)):
    sc = mirt.scene.default9()
    sc.ambient = np.asarray(ambient, dtype=f32)
    if hdri is not None:
        sc.hdri = hdri
    return sc


def random_map(w=65, h=33, seed=5):
    m = np.random.default_rng(seed).random((h, w, 4)).astype(f32) * f32(2.0)
    m[h // 4, w // 6, :3] = 300.0
    return m


def outputs(r, sky=False):
    """Everything the property speaks of: accumulator, frame, AOVs, counters (and the sampling table)."""
    assert r.Render()
    out = dict(acc=r.accumulator(), frame=r.GetFrame().copy(), aov=r.aov(), counters=r.counters())
    if sky:
        t = r.debug_sky_table()
        out["table"] = np.concatenate([np.ravel(t[k]) for k in ("marg", "rowsum", "tn", "ts", "cond", "dens")])
    return out


def same_outputs(a, b, what):
    for k in a:
        if k == "counters":
            assert a[k] == b[k], (what, k)
        else:
            same_words(a[k], b[k], f"{what}: {k}")


def fresh(mirt, sc, n=N_ACC, **kw):
    r = mirt.Renderer(sc, max_bounces=6, buckets=BUCKETS, aov=True, **kw)
    r.Resize(W, H)
    if n:
        r.Accumulate(n)
    return r


# ---- the bake against the definition -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def baker(mirt):
    r = mirt.Renderer(lit_scene(mirt), max_bounces=2)
    yield r
    r.close()


@pytest.mark.parametrize("case", SWEEP + ["disc"], ids=lambda c: c if isinstance(c, str) else "%dx%d-el%g-T%g-sun%g" % (c[0], c[1], c[2], c[4], c[5]))
def test_baked_map_within_the_derived_bound(baker, case):
    p = disc_case() if case == "disc" else sweep_params(*case)
    baker.set_sun_sky(**p)
    amb, got, baked = baker.environment()
    assert baked and got.shape == (p["height"], p["width"], 4) and np.array_equal(amb, baker.scene.ambient)
    check_against_definition(got, p, "gpu " + str(case))                       # every texel; duplicates bit-equal; alpha 1
    baker.set_sun_sky(**p)
    same_words(baker.environment()[1], got, "two bakes of the same parameters")


# ---- baked and passed back -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(sky_sampling=True), dict(sky_sampling=True, light_ris=4)], ids=["plain", "sky", "sky_ris4"])
def test_baked_equals_the_same_map_handed_over(mirt, kw):
    p = ss.params(sun_dir=ss.sun_from_angles(35, 40), sun_radius=0.1, width=65, height=33)
    a = fresh(mirt, lit_scene(mirt), n=0, use_bvh=True, **kw)
    a.set_sun_sky(**p)
    a.Accumulate(N_ACC)
    _, baked_map, baked = a.environment()
    b = fresh(mirt, lit_scene(mirt, hdri=baked_map), use_bvh=True, **kw)
    assert baked and not b.environment()[2]
    same_outputs(outputs(a, "sky_sampling" in kw), outputs(b, "sky_sampling" in kw), "set_sun_sky against set_scene with the read-back map")
    if kw:
        assert a.counters()["shadow_rays"] > 0
    a.close(); b.close()


# ---- the property of the Ambient update ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_bvh,gpu_build,tpr,sky", [(False, False, False, False), (True, False, False, True), (True, True, False, False), (True, False, True, True),
                                                       (True, True, True, True)])
@pytest.mark.parametrize("which", ["random", "sun_map"])
def test_set_environment_equals_a_fresh_scene(mirt, which, use_bvh, gpu_build, tpr, sky):
    new_map = random_map() if which == "random" else sd.sun_map()
    new_amb = (0.5, 1.0, 2.0)
    kw = dict(use_bvh=use_bvh, gpu_build=gpu_build, trace_primary_rays=tpr, sky_sampling=sky)
    a = fresh(mirt, lit_scene(mirt, hdri=random_map(9, 5, seed=1)), n=5, **kw)         # another map, another size, and the lists of this view built
    a.set_environment(new_amb, new_map)
    a.ResetAccumulator()
    a.Accumulate(N_ACC)
    b = fresh(mirt, lit_scene(mirt, hdri=new_map, ambient=new_amb), **kw)
    same_outputs(outputs(a, sky), outputs(b, sky), f"set_environment against set_scene ({which}, {kw})")
    amb, got, baked = a.environment()
    same_words(got, new_map, "read back"); assert not baked and np.array_equal(amb, np.asarray(new_amb, dtype=f32))
    a.close(); b.close()


@pytest.mark.parametrize("sky", [False, True])
def test_ambient_only(mirt, sky):
    m = random_map()
    a = fresh(mirt, lit_scene(mirt, hdri=m), n=0, use_bvh=True, sky_sampling=sky)
    a.set_environment((0.25, 0.5, 0.0))
    a.Accumulate(N_ACC)
    b = fresh(mirt, lit_scene(mirt, hdri=m, ambient=(0.25, 0.5, 0.0)), use_bvh=True, sky_sampling=sky)
    same_outputs(outputs(a, sky), outputs(b, sky), "the ambient-only form")
    same_words(a.environment()[1], m, "the map is kept")
    a.set_environment((0.0, 0.0, 0.0)); a.ResetAccumulator(); a.Accumulate(BUCKETS)      # no ambient light: the miss shader adds nothing
    c = fresh(mirt, lit_scene(mirt, hdri=m, ambient=(0, 0, 0)), n=BUCKETS, use_bvh=True, sky_sampling=sky)
    same_words(a.accumulator(), c.accumulator(), "ambient 0")
    a.close(); b.close(); c.close()


# ---- lifetime ------------------------------------------------------------------------------------------------------------------------------
def test_history_and_candidate_lists_survive(mirt):
    m = random_map()
    a = fresh(mirt, lit_scene(mirt), use_bvh=True, trace_primary_rays=False)
    a.render_temporal()
    assert a.history_info()["valid"]
    before = a.accumulator()
    a.set_environment((1, 1, 1), m)
    assert a.history_info()["valid"], "mirt_set_environment dropped the temporal history"
    same_words(a.accumulator(), before, "the accumulator is not reset")
    a.set_sun_sky(width=65, height=33)
    assert a.history_info()["valid"], "mirt_set_sun_sky dropped the temporal history"
    a.set_environment((1, 1, 1), m)
    a.ResetAccumulator(); a.Accumulate(N_ACC)                                           # with the candidate lists built before the update
    b = fresh(mirt, lit_scene(mirt, hdri=m, ambient=(1, 1, 1)), use_bvh=True, trace_primary_rays=False)
    same_outputs(outputs(a), outputs(b), "trace_primary_rays = 0 after the update")
    a.close(); b.close()


def test_deferred_accumulations_render_under_the_old_map(mirt):
    old, new = random_map(seed=2), random_map(17, 9, seed=3)
    a = fresh(mirt, lit_scene(mirt, hdri=old), n=0, use_bvh=True)
    a.AccumulateAsync(3)                                                                # deferred (below a batch): launched by the update, under the old map
    a.set_environment(None, new)
    a.AccumulateAsync(7)
    b = fresh(mirt, lit_scene(mirt, hdri=old), n=3, use_bvh=True)
    b.set_environment(None, new)
    b.Accumulate(7)
    same_outputs(outputs(a), outputs(b), "asynchronous against two synchronous halves")
    c = fresh(mirt, lit_scene(mirt, hdri=new), n=10, use_bvh=True)
    assert not np.array_equal(words(a.accumulator()), words(c.accumulator()))         # the first three did see the old map
    a.close(); b.close(); c.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_with_a_context(mirt):
    import ctypes as C
    lib = mirt.load_library()
    ctx = C.c_void_p()
    assert lib.mirt_create(0, C.byref(ctx)) == 0
    amb = (C.c_float * 3)(1, 1, 1)
    one = (C.c_float * 4)(1, 1, 1, 1)
    p = mirt.SunSkyParams(); lib.mirt_sun_sky_defaults(C.byref(p))
    info = (C.c_uint32 * 4)()
    assert lib.mirt_set_environment(ctx, amb, one, 1, 1) == -3                          # MIRT_ERR_STATE: before mirt_set_scene
    assert lib.mirt_set_sun_sky(ctx, C.byref(p)) == -3
    assert lib.mirt_read_environment(ctx, None, 0, info) == -3
    assert lib.mirt_set_environment(ctx, None, one, 1, 1) == -1 and lib.mirt_set_environment(ctx, amb, None, 1, 1) == -1 and lib.mirt_set_environment(ctx, amb, one, 0, 1) == -1
    lib.mirt_destroy(ctx)

    m = random_map()
    r = fresh(mirt, lit_scene(mirt, hdri=m), n=0, use_bvh=True, sky_sampling=True)
    table = r.debug_sky_table()["dens"].copy()
    for field, value in (("turbidity", 1.5), ("turbidity", 11), ("sun_radius", 0.0), ("sun_radius", 0.2), ("sky_scale", -1), ("sun_scale", -1), ("width", 1), ("height", 1),
                         ("sun_dir", (0, 0, 0)), ("sun_dir", (0, -0.1, 1)), ("sun_dir", (np.nan, 1, 0)), ("ground", (np.inf, 0, 0))):
        with pytest.raises(mirt.MirtError):
            r.set_sun_sky(**{field: value})
    bad = m.copy(); bad[3, 5, 1] = np.nan
    with pytest.raises(mirt.MirtError, match="importance"):
        r.set_environment(None, bad)                                                    # sky sampling is on: refused before anything is changed
    with pytest.raises(mirt.MirtError, match="importance"):
        r.set_environment((-1, -1, -1))                                                 # the kept map under a negative ambient colour
    assert lib.mirt_read_environment(r._ctx, one, 4, info) == -1                         # too small
    amb_now, got, baked = r.environment()
    same_words(got, m, "a refused call leaves the old map in place"); assert not baked
    same_words(r.debug_sky_table()["dens"], table, "and the old table")
    r.Accumulate(BUCKETS)
    q = fresh(mirt, lit_scene(mirt, hdri=m), n=BUCKETS, use_bvh=True, sky_sampling=True)
    same_words(r.accumulator(), q.accumulator(), "and renders as before")
    r.set_sky_sampling(False)
    r.set_environment(None, bad)                                                        # off: nothing is asked of the texels, as mirt_set_scene
    r.close(); q.close()


# ---- group, exact stream order ----------------------------------------------------------------------------------------------------------------
def test_three_member_group_equals_the_single_context(mirt):
    p = ss.params(sun_dir=ss.sun_from_angles(35, 40), sun_radius=0.1, width=65, height=33)
    m = random_map()
    r = fresh(mirt, lit_scene(mirt), n=0, use_bvh=True, sky_sampling=True)
    g = mirt.GroupRenderer(lit_scene(mirt), devices=(0, 0, 0), max_bounces=6, buckets=BUCKETS, aov=True, sky_sampling=True)
    g.Resize(W, 48)                                                                     # three tile rows: one per member
    r.Resize(W, 48)
    for x in (r, g):
        x.set_sun_sky(**p); x.Accumulate(N_ACC)
    same_words(g.accumulator(), r.accumulator(), "group: baked"); same_words(g.aov(), r.aov(), "group: baked AOVs")
    assert g.counters() == r.counters()
    _, gm, gb = g.environment(); _, rm, rb = r.environment()
    same_words(gm, rm, "every device bakes the same words"); assert gb and rb
    for x in (r, g):
        x.set_environment((0.5, 1, 2), m); x.ResetAccumulator(); x.Accumulate(N_ACC)
    same_words(g.accumulator(), r.accumulator(), "group: set_environment")
    assert g.Render() and r.Render()
    same_words(g.GetFrame(), r.GetFrame(), "group: frame")
    g.close(); r.close()


def test_exact_stream_order_takes_the_update(mirt):
    m = random_map()
    r = mirt.Renderer(lit_scene(mirt), max_bounces=6, buckets=BUCKETS, exact_stream_order=True); r.Resize(W, H)
    r.set_environment((0.5, 1, 2), m); r.Accumulate(BUCKETS)
    q = mirt.Renderer(lit_scene(mirt, hdri=m, ambient=(0.5, 1, 2)), max_bounces=6, buckets=BUCKETS, exact_stream_order=True); q.Resize(W, H); q.Accumulate(BUCKETS)
    same_words(r.accumulator(), q.accumulator(), "exact stream order: set_environment")
    r.set_sun_sky(width=65, height=33); r.ResetAccumulator(); r.Accumulate(BUCKETS)
    _, baked_map, _ = r.environment()
    q.scene.hdri = baked_map; q.UpdateScene(); q.ResetAccumulator(); q.Accumulate(BUCKETS)
    same_words(r.accumulator(), q.accumulator(), "exact stream order: set_sun_sky")
    r.close(); q.close()


# ---- what it is for ------------------------------------------------------------------------------------------------------------------------
def test_sky_sampling_pays_under_the_default_sun(mirt):
    """A Lambertian ground under the default sun baked at 65 x 33, equal accumulations: the median of mirt_noise's map is lower with sky sampling
    on (asserted as < only; the two figures of one run are in profiles/sun_sky.txt).  The disc's radius is 0.1 rad: at 65 x 33 the sub-samples
    lie 0.025 rad apart and the default disc of 0.00465 rad falls between them, leaving a sky without a sun."""
    med = {}
    for on in (False, True):
        r = mirt.Renderer(sun_scene(mirt, "plain"), max_bounces=6, buckets=16, use_bvh=True, sky_sampling=on)
        r.Resize(64, 64)
        r.set_sun_sky(sun_radius=0.1, width=65, height=33)
        r.Accumulate(80)
        med[on] = float(np.median(r.noise(want_map=True)["map"]))
        r.close()
    report("noise median under the default sun, 65x33, 64x64x80", off=med[False], on=med[True])
    assert med[True] < med[False]
