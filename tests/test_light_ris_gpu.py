"""Resampled importance sampling of the NEE light on the device (mirt_set_light_ris; k_shade<..., RIS = true>, shade_hit_body.inc).

1  one candidate is the plain path word for word, so the RIS kernels must give the ORACLE's words;
1b the oracle carries the candidate loop itself (orc_set_light_ris, held to the float64 estimator in tests/test_light_ris_cpu.py): every RIS twin
   kernel - first and later bounces, Lambertian and GGX, dense and sparse - gives the oracle's words for M > 1, and at the draw that is 1.0f;
2  more candidates keep the expectation: part F's quadrature, with the variance of tests/ris_definitions.py;
3  a hit whose candidates all weigh nothing casts nothing;
4  on MANY the noise estimate falls, by what the float64 estimator predicts;
5  the words do not depend on how the work is cut up;  6  the refusals.
The float64 side and its guards: tests/test_light_ris_cpu.py."""
import math
import os

import numpy as np
import pytest

import oracle_binding as ob
import test_definitions_cpu as cpu
import test_light_ris_cpu as ris
import views_and_scales as vs
from test_definitions_cpu import F_CASES, F_H, F_RHO, F_W, SIGMA, backend_image, guard_first_hits, lit_scene, report

pytestmark = pytest.mark.gpu
COUNTERS = ("rays", "terminated")      # what the oracle and the wavefront pipeline count alike


def same_words(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape, what
    diff = a.view(np.uint32) != b.view(np.uint32)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} words differ"


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------
def cloud_compound(mirt):
    return vs.VIEWS["compound"].make(mirt)


DECAY = [0.0, 0.3, 0.6, 0.8]
ORACLE_CASES = {   # scene, width, height, accumulations, renderer keywords shared with the oracle
    "default9": (lambda m: m.scene.default9(), 160, 96, 10, {}),
    "S1000": (lambda m: m.scene.synthetic(1000), 128, 128, 5, {}),
    "cloud37": (cloud_compound, 64, 48, 5, {}),
    "brdf_test_ggx": (lambda m: m.scene.brdf_test(), 96, 64, 5, dict(brdf=1, gloss_decay=DECAY)),
    "default9_ggx": (lambda m: m.scene.default9(), 96, 64, 5, dict(brdf=1, gloss_decay=DECAY)),
}


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_one_candidate_is_the_oracle(mirt, name):
    """The test that fails without the feature: the candidate loop with M = 1 - its draws in their order, the reservoir's 1.0f, the scaling
    of the carried radiance - must leave every word and every counter the oracle's."""
    make, w, h, n, kw = ORACLE_CASES[name]
    sc = make(mirt)
    if name == "cloud37":
        assert len(mirt.light_list(sc.geometry, sc.material)) == 37
    ref = ob.Oracle(sc, max_bounces=16, buckets=5, trav_mode=ob.TRAV_BRUTE, **kw)
    ref.Resize(w, h); ref.Accumulate(n)
    want_acc, want_img, want_c = ref.accumulator(), ref.Render().copy(), ref.counters()
    ref.close()
    for label, route in (("tree", dict(use_bvh=True)), ("brute", dict(use_bvh=False)), ("tree, traced camera rays", dict(use_bvh=True, trace_primary_rays=True))):
        r = mirt.Renderer(sc, max_bounces=16, buckets=5, light_ris=1, **route, **kw)
        assert r.light_ris() == 1
        r.Resize(w, h); r.Accumulate(n)
        assert r.Render()
        same_words(r.accumulator(), want_acc, f"{name}, {label}: accumulator")
        same_words(r.GetFrame(), want_img, f"{name}, {label}: frame")
        got = r.counters()
        assert {k: got[k] for k in COUNTERS} == {k: want_c[k] for k in COUNTERS}, (name, label)
        # the reference also casts the shadow rays of last-bounce hits, whose paths it then drops (Q5), and counts no dropped paths: the pipeline
        # casts none of those, so these two are held to the plain draw's, word for word, and to the oracle's from their side
        plain = mirt.Renderer(sc, max_bounces=16, buckets=5, **route, **kw)
        plain.Resize(w, h); plain.Accumulate(n)
        pc = plain.counters(); plain.close()
        assert got["shadow_rays"] == pc["shadow_rays"] <= want_c["shadow_rays"] and got["dropped"] == pc["dropped"], (name, label)
        assert got["dropped"] == n * (w // 16) * (h // 16) * 256 - want_c["terminated"], (name, label)
        r.close()


# ---- 1b: M > 1 against the oracle's own candidate loop ------------------------------------------------------------------------------------
ROUTES = (("tree", dict(use_bvh=True)), ("brute", dict(use_bvh=False)), ("tree, traced camera rays", dict(use_bvh=True, trace_primary_rays=True)))
MANY_CANDIDATES = {   # scene, width, height, keywords shared with the oracle: 5 accumulations, max_bounces 16 - later-bounce launches with partly filled waves
    "default9": (lambda m: m.scene.default9(), 96, 64, {}),
    "S1000": (lambda m: m.scene.synthetic(1000), 64, 64, {}),
    "cloud37": (cloud_compound, 64, 48, {}),
    "brdf_test_ggx": (lambda m: m.scene.brdf_test(), 96, 64, dict(brdf=1, gloss_decay=DECAY)),
    "default9_ggx": (lambda m: m.scene.default9(), 96, 64, dict(brdf=1, gloss_decay=DECAY)),
}
# 2: the first carried selection; 7: odd; 32: the cap; 16 (default9): where the timing jumps
CANDIDATE_CASES = [(name, m) for name in MANY_CANDIDATES for m in (2, 7, 32)] + [("default9", 16)]
_oracle_cache = {}


def oracle_states(sc, key, w, h, counts, max_bounces=16, tiles_after=None, **kw):
    """The oracle after each of `counts` accumulations: acc, frame, counters of the brute-force mode (the reference as shipped) and `twin`, the counters
    of its mode 2, which casts no shadow ray for a last-bounce hit (Q5) as the pipeline does not - its words must be the brute-force words.
    tiles_after = (n, tiles): also `active`, both modes' counters of the calls after number n on those tiles alone (what a context with the other tiles
    frozen at n goes on to trace).  Computed once a process for a key."""
    key = (key, w, h, tuple(counts), max_bounces, None if tiles_after is None else (tiles_after[0], tuple(tiles_after[1])))
    if key in _oracle_cache:
        return _oracle_cache[key]
    out = {}
    for mode in (ob.TRAV_BRUTE, ob.TRAV_PER_RAY_BVH):
        o = ob.Oracle(sc, max_bounces=max_bounces, buckets=5, trav_mode=mode, **kw)
        o.Resize(w, h)
        done = 0
        for n in counts:
            o.Accumulate(n - done); done = n
            if mode == ob.TRAV_BRUTE:
                out[n] = dict(acc=o.accumulator(), frame=o.Render().copy(), counters=o.counters())
            else:
                same_words(o.accumulator(), out[n]["acc"], f"oracle, {n} accumulations: mode 2 against brute force")
                out[n]["twin"] = o.counters()
        if tiles_after is not None:
            n, tiles = tiles_after
            o.Resize(w, h, tiles=tiles)
            o.ResetAccumulator()
            o.load_accumulator(np.zeros(len(tiles) * 5 * 3 * 256, dtype=np.float32), n)
            o.Accumulate(counts[-1] - n)
            out.setdefault("active", {})[mode] = o.counters()
        o.close()
    _oracle_cache[key] = out
    return out


def check_against_oracle(r, want, what):
    """Accumulator and frame word for word; rays and terminated the oracle's; shadow_rays the twin mode's exactly and at most the brute-force mode's."""
    assert r.Render()
    same_words(r.accumulator(), want["acc"], f"{what}: accumulator")
    same_words(r.GetFrame(), want["frame"], f"{what}: frame")
    got = r.counters()
    assert {k: got[k] for k in COUNTERS} == {k: want["counters"][k] for k in COUNTERS}, what
    assert {k: got[k] for k in COUNTERS} == {k: want["twin"][k] for k in COUNTERS}, what
    assert got["shadow_rays"] == want["twin"]["shadow_rays"] <= want["counters"]["shadow_rays"], what


@pytest.mark.parametrize("name,candidates", CANDIDATE_CASES)
def test_many_candidates_are_the_oracle(mirt, name, candidates):
    """What the suite could not see before: a register lost over a spill in the candidate loop, a draw out of order for candidate i >= 2, or
    weight_sum / (float(M) * w_sel) formed another way would all keep the expectation and the route invariance.  Every word is the oracle's."""
    make, w, h, kw = MANY_CANDIDATES[name]
    sc = make(mirt)
    want = oracle_states(sc, (name, candidates), w, h, (5,), light_ris=candidates, **kw)[5]
    plain = oracle_states(sc, (name, 0), w, h, (5,), **kw)[5]
    assert (want["acc"].view(np.uint32) != plain["acc"].view(np.uint32)).any()                     # the candidates change the words
    for label, route in ROUTES:
        r = mirt.Renderer(sc, max_bounces=16, buckets=5, light_ris=candidates, **route, **kw)
        r.Resize(w, h); r.Accumulate(5)
        check_against_oracle(r, want, f"{name}, M = {candidates}, {label}")
        r.close()


def tile_pixels(mask, w, h):
    return np.repeat(np.repeat(np.asarray(mask).reshape(h // 16, w // 16), 16, axis=0), 16, axis=1)


def check_frozen_against_oracle(mirt, sc, key, w, h, routes, max_bounces=16, setup=None, **kw):
    """5 accumulations, every third tile frozen, 5 more (the SPARSE kernels): the frozen tiles hold the oracle's words at 5, the active ones its words
    at 10, in the accumulator and in the frame; the counters are the oracle's first five calls plus its calls 6..10 on the active tiles alone."""
    mask = np.arange((w // 16) * (h // 16)) % 3 == 0
    want = oracle_states(sc, key, w, h, (5, 10), max_bounces=max_bounces, tiles_after=(5, np.flatnonzero(~mask)), **kw)
    five, ten, px = want[5], want[10], tile_pixels(mask, w, h)
    for label, route in routes:
        what = f"{key}, frozen tiles, {label}"
        r = mirt.Renderer(sc, max_bounces=max_bounces, buckets=5, **route, **{k: v for k, v in kw.items() if k != "lens"})
        r.Resize(w, h)
        if "lens" in kw:
            r.set_lens(*kw["lens"])
        r.Accumulate(5); r.freeze_tiles(mask); r.Accumulate(5)
        assert r.Render()
        acc, frame = r.accumulator(), r.GetFrame()
        same_words(acc[mask], five["acc"][mask], f"{what}: frozen tiles"); same_words(acc[~mask], ten["acc"][~mask], f"{what}: active tiles")
        same_words(frame[px], five["frame"][px], f"{what}: frame of the frozen tiles"); same_words(frame[~px], ten["frame"][~px], f"{what}: frame of the active tiles")
        got = r.counters()
        for k in COUNTERS:
            assert got[k] == five["counters"][k] + want["active"][ob.TRAV_BRUTE][k] == five["twin"][k] + want["active"][ob.TRAV_PER_RAY_BVH][k], (what, k)
        assert got["shadow_rays"] == five["twin"]["shadow_rays"] + want["active"][ob.TRAV_PER_RAY_BVH]["shadow_rays"], what
        assert got["shadow_rays"] <= five["counters"]["shadow_rays"] + want["active"][ob.TRAV_BRUTE]["shadow_rays"], what
        r.close()


@pytest.mark.parametrize("name", ["default9", "brdf_test_ggx"])
def test_sparse_twins_are_the_oracle(mirt, name):
    """k_shade<true, GGX, LENS = false, SPARSE = true, RIS = true>, through the camera-ray lists and through traced camera rays."""
    make, w, h, kw = MANY_CANDIDATES[name]
    check_frozen_against_oracle(mirt, make(mirt), name, w, h, (ROUTES[0], ROUTES[2]), light_ris=7, **kw)


def test_the_draw_that_is_one(mirt):
    """At the call and pixel where the first candidate's reservoir draw is exactly 1.0f (tests/test_light_ris_cpu.py ONE_ACC, ONE_PIXEL, where the
    oracle's side is asserted): device M = 1 = device M = 0 = the oracle; device M = 7 = the oracle's M = 7.  Both sides load an empty slab at the count."""
    sc = ris.one_scene(mirt)
    dev = {m: ris.one_run(lambda: mirt.Renderer(sc, max_bounces=ris.ONE_BOUNCES, buckets=5, use_bvh=True, light_ris=m)) for m in (0, 1, 7)}
    orc = {m: ris.one_run(lambda: ob.Oracle(sc, max_bounces=ris.ONE_BOUNCES, buckets=5, light_ris=m)) for m in (0, 7)}
    assert dev[0][0, ris.ONE_ACC % 5, :, ris.ONE_PIXEL].min() > 0
    same_words(dev[0], orc[0], "plain draw against the oracle"); same_words(dev[1], dev[0], "M = 1 against the plain draw")
    same_words(dev[7], orc[7], "M = 7 against the oracle")
    assert (dev[7].view(np.uint32) != dev[0].view(np.uint32)).any()


# ---- 2, 3 -------------------------------------------------------------------------------------------------------------------------
def render_f(mirt, lights, n_acc, candidates, **kw):
    sc = lit_scene(mirt, lights)
    r = mirt.Renderer(sc, max_bounces=3, buckets=5, light_ris=candidates, **kw)
    r.Resize(F_W, F_H); r.Accumulate(n_acc)
    out = dict(acc=r.accumulator(), counters=r.counters())
    r.close()
    return sc, out


@pytest.mark.parametrize("name,candidates", ris.RIS_CASES)
def test_unbiased(mirt, name, candidates):
    """check_direct's bounds with the estimator's own variance: every regional mean within SIGMA standard errors of the quadrature,
    `shadow_rays` within SIGMA Bernoulli sigma of the exact share 1 - (1 - p)^M, `rays` and `terminated` exactly the plain path's."""
    n_acc = ris.MANY_ACC if name == "MANY" else F_CASES[name]["n_acc"]
    lights = ris.case_lights(name)
    exp, var = ris.expectation(name), ris.sampler(name, candidates)
    sc, res = render_f(mirt, lights, n_acc, candidates, use_bvh=True)
    _, plain = render_f(mirt, lights, n_acc, 0, use_bvh=True)
    be = type("be", (), {"raygen": staticmethod(lambda s, w, h, acc, max_bounces=16: raygen(mirt, s, w, h, acc, max_bounces))})
    guard_first_hits(be, sc, 3)
    img = backend_image(res, n_acc)
    zs = {}
    for label, mask in ris.regions(name).items():
        k = mask.reshape(-1)
        want = exp["E"][k].mean(axis=0)
        se = np.sqrt(var["var"][k].sum(axis=0) / n_acc) / k.sum()
        assert mask.sum() >= 64 and (want > 0).all() and (se / want < 0.01).all(), (name, label, se / want)
        zs[label] = (img[mask].mean(axis=0) - want) / se
    c = res["counters"]
    share = np.load(ris.GOLDEN)["shadow_probability"] if name == "MANY" else ris.shadow_share(name, candidates)      # exact: 1 - (1 - p)^M
    want_sh = n_acc * share.sum()
    sigma_sh = math.sqrt(n_acc * (share * (1 - share)).sum())
    report(f"gpu/ris/{name}/M{candidates}", **{f"z_{k}": "/".join(f"{v:+.2f}" for v in z) for k, z in zs.items()},
           shadow_rays=c["shadow_rays"], shadow_expected=float(want_sh), shadow_sigma=float(sigma_sh), shadow_plain=plain["counters"]["shadow_rays"])
    for label, z in zs.items():
        assert np.abs(z).max() <= SIGMA, f"{name}/{label}: {z} sigma from the expectation"
    assert abs(c["shadow_rays"] - want_sh) <= SIGMA * sigma_sh, f"{name}: {c['shadow_rays']} shadow rays, expected {want_sh:.1f} +- {sigma_sh:.1f}"
    for k in ("rays", "terminated", "dropped"):
        assert c[k] == plain["counters"][k], k


def raygen(mirt, sc, w, h, acc, max_bounces):
    r = mirt.Renderer(sc, max_bounces=max_bounces); r.Resize(w, h)
    p, d = r.debug_raygen(acc); r.close()
    return p, d


def test_all_candidates_weigh_nothing(mirt):
    """F1 BELOW, eight candidates: every one leaves at the horizon test, nothing is selected, nothing is cast, nothing arrives."""
    _, res = render_f(mirt, [cpu.BELOW], 100, 8, use_bvh=True)
    assert not res["acc"].any() and res["counters"]["shadow_rays"] == 0


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
def test_noise_falls_on_many(mirt):
    """mirt_noise's mean relative standard error on MANY, 16 buckets x 15 samples, eight candidates against none.  The float64 estimator
    gives the ratio of the variances (tests/golden/light_ris_many.npz); the measurement is a standard error, hence its square root, widened
    by half its distance to 1 because a bucket estimate of a few samples is itself noisy."""
    g = np.load(ris.GOLDEN)
    bound = math.sqrt(float(g["var_ratio"])); bound += 0.5 * (1.0 - bound)
    sc = lit_scene(mirt, ris.MANY)
    got = {}
    for m in (0, 8):
        r = mirt.Renderer(sc, max_bounces=3, buckets=16, use_bvh=True, light_ris=m)
        r.Resize(F_W, F_H); r.Accumulate(16 * 15)
        got[m] = float(r.noise()["mean"])
        r.close()
    report("gpu/ris/noise", noise_0=got[0], noise_8=got[8], ratio=got[8] / got[0], bound=bound, predicted=math.sqrt(float(g["var_ratio"])))
    if os.environ.get("MIRT_LIGHT_RIS_REPORT"):                                      # a file to append the two values to (profiles/light_ris.txt, part 5)
        with open(os.environ["MIRT_LIGHT_RIS_REPORT"], "a") as f:
            f.write(f"MANY 64x64, 240 accumulations, 16 buckets: mirt_noise mean M=0 {got[0]:.6f}  M=8 {got[8]:.6f}  ratio {got[8] / got[0]:.4f}  bound {bound:.4f}\n")
    assert got[8] < bound * got[0]


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------
INVARIANCE_SCENES = {"default9": (lambda m: m.scene.default9(), 160, 96), "S1000": (lambda m: m.scene.synthetic(1000), 128, 128)}


@pytest.mark.parametrize("name", list(INVARIANCE_SCENES))
def test_words_do_not_depend_on_the_route(mirt, name):
    make, w, h = INVARIANCE_SCENES[name]
    sc, n, mb = make(mirt), 13, 8

    def run(n_acc=n, setup=None, accumulate=None, **kw):
        r = mirt.Renderer(sc, max_bounces=mb, buckets=5, **{"light_ris": 8, "use_bvh": True, **kw})
        r.Resize(w, h)
        if setup:
            setup(r)
        (accumulate or (lambda q: q.Accumulate(n_acc)))(r)
        acc = r.accumulator()
        r.close()
        return acc

    base = run()
    routes = {
        "brute force": dict(use_bvh=False), "tree built on the device": dict(gpu_build=True), "traced camera rays": dict(trace_primary_rays=True),
        "max_batch 1": dict(max_batch=1), "max_batch 5": dict(max_batch=5), "streams 1": dict(streams=1), "streams 3, max_batch 2": dict(streams=3, max_batch=2),
        "AOVs on": dict(aov=True),
        "13 x async(1)": dict(accumulate=lambda r: [r.AccumulateAsync(1) for _ in range(n)]),
        "set after construction": dict(light_ris=0, setup=lambda r: r.set_light_ris(8)),
    }
    for label, kw in routes.items():
        same_words(run(**kw), base, f"{name}: {label}")
    # deferred calls are launched first, under the old setting: 4 plain accumulations left deferred, then eight candidates for the rest
    def switch(accumulate):
        def go(q):
            accumulate(q, 4); q.set_light_ris(8); q.Accumulate(n - 4)
        return go
    mixed = run(light_ris=0, accumulate=switch(lambda q, k: q.Accumulate(k)))
    same_words(run(light_ris=0, accumulate=switch(lambda q, k: q.AccumulateAsync(k))), mixed, f"{name}: the setter after a deferred call")
    assert (mixed.view(np.uint32) != base.view(np.uint32)).any() and (mixed.view(np.uint32) != run(light_ris=0).view(np.uint32)).any()
    # two runs of one context
    r = mirt.Renderer(sc, max_bounces=mb, buckets=5, use_bvh=True, light_ris=8)
    r.Resize(w, h); r.Accumulate(n); r.ResetAccumulator(); r.Accumulate(n)
    same_words(r.accumulator(), base, f"{name}: second run of a context")
    # off again: the words of a context that never called the setter
    r.set_light_ris(0); r.ResetAccumulator(); r.Accumulate(n)
    assert r.light_ris() == 0
    same_words(r.accumulator(), run(light_ris=0), f"{name}: M = 0 after M = 8")
    r.close()
    # two contexts with interleaved tile rows; a group of three
    h_tiles, v_tiles = w // 16, h // 16
    merged = np.zeros((v_tiles, h_tiles) + base.shape[1:], dtype=np.float32)
    for rank in range(2):
        part = run(setup=lambda q: q.SetTileRows(rank, 2))
        merged[rank::2] = part.reshape((-1, h_tiles) + base.shape[1:])
    same_words(merged.reshape(base.shape), base, f"{name}: two contexts with interleaved tile rows")
    g = mirt.GroupRenderer(sc, devices=[0, 0, 0], max_bounces=mb, buckets=5, use_bvh=True, light_ris=8)
    assert g.light_ris() == 8
    g.Resize(w, h); g.Accumulate(n)
    same_words(g.accumulator(), base, f"{name}: a group of three")
    g.close()
    # a lens: the words of the same lens through the traced-camera-ray route and through brute force (against the oracle: tests/test_lens_gpu.py)
    lens = dict(setup=lambda q: q.set_lens(0.05, 4.0))
    same_words(run(**lens), run(use_bvh=False, **lens), f"{name}: lens, tree against brute force")
    # frozen tiles: the active tiles go on as if nothing were frozen, the frozen ones keep their words
    mask = (np.arange(h_tiles * v_tiles) % 3 == 0)

    def freeze(q):
        q.Accumulate(5); q.freeze_tiles(mask); q.Accumulate(5)
    got, five, ten = run(accumulate=freeze), run(n_acc=5), run(n_acc=10)
    same_words(got[~mask], ten[~mask], f"{name}: active tiles beside frozen ones")
    same_words(got[mask], five[mask], f"{name}: frozen tiles")


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(mirt):
    lib = mirt.load_library()
    r = mirt.Renderer(mirt.scene.default9(), max_bounces=4)
    assert r.light_ris() == 0
    with pytest.raises(mirt.MirtError, match="33 candidates"):
        r.set_light_ris(33)
    assert lib.mirt_set_light_ris(r._ctx, 33) == -1 and r.light_ris() == 0            # MIRT_ERR_ARG
    r.set_light_ris(32); assert r.light_ris() == 32
    assert lib.mirt_set_stream_order(r._ctx, 1) == -3 and r.stream_order == 0          # MIRT_ERR_STATE
    with pytest.raises(mirt.MirtError, match="mirt_set_light_ris"):
        r.set_stream_order(True)
    r.set_light_ris(0); r.set_stream_order(True)
    assert lib.mirt_set_light_ris(r._ctx, 4) == -3 and r.light_ris() == 0
    with pytest.raises(mirt.MirtError, match="mirt_set_stream_order"):
        r.set_light_ris(4)
    r.set_light_ris(0)                                                                   # off is always accepted
    r.close()
    # accepted and without effect: MIS off, and a scene without lights
    dark = mirt.scene.default9()
    dark.material["emission"] = 0
    dark.ambient[:] = 0.5
    assert len(mirt.light_list(dark.geometry, dark.material)) == 0
    for sc, kw in ((mirt.scene.default9(), dict(mis=False)), (dark, {})):
        words = []
        for m in (0, 8):
            q = mirt.Renderer(sc, max_bounces=4, light_ris=m, **kw)
            q.Resize(64, 64); q.Accumulate(5)
            words.append(q.accumulator()); q.close()
        same_words(words[1], words[0], "light_ris without NEE")
