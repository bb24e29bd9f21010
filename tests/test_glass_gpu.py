"""The dielectric interface on the device (mirt_set_transmission; k_shade<..., GLASS = true>, shade_hit_body.inc, device_math.hpp).

There is no oracle for it: the pins are the float64 definitions of tests/glass_definitions.py and exact invariants.
1  mirt_debug_math fn 11 within the error model;  2  no transmissive material: the switch changes no word;  3  an index-matched ball, exact;
4  a furnace, exact, and its dropped share;  5  the refraction image against the reflect / refract tree;  6  an emitter seen through the ball
weighs 1 (the carrier bit);  7  the words do not depend on how the work is cut up;  8  the state rules.
Images are 48 x 32: six tiles and three k_shade chunks, a pixel count that is no power of two, max_batch 3."""
import numpy as np
import pytest

import glass_definitions as gd

pytestmark = pytest.mark.gpu
W, H, FOCAL, EYE_Z = 48, 32, 35.0, 4.0       # the ball of radius 1 about the origin spans about 24 of the 32 rows


def same_words(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape, what
    diff = a.view(np.uint32) != b.view(np.uint32)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} words differ"


def ball_scene(mirt, ior_minus_one, transmission, hdri, ambient=1.0, emitter=None, ball_at=(0.0, 0.0, 0.0)):
    """glass_definitions' scene: one sphere of radius 1 whose opaque lobe is black, a pinhole on the +z axis looking at it, an optional emitter."""
    s = mirt.scene
    mats = [s._material(transmission=transmission, IOR_minus_one=ior_minus_one)]
    geo = [s._sphere(ball_at, 1.0, 0)]
    if emitter is not None:
        mats.append(s._material(emission=emitter[2]))
        geo.append(s._sphere(emitter[0], emitter[1] ** 2, 1))
    return s.Scene(geometry=np.array(geo, dtype=s.SPHERE), material=np.array(mats, dtype=s.MATERIAL),
                   camera=s.Camera(eye=(0.0, 0.0, EYE_Z), direction=(0.0, 0.0, -1.0), focal_length=FOCAL),
                   ambient=np.full(3, ambient, dtype=np.float32), hdri=np.asarray(hdri, dtype=np.float32), name="glass_ball")


def flat_sky(rgb):
    return np.array([[list(rgb) + [1.0]]], dtype=np.float32)


def render(mirt, sc, n_acc, **kw):
    r = mirt.Renderer(sc, **{"max_batch": 3, "use_bvh": True, "transmission": True, **kw})
    r.Resize(W, H)
    r.Accumulate(n_acc)
    acc, ctr = r.accumulator(), r.counters()
    r.close()
    return acc, ctr


def device_index(ior_minus_one):
    return float(np.float32(1.0) + np.float32(ior_minus_one))


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------
def test_fn11_against_the_definition(mirt):
    Vl, n, entering, s1 = gd.fn11_grid()
    r = mirt.Renderer(mirt.scene.default9(), max_bounces=2)
    out = r.debug_math(11, np.stack([Vl[:, 0], Vl[:, 1], Vl[:, 2], n, entering.astype(np.float32), s1]), 6).astype(np.float64)
    r.close()
    want_dir, want_F, want_refl, want_tir = gd.interface(Vl, n, entering, s1)
    model = gd.interface_error_model(Vl, n, entering)
    ties = gd.interface_ties(model, want_F, s1)
    assert ties.mean() <= 0.01
    got_dir, got_F, got_refl, got_tir = out[:3].T, out[3], out[4] != 0, out[5] != 0
    assert set(np.unique(out[4:])) <= {0.0, 1.0}
    ok = ~ties
    assert np.array_equal(got_tir[ok], want_tir[ok]) and np.array_equal(got_refl[ok], want_refl[ok])
    same = (got_tir == want_tir) & (got_refl == want_refl)                          # a tie may fall either way; where it falls the definition's way it is held too
    err_F = np.abs(got_F - want_F)
    print(f"fn 11: {len(Vl)} inputs, {int(ties.sum())} ties, largest F error / bound {np.max(err_F[same & (model['E_F'] > 0)] / model['E_F'][same & (model['E_F'] > 0)]):.3f}")
    assert (err_F[same] <= model["E_F"][same]).all()
    err_d = np.abs(got_dir - want_dir).max(axis=1)
    bound_d = np.where(want_refl, 0.0, model["E_dir"])                              # the mirror direction is exact
    assert (err_d[same] <= bound_d[same]).all(), float(np.max(err_d[same] - bound_d[same]))


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("brdf", [0, 1])
@pytest.mark.parametrize("light_ris", [0, 4])
def test_switch_on_without_a_transmissive_material_changes_nothing(mirt, brdf, light_ris):
    sc = mirt.scene.default9()
    sc.material["transmission"] = 0
    got = {}
    for on in (False, True):
        r = mirt.Renderer(sc, max_bounces=8, buckets=5, use_bvh=True, max_batch=3, brdf=brdf, gloss_decay=[0.0, 0.3, 0.6], light_ris=light_ris, aov=True, transmission=on)
        assert r.transmission() == on
        r.Resize(W, H); r.Accumulate(10)
        assert r.Render()
        got[on] = (r.accumulator(), r.GetFrame().copy(), r.aov(), r.counters())
        r.close()
    for k, what in enumerate(("accumulator", "frame", "AOVs")):
        same_words(got[True][k], got[False][k], what)
    assert got[True][3] == got[False][3]


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------
def test_index_matched_ball_is_exact(mirt):
    sky, n_acc = (0.75, 0.5, 0.25), 6
    acc, ctr = render(mirt, ball_scene(mirt, 0.0, (0.5, 1.0, 0.25), flat_sky(sky)), n_acc, max_bounces=4, buckets=1)
    assert ctr["shadow_rays"] == 0 and ctr["dropped"] == 0
    px = gd.acc_pixels(acc, W)[0]                                                  # (H, W, 3) sums of six samples
    # a sample that meets the ball carries 0.5f * sky in ALL channels (Q10: the miss shader scales by throughput.r, and 0.5 / 1 is the tint's r);
    # any other sample carries sky: every word is (12 - k) * 0.5 * sky, k of the six samples on the ball - exact in binary32 for this sky
    k = 2.0 * n_acc - px / (0.5 * np.asarray(sky))
    assert np.array_equal(k, np.round(k)) and k.min() == 0 and k.max() == n_acc
    assert np.array_equal(k[..., 0], k[..., 1]) and np.array_equal(k[..., 0], k[..., 2])
    O, D, pix = gd.camera_rays(W, H, FOCAL, EYE_Z, sub=8)
    hit = np.isfinite(gd._hit_sphere(O, D, np.zeros(3), 1.0)).reshape(W, H, 64).transpose(1, 0, 2)
    assert (k[..., 0][hit.all(axis=2)] == n_acc).all() and (k[..., 0][~hit.any(axis=2)] == 0).all() and hit.all(axis=2).sum() > 300
    # a clear ball is no ball
    clear, _ = render(mirt, ball_scene(mirt, 0.0, (1.0, 1.0, 1.0), flat_sky(sky)), n_acc, max_bounces=4, buckets=1)
    empty, _ = render(mirt, ball_scene(mirt, 0.0, (1.0, 1.0, 1.0), flat_sky(sky), ball_at=(0.0, 0.0, 40.0)), n_acc, max_bounces=4, buckets=1)
    same_words(clear, empty, "index-matched, transmission 1: the scene whose ball no ray meets")
    assert (empty == np.float32(n_acc) * np.asarray(sky, dtype=np.float32)[None, None, :, None]).all()


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb,n_acc", [(4, 192), (8, 960)])
def test_furnace_is_exact_and_drops_what_the_tree_drops(mirt, mb, n_acc):
    """Nothing is absorbed: every word is a multiple of the sky, and the multiples missing are the dropped paths (Q5), one for one.  Their
    number is compared with the tree's tail at five binomial standard errors, at two depths: max_bounces 4 (two reflections inside; about 1046
    dropped paths expected) and 8 (six reflections of paths that entered within about 5e-4 of the silhouette; about 189 expected at 960
    accumulations - a count at which a gap of a few tens of percent shows).  The deep tail is what found the tangent frame: routed through
    to_local / to_world (ill-conditioned near N.z = -1, the normals a ball seen from inside turns to the camera) the interface stretched some
    directions, which then met the ball again from outside or reflected totally, and 621 paths were dropped in 1920 accumulations where the tree
    expects 378; dielectric_interface therefore works on world-space vectors."""
    sky = (0.5, 0.25, 1.0)
    acc, ctr = render(mirt, ball_scene(mirt, 0.5, (1.0, 1.0, 1.0), flat_sky(sky)), n_acc, max_bounces=mb, buckets=1)
    px = gd.acc_pixels(acc, W)[0]
    k = px / np.asarray(sky)
    assert np.array_equal(k, np.round(k)) and k.max() == n_acc and k.min() >= 0     # nothing is absorbed, nothing is gained
    assert np.array_equal(k[..., 0], k[..., 1]) and np.array_equal(k[..., 0], k[..., 2])
    missing = int((n_acc - k[..., 0]).sum())
    assert missing == ctr["dropped"] and ctr["shadow_rays"] == 0
    # the tree's tail (Q5): the probability that a path is still alive after bounce mb - 1, over the sub-pixel positions
    _, p_drop, _, _ = gd.pixel_expectation(W, H, FOCAL, EYE_Z, 1.5, (1, 1, 1), mb, ((np.ones(3),) * 2,) * 2, sub=16)
    want = n_acc * p_drop.sum()
    sigma = np.sqrt(n_acc * (p_drop * (1 - p_drop)).sum())                          # a sum of Bernoulli draws: at most the binomial's variance pixel by pixel
    print(f"furnace: dropped {missing}, the tree's tail {want:.1f}, sigma {sigma:.2f}, share {missing / (n_acc * W * H):.2e}")
    assert want > 25, "the tail is too thin to be compared"
    assert abs(missing - want) <= 5 * sigma


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------
SKY4 = (((0.9, 0.6, 0.3), (0.2, 0.5, 0.1)), ((0.1, 0.3, 0.8), (0.6, 0.1, 0.4)))      # (row: y > 0, y <= 0) x (column: z < 0, z >= 0)
IMAGE_CASES = {"glass 1.44": (0.44, (0.95, 0.95, 0.95)), "tinted 1.762": (0.762, (0.670, 0.764, 0.855))}
SUB, BLOCK, BUCKETS, PER_BUCKET = 8, 2, 16, 12


@pytest.mark.parametrize("name", list(IMAGE_CASES))
def test_refraction_image_against_the_tree(mirt, name):
    """Region means over 2 x 2 pixel blocks that the definition picks: every sub-pixel position on the ball; the leaves within 0.02 of a texel border
    (the planes y = 0 and z = 0: the middle rows of the image, and the deep end of the in-ball chain) weigh less than 1e-3 of the sky's spread; the
    radiance varies by less than 0.02 inside a pixel, so no jump crosses it and the 8 x 8 midpoint mean is good to second order (under 1e-4); at most
    12 blocks spread over the ball.  Bound: five standard errors from the 16 buckets' own spread, plus the border leaves' weight (slack)."""
    iom, tint = IMAGE_CASES[name]
    mb, n_acc = 8, BUCKETS * PER_BUCKET
    sc = ball_scene(mirt, iom, tint, gd.quadrant_sky(SKY4))
    want, _, slack, spread = gd.pixel_expectation(W, H, FOCAL, EYE_Z, device_index(iom), np.asarray(tint, dtype=np.float32).astype(np.float64), mb, SKY4, sub=SUB)
    O, D, _ = gd.camera_rays(W, H, FOCAL, EYE_Z, sub=SUB)
    on_ball = np.isfinite(gd._hit_sphere(O, D, np.zeros(3), 1.0)).reshape(W, H, SUB * SUB).transpose(1, 0, 2).all(axis=2)
    blocks = [(y, x) for y in range(0, H, BLOCK) for x in range(0, W, BLOCK)
              if on_ball[y:y + BLOCK, x:x + BLOCK].all() and slack[y:y + BLOCK, x:x + BLOCK].max() < 1e-3 and spread[y:y + BLOCK, x:x + BLOCK].max() < 0.02]
    assert len(blocks) >= 6, blocks
    blocks = blocks[::max(1, len(blocks) // 12)][:12]
    acc, _ = render(mirt, sc, n_acc, max_bounces=mb, buckets=BUCKETS)
    px = gd.acc_pixels(acc, W) / PER_BUCKET                                         # (bucket, H, W, 3) means
    widths = []
    for y, x in blocks:
        got = px[:, y:y + BLOCK, x:x + BLOCK].mean(axis=(1, 2))                      # (bucket, 3)
        mean, se = got.mean(axis=0), got.std(axis=0, ddof=1) / np.sqrt(BUCKETS)
        bound = 5 * se + slack[y:y + BLOCK, x:x + BLOCK].max(axis=(0, 1))
        exp = want[y:y + BLOCK, x:x + BLOCK].mean(axis=(0, 1))
        widths.append(bound.max() / exp.max())
        assert (np.abs(mean - exp) <= bound).all(), (name, (y, x), mean, exp, bound)
        assert bound.max() < 0.25 * exp.max(), (name, (y, x), bound, exp)              # the bound is a small part of the block's colour
    print(f"{name}: {len(blocks)} blocks, largest relative half-width {max(widths):.4f}, joint (root mean square) {np.sqrt(np.mean(np.square(widths))):.4f}")


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------
def test_an_emitter_seen_through_the_ball_weighs_one(mirt):
    emitter = (np.array([0.0, 0.0, -3.0]), 0.3, np.array([8.0, 6.0, 4.0]))           # hidden behind the ball from every camera ray: seen through it only
    mb, buckets, per = 8, 16, 6
    sc = ball_scene(mirt, 0.5, (1.0, 1.0, 1.0), flat_sky((0, 0, 0)), ambient=0.0, emitter=emitter)
    assert len(mirt.light_list(sc.geometry, sc.material)) == 1
    sub = 16
    args = (W, H, FOCAL, EYE_Z, 1.5, (1, 1, 1), mb, None)
    want, _, _, spread = gd.pixel_expectation(*args, emitter=emitter, carrier=True, sub=sub)
    blind, _, _, _ = gd.pixel_expectation(*args, emitter=emitter, carrier=False, sub=sub)
    O, D, _ = gd.camera_rays(W, H, FOCAL, EYE_Z, sub=4)
    ball = np.isfinite(gd._hit_sphere(O, D, np.zeros(3), 1.0)).reshape(W, H, 16).transpose(1, 0, 2).all(axis=2)
    assert not want[~np.isfinite(gd._hit_sphere(O, D, np.zeros(3), 1.0)).reshape(W, H, 16).transpose(1, 0, 2).any(axis=2)].any()      # no camera ray sees it directly
    acc, ctr = render(mirt, sc, buckets * per, max_bounces=mb, buckets=buckets, mis=True)
    got = (gd.acc_pixels(acc, W) / per)[:, ball].mean(axis=1)                        # (bucket, 3)
    mean, se = got.mean(axis=0), got.std(axis=0, ddof=1) / np.sqrt(buckets)
    reach = spread[ball].mean(axis=0) * 2.0 / sub                                    # the emitter's rim crosses pixels: a jump touches at most 2 / sub of a pixel's cells
    bound = 5 * se + reach
    print(f"emitter through glass: device {mean}, definition {want[ball].mean(axis=0)}, without the carrier bit {blind[ball].mean(axis=0)}, bound {bound}")
    assert (np.abs(mean - want[ball].mean(axis=0)) <= bound).all()
    assert (np.abs(want[ball].mean(axis=0) - blind[ball].mean(axis=0)) > 2 * bound).all()      # the test tells the two weights apart


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------
def test_words_do_not_depend_on_the_route(mirt):
    sc, n, mb = mirt.scene.default9(), 6, 8
    assert (sc.material["transmission"].max(axis=1) > 0).sum() == 2                  # its two glass materials, as authored

    def run(n_acc=n, setup=None, accumulate=None, **kw):
        r = mirt.Renderer(sc, max_bounces=mb, buckets=3, **{"transmission": True, "use_bvh": True, "max_batch": 3, **kw})
        r.Resize(W, H)
        if setup:
            setup(r)
        (accumulate or (lambda q: q.Accumulate(n_acc)))(r)
        acc = r.accumulator()
        r.close()
        return acc

    base = run()
    assert (base.view(np.uint32) != run(transmission=False).view(np.uint32)).any()  # the switch does something here
    routes = {
        "max_batch 1": dict(max_batch=1), "max_batch 6": dict(max_batch=6), "streams 1": dict(streams=1), "streams 3": dict(streams=3),
        "traced camera rays": dict(trace_primary_rays=True), "tree built on the device": dict(gpu_build=True), "the reference's tree": dict(reference_tree=True),
        "brute force": dict(use_bvh=False), "AOVs on": dict(aov=True),
        "6 x async(1)": dict(accumulate=lambda r: [r.AccumulateAsync(1) for _ in range(n)]),
        "set after construction": dict(transmission=False, setup=lambda r: r.set_transmission(True)),
    }
    for label, kw in routes.items():
        same_words(run(**kw), base, label)
    h_tiles, v_tiles = W // 16, H // 16
    merged = np.zeros((v_tiles, h_tiles) + base.shape[1:], dtype=np.float32)
    for rank in range(2):
        merged[rank::2] = run(setup=lambda q: q.SetTileRows(rank, 2)).reshape((-1, h_tiles) + base.shape[1:])
    same_words(merged.reshape(base.shape), base, "two contexts with interleaved tile rows")
    g = mirt.GroupRenderer(sc, devices=[0, 0], max_bounces=mb, buckets=3, use_bvh=True, max_batch=3, transmission=True)
    assert g.transmission() is True
    g.Resize(W, H); g.Accumulate(n)
    same_words(g.accumulator(), base, "a group of the same device twice")
    g.close()
    mask = np.arange(h_tiles * v_tiles) % 3 == 0

    def freeze(q):
        q.Accumulate(3); q.freeze_tiles(mask); q.Accumulate(3)
    got, three = run(accumulate=freeze), run(n_acc=3)
    same_words(got[~mask], base[~mask], "active tiles beside frozen ones")
    same_words(got[mask], three[mask], "frozen tiles keep the words of their count")
    # a lens and the GGX closure combine with it: the same words by tree and by brute force
    for kw in (dict(setup=lambda q: q.set_lens(0.05, 4.0)), dict(brdf=1, gloss_decay=[0.0, 0.3, 0.6]), dict(light_ris=4)):
        same_words(run(**kw), run(use_bvh=False, **kw), f"tree against brute force, {sorted(kw)}")


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------
def test_state_rules(mirt):
    lib = mirt.load_library()
    sc = mirt.scene.default9()
    r = mirt.Renderer(sc, max_bounces=4, buckets=1)
    assert r.transmission() is False
    assert lib.mirt_set_transmission(r._ctx, 2) == -1 and r.transmission() is False  # MIRT_ERR_ARG
    r.Resize(W, H); r.Accumulate(2)
    before = r.accumulator()
    r.set_transmission(True)
    assert r.transmission() is True and r.accumulations == 2
    same_words(r.accumulator(), before, "the switch does not reset the accumulator")
    assert lib.mirt_set_stream_order(r._ctx, 1) == -3 and r.stream_order == 0        # MIRT_ERR_STATE
    with pytest.raises(mirt.MirtError, match="mirt_set_transmission"):
        r.set_stream_order(True)
    r.set_transmission(False); r.set_stream_order(True)
    assert lib.mirt_set_transmission(r._ctx, 1) == -3 and r.transmission() is False
    with pytest.raises(mirt.MirtError, match="mirt_set_stream_order"):
        r.set_transmission(True)
    r.set_transmission(False)                                                        # off is always accepted
    r.set_stream_order(False)
    # a transmissive material needs a finite index above 0; the components lie in [0, 1]
    for field, value in (("IOR_minus_one", -1.0), ("IOR_minus_one", -2.5), ("IOR_minus_one", np.nan), ("IOR_minus_one", np.inf), ("transmission", 1.5), ("transmission", -0.1), ("transmission", np.nan)):
        bad = mirt.scene.default9()
        glass = int(np.argmax(bad.material["transmission"].max(axis=1)))
        bad.material[field][glass] = value
        q = mirt.Renderer(bad, max_bounces=4)                                        # off: nothing reads the fields, nothing is asked of them
        assert lib.mirt_set_transmission(q._ctx, 1) == -1 and q.transmission() is False
        with pytest.raises(mirt.MirtError, match=field if field == "transmission" else "IOR_minus_one"):
            q.set_transmission(True)
        q.scene = sc; q.UpdateScene(); q.set_transmission(True)
        q.scene = bad
        with pytest.raises(mirt.MirtError):
            q.UpdateScene()                                                          # mirt_set_scene with the switch on
        q.close()
    # an opaque material may carry any index
    odd = mirt.scene.default9()
    odd.material["IOR_minus_one"][0] = -3.0
    assert odd.material["transmission"][0].max() == 0
    q = mirt.Renderer(odd, max_bounces=4, transmission=True)
    q.close()
    r.close()
