"""The temporal history of the denoised resolve on the GPU (mirt_render_temporal / mirt_group_render_temporal; csrc/temporal.hpp k_reproject)
against the binary32 numpy twin of temporal_twin.py, which restates THE DEFINITION of include/mirt.h operation for operation: frames, history
lengths and class counts are compared on their raw words over sequences of render, move, reset, render.  Then what the definition promises: a
call that takes no history is mirt_render_atrous, the identity map leaves x alone, update = 0 leaves the history alone, the lifetime and error
tables, a group's words — and what it buys over an orbit (figures printed, asserted only as `<`; profiles/temporal.txt records them)."""
import ctypes as C

import numpy as np
import pytest

import denoise_twin as dt
import temporal_twin as tt
from oracle_binding import bits

pytestmark = pytest.mark.gpu

f32 = np.float32
MIRT_OK, MIRT_NOT_READY, MIRT_ERR_ARG, MIRT_ERR_STATE = 0, 1, -1, -3
SENTINEL = f32(-7.0)


def assert_same(got, want, what):
    got, want = bits(np.asarray(got, dtype=f32)), bits(np.asarray(want, dtype=f32))
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    bad = got != want
    n = int(bad.sum())
    where = np.argwhere(bad)[:4].tolist() if n else []
    assert n == 0, f"{what}: {n} of {got.size} words differ, first at {where}: got {[hex(int(got[tuple(i)])) for i in where]}, want {[hex(int(want[tuple(i)])) for i in where]}"


# ---- camera moves ------------------------------------------------------------------------------------------------------------------------------
def quat_mul(a, b):
    ax, ay, az, aw = [float(v) for v in a]
    bx, by, bz, bw = [float(v) for v in b]
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def yaw(r, degrees):
    """Turns the camera about the world's +y through its own position."""
    h = np.radians(degrees) / 2.0
    q = quat_mul([0.0, np.sin(h), 0.0, np.cos(h)], r.scene.camera.orient)
    r.scene.camera.orient = (q / np.linalg.norm(q)).astype(f32)
    r.UpdateCamera()


def strafe(r, dx, dy=0.0, dz=0.0):
    r.scene.camera.pos = (np.asarray(r.scene.camera.pos, dtype=np.float64) + [dx, dy, dz]).astype(f32)
    r.UpdateCamera()


def twin_camera(r):
    c = r.scene.camera
    return tt.camera(c.pos, c.orient, c.half_width, c.half_height, c.z, c.exposure)


def scene_of(mirt, name):
    return mirt.scene.default9() if name == "default9" else mirt.scene.synthetic(1000)


def make(mirt, name, w, h, k, **kw):
    r = mirt.Renderer(scene_of(mirt, name), buckets=k, max_bounces=4, aov=True, **{"use_bvh": True, **kw})
    r.Resize(w, h)
    return r


def next_frame(r, k):
    r.ResetAccumulator()
    r.Accumulate(k)


def slabs(r):
    return r.accumulator().copy(), r.aov().copy(), r.tile_counts().copy()


MOVES = (None, lambda r: yaw(r, 2.0), lambda r: strafe(r, 0.05, 0.01))       # frame 1; a yaw, then frame 2; a strafe, then frame 3
CASES = [("default9", 64, 48, 5), ("default9", 32, 32, 2), ("S1000", 32, 32, 5), ("S1000", 64, 48, 2)]


# ---- (a) no history: the à-trous resolve ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h,k", CASES[:2])
def test_without_history_it_is_the_atrous_resolve(mirt, name, w, h, k):
    r = make(mirt, name, w, h, k)
    r.Accumulate(k)
    assert r.Render()
    plain = r.GetFrame().copy()
    want = r.render_denoised(iterations=3)
    frame, length, st = r.render_temporal(iterations=3, update=0, want_len=True, want_stats=True)
    assert_same(frame, want, "no history yet")
    assert st["reprojected"] == st["outside"] == st["rejected"] == 0 and st["no_history"] + st["unusable"] == w * h
    assert set(np.unique(length)) <= {0.0, float(k)}
    assert r.history_info() == {"valid": False, "bytes": 0}
    assert r.render_temporal(iterations=3) is not None and r.history_info()["valid"]
    assert r.history_info()["bytes"] == w * h * 36
    assert_same(r.render_temporal(iterations=3, max_ratio=0.0, update=0), want, "max_ratio = 0 takes no history")
    assert_same(r.render_temporal(iterations=0, demodulate=0, max_ratio=0.0, update=0), plain, "... and iterations = 0, demodulate = 0 is Render()")
    assert not np.array_equal(bits(r.render_temporal(iterations=3, update=0)), bits(want)), "a history that is taken changes the frame (v at least)"
    r.scene.camera.exposure = 2.0                                                 # x is in exposure-scaled units: a history of another exposure is not taken
    r.UpdateCamera()
    brighter, st = r.render_temporal(iterations=3, update=0, want_stats=True)
    assert_same(brighter, r.render_denoised(iterations=3), "another exposure: the history is ignored for the call")
    assert st["reprojected"] == 0 and r.history_info()["valid"]
    r.scene.camera.exposure = 1.0
    r.UpdateCamera()
    r.drop_history()
    assert r.history_info() == {"valid": False, "bytes": 0}
    assert_same(r.render_temporal(iterations=3, update=0), want, "after drop_history")
    assert_same(r.render_temporal(iterations=0, demodulate=0, update=0), plain, "iterations = 0, demodulate = 0, no history: Render()")
    r.close()


# ---- (b) the twin, over render / move / reset / render -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h,k", CASES)
def test_sequence_equals_the_twin_rendered_and_loaded(mirt, name, w, h, k):
    params = {"iterations": 2}
    a = make(mirt, name, w, h, k, max_batch=1, streams=1)
    b = make(mirt, name, w, h, k, max_batch=8, streams=3, use_bvh=(name != "default9"))      # loads a's slabs: the words depend on the slabs alone
    hist = None
    seen = {n: 0 for n in tt.CLASSES}
    for i, move in enumerate(MOVES):
        if move is not None:
            move(a); move(b)
        next_frame(a, k)
        acc, aov, counts = slabs(a)
        b.load_accumulator(acc, k); b.load_aov(aov); b.load_tile_counts(counts)
        want_frame, want_len, want_st, hist = tt.render(acc, aov, counts, 1.0, params, {}, w, h, twin_camera(a), hist)
        for who, r in (("rendered", a), ("loaded", b)):
            frame, length, st = r.render_temporal(want_len=True, want_stats=True, **params)
            print(f"[temporal] {name} {w}x{h} k={k} frame {i + 1} ({who}): {st}")
            assert st == want_st, f"frame {i + 1} ({who}): class counts"
            assert_same(length, want_len, f"frame {i + 1} ({who}): history_len")
            assert_same(frame, want_frame, f"frame {i + 1} ({who}): frame")
        assert sum(want_st.values()) == w * h
        for n in tt.CLASSES:
            seen[n] += want_st[n]
    assert seen["reprojected"] > w * h // 4 and seen["rejected"] > 0 and seen["outside"] > 0 and seen["no_history"] > 0, f"the sequence meets the classes: {seen}"
    a.close(); b.close()


# ---- (c) identical camera, identical slabs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h,k", CASES[:2])
def test_identity_leaves_x_alone_and_adds_lengths(mirt, name, w, h, k):
    r = make(mirt, name, w, h, k)
    r.Accumulate(k)
    acc, aov, counts = slabs(r)
    unfiltered = r.render_denoised(iterations=0)
    st0 = dt.prepare(acc, aov, counts, 1.0, dict(dt.DEFAULTS), w, h)
    follows = st0["usable"] & ~((st0["N"][0] == 0) & (st0["N"][1] == 0) & (st0["N"][2] == 0))       # the pixels step 2 applies to
    assert follows.sum() > w * h // 4
    n = f32(k)
    f1, l1 = r.render_temporal(iterations=0, want_len=True)
    assert_same(f1, unfiltered, "first call")
    assert_same(l1, np.where(st0["usable"], n, f32(0)), "first call: len = n")
    f2, l2, s2 = r.render_temporal(iterations=0, max_ratio=0.5, want_len=True, want_stats=True)       # hn = n, capped at n / 2
    assert_same(f2, unfiltered, "identity, max_ratio 0.5: x unchanged, so the unfiltered frame")
    assert s2["reprojected"] == int(follows.sum()) and s2["rejected"] == s2["outside"] == 0
    assert_same(l2, np.where(follows, n + f32(0.5) * n, np.where(st0["usable"], n, f32(0))), "len = n + min(hn, max_ratio n)")
    f3, l3 = r.render_temporal(iterations=0, want_len=True)                                             # hn = 1.5 n, max_ratio 7
    assert_same(f3, unfiltered, "identity again")
    assert_same(l3, np.where(follows, n + (n + f32(0.5) * n), np.where(st0["usable"], n, f32(0))), "len = n + hn")
    r.close()


# ---- (d) update = 0 --------------------------------------------------------------------------------------------------------------------------------
def test_update_zero_leaves_history_and_state_alone(mirt):
    name, w, h, k = CASES[0]
    a, b = make(mirt, name, w, h, k), make(mirt, name, w, h, k)
    for r in (a, b):
        r.Accumulate(k)
        assert r.render_temporal(iterations=1) is not None
        yaw(r, 1.5)
        next_frame(r, k)
    assert a.Render()
    before = (a.accumulator().copy(), a.aov().copy(), a.counters(), a.GetFrame().copy(), a.accumulations, a.tile_counts().copy(), a.history_info())
    peek = a.render_temporal(iterations=1, update=0, want_len=True)
    assert a.render_temporal(iterations=4, update=0, depth_tol=0.5) is not None
    assert a.Render()
    after = (a.accumulator(), a.aov(), a.counters(), a.GetFrame(), a.accumulations, a.tile_counts(), a.history_info())
    assert_same(after[0], before[0], "accumulator")
    assert_same(after[1], before[1], "AOV slab")
    assert after[2] == before[2] and after[4] == before[4] and np.array_equal(after[5], before[5]) and after[6] == before[6]
    assert_same(after[3], before[3], "Render() afterwards")
    got, want = a.render_temporal(iterations=1, want_len=True), b.render_temporal(iterations=1, want_len=True)
    assert_same(got[0], want[0], "frame after two update = 0 calls against a context that never made them")
    assert_same(got[1], want[1], "history_len likewise")
    assert_same(peek[0], want[0], "... and the update = 0 call itself saw that frame")
    for r in (a, b):
        strafe(r, 0.03)
        next_frame(r, k)
    assert_same(a.render_temporal(iterations=1), b.render_temporal(iterations=1), "one frame later")
    a.close(); b.close()


# ---- (e) lifetime, errors, groups ------------------------------------------------------------------------------------------------------------------
def test_history_lifetime(mirt):
    name, w, h, k = CASES[1]
    r = make(mirt, name, w, h, k)

    def establish():
        next_frame(r, r.policy.buckets)
        assert r.render_temporal(iterations=0) is not None and r.history_info()["valid"]

    establish()
    keeps = (("Reset", r.ResetAccumulator), ("camera", lambda: yaw(r, 1.0)), ("lens", lambda: r.set_lens(0.01, 1.0)), ("lens off", lambda: r.set_lens(0.0, 1.0)),
             ("light RIS", lambda: r.set_light_ris(4)), ("sky sampling", lambda: r.set_sky_sampling(True)), ("transmission", lambda: r.set_transmission(True)),
             ("gloss decay", lambda: r.set_gloss_decay([0.5])), ("max_bounces", lambda: r.set_policy(max_bounces=3)))
    for what, call in keeps:
        call()
        assert r.history_info()["valid"], f"{what} keeps the history"
    drops = (("drop_history", r.drop_history), ("set_scene", r.UpdateScene), ("resize", lambda: r.Resize(w, h)), ("tile range", lambda: r.SetTileRange(0, (w // 16) * (h // 16))),
             ("tile rows", lambda: r.SetTileRows(0, 1)), ("buckets", lambda: r.set_policy(buckets=k + 1)), ("buckets back", lambda: r.set_policy(buckets=k)))
    for what, call in drops:
        if not r.history_info()["valid"]:
            establish()
        call()
        assert r.history_info() == {"valid": False, "bytes": 0}, f"{what} drops the history"
    r.close()


def raw_call(mirt, r, buf, dparams=None, **tparams):
    d = mirt.denoise_defaults()
    d.update(dparams or {})
    p = mirt.DenoiseParams(*(d[n] for n, _ in mirt.DenoiseParams._fields_))
    t = mirt.temporal_defaults()
    t.update(tparams)
    tp = mirt.TemporalParams(*(t[n] for n, _ in mirt.TemporalParams._fields_))
    return r._lib.mirt_render_temporal(r._ctx, C.byref(p), C.byref(tp), buf.ctypes.data_as(C.c_void_p), None, None)


def test_refusals(mirt):
    sc = mirt.scene.default9()
    buf = np.full((32, 48, 4), SENTINEL, dtype=f32)

    r = mirt.Renderer(sc, buckets=5)                                             # AOVs off
    r.Resize(48, 32); r.Accumulate(5)
    assert raw_call(mirt, r, buf) == MIRT_ERR_STATE and b"AOVs are off" in r._lib.mirt_last_error(r._ctx)
    with pytest.raises(mirt.MirtError):
        r.render_temporal()
    r.close()

    r = mirt.Renderer(sc, buckets=1, aov=True)
    r.Resize(48, 32); r.Accumulate(2)
    assert raw_call(mirt, r, buf) == MIRT_ERR_STATE and b"buckets >= 2" in r._lib.mirt_last_error(r._ctx)
    r.close()

    r = mirt.Renderer(sc, buckets=5, exact_stream_order=True)                    # exact stream order has no AOVs
    r.Resize(48, 32); r.Accumulate(5)
    assert raw_call(mirt, r, buf) == MIRT_ERR_STATE
    r.close()

    r = mirt.Renderer(sc, buckets=5, aov=True)
    r.Resize(48, 32)
    r.SetTileRange(0, 3); r.Accumulate(5)
    assert raw_call(mirt, r, buf) == MIRT_ERR_STATE and b"owns 3 of the image's 6 tiles" in r._lib.mirt_last_error(r._ctx)
    r.SetTileRows(1, 2); r.Accumulate(5)
    assert raw_call(mirt, r, buf) == MIRT_ERR_STATE
    r.SetTileRange(0, 6); r.Accumulate(5)
    assert raw_call(mirt, r, buf) == MIRT_OK and r.history_info()["valid"]
    held = r.render_temporal(update=0, want_len=True)
    r.Accumulate(2)                                                               # 7 is not a multiple of 5
    assert raw_call(mirt, r, np.full_like(buf, SENTINEL)) == MIRT_NOT_READY and r.render_temporal(out=buf.copy()) is None
    r.Accumulate(3)
    buf[:] = SENTINEL
    for bad in ({"max_ratio": -1.0}, {"max_ratio": float("nan")}, {"max_ratio": float("inf")}, {"depth_tol": -0.1}, {"depth_tol": float("nan")}, {"normal_min": 1.5},
                {"normal_min": -1.5}, {"normal_min": float("nan")}, {"update": 2}):
        assert raw_call(mirt, r, buf, **bad) == MIRT_ERR_ARG, bad
    for bad in ({"iterations": 9}, {"lum_floor": 0.0}, {"sigma_lum": -1.0}, {"albedo_floor": float("nan")}):
        assert raw_call(mirt, r, buf, dparams=bad) == MIRT_ERR_ARG, bad
    p, tp = mirt.DenoiseParams(*mirt.denoise_defaults().values()), mirt.TemporalParams(*mirt.temporal_defaults().values())
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert r._lib.mirt_render_temporal(r._ctx, None, C.byref(tp), ptr, None, None) == MIRT_ERR_ARG
    assert r._lib.mirt_render_temporal(r._ctx, C.byref(p), None, ptr, None, None) == MIRT_ERR_ARG
    assert r._lib.mirt_render_temporal(r._ctx, C.byref(p), C.byref(tp), None, None, None) == MIRT_ERR_ARG
    assert r._lib.mirt_render_temporal(None, C.byref(p), C.byref(tp), ptr, None, None) == MIRT_ERR_ARG
    assert (buf == SENTINEL).all(), "no refusal wrote a word"
    with pytest.raises(TypeError):
        r.render_temporal(ratio=1.0)
    # none of these touched the history: over the slabs it was taken from, the same words as before them
    r.ResetAccumulator(); r.Accumulate(5)
    again = r.render_temporal(update=0, want_len=True)
    assert_same(again[0], held[0], "the history survived every refusal")
    assert_same(again[1], held[1], "history_len likewise")
    r.close()


@pytest.mark.parametrize("members", [2, 3, 4])
def test_group_gives_the_single_context_words(mirt, members):
    name, w, h, k = "S1000", 64, 48, 5
    single = make(mirt, name, w, h, k)
    g = mirt.GroupRenderer(scene_of(mirt, name), devices=[0] * members, buckets=k, max_bounces=4, use_bvh=True, aov=True)
    g.Resize(w, h)
    buf = np.full((h, w, 4), SENTINEL, dtype=f32)
    assert g.render_temporal(out=buf) is None and (buf == SENTINEL).all() and not g.history_info()["valid"]
    for i, move in enumerate(MOVES):
        for r in (single, g):
            if move is not None:
                move(r)
            next_frame(r, k)
        got, want = g.render_temporal(want_len=True, want_stats=True, iterations=2), single.render_temporal(want_len=True, want_stats=True, iterations=2)
        assert got[2] == want[2]
        assert_same(got[1], want[1], f"group of {members}, frame {i + 1}: history_len")
        assert_same(got[0], want[0], f"group of {members}, frame {i + 1}: frame")
    assert g.history_info() == single.history_info() and g.history_info()["valid"]
    g.drop_history()
    assert not g.history_info()["valid"]
    g.close(); single.close()


# ---- (f) what it buys ------------------------------------------------------------------------------------------------------------------------------
def test_orbit_beats_the_single_frame(mirt):
    """An 8-frame orbit of default9 at 96 x 64, 0.5 degrees a frame about the point the camera looks at, one sample per bucket and frame,
    iterations = 0.  The pre-tonemap values x * m of the last call come from the twin, which this test first holds to the kernel's frame and
    lengths word for word; the converged frame is the plain resolve of the last view."""
    w, h, k, frames, n_ref = 96, 64, 5, 8, 2000
    r = make(mirt, "default9", w, h, k)
    cam = r.scene.camera
    fwd = tt.rotate([f32(v) for v in cam.orient[:3]], f32(cam.orient[3]), [f32(0), f32(0), f32(-1)])
    centre = np.asarray(cam.pos, dtype=np.float64) + 1.2 * np.array([float(v) for v in fwd])
    hist, params = None, {"iterations": 0}
    for i in range(frames):
        if i:
            a = np.radians(0.5)
            d = np.asarray(cam.pos, dtype=np.float64) - centre
            cam.pos = (centre + [np.cos(a) * d[0] + np.sin(a) * d[2], d[1], np.cos(a) * d[2] - np.sin(a) * d[0]]).astype(f32)
            yaw(r, 0.5)
        next_frame(r, k)
        acc, aov, counts = slabs(r)
        dp = dict(dt.DEFAULTS, **params)
        st = dt.prepare(acc, aov, counts, 1.0, dp, w, h)
        n_img = np.full((h, w), f32(k))
        st["x"], st["v"], want_len, cls = tt.reproject_blend(st, n_img, twin_camera(r), hist, dp, dict(tt.DEFAULTS))
        hist = {"x": st["x"], "v": st["v"], "N": st["N"], "z": st["z"], "usable": st["usable"], "n": want_len, "cam": twin_camera(r), "demodulate": 1,
                "albedo_floor": f32(dp["albedo_floor"]), "shape": (h, w)}
        frame, length = r.render_temporal(want_len=True, **params)
        assert_same(length, want_len, f"orbit frame {i + 1}: history_len")
        assert_same(frame, dt.finish(st, w, h), f"orbit frame {i + 1}: frame")
    temporal = np.stack([np.where(st["usable"], st["x"][c] * st["m"][c], st["s"][c]) for c in range(3)], axis=-1).astype(np.float64)
    single = np.stack([dt.to_image(c, w, h) for c in dt.signal(acc, counts, 1.0)], axis=-1).astype(np.float64)
    noise_single = r.noise_quantile(r.noise()["hist"], 0.5)
    r.ResetAccumulator()
    r.Accumulate(n_ref)
    noise_ref = r.noise_quantile(r.noise()["hist"], 0.5)
    reference = np.stack([dt.to_image(c, w, h) for c in dt.signal(r.accumulator(), r.tile_counts(), 1.0)], axis=-1).astype(np.float64)
    assert noise_ref < 0.25 * noise_single, f"the reference's bucket noise (median {noise_ref}) is well below the single frame's ({noise_single})"
    long = want_len >= f32(4 * k)
    assert long.sum() > w * h // 4, f"{int(long.sum())} pixels hold a history of 4 n or more"
    rm = lambda img: float(np.sqrt(np.mean((img[long] - reference[long]) ** 2)))
    e_t, e_s = rm(temporal), rm(single)
    print(f"[temporal] orbit: {int(long.sum())} of {w * h} pixels with history_len >= 4 n; pre-tonemap RMSE to the {n_ref}-accumulation frame: "
          f"single frame {e_s:.5f}, temporal {e_t:.5f}, ratio {e_t / e_s:.3f}; bucket-noise medians: single {noise_single:.4f}, reference {noise_ref:.4f}")
    assert e_t < e_s
    r.close()
