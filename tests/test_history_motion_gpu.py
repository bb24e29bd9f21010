"""The first-hit id map (mirt_id_map; csrc/id_map.hpp k_id_map) and the temporal history kept across sphere moves (mirt_set_sphere_motion;
csrc/temporal.hpp k_reproject<true>) on the GPU.  The id map against the single-ray paths the library already has; the motion-aware reprojection
against the binary32 twin of temporal_motion_twin.py word for word (frame, history_len, the five class counts), which takes the device's id map
and the two sphere tables as inputs; then what the definition promises about the pixels of a moved sphere and of the ground it uncovers, the
switch's lifetime table, a group and the headless tool.

The ray of a pixel centre: mirt_debug_raygen draws its camera samples from the accumulation's hash and takes none from the caller, so the ray of
samples (0.5, 0.5) is temporal_twin.camera_ray_dir, the binary32 restatement of camera_ray_dir the temporal tests already hold to the device's words.

Images are 64 x 48 and 80 x 48, buckets = 2, two accumulations a frame, default9 and S(200): every case is seconds."""
import os
import subprocess

import numpy as np
import pytest

import temporal_motion_twin as mt
import temporal_twin as tt
from oracle_binding import bits

pytestmark = pytest.mark.gpu

f32 = np.float32
K = 2
PARAMS = {"iterations": 2}


def assert_same(got, want, what):
    got, want = bits(np.asarray(got, dtype=f32)), bits(np.asarray(want, dtype=f32))
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    bad = got != want
    n = int(bad.sum())
    where = np.argwhere(bad)[:4].tolist() if n else []
    assert n == 0, f"{what}: {n} of {got.size} words differ, first at {where}"


def twin_camera(r):
    c = r.scene.camera
    return tt.camera(c.pos, c.orient, c.half_width, c.half_height, c.z, c.exposure)


def scene_of(mirt, name):
    return mirt.scene.default9() if name == "default9" else mirt.scene.synthetic(200)


def centre_rays(r):
    """Origin and direction planes (3, w * h) of the pixel-centre rays, row-major over the whole image."""
    cam = twin_camera(r)
    py, px = np.meshgrid(np.arange(r.height, dtype=f32), np.arange(r.width, dtype=f32), indexing="ij")
    d = tt.camera_ray_dir(cam, px.ravel(), py.ravel())
    p = np.repeat(cam["pos"].reshape(3, 1), px.size, axis=1)
    return np.ascontiguousarray(p, dtype=f32), np.ascontiguousarray(np.stack(d), dtype=f32)


# ---- 1. the id map against the single-ray paths ------------------------------------------------------------------------------------------------
CONFIGS = {"host_sah": {"use_bvh": True}, "gpu_build": {"use_bvh": True, "gpu_build": True}, "reference_tree": {"use_bvh": True, "reference_tree": True},
           "brute": {"use_bvh": False}, "f32_records": {"use_bvh": True, "allow_half_boxes": False}}


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", ["default9", "S200"])
def test_id_map_is_the_single_ray_paths(mirt, name, config):
    w, h = 64, 48
    r = mirt.Renderer(scene_of(mirt, name), buckets=K, max_bounces=4, aov=True, **CONFIGS[config])
    r.Resize(w, h)
    r.Accumulate(K)
    before = (r.counters(), r.accumulator().copy(), r.aov().copy(), r.accumulations)
    prim, dist = r.id_map()
    after = (r.counters(), r.accumulator(), r.aov(), r.accumulations)
    assert after[0] == before[0] and after[3] == before[3], "counters (rays included) and the accumulation count"
    assert_same(after[1], before[1], "accumulator")
    assert_same(after[2], before[2], "AOV slab")
    p, d = centre_rays(r)
    tfar, want_prim = r.debug_trace_closest(p, d)
    want_prim, tfar = want_prim.reshape(h, w), tfar.reshape(h, w)
    hit = want_prim >= 0
    print(f"[id map] {name} {config}: {int(hit.sum())} of {w * h} pixels hit, {len(np.unique(want_prim[hit]))} spheres seen")
    assert hit.sum() > w * h // 8 and (~hit).sum() > 0
    assert np.array_equal(prim, want_prim), "prim against mirt_debug_trace_closest"
    assert_same(dist[hit], tfar[hit], "distance is tfar")
    assert np.isposinf(dist[~hit]).all(), "INFINITY on a miss"
    rng = np.random.default_rng(11)
    picks = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)] + [(int(rng.integers(w)), int(rng.integers(h))) for _ in range(16)]
    for x, y in picks:
        got, _ = r.pick_focus(x, y)
        assert bits(f32(got)) == bits(dist[y, x]), f"mirt_pick_focus at ({x}, {y})"
    r.set_lens(0.05, 2.0)
    lens_prim, lens_dist = r.id_map()
    assert np.array_equal(lens_prim, prim), "a lens leaves the map alone"
    assert_same(lens_dist, dist, "a lens leaves the distances alone")
    r.set_lens(0.0, 2.0)
    r.SetTileRange((w // 16) * 1, (w // 16) * 2)                                  # tile rows 1-2 of three: the map still covers the image
    part_prim, part_dist = r.id_map()
    assert np.array_equal(part_prim, prim), "a context that owns two tile rows"
    assert_same(part_dist, dist, "... distances")
    geo, _ = r.id_map(order="geometry")
    assert np.array_equal(r._bvh_of_geometry[geo[hit]].astype(np.int32), prim[hit]) and (geo[~hit] == -1).all()
    r.close()


def test_id_map_needs_a_scene_and_a_size(mirt):
    lib = mirt.load_library()
    import ctypes as C
    ctx = C.c_void_p()
    assert lib.mirt_create(0, C.byref(ctx)) == 0
    out = np.zeros(4, dtype=np.int32)
    assert lib.mirt_id_map(ctx, out.ctypes.data_as(C.c_void_p), None) == -3       # MIRT_ERR_STATE
    on = C.c_uint32(9)
    assert lib.mirt_get_sphere_motion(ctx, C.byref(on)) == 0 and on.value == 0
    assert lib.mirt_set_sphere_motion(ctx, 2) == -1                              # MIRT_ERR_ARG
    lib.mirt_destroy(ctx)


# ---- the temporal set-up -----------------------------------------------------------------------------------------------------------------------------
W, H = 80, 48
BALL = 1                                                                          # geometry-order sphere of default9 that moves: a small emissive ball on the ground


def make(mirt, motion=True, cls=None, **kw):
    cls = cls or mirt.Renderer
    kw.setdefault("use_bvh", True)
    r = cls(mirt.scene.default9(), buckets=K, max_bounces=4, aov=True, **kw)
    if motion:
        r.set_history_motion(True)
    r.Resize(W, H)
    return r


def table(r):
    return np.concatenate([r.prims["position"], r.prims["radius_sq"][:, None]], axis=1).astype(f32)


def pixel_step(r, pixels):
    """The world-space step that moves BALL `pixels` pixels along the image's +x (the camera's right axis), at the ball's axial depth."""
    c = r.scene.camera
    q = np.asarray(c.orient, dtype=np.float64)
    rot = lambda v: v + 2.0 * (q[3] * np.cross(q[:3], v) + np.cross(q[:3], np.cross(q[:3], v)))
    right, fwd = rot(np.array([1.0, 0.0, 0.0])), rot(np.array([0.0, 0.0, -1.0]))
    depth = float((r.geometry["position"][BALL].astype(np.float64) - np.asarray(c.pos, dtype=np.float64)) @ fwd)
    return right * pixels * depth / abs(float(c.z))


def move_ball(r, step=None, radius_scale=None):
    pos = r.geometry["position"][BALL].astype(np.float64) + (np.zeros(3) if step is None else step)
    rsq = float(r.geometry["radius_sq"][BALL]) * (1.0 if radius_scale is None else radius_scale ** 2)
    r.update_spheres([BALL], position=[pos.astype(f32)], radius_sq=[f32(rsq)])


def strafe(r, dx, dy=0.0, dz=0.0):
    r.scene.camera.pos = (np.asarray(r.scene.camera.pos, dtype=np.float64) + [dx, dy, dz]).astype(f32)
    r.UpdateCamera()


def temporal_frame(r, hist, what, check=True, **tparams):
    """One frame of the loop: reset, accumulate, resolve through the history; the device against the twin.  -> (the twin's history, class image, id map, frame, len)."""
    r.ResetAccumulator()
    r.Accumulate(K)
    acc, aov, counts = r.accumulator().copy(), r.aov().copy(), r.tile_counts().copy()
    ids, _ = r.id_map()
    want_frame, want_len, want_st, new_hist, cls = mt.render(acc, aov, counts, 1.0, PARAMS, tparams, W, H, twin_camera(r), hist, ids, table(r))
    frame, length, st = r.render_temporal(want_len=True, want_stats=True, **PARAMS, **tparams)
    print(f"[history motion] {what}: {st}")
    if check:
        assert st == want_st, f"{what}: class counts, twin {want_st}"
        assert_same(length, want_len, f"{what}: history_len")
        assert_same(frame, want_frame, f"{what}: frame")
    return new_hist, cls, ids, frame, length


def eroded(mask):
    """Pixels whose 3 x 3 neighbourhood lies in the mask."""
    p = np.pad(mask, 1, constant_values=False)
    out = np.ones_like(mask)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out &= p[dy:dy + mask.shape[0], dx:dx + mask.shape[1]]
    return out


def established(mirt, **kw):
    """A renderer with the switch on, the ball enlarged to a dozen pixels (so that a 5-pixel move leaves pixels that show it before and after), and a
    history written."""
    r = make(mirt, **kw)
    move_ball(r, radius_scale=1.6)
    hist, _, ids, _, _ = temporal_frame(r, None, "set-up")
    assert r.history_info()["valid"]
    return r, hist, ids


def check_moved_ball(r, cls, length, old_ids, new_ids):
    b = int(r._bvh_of_geometry[BALL])
    ground = int(r._bvh_of_geometry[0])
    both = eroded(old_ids == b) & eroded(new_ids == b)
    assert both.sum() >= 4, f"the move leaves {int(both.sum())} pixels that show the ball before and after"
    assert (cls[both] == mt.REPROJECTED).all(), "pixels inside the ball before and after are reprojected"
    assert (length[both] > f32(K)).all(), "... with len > n"
    uncovered = (new_ids == ground) & (old_ids == b)
    assert uncovered.sum() >= 4
    assert np.isin(cls[uncovered], (mt.REJECTED, mt.OUTSIDE)).all(), "the ground the ball uncovers does not inherit the ball's history"
    return int(both.sum()), int(uncovered.sum())


# ---- 2. default off ----------------------------------------------------------------------------------------------------------------------------------
def test_default_is_off_and_a_move_drops_the_history(mirt):
    r = make(mirt, motion=False)
    import ctypes as C
    on = C.c_uint32(9)
    assert r._lib.mirt_get_sphere_motion(r._ctx, C.byref(on)) == 0 and on.value == 0
    r.Accumulate(K)
    assert r.render_temporal(**PARAMS) is not None and r.history_info()["valid"]
    pos = r.geometry["position"][BALL].astype(np.float64) + [0.01, 0.0, 0.0]
    r.update_spheres([BALL], position=[pos.astype(f32)])
    assert r.history_info() == {"valid": False, "bytes": 0}
    r.close()


# ---- 3. the twin, word for word ------------------------------------------------------------------------------------------------------------------------
def test_moved_ball_equals_the_twin(mirt):
    r, hist, old_ids = established(mirt)
    move_ball(r, pixel_step(r, -5.0))
    assert r.history_info()["valid"], "the switch keeps the history across mirt_update_spheres"
    hist, cls, ids, _, length = temporal_frame(r, hist, "ball moved 5 pixels")
    both, uncovered = check_moved_ball(r, cls, length, old_ids, ids)
    print(f"[history motion] {both} pixels inside the ball before and after, {uncovered} ground pixels uncovered")
    hist, cls, _, _, _ = temporal_frame(r, hist, "one frame later, nothing moved")           # the snapshot followed the table: no sphere has moved now
    assert (cls[ids == int(r._bvh_of_geometry[BALL])] != mt.NO_HISTORY).all()
    r.close()


def test_camera_and_ball_both_moved(mirt):
    r, hist, old_ids = established(mirt)
    move_ball(r, pixel_step(r, -5.0))
    strafe(r, 0.004, 0.002)
    _, cls, ids, _, _ = temporal_frame(r, hist, "ball and camera moved")
    b = int(r._bvh_of_geometry[BALL])
    inside = eroded(ids == b)
    assert (cls[inside] == mt.REPROJECTED).sum() >= 4
    r.close()


@pytest.mark.parametrize("scale", [0.8, 1.25])
def test_radius_change(mirt, scale):
    r, hist, old_ids = established(mirt)
    move_ball(r, pixel_step(r, -3.0), radius_scale=scale)
    _, cls, ids, _, length = temporal_frame(r, hist, f"ball moved 3 pixels, radius x {scale}")
    b = int(r._bvh_of_geometry[BALL])
    deep = eroded(eroded(ids == b)) & eroded(eroded(old_ids == b))
    assert deep.sum() >= 1 and (cls[deep] == mt.REPROJECTED).all() and (length[deep] > f32(K)).all()
    r.close()


@pytest.mark.parametrize("where", ["out_of_frame", "behind"])
def test_ball_that_was_not_in_the_old_view_is_outside(mirt, where):
    r = make(mirt)
    move_ball(r, radius_scale=1.6)
    home = r.geometry["position"][BALL].copy()
    c = r.scene.camera
    if where == "out_of_frame":
        away = home.astype(np.float64) + pixel_step(r, 60.0)                                 # beyond the right edge of an 80-pixel image
    else:
        away = 2.0 * np.asarray(c.pos, dtype=np.float64) - home.astype(np.float64)        # mirrored through the camera: behind its image plane
    r.update_spheres([BALL], position=[away.astype(f32)])
    hist, _, old_ids, _, _ = temporal_frame(r, None, f"set-up, ball {where}")
    b = int(r._bvh_of_geometry[BALL])
    assert (old_ids != b).all()
    r.update_spheres([BALL], position=[home])
    _, cls, ids, _, _ = temporal_frame(r, hist, f"ball back from {where}")
    # a pixel inside the ball (its 3 x 3 neighbourhood shows it, so every jittered sample of its depth guide hit it) is carried to where the ball was:
    # `outside`.  A silhouette pixel's summed depth mixes in what lies behind the ball, which slides its point along the ray, possibly back into
    # the old image; the history shows no ball anywhere, so the id rule takes no tap for it: whatever its class, it is not `reprojected`.
    inside = eroded(ids == b)
    assert inside.sum() >= 40 and (cls[inside] == mt.OUTSIDE).all(), "where the ball was, the old camera saw nothing of this image"
    assert (cls[ids == b] != mt.REPROJECTED).all()
    r.close()


def test_two_updates_between_two_history_writes(mirt):
    r, hist, old_ids = established(mirt)
    move_ball(r, pixel_step(r, -9.0))
    move_ball(r, pixel_step(r, 4.0))                                                          # the map compares now with then: -5 pixels in all
    _, cls, ids, _, length = temporal_frame(r, hist, "two updates, one history write")
    check_moved_ball(r, cls, length, old_ids, ids)
    r.close()


def test_update_zero_changes_neither_snapshot_nor_id_plane(mirt):
    r, hist, old_ids = established(mirt)
    move_ball(r, pixel_step(r, -2.0))
    peek_hist, _, _, _, _ = temporal_frame(r, hist, "a call with update = 0", update=0)
    assert peek_hist is hist
    move_ball(r, pixel_step(r, -3.0))
    _, cls, ids, _, length = temporal_frame(r, hist, "then the writing call: still against the first snapshot and id plane")
    check_moved_ball(r, cls, length, old_ids, ids)
    r.close()


# ---- 4. nothing moved, camera identical: consequence (b) survives the id rule -------------------------------------------------------------------------
def test_identity_leaves_x_alone_with_the_switch_on(mirt):
    import denoise_twin as dt
    r = make(mirt)
    r.Accumulate(K)
    acc, aov, counts = r.accumulator().copy(), r.aov().copy(), r.tile_counts().copy()
    unfiltered = r.render_denoised(iterations=0)
    st0 = dt.prepare(acc, aov, counts, 1.0, dict(dt.DEFAULTS), W, H)
    follows = st0["usable"] & ~((st0["N"][0] == 0) & (st0["N"][1] == 0) & (st0["N"][2] == 0))
    assert follows.sum() > W * H // 4
    n = f32(K)
    f1, l1 = r.render_temporal(iterations=0, want_len=True)
    assert_same(f1, unfiltered, "first call")
    f2, l2, s2 = r.render_temporal(iterations=0, max_ratio=0.5, want_len=True, want_stats=True)
    assert_same(f2, unfiltered, "identity, switch on: x unchanged word for word")
    assert s2["reprojected"] == int(follows.sum()) and s2["rejected"] == s2["outside"] == 0
    assert_same(l2, np.where(follows, n + f32(0.5) * n, np.where(st0["usable"], n, f32(0))), "len = n + min(hn, max_ratio n)")
    r.close()


# ---- 5. switch and lifetime, a group, the headless tool -----------------------------------------------------------------------------------------------
def test_switch_and_lifetime(mirt):
    r = make(mirt, motion=False)
    n_spheres = len(r.geometry)

    def establish():
        r.ResetAccumulator()
        r.Accumulate(K)
        assert r.render_temporal(iterations=0) is not None and r.history_info()["valid"]
        return r.history_info()["bytes"]

    plain = establish()
    assert plain == W * H * 36
    r.set_history_motion(True)
    assert r.history_motion() and r.history_info() == {"valid": False, "bytes": 0}, "turning the switch on drops the history"
    assert establish() == plain + 4 * W * H + 16 * n_spheres
    r.set_history_motion(True)
    assert r.history_info()["valid"], "a value already held changes nothing"
    r.update_materials(materials={4: r.material[4]})
    assert r.history_info()["valid"], "mirt_update_materials keeps the history"
    move_ball(r, pixel_step(r, 1.0))
    assert r.history_info()["valid"]
    r.UpdateScene()
    assert r.history_info() == {"valid": False, "bytes": 0}, "mirt_set_scene drops it: ids change meaning"
    establish()
    r.set_history_motion(False)
    assert not r.history_motion() and r.history_info() == {"valid": False, "bytes": 0}, "turning the switch off drops the history"
    assert establish() == plain
    r.close()


def test_group_of_two_equals_the_single_context(mirt):
    single, hist, old_ids = established(mirt, use_bvh=True)
    group = make(mirt, cls=mirt.GroupRenderer, devices=(0, 0))
    assert group.history_motion()
    move_ball(group, radius_scale=1.6)
    group.Accumulate(K)
    assert group.render_temporal(**PARAMS) is not None
    gids, gdist = group.id_map()
    assert np.array_equal(gids, old_ids), "mirt_group_id_map"
    for r in (single, group):
        move_ball(r, pixel_step(r, -5.0))
    assert group.history_info()["valid"]
    _, _, _, want_frame, want_len = temporal_frame(single, hist, "single context")
    group.ResetAccumulator()
    group.Accumulate(K)
    frame, length, st = group.render_temporal(want_len=True, want_stats=True, **PARAMS)
    assert_same(frame, want_frame, "the group's frame")
    assert_same(length, want_len, "the group's history_len")
    assert st["reprojected"] > 0
    single.close(); group.close()


def test_headless_keeps_the_history_across_moves(mirt, tmp_path):
    exe = os.path.join(mirt.CSRC, "mirt_headless")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", mirt.CSRC, "mirt_headless"], check=True)
    step = (-0.01, 0.0, 0.0)
    pfm, ids_pfm = tmp_path / "frame.pfm", tmp_path / "ids.pfm"
    run = subprocess.run([exe, "--scene", "default9", "--size", f"{W}x{H}", "--bounces", "4", "--buckets", str(K), "--frames", "3", "--temporal", "--history-motion",
                          "--move-sphere", f"{BALL}:{step[0]},{step[1]},{step[2]}", "--out", str(pfm), "--ids-out", str(ids_pfm)], check=True, timeout=120, capture_output=True, text=True)
    got = np.fromfile(pfm, dtype=np.float32, offset=len(f"PF\n{W} {H}\n-1.0\n".encode())).reshape(H, W, 3)
    got_ids = np.fromfile(ids_pfm, dtype=np.float32, offset=len(f"Pf\n{W} {H}\n-1.0\n".encode())).reshape(H, W)
    r = make(mirt, use_bvh=True)
    stats = []
    for frame in range(3):
        r.Accumulate(K)
        out, st = r.render_temporal(want_stats=True)
        stats.append(st)
        if frame < 2:
            pos = r.geometry["position"][BALL] + np.asarray(step, dtype=f32)
            r.update_spheres([BALL], position=[pos])
            r.ResetAccumulator()
    assert stats[1]["reprojected"] > 0 and stats[2]["reprojected"] > 0, "the history survived the moves"
    assert_same(got, out[:, :, :3], "mirt_headless --history-motion against the Python frame")
    assert np.array_equal(got_ids.astype(np.int32), r.id_map()[0]), "--ids-out"
    lines = [l for l in run.stdout.splitlines() if l.startswith('{"temporal"')]
    assert len(lines) == 3 and all(f'"reprojected": {st["reprojected"]},' in l for l, st in zip(lines, stats)), "the tool's class counts are the Python path's"
    r.close()
