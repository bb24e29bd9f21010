"""Ragged image sizes without a GPU (ragged_sizes.py names the five sizes and what each isolates): the twins and definitions the GPU file compares
the kernels with, at those sizes, held to their float64 definitions with the bounds their own CPU tests use; and the DISCRIMINATION CONDITIONS, which
keep the GPU comparisons from passing vacuously — each shows, on the twins alone, that the chosen inputs tell `width` from `w_img`:

  (a) the à-trous twin run as if w_img = width (the planes' remainder readable and usable) differs from the definition's run in >= 1 % of the owned pixels;
  (b) the temporal twin bounded by width x height instead of w_img x h_img changes the class of >= 16 pixels per move;
  (c) a frame resolved with row pitch w_img instead of width differs in more than half of the rows.

Figures of the last run are printed by the tests and recorded in DESIGN.md section 2, "Ragged image sizes"."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import definitions as df
import denoise_twin as dt
import noise_twin as nt
import oracle_binding as ob
import ragged_sizes as rs
import temporal_definitions as td
import temporal_motion_twin as mt
import temporal_twin as tt
import test_aov as ta
from oracle_binding import bits
from test_definitions_cpu import RESOLVE_ABS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ---- the frame: oracle, binary32 twin, float64 median of means --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, 5])
@pytest.mark.parametrize("w,h", rs.SIZES)
def test_frame_twin_and_oracle_meet_the_float64_resolve(mirt, w, h, k):
    sc = mirt.scene.default9()
    o = ob.Oracle(sc, max_bounces=4, buckets=k); o.Resize(w, h); o.Accumulate(2 * k)
    acc, frame = o.accumulator().copy(), o.Render().copy()
    o.close()
    wi, hi = rs.img(w, h)
    assert acc.shape == (rs.tiles(w, h), k, 3, 256) and frame.shape == (h, w, 4)
    want = df.resolve(acc, 2 * k, 1.0, w, h)
    err = float(np.abs(frame.astype(np.float64) - want).max())
    print(f"[ragged] frame {w}x{h} k={k}: oracle against the float64 resolve {err:.3g} ({err / RESOLVE_ABS:.3f} of the bound)")
    assert err <= RESOLVE_ABS
    assert not want[hi:].any() and not want[:, wi:].any() and (want[:hi, :wi, 3] == 1).all(), "the definition owns exactly the tiled pixels"
    twin = dt.render_frame(acc, np.full(rs.tiles(w, h), 2 * k, dtype=np.uint32), 1.0, w, h)
    assert np.array_equal(bits(twin), bits(frame)), "denoise_twin.render_frame is the oracle's Render() word for word, remainder included"


@pytest.mark.parametrize("w,h", rs.COLUMN_REMAINDER)
def test_c_row_pitch_w_img_is_told_from_width(w, h):
    """(c): the rows of the owned image laid down at pitch w_img in a buffer of pitch width."""
    wi, hi = rs.img(w, h)
    slab, _, n = rs.synthetic(w, h, 5, 3 * w + h)
    good = dt.render_frame(slab, np.full(rs.tiles(w, h), n, dtype=np.uint32), 1.0, w, h)
    wrong = np.zeros(h * w * 4, dtype=f32)
    wrong[:hi * wi * 4] = good[:hi, :wi].reshape(-1)
    wrong = wrong.reshape(h, w, 4)
    rows = (bits(good) != bits(wrong)).any(axis=(1, 2))[:hi]
    print(f"[ragged] (c) {w}x{h}: {int(rows.sum())} of {hi} owned rows differ at pitch w_img")
    assert rows.mean() > 0.5


# ---- the à-trous twin ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", rs.SIZES)
def test_a_stencil_bounded_by_width_is_told_from_w_img(w, h):
    """(a), at every size with a column remainder; at 16 x 31 the same for the row remainder (bounded by height against h_img)."""
    wi, hi = rs.img(w, h)
    slab, aov, n = rs.synthetic(w, h, 5, 7 * w + h)
    counts = np.full(rs.tiles(w, h), n, dtype=np.uint32)
    st = dt.prepare(slab, aov, counts, 1.0, dict(dt.DEFAULTS), w, h)
    assert not st["usable"][5, wi - 1] and not st["usable"][hi - 1, 3] and int((~st["usable"]).sum()) == 2, "the NaN pixels of the last owned column and row"
    for it in (1, 3, 5):
        right = dt.denoise(slab, aov, counts, 1.0, {"iterations": it}, w, h)
        wide = rs.wide_denoise(slab, aov, counts, 1.0, {"iterations": it}, w, h)
        share = float((bits(right) != bits(wide))[:hi, :wi, :3].any(axis=-1).mean())
        print(f"[ragged] (a) {w}x{h}, iterations {it}: {100 * share:.1f} % of the owned pixels differ")
        assert share >= 0.01
    zero = dt.denoise(slab, aov, counts, 1.0, {"iterations": 0}, w, h)
    assert np.array_equal(bits(zero), bits(rs.wide_denoise(slab, aov, counts, 1.0, {"iterations": 0}, w, h))), "no pass, no stencil: the two readings agree"
    assert not zero[hi:].any() and not zero[:, wi:].any()


def test_to_image_is_the_plain_double_loop():
    for w, h in rs.SIZES:
        wi, hi = rs.img(w, h)
        per_tile = np.arange(rs.tiles(w, h) * 256, dtype=f32).reshape(-1, 256)
        want = np.zeros((hi, wi), dtype=f32)
        for t in range(rs.tiles(w, h)):
            for i in range(256):
                want[16 * (t // (w // 16)) + i // 16, 16 * (t % (w // 16)) + i % 16] = per_tile[t, i]
        assert np.array_equal(dt.to_image(per_tile, w, h), want)
        assert np.array_equal(nt.image(per_tile, range(rs.tiles(w, h)), w, h, f32(-7))[:hi, :wi], want)
        painted = nt.image(per_tile, range(rs.tiles(w, h)), w, h, f32(-7))
        assert (painted[hi:] == -7).all() and (painted[:, wi:] == -7).all()
        x, y = df.pixel_of_slot(np.arange(per_tile.size), w)
        assert np.array_equal(want[y, x], per_tile.reshape(-1))


def test_aov_twin_resolve_owns_the_tiled_pixels(mirt):
    for w, h in rs.SIZES[:2]:
        wi, hi = rs.img(w, h)
        sums, counts = ta.twin(mirt.scene.default9(), w, h, 2, max_bounces=4)
        assert sums.shape == (rs.tiles(w, h), 7, 256) and counts["hit"] > 0 and counts["miss"] > 0
        depth, nrm, alb = ta.twin_resolve(sums, w, h, 2)
        assert depth.shape == (h, w) and nrm.shape == alb.shape == (h, w, 3)
        for image in (depth, nrm, alb):
            assert not image[hi:].any() and not image[:, wi:].any()
        assert (depth[:hi, :wi] > 0).all()


# ---- the temporal twin on the analytic scene (temporal_definitions.py), camera built from width x height, images w_img x h_img --------------------
N_SAMPLES = 5.0
GC, G0 = np.array([[0.4, 0.0, 0.0], [0.0, 0.1, 0.3], [0.3, -0.2, 0.25]]), 1.5
TP = dict(tt.DEFAULTS)


def look(eye, direction, w, h):
    d = np.asarray(direction, dtype=np.float64) / np.linalg.norm(direction)
    c2 = -d
    c0 = np.cross([0.0, 1.0, 0.0], c2); c0 /= np.linalg.norm(c0)
    c1 = np.cross(c2, c0)
    m = np.stack([c0, c1, c2], axis=1)
    qw = np.sqrt(1.0 + m[0, 0] + m[1, 1] + m[2, 2]) / 2.0
    q = np.array([(m[2, 1] - m[1, 2]) / (4 * qw), (m[0, 2] - m[2, 0]) / (4 * qw), (m[1, 0] - m[0, 1]) / (4 * qw), qw])
    return tt.camera(np.asarray(eye, dtype=f32), q.astype(f32), w / 2, h / 2, (h / 2) * (-2.0 / 24.0 * 40.0))


def analytic_moves(w, h):
    """Camera A (the history's) and the three cameras B.  A looks down at the ground so that every remainder row and column shows it."""
    a = look((0.3, 1.6, 3.0), (-0.08, -0.75, -1.0), w, h)
    turned = tt.camera(a["pos"], (lambda q: (q / np.linalg.norm(q)).astype(f32))(rs.quat_mul([0.0, np.sin(np.radians(-1.7) / 2), 0.0, np.cos(np.radians(-1.7) / 2)], a["orient"])),
                       a["half_width"], a["half_height"], a["z"])
    moved = lambda delta: tt.camera((a["pos"].astype(np.float64) + delta).astype(f32), a["orient"], a["half_width"], a["half_height"], a["z"])
    return a, {"yaw": turned, "strafe": moved(np.array([0.21, 0.05, 0.0])), "dolly": moved(np.array([0.017, 0.15, 0.2]))}


def guides(cam, w, h):
    """The analytic scene over all width x height pixels, as binary32 images."""
    c64 = td.cam64(cam)
    depth, normal, on_sphere, hit = td.first_hit(c64, w, h)
    P = c64["pos"] + td.ray_dirs(c64, w, h) * depth[..., None]
    return {"x": (G0 + P @ GC.T).astype(f32), "v": np.full((h, w), 0.01, dtype=f32), "z": depth.astype(f32), "N": normal.astype(f32),
            "usable": np.ones((h, w), dtype=bool), "n": np.full((h, w), 3 * N_SAMPLES, dtype=f32), "cam": cam}


def cropped(g, w, h):
    wi, hi = rs.img(w, h)
    return {key: (v if key == "cam" else v[:hi, :wi]) for key, v in g.items()}


def twin_state(g):
    return {"x": [g["x"][..., c].copy() for c in range(3)], "v": g["v"].copy(), "z": g["z"], "N": [g["N"][..., c].copy() for c in range(3)], "usable": g["usable"]}


def twin_history(g):
    return dict(twin_state(g), n=g["n"], cam=g["cam"], demodulate=1, albedo_floor=f32(1 / 256), shape=g["z"].shape)


def twin_run(cur, hist, cam):
    n_img = np.full(cur["z"].shape, f32(N_SAMPLES))
    return tt.reproject_blend(twin_state(cur), n_img, cam, twin_history(hist), {"demodulate": 1, "albedo_floor": 1 / 256}, TP)


@pytest.mark.parametrize("move", ["yaw", "strafe", "dolly"])
@pytest.mark.parametrize("w,h", rs.TEMPORAL_SIZES)
def test_temporal_twin_against_the_float64_definition_and_b(w, h, move):
    """test_temporal_cpu's comparison (classes away from every threshold, |x32 - x64| within the derived bound) on the w_img x h_img image of a camera
    built from width x height; then (b): the same twin over all width x height pixels classes >= 16 owned pixels otherwise."""
    wi, hi = rs.img(w, h)
    cam_a, cams_b = analytic_moves(w, h)
    cam_b = cams_b[move]
    hist_full, cur_full = guides(cam_a, w, h), guides(cam_b, w, h)
    hist, cur = cropped(hist_full, w, h), cropped(cur_full, w, h)
    x32, v32, len32, cls32 = twin_run(cur, hist, cam_b)
    x32 = np.stack(x32, axis=-1)
    d = td.reproject_blend(cur, N_SAMPLES, cam_b, hist, TP)
    keep = ~d["near"]
    st = tt.stats_of(cls32)
    print(f"[ragged] temporal {w}x{h} {move}: classes {st}; {100 * d['near'].mean():.2f} % within rounding of a threshold")
    assert sum(st.values()) == wi * hi and d["near"].mean() <= 0.02
    assert st["reprojected"] > wi * hi // 3 and st["outside"] > 0
    assert np.array_equal(cls32[keep], d["cls"][keep]), "away from every threshold the classes agree"
    re = keep & (d["cls"] == 0)
    err = np.abs(x32.astype(np.float64) - d["x"])
    worst = float((err[re] / d["bound"][re]).max())
    print(f"[ragged] temporal {w}x{h} {move}: largest |x32 - x64| / bound over {int(re.sum())} reprojected pixels: {worst:.3f}")
    assert (err[re] <= d["bound"][re]).all()
    assert np.allclose(len32[keep], d["len"][keep], rtol=1e-5)
    # (b)
    _, _, _, cls_wide = twin_run(cur_full, hist_full, cam_b)
    changed = cls_wide[:hi, :wi] != cls32
    lands = rs.landers(twin_state(cur), cam_b, cam_a, w, h)
    print(f"[ragged] (b) {w}x{h} {move}: {int(changed.sum())} owned pixels change class under bounds width x height; {int(lands.sum())} land in the remainder")
    assert changed.sum() >= 16 and lands.sum() >= 16
    assert (cls32[lands] == tt.OUTSIDE).all(), "a pixel whose point lands in the planes' remainder is outside"


@pytest.mark.parametrize("w,h", rs.TEMPORAL_SIZES)
def test_the_gpu_files_moves_land_in_the_remainder(mirt, w, h):
    """default9 through the oracle (accumulator) and the AOV twin, under the moves test_ragged_sizes_gpu.py makes: each sends >= 16 pixels' points into
    columns [w_img, width) or rows [h_img, height) of the history."""
    k = 2
    sc = mirt.scene.default9()
    sc.camera.resize(w, h)
    counts = np.full(rs.tiles(w, h), k, dtype=np.uint32)
    prev = rs.twin_camera(sc.camera)
    for name, move in rs.MOVES.items():
        move(sc.camera)
        o = ob.Oracle(sc, max_bounces=4, buckets=k); o.Resize(w, h); o.Accumulate(k)
        acc = o.accumulator().copy(); o.close()
        aov, _ = ta.twin(sc, w, h, k, max_bounces=4)
        cam = rs.twin_camera(sc.camera)
        n = int(rs.landers(dt.prepare(acc, aov, counts, 1.0, dict(dt.DEFAULTS), w, h), cam, prev, w, h).sum())
        print(f"[ragged] default9 {w}x{h} {name}: {n} pixels land in the remainder")
        assert n >= 16
        prev = cam


def test_motion_twin_takes_the_id_map_of_the_whole_image():
    """temporal_motion_twin.render is handed mirt_id_map's (height, width) map and reads its w_img x h_img part; at a whole-tile size that is all of it."""
    w, h, k = 40, 70, 2
    wi, hi = rs.img(w, h)
    slab, aov, n = rs.synthetic(w, h, k, 9)
    counts = np.full(rs.tiles(w, h), n, dtype=np.uint32)
    cam = look((0.3, 1.6, 3.0), (-0.08, -0.75, -1.0), w, h)
    ids = np.arange(h * w, dtype=np.int32).reshape(h, w) % 3
    table = np.array([[0, 0, 0, 1], [1, 0, 0, 1], [0, 1, 0, 1]], dtype=f32)
    full = mt.render(slab, aov, counts, 1.0, {"iterations": 1}, {}, w, h, cam, None, ids, table)
    part = mt.render(slab, aov, counts, 1.0, {"iterations": 1}, {}, w, h, cam, None, ids[:hi, :wi], table)
    assert np.array_equal(bits(full[0]), bits(part[0])) and full[3]["ids"].shape == (hi, wi) and np.array_equal(full[3]["ids"], ids[:hi, :wi])
    moved = table.copy(); moved[1, 0] += f32(0.01)
    again = mt.render(slab, aov, counts, 1.0, {"iterations": 1}, {}, w, h, cam, full[3], ids, moved)
    assert sum(again[2].values()) == wi * hi and again[2]["reprojected"] > 0


# ---- the tile map's own check, at the five sizes --------------------------------------------------------------------------------------------------------
def test_tile_map_check_sweeps_the_five_sizes(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "tile_map_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "native", "tile_map_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    for w, h in rs.SIZES:
        assert f"ragged {w} {h} ok" in out.stdout, (w, h)
