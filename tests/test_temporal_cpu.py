"""The temporal history of the denoised resolve without a GPU: the interface at every layer, mirt_temporal_defaults (host code), and the binary32
twin (temporal_twin.py) against the float64 definition (temporal_definitions.py) on an analytic sphere over a ground plane, 64 x 48, under a yaw,
a strafe and a dolly.

Figures of the last run (printed by the tests): pixels left out as within rounding of a threshold, yaw 0.49 %, strafe 0.20 %, dolly 0.16 % of the
image (limit 2 %); |x32 - x64| stays within 0.12 of the derived bound.  The reprojected value against the linear colour AT P
differs by up to 0.84 (yaw), 0.91 (strafe), 0.083 (dolly) colour units, all near the horizon (median 5e-5 to 1.4e-4 over the pixels that blend
four ground taps): that is the bilinear remainder — a bilinear interpolant
over the perspective image of a plane is not exact, for a yaw no more than for the other moves — so it is reported for all three and bounded for
none.  What geometry does promise is asserted instead, on all three moves: the colour at P lies between the smallest and the largest of the four
tap colours of the cell the twin's (fx, fy) names (test_reprojection_lands_in_the_cell_that_holds_p)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import temporal_definitions as td
import temporal_twin as tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
MIRT_ERR_ARG = -1
NEW_NAMES = ("mirt_temporal_defaults", "mirt_render_temporal", "mirt_drop_history", "mirt_history_info", "mirt_group_render_temporal", "mirt_group_drop_history",
             "mirt_group_history_info")


# ---- interface -----------------------------------------------------------------------------------------------------------------------------------
def test_temporal_interface_is_declared_at_every_layer(mirt):
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    declared = set(re.findall(r"^int\s+(mirt_\w+)\s*\(", header, flags=re.M))
    lib = mirt.load_library()
    raw = C.CDLL(mirt.LIB_PATH)
    for n in NEW_NAMES:
        assert n in declared, f"{n} is not declared in include/mirt.h"
        assert hasattr(raw, n), f"{n} is not exported by libmirt.so"
        assert n in lib._declared, f"{n} is not bound in Python"
        assert not any(word in n for word in ("atrous", "noise", "until", "aov"))
    assert {n for n in declared if "temporal" in n or "history" in n} == set(NEW_NAMES)
    assert "typedef struct mirt_temporal_params {" in header and "typedef struct mirt_temporal_stats {" in header
    for text in ("THE DEFINITION", "LIFETIME", "THE SHADING SWITCHES DO NOT DROP IT", "604 MB at 4096 x 4096", "nh = cap < nh ? cap : nh"):
        assert text in header, text
    assert C.sizeof(mirt.TemporalParams) == 16 and mirt.TemporalParams.update.offset == 12 and C.sizeof(mirt.TemporalStats) == 40
    for cls in (mirt.Renderer, mirt.GroupRenderer):
        for method in ("render_temporal", "temporal_defaults", "drop_history", "history_info"):
            assert callable(getattr(cls, method)), method
        assert list(inspect.signature(cls.render_temporal).parameters)[1:4] == ["out", "want_len", "want_stats"]
    host = open(os.path.join(mirt.CSRC, "mirt_host.hpp")).read()
    for member in ("RenderTemporal(", "void DropHistory(", "static mirt_temporal_params TemporalDefaults("):
        assert member in host
    headless = open(os.path.join(mirt.CSRC, "mirt_headless.cpp")).read()
    for option in ("--temporal", "--orbit"):
        assert f'"{option}"' in headless
    makefile = open(os.path.join(mirt.CSRC, "Makefile")).read()
    assert re.search(r"^KERNEL_DEPS = .*\btemporal\.hpp\b", makefile, flags=re.M)


def test_defaults_are_the_documented_values(mirt):
    lib = mirt.load_library()
    assert lib.mirt_temporal_defaults(None) == MIRT_ERR_ARG
    p = mirt.TemporalParams(-1.0, -1.0, -9.0, 9)
    assert lib.mirt_temporal_defaults(C.byref(p)) == 0
    want = {"max_ratio": 7.0, "depth_tol": float(f32(0.02)), "normal_min": float(f32(0.9)), "update": 1}
    assert p.as_dict() == want and mirt.temporal_defaults() == want
    assert {k: float(f32(v)) if isinstance(v, float) else v for k, v in tt.DEFAULTS.items()} == want, "the twin starts from the same values"
    d = mirt.DenoiseParams(*mirt.denoise_defaults().values())
    assert lib.mirt_render_temporal(None, C.byref(d), C.byref(p), None, None, None) == MIRT_ERR_ARG
    assert lib.mirt_group_render_temporal(None, C.byref(d), C.byref(p), None, None, None) == MIRT_ERR_ARG
    assert lib.mirt_drop_history(None) == MIRT_ERR_ARG and lib.mirt_group_drop_history(None) == MIRT_ERR_ARG
    assert lib.mirt_history_info(None, None, None) == MIRT_ERR_ARG and lib.mirt_group_history_info(None, None, None) == MIRT_ERR_ARG
    with pytest.raises(TypeError):
        mirt._split_temporal_params({"ratio": 1.0})


# ---- the analytic scene: camera A (history) and camera B (current) -------------------------------------------------------------------------------
W, H, N_SAMPLES = 64, 48, 5.0
GC, G0 = np.array([[0.4, 0.0, 0.0], [0.0, 0.1, 0.3], [0.3, -0.2, 0.25]]), 1.5      # history colour channel c: G0 + GC[c] . P, linear in world position: one channel along x alone, one along depth, one mixed
SENTINEL = 1.0e6
TP = dict(tt.DEFAULTS)


def look(eye, direction):
    d = np.asarray(direction, dtype=np.float64) / np.linalg.norm(direction)
    # quatLookAt(direction, +y), right-handed: columns right, up, -direction
    c2 = -d
    c0 = np.cross([0.0, 1.0, 0.0], c2); c0 /= np.linalg.norm(c0)
    c1 = np.cross(c2, c0)
    m = np.stack([c0, c1, c2], axis=1)
    w = np.sqrt(1.0 + m[0, 0] + m[1, 1] + m[2, 2]) / 2.0
    q = np.array([(m[2, 1] - m[1, 2]) / (4 * w), (m[0, 2] - m[2, 0]) / (4 * w), (m[1, 0] - m[0, 1]) / (4 * w), w])
    return tt.camera(np.asarray(eye, dtype=f32), q.astype(f32), W / 2, H / 2, (H / 2) * (-2.0 / 24.0 * 40.0))


def yawed(cam, degrees):
    h = np.radians(degrees) / 2
    a, b = [0.0, np.sin(h), 0.0, np.cos(h)], [float(v) for v in cam["orient"]]
    q = np.array([a[3] * b[0] + a[1] * b[2], a[3] * b[1] + a[1] * b[3], a[3] * b[2] - a[1] * b[0], a[3] * b[3] - a[1] * b[1]])
    return tt.camera(cam["pos"], (q / np.linalg.norm(q)).astype(f32), cam["half_width"], cam["half_height"], cam["z"])


def moved(cam, delta):
    return tt.camera((cam["pos"].astype(np.float64) + delta).astype(f32), cam["orient"], cam["half_width"], cam["half_height"], cam["z"])


CAM_A = look((0.3, 1.1, 3.0), (-0.08, -0.2, -1.0))
CAMS_B = {"yaw": yawed(CAM_A, 1.7), "strafe": moved(CAM_A, np.array([0.21, 0.013, 0.0])), "dolly": moved(CAM_A, np.array([0.0, -0.05, -0.33]))}


def guides(cam, sentinel_on_sphere=False):
    """What k_denoise_prepare would leave for the analytic scene seen from `cam`, as binary32 images, and the float64 hit points."""
    c64 = td.cam64(cam)
    depth, normal, on_sphere, hit = td.first_hit(c64, W, H)
    P = c64["pos"] + td.ray_dirs(c64, W, H) * depth[..., None]
    colour = (G0 + P @ GC.T)
    if sentinel_on_sphere:
        colour = np.where(on_sphere[..., None], SENTINEL, colour)
    z32 = depth.astype(f32)
    P32 = c64["pos"] + td.ray_dirs(c64, W, H) * z32.astype(np.float64)[..., None]          # the point the binary32 depth names
    return {"x": colour.astype(f32), "v": np.full((H, W), 0.01, dtype=f32), "z": z32, "N": normal.astype(f32), "usable": np.ones((H, W), dtype=bool),
            "n": np.full((H, W), 3 * N_SAMPLES, dtype=f32), "cam": cam, "on_sphere": on_sphere, "hit": hit, "P": P32, "P_colour": P}


def twin_state(g):
    return {"x": [g["x"][..., c].copy() for c in range(3)], "v": g["v"].copy(), "z": g["z"], "N": [g["N"][..., c].copy() for c in range(3)], "usable": g["usable"]}


def twin_history(g):
    return dict(twin_state(g), n=g["n"], cam=g["cam"], demodulate=1, albedo_floor=f32(1 / 256), shape=(H, W))


def run(move, sentinel=False):
    hist, cur = guides(CAM_A, sentinel), guides(CAMS_B[move])
    n_img = np.full((H, W), f32(N_SAMPLES))
    x32, v32, len32, cls32 = tt.reproject_blend(twin_state(cur), n_img, CAMS_B[move], twin_history(hist), {"demodulate": 1, "albedo_floor": 1 / 256}, TP)
    return hist, cur, td.reproject_blend(cur, N_SAMPLES, CAMS_B[move], hist, TP), np.stack(x32, axis=-1), v32, len32, cls32


@pytest.mark.parametrize("move", ["yaw", "strafe", "dolly"])
def test_twin_against_the_float64_definition(move):
    hist, cur, d, x32, v32, len32, cls32 = run(move)
    left_out = d["near"]
    share = left_out.mean()
    keep = ~left_out
    st = tt.stats_of(cls32)
    print(f"[temporal] {move}: classes {st}; {int(left_out.sum())} pixels ({100 * share:.2f} %) within rounding of a threshold")
    assert sum(st.values()) == W * H
    assert share <= 0.02, "the definition alone keeps the left-out share within 2 %"
    assert st["reprojected"] > W * H // 3 and (move == "yaw" or st["rejected"] > 0) and st["no_history"] > 0 and st["unusable"] == 0
    assert np.array_equal(cls32[keep], d["cls"][keep]), "away from every threshold the classes agree"
    re = keep & (d["cls"] == 0)
    err = np.abs(x32.astype(np.float64) - d["x"])
    worst = float((err[re] / d["bound"][re]).max())
    print(f"[temporal] {move}: largest |x32 - x64| / bound over {int(re.sum())} reprojected pixels: {worst:.3f}; largest bound {d['bound'][re].max():.3e}")
    assert (err[re] <= d["bound"][re]).all()
    print(f"[temporal] {move}: largest bound relative to the colour: {(d['bound'][re] / np.abs(d['x'][re])).max():.3e}")
    assert np.allclose(len32[keep], d["len"][keep], rtol=1e-5) and np.array_equal(x32[keep & (d["cls"] != 0)], cur["x"][keep & (d["cls"] != 0)])
    # against the colour AT P: exact only up to the bilinear remainder; reported, not bounded
    at_p = (G0 + d["P"] @ GC.T)
    print(f"[temporal] {move}: largest |xh - colour(P)| over those pixels: {np.abs(d['xh'] - at_p)[re].max():.3e} (the bilinear remainder)")


@pytest.mark.parametrize("move", ["yaw", "strafe", "dolly"])
def test_reprojection_lands_in_the_cell_that_holds_p(move):
    """The map itself, held to geometry that does not go through its formula.  The history colour is linear in world position and painted from
    camera A's own float64 hit points; the current pixel's P comes from camera B's float64 ray and depth.  On the ground plane the four pixels
    of a 2 x 2 cell of A see a quadrilateral of the plane, and P lies inside it exactly when P projects into that cell of A — so the colour at
    P lies within [min, max] of the four tap colours.  The taps are the ones the TWIN's binary32 (fx, fy) names.  Slack: the colours' rounding
    to binary32 and a floor that comes out the other way within delta_f of a cell border, spread * 2 delta_f.  A shift
    of half a pixel, a swapped sign or a wrong t puts P outside the cell for about half the pixels."""
    hist, cur = guides(CAM_A), guides(CAMS_B[move])
    d = td.reproject_blend(cur, N_SAMPLES, CAMS_B[move], hist, TP)
    py, px = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")
    fx, fy, _, behind = tt.project(CAMS_B[move], CAM_A, cur["z"], px, py)
    ix, iy = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    inside = ~behind & (ix >= 0) & (iy >= 0) & (ix + 1 < W) & (iy + 1 < H)
    cx, cy = np.clip(ix, 0, W - 2), np.clip(iy, 0, H - 2)
    ground_a = hist["hit"] & ~hist["on_sphere"]
    on_plane = cur["hit"] & ~cur["on_sphere"] & inside
    taps = []
    for j in (0, 1):
        for i in (0, 1):
            on_plane &= ground_a[cy + j, cx + i]
            taps.append(hist["x"][cy + j, cx + i].astype(np.float64))
    assert on_plane.sum() > W * H // 4, f"{int(on_plane.sum())} ground pixels whose cell of the history is all ground"
    lo, hi = np.minimum.reduce(taps), np.maximum.reduce(taps)
    at_p = (G0 + cur["P_colour"] @ GC.T)
    slack = 2.0 ** -22 * np.maximum(np.abs(lo), np.abs(hi)) + (hi - lo) * 2.0 * d["delta_f"][..., None]
    below, above = (lo - at_p)[on_plane], (at_p - hi)[on_plane]
    worst = np.maximum(below, above) / slack[on_plane]
    spread = (hi - lo)[on_plane]
    print(f"[temporal] {move}: colour(P) against its cell's four taps over {int(on_plane.sum())} pixels: largest excursion / slack {worst.max():.3f}; median tap spread {np.median(spread):.3e}")
    assert (below <= slack[on_plane]).all() and (above <= slack[on_plane]).all()
    # the twin's own reprojected value lies in the same interval wherever the definition blends all four taps
    full = on_plane & (d["cls"] == 0) & ~d["near"] & (d["B"] > 1 - 1e-9) & np.all([t["taken"] for t in d["taps"]], axis=0)
    x32 = np.stack(tt.reproject_blend(twin_state(cur), np.full((H, W), f32(N_SAMPLES)), CAMS_B[move], twin_history(hist), {"demodulate": 1, "albedo_floor": 1 / 256}, TP)[0], axis=-1)
    a = d["a"][..., None]
    with np.errstate(all="ignore"):
        xh32 = (x32.astype(np.float64) - a * cur["x"]) / (1 - a)
        room = slack + d["bound"] / (1 - a)
    assert full.sum() >= 20 and (xh32[full] >= (lo - room)[full]).all() and (xh32[full] <= (hi + room)[full]).all()
    print(f"[temporal] {move}: largest |xh - colour(P)| over the {int(full.sum())} pixels that blend four ground taps: {np.abs(xh32 - at_p)[full].max():.3e}, median {np.median(np.abs(xh32 - at_p)[full]):.3e} (the bilinear remainder)")


def test_disocclusion_rejects_the_sphere(mirt=None):
    """The history paints the sphere with a sentinel.  After the strafe, a pixel whose current first hit is the ground and whose reprojection
    lands on the history's sphere — both decided in float64 geometry — carries no sentinel and counts as rejected."""
    hist, cur, d, x32, v32, len32, cls32 = run("strafe", sentinel=True)
    inside = (d["fx"] >= 0.5) & (d["fy"] >= 0.5) & (d["fx"] <= W - 1.5) & (d["fy"] <= H - 1.5)
    lands = np.zeros((H, W), dtype=bool)
    for t in d["taps"]:                                                            # every tap of the 2 x 2 on the history's sphere
        lands_t = hist["on_sphere"][t["cy"], t["cx"]]
        lands = lands_t if t is d["taps"][0] else lands & lands_t
    behind_sphere = cur["hit"] & ~cur["on_sphere"] & inside & lands
    assert behind_sphere.sum() >= 8, f"{int(behind_sphere.sum())} ground pixels reproject onto the history's sphere"
    assert np.array_equal(x32[behind_sphere], cur["x"][behind_sphere]), "no sentinel: x untouched"
    assert (cls32[behind_sphere] == tt.REJECTED).all() and (len32[behind_sphere] == f32(N_SAMPLES)).all()
    ground = cur["hit"] & ~cur["on_sphere"]
    clean = run("strafe")[3]
    assert np.array_equal(x32[ground].view(np.uint32), clean[ground].view(np.uint32)), "no ground pixel anywhere carries any sentinel: the words of a history without one"
