"""The id map and the history kept across sphere moves, without a device: the binary32 twin of the moved-sphere map (temporal_motion_twin.py)
against its float64 statement (temporal_motion_definitions.py) within the bound DESIGN.md section 2 derives, and the interface at every layer.

The bound is operation count x unit roundoff x the magnitudes involved, all magnitudes from the float64 run (temporal_motion_definitions.moved_map
spells the terms out); it is not fitted to the twin: the largest ratio met is printed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import temporal_motion_definitions as md
import temporal_motion_twin as mt
import temporal_twin as tt

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unit_quat(rng):
    q = rng.normal(size=4)
    return (q / np.linalg.norm(q)).astype(f32)


def small_turn(rng, q, angle):
    """q turned by up to `angle` radians about a random axis, as binary32 words."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    h = rng.uniform(-angle, angle) / 2.0
    a = np.concatenate([axis * np.sin(h), [np.cos(h)]])
    x, y, z, w = [float(v) for v in q]
    bx, by, bz, bw = a
    out = np.array([bw * x + bx * w + by * z - bz * y, bw * y - bx * z + by * w + bz * x, bw * z + bx * y - by * x + bz * w, bw * w - bx * x - by * y - bz * z])
    return (out / np.linalg.norm(out)).astype(f32)


def rotate64(q, v):
    q = np.asarray(q, dtype=np.float64)
    uv = np.cross(q[:3], v)
    return v + 2.0 * (q[3] * uv + np.cross(q[:3], uv))


def draw_case(rng, scale, s_ratio, w=64, h=48):
    """One camera pair, one sphere that moves and scales, and the pixels of the camera that see it (grazing ones included): binary32 inputs."""
    cam = tt.camera((rng.normal(size=3) * scale).astype(f32), unit_quat(rng), w / 2.0, h / 2.0, -float(rng.uniform(0.8, 1.6) * h), 1.0)
    prev = tt.camera((cam["pos"].astype(np.float64) + rng.normal(size=3) * 0.05 * scale).astype(f32), small_turn(rng, cam["orient"], 0.05), w / 2.0, h / 2.0, float(cam["z"]), 1.0)
    # the sphere: on the ray through a pixel of the inner image, a few pixels across
    cx, cy = rng.uniform(0.25 * w, 0.75 * w), rng.uniform(0.25 * h, 0.75 * h)
    axis = rotate64(cam["orient"], np.array([cx - w / 2.0, cy - h / 2.0, float(cam["z"])]))
    axis /= np.linalg.norm(axis)
    dist = rng.uniform(2.0, 8.0) * scale
    radius = dist * rng.uniform(3.0, 9.0) / abs(float(cam["z"]))          # 3 to 9 pixels
    now = np.concatenate([cam["pos"].astype(np.float64) + axis * dist, [radius * radius]]).astype(f32)
    then = np.concatenate([now[:3].astype(np.float64) + rng.normal(size=3) * 0.5 * radius, [float(now[3]) * s_ratio * s_ratio]]).astype(f32)
    # every pixel of the patch around it: the float64 intersection of the binary32 inputs gives z; a miss is dropped, a grazing hit stays
    py, px = np.meshgrid(np.arange(int(cy) - 12, int(cy) + 13, dtype=np.float64), np.arange(int(cx) - 12, int(cx) + 13, dtype=np.float64), indexing="ij")
    px, py = px.ravel(), py.ravel()
    keep = (px >= 0) & (px < w) & (py >= 0) & (py < h)
    px, py = px[keep], py[keep]
    d = md.ray_dirs(md.td.cam64(cam), px, py)
    oc = cam["pos"].astype(np.float64) - now[:3].astype(np.float64)
    b = d @ oc
    disc = b * b - (oc @ oc - float(now[3]))
    hit = disc >= 0
    t = -b[hit] - np.sqrt(disc[hit])
    grazing = int((disc[hit] < 0.05 * float(now[3])).sum())
    return cam, prev, px[hit].astype(f32), py[hit].astype(f32), t.astype(f32), now, then, grazing


@pytest.mark.parametrize("scale", [1e-2, 1.0, 1e3])
def test_twin_against_the_float64_definition(scale):
    rng = np.random.default_rng(20260 + int(np.log10(scale)))
    worst_f = worst_z = 0.0
    compared = grazing = 0
    for s_ratio in (0.25, 0.5, 1.0, 1.7, 4.0):
        for _ in range(12):
            cam, prev, px, py, z, now, then, g = draw_case(rng, scale, s_ratio)
            n = len(px)
            assert n > 20
            ids = np.zeros(n, dtype=np.int32)
            fx, fy, zr, behind = mt.project(cam, prev, z, px, py, ids, now[None, :], then[None, :])
            want = md.moved_map(cam, prev, px, py, z, np.repeat(now[None, :], n, axis=0), np.repeat(then[None, :], n, axis=0))
            # the first-order analysis holds away from the history camera's own plane: points that project within four image widths of its axis
            ok = ~want["behind"] & (want["R"] < 4.0 * 64.0)
            assert np.array_equal(behind[ok], want["behind"][ok])
            ef = np.maximum(np.abs(fx.astype(np.float64) - want["fx"]), np.abs(fy.astype(np.float64) - want["fy"]))[ok]
            ez = np.abs(zr.astype(np.float64) - want["zr"])[ok]
            assert (ef <= want["delta_f"][ok]).all(), f"scale {scale}, s {s_ratio}: |f32 - f64| up to {ef.max():.3e} against a bound of {want['delta_f'][ok][ef.argmax()]:.3e}"
            assert (ez <= want["delta_z"][ok]).all(), f"scale {scale}, s {s_ratio}: |z'32 - z'64| up to {ez.max():.3e} against a bound of {want['delta_z'][ok][ez.argmax()]:.3e}"
            if ok.any():
                worst_f, worst_z = max(worst_f, float((ef / want["delta_f"][ok]).max())), max(worst_z, float((ez / want["delta_z"][ok]).max()))
            compared += int(ok.sum())
            grazing += g
            if s_ratio != 1.0:                                                 # the scale really is applied: P' lies on the old sphere
                dist = np.linalg.norm(want["Pp"] - then[:3].astype(np.float64), axis=-1)
                assert np.allclose(dist, np.sqrt(float(then[3])), rtol=2e-3)
    print(f"[history motion] scale {scale:g}: {compared} points ({grazing} grazing), largest |f32 - f64| / bound {worst_f:.3f}, largest |z'32 - z'64| / bound {worst_z:.3f}")
    assert compared > 2000 and grazing > 50


def test_unmoved_pixels_take_the_camera_only_map():
    """Not moved, or i < 0: the map is temporal_twin's word for word, the identity exception included; a moved sphere has no identity."""
    rng = np.random.default_rng(7)
    cam, prev, px, py, z, now, then, _ = draw_case(rng, 1.0, 2.0)
    n = len(px)
    table_now, table_then = np.stack([now, now]), np.stack([then, now])                          # sphere 0 moved, sphere 1 did not
    for p in (prev, cam):
        want = tt.project(cam, p, z, px, py)
        for ids in (np.full(n, -1, dtype=np.int32), np.full(n, 1, dtype=np.int32)):
            got = mt.project(cam, p, z, px, py, ids, table_now, table_then)
            for a, b in zip(got, want):
                assert np.array_equal(np.asarray(a).view(np.uint32) if a.dtype == f32 else a, np.asarray(b).view(np.uint32) if b.dtype == f32 else b)
    moved = mt.project(cam, cam, z, px, py, np.zeros(n, dtype=np.int32), table_now, table_then)
    assert not np.array_equal(moved[0], px) and not np.array_equal(moved[2], z)


# ---- the interface at every layer ------------------------------------------------------------------------------------------------------------------
HEADER = {
    "mirt_id_map": "int mirt_id_map(mirt_ctx* ctx, int32_t* prim_out /* w*h or NULL */, float* distance_out /* w*h or NULL */);",
    "mirt_set_sphere_motion": "int mirt_set_sphere_motion(mirt_ctx* ctx, uint32_t on);",
    "mirt_get_sphere_motion": "int mirt_get_sphere_motion(const mirt_ctx* ctx, uint32_t* on);",
    "mirt_set_motion_geometry": "int mirt_set_motion_geometry(mirt_ctx* ctx, mirt_ctx* geometry);",
    "mirt_group_set_sphere_motion": "int mirt_group_set_sphere_motion(mirt_group* group, uint32_t on);",
    "mirt_group_id_map": "int mirt_group_id_map(mirt_group* group, int32_t* prim_out, float* distance_out);",
}
CTYPE = {"mirt_ctx*": C.c_void_p, "const mirt_ctx*": C.c_void_p, "mirt_group*": C.c_void_p, "int32_t*": C.c_void_p, "float*": C.c_void_p, "uint32_t": C.c_uint32,
         "uint32_t*": C.POINTER(C.c_uint32)}


def test_interface_is_declared_at_every_layer(mirt):
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    lib, raw = mirt.load_library(), C.CDLL(mirt.LIB_PATH)
    for name, decl in HEADER.items():
        assert decl in header, f"include/mirt.h does not declare: {decl}"
        assert hasattr(raw, name), f"{name} is not exported by libmirt.so"
        assert name in lib._declared, f"{name} is not bound in Python"
        params = re.sub(r"/\*.*?\*/", "", decl[decl.index("(") + 1:decl.rindex(")")]).split(",")
        types = [p.strip().rsplit(" ", 1)[0].strip() for p in params]
        assert [CTYPE[t] for t in types] == list(getattr(lib, name).argtypes), f"{name}: ctypes signature against mirt.h"
        assert getattr(lib, name).restype is C.c_int
    # NULL handles and bad values are refused before any device is touched
    on = C.c_uint32(7)
    assert lib.mirt_id_map(None, None, None) < 0 and lib.mirt_group_id_map(None, None, None) < 0
    assert lib.mirt_set_sphere_motion(None, 1) < 0 and lib.mirt_group_set_sphere_motion(None, 1) < 0 and lib.mirt_get_sphere_motion(None, C.byref(on)) < 0
    assert lib.mirt_set_motion_geometry(None, None) < 0
    for cls in (mirt.Renderer, mirt.GroupRenderer):
        for method in ("set_history_motion", "history_motion", "id_map"):
            assert callable(getattr(cls, method)) and getattr(cls, method).__doc__
    host = open(os.path.join(mirt.CSRC, "mirt_host.hpp")).read()
    assert "SetHistoryMotion" in host and "IdMap" in host and "mirt_group_set_sphere_motion" in host and "mirt_group_id_map" in host
    tool = open(os.path.join(mirt.CSRC, "mirt_headless.cpp")).read()
    assert "--history-motion" in tool and "--ids-out" in tool


def test_id_map_in_geometry_order(mirt):
    """id_map(order="geometry") on a scene whose BVH order differs from the authoring order: pure host logic over a stubbed map."""
    geometry = np.array(mirt.scene.default9().geometry, dtype=mirt.SPHERE)
    _, prims = mirt.bvh_build(geometry)
    perm = mirt.geometry_to_bvh_order(geometry, prims)
    assert not np.array_equal(perm, np.arange(len(perm))), "default9's BVH order is not its authoring order"
    rng = np.random.default_rng(3)
    stub = rng.integers(-1, len(perm), size=(6, 8)).astype(np.int32)
    stub[0, :3] = (-1, 0, len(perm) - 1)

    class Stubbed(mirt.Renderer):
        def __init__(self):
            self.height, self.width = stub.shape
            self._bvh_of_geometry = perm

        def _call(self, name, *args):
            assert name == "id_map"
            C.memmove(args[0], stub.ctypes.data, stub.nbytes)
            return 0

        def close(self):
            pass

    r = Stubbed()
    bvh, dist = r.id_map()
    assert np.array_equal(bvh, stub) and dist.shape == stub.shape
    geo, _ = r.id_map(order="geometry")
    hit = stub >= 0
    assert (geo[~hit] == -1).all()
    assert np.array_equal(perm[geo[hit]], stub[hit].astype(perm.dtype)), "bvh_of_geometry[geometry id] is the BVH id the map held"
    assert np.array_equal(geometry[geo[hit]].tobytes(), prims[stub[hit]].tobytes()), "... and names the same sphere, row for row"
    with pytest.raises(ValueError):
        r.id_map(order="authoring")
    with pytest.raises(ValueError):
        mirt.id_map_to_geometry_order(np.array([len(perm)], dtype=np.int32), perm)
