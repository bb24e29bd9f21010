"""mirt — MI355X-native wavefront path tracer for the reference's Renderer::Accumulate hot path.

This package is the thin Python host layer over the C-ABI in ``include/mirt.h`` (implemented by the
hand-written HIP kernels in ``csrc/``).  ``Renderer`` mirrors the reference's ``Renderer<Policy>``
interface (Renderer.hpp:51-68,73,436): ``Resize``, ``ResetAccumulator``, ``Accumulate``, ``Render``,
``GetFrame`` with the same meaning; the scene is handed over in the reference's byte layouts.

There is no CPU fallback: if ``libmirt.so`` or a gfx950 device is missing, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from . import distributed as distributed  # noqa: F401
from . import hdr as hdr  # noqa: F401
from . import scene as scene  # noqa: F401  (re-export)
from .scene import MATERIAL, NODE, SPHERE, Camera, Scene

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libmirt.so")

MIRT_OK, MIRT_NOT_READY = 0, 1
MIRT_NOT_CONVERGED = 2                            # mirt.h: accumulate_until gave up at max_accumulations
NOISE_BINS = 2048                                 # mirt.h MIRT_NOISE_BINS
AOV_DEPTH, AOV_NORMAL, AOV_ALBEDO = 0, 1, 2       # mirt.h MIRT_AOV_*
AOV_PLANES = 7
MAX_MATERIALS = 63                                # mirt.h MIRT_MAX_MATERIALS
MAX_LIGHT_RIS = 32                              # mirt.h MIRT_MAX_LIGHT_RIS
KERNEL_CLASSES = ("raygen", "trace", "shade", "shadow", "resolve")

# The switches on the per-hit shading, each stated once: (name, kind, constructor default), in the order the constructors apply them.  bool and int are
# one uint32 in the C-ABI; list is a table of one byte per material.  From a row follow the signatures of mirt_set_X, mirt_get_X and mirt_group_set_X
# (load_library), the getter X() of both renderers (_Binding) and what _configure does with the constructors' keyword X.
_SWITCHES = (("ggx_pdf", bool, False), ("material_closures", list, None), ("sky_sampling", bool, False), ("transmission", bool, False), ("light_ris", int, 0))


class MirtError(RuntimeError):
    pass


class Policy(C.Structure):
    """mirt_policy — RendererPolicy (Renderer.hpp:19-26) + the path's compile-time switches."""
    _fields_ = [("max_bounces", C.c_uint32), ("buckets", C.c_uint32), ("mis", C.c_uint32), ("use_bvh", C.c_uint32),
                ("count_traffic", C.c_uint32), ("profile", C.c_uint32), ("max_batch", C.c_uint32), ("reference_tree", C.c_uint32),
                ("streams", C.c_uint32), ("gpu_build", C.c_uint32), ("trace_primary_rays", C.c_uint32), ("brdf", C.c_uint32)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rays", "shadow_rays", "nodes", "spheres", "shadow_nodes", "shadow_spheres", "terminated", "dropped")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class KernelTimes(C.Structure):
    _fields_ = [("ms", C.c_double * 5), ("launches", C.c_uint64 * 5)]


class NoiseStats(C.Structure):
    """mirt_noise_stats"""
    _fields_ = [("owned_pixels", C.c_uint64), ("finite_pixels", C.c_uint64), ("nonfinite_pixels", C.c_uint64), ("max", C.c_float), ("_pad", C.c_uint32),
                ("mean", C.c_double)]

    def as_dict(self):
        return {"owned_pixels": int(self.owned_pixels), "finite_pixels": int(self.finite_pixels), "nonfinite_pixels": int(self.nonfinite_pixels),
                "max": float(self.max), "mean": float(self.mean)}


class StopRule(C.Structure):
    """mirt_stop_rule"""
    _fields_ = [("target", C.c_float), ("quantile", C.c_float), ("floor", C.c_float), ("check_every", C.c_uint32), ("max_accumulations", C.c_uint32)]


class AdaptiveReport(C.Structure):
    """mirt_adaptive_report"""
    _fields_ = [("issued", C.c_uint32), ("checks", C.c_uint32), ("frozen_tiles", C.c_uint32), ("owned_tiles", C.c_uint32), ("tile_accumulations", C.c_uint64),
                ("last", NoiseStats)]


class DenoiseParams(C.Structure):
    """mirt_denoise_params"""
    _fields_ = [("iterations", C.c_uint32), ("normal_squarings", C.c_uint32), ("demodulate", C.c_uint32), ("sigma_lum", C.c_float), ("sigma_depth", C.c_float),
                ("lum_floor", C.c_float), ("albedo_floor", C.c_float)]

    def as_dict(self):
        return {n: (int if t is C.c_uint32 else float)(getattr(self, n)) for n, t in self._fields_}


class TemporalParams(C.Structure):
    """mirt_temporal_params"""
    _fields_ = [("max_ratio", C.c_float), ("depth_tol", C.c_float), ("normal_min", C.c_float), ("update", C.c_uint32)]

    def as_dict(self):
        return {n: (int if t is C.c_uint32 else float)(getattr(self, n)) for n, t in self._fields_}


class SunSkyParams(C.Structure):
    """mirt_sun_sky_params"""
    _fields_ = [("sun_dir", C.c_float * 3), ("turbidity", C.c_float), ("sun_radius", C.c_float), ("sky_scale", C.c_float), ("sun_scale", C.c_float),
                ("ground", C.c_float * 3), ("width", C.c_uint32), ("height", C.c_uint32)]

    def as_dict(self):
        return {"sun_dir": tuple(self.sun_dir), "turbidity": self.turbidity, "sun_radius": self.sun_radius, "sky_scale": self.sky_scale,
                "sun_scale": self.sun_scale, "ground": tuple(self.ground), "width": int(self.width), "height": int(self.height)}


class TemporalStats(C.Structure):
    """mirt_temporal_stats"""
    _fields_ = [(n, C.c_uint64) for n in ("reprojected", "no_history", "outside", "rejected", "unusable")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def build(force: bool = False) -> str:
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC]
    if force:
        args.append("-B")
    subprocess.run(args, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return LIB_PATH


_lib = None


def load_library():
    """dlopen libmirt.so and declare every symbol of include/mirt.h.  Raises if the HIP extension is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MirtError(f"{LIB_PATH} not built — run __graft_entry__.build() (hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    P, u32, i32, f, vp = C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.c_void_p
    sigs = {
        "mirt_create": [i32, C.POINTER(P)],
        "mirt_destroy": [P],
        "mirt_bvh_build": [vp, u32, vp, C.POINTER(u32), vp],
        "mirt_light_list": [vp, u32, vp, u32, vp, C.POINTER(u32)],
        "mirt_set_scene": [P, vp, vp, u32, vp, u32, vp, u32, vp, u32, vp, vp, u32, u32],
        "mirt_set_camera": [P, vp, vp, f, f, f, f],
        "mirt_set_lens": [P, f, f], "mirt_get_lens": [P, C.POINTER(f), C.POINTER(f)],
        "mirt_pick_focus": [P, u32, u32, C.POINTER(f), C.POINTER(f)],
        "mirt_set_policy": [P, C.POINTER(Policy)],
        "mirt_get_policy": [P, C.POINTER(Policy)],
        "mirt_set_gloss_decay": [P, vp, u32],
        "mirt_set_stream_order": [P, u32], "mirt_get_stream_order": [P, C.POINTER(u32)],
        "mirt_resize": [P, u32, u32],
        "mirt_set_tile_range": [P, u32, u32], "mirt_set_tile_rows": [P, u32, u32],
        "mirt_reset": [P],
        "mirt_accumulate": [P, u32],
        "mirt_accumulate_async": [P, u32],
        "mirt_synchronize": [P],
        "mirt_get_accumulations": [P, C.POINTER(u32)],
        "mirt_accumulator_floats": [P, C.POINTER(C.c_size_t)],
        "mirt_read_accumulator": [P, vp],
        "mirt_accumulator_device": [P, C.POINTER(vp), C.POINTER(C.c_size_t)],
        "mirt_load_accumulator": [P, vp, i32, u32],
        "mirt_render": [P, vp],
        "mirt_set_aov": [P, u32], "mirt_get_aov": [P, C.POINTER(u32)],
        "mirt_aov_floats": [P, C.POINTER(C.c_size_t)],
        "mirt_read_aov": [P, vp],
        "mirt_aov_device": [P, C.POINTER(vp), C.POINTER(C.c_size_t)],
        "mirt_load_aov": [P, vp, i32],
        "mirt_render_aov": [P, i32, vp],
        "mirt_atrous_defaults": [C.POINTER(DenoiseParams)],
        "mirt_render_atrous": [P, C.POINTER(DenoiseParams), vp],
        "mirt_temporal_defaults": [C.POINTER(TemporalParams)],
        "mirt_render_temporal": [P, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), vp, vp, C.POINTER(TemporalStats)],
        "mirt_drop_history": [P],
        "mirt_history_info": [P, C.POINTER(u32), C.POINTER(C.c_uint64)],
        "mirt_id_map": [P, vp, vp],
        "mirt_set_sphere_motion": [P, u32], "mirt_get_sphere_motion": [P, C.POINTER(u32)],
        "mirt_set_motion_geometry": [P, P],
        "mirt_noise":[P, f, vp, vp, vp, C.POINTER(NoiseStats)],
        "mirt_noise_quantile": [vp, C.c_double, C.POINTER(f)],
        "mirt_accumulate_until": [P, C.POINTER(StopRule), C.POINTER(NoiseStats), C.POINTER(u32)],
        "mirt_freeze_tiles": [P, vp, C.c_size_t],
        "mirt_tile_counts": [P, vp, C.c_size_t],
        "mirt_frozen_tiles": [P, vp, C.c_size_t],
        "mirt_load_tile_counts": [P, vp, C.c_size_t],
        "mirt_tile_above": [P, f, f, vp, C.c_size_t],
        "mirt_adaptive_select": [vp, vp, vp, C.c_size_t, C.c_double, vp],
        "mirt_accumulate_adaptive": [P, C.POINTER(StopRule), u32, C.POINTER(AdaptiveReport)],
        "mirt_set_environment": [P, vp, vp, u32, u32],
        "mirt_read_environment": [P, vp, C.c_size_t, vp],
        "mirt_sun_sky_defaults": [C.POINTER(SunSkyParams)],
        "mirt_set_sun_sky": [P, C.POINTER(SunSkyParams)],
        "mirt_update_spheres": [P, u32, vp, vp, vp],
        "mirt_update_materials": [P, u32, vp, vp, u32, vp, vp, vp],
        "mirt_debug_lights": [P, vp, vp, vp, C.c_size_t, vp],
        "mirt_get_counters": [P, C.POINTER(Counters)],
        "mirt_get_kernel_times": [P, C.POINTER(KernelTimes), i32],
        "mirt_get_stream": [P, C.POINTER(vp)],
        "mirt_debug_raygen": [P, u32, vp, vp],
        "mirt_debug_trace_closest": [P, C.c_size_t, vp, vp, vp, vp],
        "mirt_debug_trace_shadow": [P, C.c_size_t, vp, vp, vp, vp],
        "mirt_debug_math": [P, i32, C.c_size_t, vp, vp],
        "mirt_debug_info": [P, vp],
        "mirt_debug_tree": [P, vp, C.c_size_t, vp],
        "mirt_debug_sky_table": [P, vp, C.c_size_t, vp],
        "mirt_debug_primary_lists": [P, vp],
        "mirt_debug_primary_counts": [P, vp, C.c_size_t],
        "mirt_debug_allow_half_boxes": [P, i32],
    }
    G = C.c_void_p
    sigs.update({
        "mirt_group_create": [vp, i32, C.POINTER(G)],
        "mirt_group_destroy": [G],
        "mirt_group_size": [G, C.POINTER(i32)],
        "mirt_group_member": [G, i32, C.POINTER(P)],
        "mirt_group_set_scene": [G, vp, vp, u32, vp, u32, vp, u32, vp, u32, vp, vp, u32, u32],
        "mirt_group_set_camera": [G, vp, vp, f, f, f, f],
        "mirt_group_set_lens": [G, f, f],
        "mirt_group_pick_focus": [G, u32, u32, C.POINTER(f), C.POINTER(f)],
        "mirt_group_set_environment": [G, vp, vp, u32, u32],
        "mirt_group_set_sun_sky": [G, C.POINTER(SunSkyParams)],
        "mirt_group_update_spheres": [G, u32, vp, vp, vp],
        "mirt_group_update_materials": [G, u32, vp, vp, u32, vp, vp, vp],
        "mirt_group_set_policy": [G, C.POINTER(Policy)],
        "mirt_group_set_gloss_decay": [G, vp, u32],
        "mirt_group_set_stream_order": [G, u32],
        "mirt_group_resize": [G, u32, u32],
        "mirt_group_reset": [G],
        "mirt_group_accumulate": [G, u32],
        "mirt_group_accumulate_async": [G, u32],
        "mirt_group_synchronize": [G],
        "mirt_group_get_accumulations": [G, C.POINTER(u32)],
        "mirt_group_get_counters": [G, C.POINTER(Counters)],
        "mirt_group_gather": [G],
        "mirt_group_last_gather_ms": [G, C.POINTER(C.c_double)],
        "mirt_group_accumulator_floats": [G, C.POINTER(C.c_size_t)],
        "mirt_group_read_accumulator": [G, vp],
        "mirt_group_render": [G, vp],
        "mirt_group_set_aov": [G, u32],
        "mirt_group_aov_floats": [G, C.POINTER(C.c_size_t)],
        "mirt_group_read_aov": [G, vp],
        "mirt_group_render_aov": [G, i32, vp],
        "mirt_group_render_atrous": [G, C.POINTER(DenoiseParams), vp],
        "mirt_group_render_temporal": [G, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), vp, vp, C.POINTER(TemporalStats)],
        "mirt_group_drop_history": [G],
        "mirt_group_history_info": [G, C.POINTER(u32), C.POINTER(C.c_uint64)],
        "mirt_group_set_sphere_motion": [G, u32],
        "mirt_group_id_map": [G, vp, vp],
        "mirt_group_noise": [G, f, vp, vp, vp, C.POINTER(NoiseStats)],
        "mirt_group_accumulate_until": [G, C.POINTER(StopRule), C.POINTER(NoiseStats), C.POINTER(u32)],
        "mirt_group_freeze_tiles": [G, vp, C.c_size_t],
        "mirt_group_tile_counts": [G, vp, C.c_size_t],
        "mirt_group_frozen_tiles": [G, vp, C.c_size_t],
        "mirt_group_tile_above": [G, f, f, vp, C.c_size_t],
        "mirt_group_accumulate_adaptive": [G, C.POINTER(StopRule), u32, C.POINTER(AdaptiveReport)],
        "mirt_group_rccl_selftest": [i32, C.c_size_t],
    })
    for name, kind, _ in _SWITCHES:
        value = [vp, u32] if kind is list else [u32]
        sigs["mirt_set_" + name], sigs["mirt_group_set_" + name] = [P] + value, [G] + value
        sigs["mirt_get_" + name] = [P, vp, u32, C.POINTER(u32), C.POINTER(u32)] if kind is list else [P, C.POINTER(u32)]
    for name, argtypes in sigs.items():
        fn = getattr(lib, name)      # AttributeError if the library does not export a declared symbol
        fn.argtypes = argtypes
        fn.restype = C.c_int
    lib.mirt_last_error.argtypes = [P]
    lib.mirt_last_error.restype = C.c_char_p
    lib.mirt_group_last_error.argtypes = [P]
    lib.mirt_group_last_error.restype = C.c_char_p
    lib._declared = tuple(sigs) + ("mirt_last_error", "mirt_group_last_error")
    _lib = lib
    return lib


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def bvh_build(geometry: np.ndarray):
    """BoundingVolumeHierarchy<Sphere> ctor (BVH.hpp:90-206) -> (nodes, bvh-order prims)."""
    lib = load_library()
    geometry = np.ascontiguousarray(geometry, dtype=SPHERE)
    n = len(geometry)
    nodes = np.zeros(max(2 * n, 1), dtype=NODE)
    prims = np.zeros(n, dtype=SPHERE)
    n_nodes = C.c_uint32(0)
    rc = lib.mirt_bvh_build(_ptr(geometry), n, _ptr(nodes), C.byref(n_nodes), _ptr(prims))
    if rc != MIRT_OK:
        raise MirtError(f"mirt_bvh_build failed ({rc})")
    return nodes[: n_nodes.value].copy(), prims


def light_list(geometry: np.ndarray, material: np.ndarray) -> np.ndarray:
    """LightingAcceleration ctor (Scene.hpp:12-16)."""
    lib = load_library()
    geometry = np.ascontiguousarray(geometry, dtype=SPHERE)
    material = np.ascontiguousarray(material, dtype=MATERIAL)
    out = np.zeros(max(len(geometry), 1), dtype=np.int32)
    n = C.c_uint32(0)
    rc = lib.mirt_light_list(_ptr(geometry), len(geometry), _ptr(material), len(material), _ptr(out), C.byref(n))
    if rc != MIRT_OK:
        raise MirtError(f"mirt_light_list failed ({rc})")
    return out[: n.value].copy()


def geometry_to_bvh_order(geometry: np.ndarray, prims: np.ndarray) -> np.ndarray:
    """perm with prims[perm[g]] == geometry[g], row for row (32-byte SPHERE rows compared as bytes): where authoring-order sphere g sits in the
    BVH-order array hit.primID refers to.  Identical rows are interchangeable, so any bijection among them is right; here the k-th of a run of
    equal rows in `geometry` goes to the k-th of that run in `prims`.  Pure numpy, no GPU.  ValueError unless one is a permutation of the other."""
    g = np.ascontiguousarray(geometry, dtype=SPHERE)
    p = np.ascontiguousarray(prims, dtype=SPHERE)
    if g.shape != p.shape or g.ndim != 1:
        raise ValueError(f"geometry {g.shape} and prims {p.shape} must be two 1-D arrays of one length")
    gw, pw = g.view(np.uint64).reshape(len(g), 4), p.view(np.uint64).reshape(len(p), 4)
    og, op = np.lexsort(gw.T[::-1]), np.lexsort(pw.T[::-1])             # stable: equal rows keep their order
    if not np.array_equal(gw[og], pw[op]):
        raise ValueError("prims is not a permutation of geometry's rows")
    perm = np.empty(len(g), dtype=np.uint32)
    perm[og] = op
    return perm


def id_map_to_geometry_order(prim: np.ndarray, bvh_of_geometry: np.ndarray) -> np.ndarray:
    """An id map in BVH order (mirt_id_map) -> the same map in authoring order: bvh_of_geometry[g] is where geometry-order sphere g sits in the
    BVH-order array (geometry_to_bvh_order), so pixel value b becomes the g with bvh_of_geometry[g] == b; -1 (a miss) stays -1.  Pure numpy."""
    perm = np.asarray(bvh_of_geometry, dtype=np.int64).reshape(-1)
    inverse = np.full(len(perm) + 1, -1, dtype=np.int32)                 # the last row answers -1
    inverse[perm] = np.arange(len(perm), dtype=np.int32)
    prim = np.asarray(prim, dtype=np.int32)
    if prim.size and (prim.min() < -1 or prim.max() >= len(perm)):
        raise ValueError(f"id map holds ids outside -1 .. {len(perm) - 1}")
    return inverse[prim]


def _aov_image(height: int, width: int, which: int, out):
    """The buffer mirt_render_aov fills: (height, width) for depth, (height, width, 3) for normal and albedo."""
    shape = (height, width) if which == AOV_DEPTH else (height, width, 3)
    if out is None:
        return np.zeros(shape, dtype=np.float32)
    if out.dtype != np.float32 or out.shape != shape or not out.flags.c_contiguous:
        raise ValueError(f"out must be a C-contiguous float32 array of shape {shape}")
    return out


def _lens_arguments(camera: Camera, aperture_radius, focus_depth):
    """Arguments of mirt_set_lens: what the caller gave, else the scene camera's (aperture_radius in world units, focus_distance)."""
    a = camera.aperture_radius if aperture_radius is None else aperture_radius
    d = camera.focus_distance if focus_depth is None else focus_depth
    return float(np.float32(a)), float(np.float32(d))


def _closure_table(closures) -> np.ndarray:
    """The table mirt_set_material_closures takes, validated before any call into the library: at most MAX_MATERIALS entries, each 0 or 1."""
    t = [] if closures is None else list(closures)
    if len(t) > MAX_MATERIALS:
        raise ValueError(f"material_closures holds {len(t)} entries; a scene has at most {MAX_MATERIALS} materials")
    for m, v in enumerate(t):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v not in (0, 1):
            raise ValueError(f"material_closures[{m}] = {v!r} is neither 0 (Lambertian) nor 1 (GGX)")
    return np.ascontiguousarray(t, dtype=np.uint8)


def _index_value_pair(arg, dtype, what: str):
    """update_materials' two arguments: None, a mapping index -> value or a pair (indices, values) -> (int64 indices, C-contiguous values of `dtype`),
    one value per index; refused before any call into the library otherwise."""
    if arg is None:
        idx, val = [], []
    elif hasattr(arg, "keys"):
        idx, val = list(arg.keys()), [arg[k] for k in arg.keys()]
    else:
        try:
            idx, val = arg
        except (TypeError, ValueError):
            raise ValueError(f"{what} must be a mapping index -> value or a pair (indices, values)") from None
    idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
    if len(idx) == 0:
        return idx, np.zeros(0, dtype=dtype)
    if isinstance(val, np.ndarray):
        val = val.astype(dtype, copy=False).reshape(-1)
    elif np.dtype(dtype).fields:                                         # rows of a structured dtype: records, or tuples field by field
        val = np.array([v if isinstance(v, np.void) else tuple(v) for v in val], dtype=dtype)
    else:
        val = np.asarray(val).astype(dtype).reshape(-1)
    val = np.ascontiguousarray(val, dtype=dtype)
    if len(val) != len(idx):
        raise ValueError(f"{what}: {len(idx)} indices and {len(val)} values")
    return idx, val


def noise_quantile(hist, q: float):
    """mirt_noise_quantile (host code, no GPU): the UPPER EDGE of the histogram bin that holds the q-quantile (q in (0, 1]) of the usable
    pixels — at most 12.5 % above the quantile itself.  None for an empty histogram."""
    lib = load_library()
    h = np.ascontiguousarray(hist, dtype=np.uint32).reshape(-1)
    if h.size != NOISE_BINS:
        raise ValueError(f"hist must hold {NOISE_BINS} words")
    v = C.c_float(0)
    rc = lib.mirt_noise_quantile(_ptr(h), float(q), C.byref(v))
    if rc < 0:
        raise MirtError(f"mirt_noise_quantile failed ({rc}): q = {q} is not in (0, 1]")
    return v.value if rc == MIRT_OK else None


def denoise_defaults() -> dict:
    """mirt_atrous_defaults (host code, no GPU): the parameters render_denoised() starts from, by name."""
    p = DenoiseParams()
    rc = load_library().mirt_atrous_defaults(C.byref(p))
    if rc != MIRT_OK:
        raise MirtError(f"mirt_atrous_defaults failed ({rc})")
    return p.as_dict()


def _denoise_params(params: dict) -> DenoiseParams:
    """The defaults with the caller's keywords laid over them; an unknown keyword is a TypeError before any call into the library."""
    d = denoise_defaults()
    unknown = sorted(set(params) - set(d))
    if unknown:
        raise TypeError(f"not a denoise parameter: {unknown} (known: {sorted(d)})")
    d.update(params)
    return DenoiseParams(int(d["iterations"]), int(d["normal_squarings"]), int(d["demodulate"]), float(d["sigma_lum"]), float(d["sigma_depth"]),
                         float(d["lum_floor"]), float(d["albedo_floor"]))


def temporal_defaults() -> dict:
    """mirt_temporal_defaults (host code, no GPU): the temporal parameters render_temporal() starts from, by name."""
    p = TemporalParams()
    rc = load_library().mirt_temporal_defaults(C.byref(p))
    if rc != MIRT_OK:
        raise MirtError(f"mirt_temporal_defaults failed ({rc})")
    return p.as_dict()


def _split_temporal_params(params: dict):
    """render_temporal's keywords -> (mirt_denoise_params, mirt_temporal_params): each name belongs to exactly one of the two sets of defaults."""
    t = temporal_defaults()
    own = {k: params[k] for k in params if k in t}
    t.update(own)
    return _denoise_params({k: v for k, v in params.items() if k not in own}), TemporalParams(float(t["max_ratio"]), float(t["depth_tol"]), float(t["normal_min"]), int(t["update"]))


def sun_sky_defaults() -> dict:
    """mirt_sun_sky_defaults (host code, no GPU): the parameters set_sun_sky() starts from, by name — starting values and design choices."""
    p = SunSkyParams()
    rc = load_library().mirt_sun_sky_defaults(C.byref(p))
    if rc != MIRT_OK:
        raise MirtError(f"mirt_sun_sky_defaults failed ({rc})")
    return p.as_dict()


def _sun_sky_params(params: dict) -> SunSkyParams:
    """The defaults with the caller's keywords laid over them; an unknown keyword is a TypeError before any call into the library."""
    d = sun_sky_defaults()
    unknown = sorted(set(params) - set(d))
    if unknown:
        raise TypeError(f"not a sun and sky parameter: {unknown} (known: {sorted(d)})")
    d.update(params)
    vec = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    return SunSkyParams(vec(d["sun_dir"]), float(d["turbidity"]), float(d["sun_radius"]), float(d["sky_scale"]), float(d["sun_scale"]), vec(d["ground"]),
                        int(d["width"]), int(d["height"]))


def adaptive_select(tiles, above, frozen=None, quantile: float = 0.95) -> np.ndarray:
    """mirt_adaptive_select (host code, no GPU): from noise()["tiles"] and noise_above() the mask of tiles to freeze — a tile not yet frozen
    freezes when it has no non-finite pixel and above <= floor((1 - quantile) * usable); tiles already in `frozen` are passed through as 1."""
    lib = load_library()
    t = np.ascontiguousarray(tiles, dtype=np.float32).reshape(-1, 4)
    a = np.ascontiguousarray(above, dtype=np.uint32).reshape(-1)
    fr = None if frozen is None else np.ascontiguousarray(np.asarray(frozen) != 0, dtype=np.uint8).reshape(-1)
    if len(a) != len(t) or (fr is not None and len(fr) != len(t)):
        raise ValueError("tiles, above and frozen must describe the same tiles")
    out = np.zeros(len(t), dtype=np.uint8)
    rc = lib.mirt_adaptive_select(_ptr(t), _ptr(a), _ptr(fr) if fr is not None else None, len(t), float(quantile), _ptr(out))
    if rc < 0:
        raise MirtError(f"mirt_adaptive_select failed ({rc}): quantile = {quantile} is not in (0, 1]")
    return out


class _Binding:
    """What ``Renderer`` and ``GroupRenderer`` share: the methods that differ only in the handle (``_ctx`` / ``_g``) and in the prefix of
    the entry point (``mirt_`` / ``mirt_group_``).  A subclass names both and creates the handle."""
    _prefix = _handle = None

    # -- plumbing ---------------------------------------------------------------------------
    def _check(self, rc):
        if rc < 0:
            last_error = getattr(self._lib, self._prefix + "last_error")
            raise MirtError(f"{self._prefix[:-1]} call failed ({rc}): {last_error(getattr(self, self._handle)).decode()}")
        return rc

    def _call(self, name, *args):
        """mirt_<name> or mirt_group_<name> on this object's handle, checked."""
        return self._check(getattr(self._lib, self._prefix + name)(getattr(self, self._handle), *args))

    def _configure(self, *, gloss_decay, exact_stream_order, aov, **switches):
        """The end of both constructors, after the policy is set: the rows of _SWITCHES by keyword, in the table's order (a switch left off and a
        table left out are not set), then the rest."""
        for name, kind, _ in _SWITCHES:
            value = switches.pop(name)                     # KeyError: a constructor that does not pass a row on
            if value is not None and (kind is list or value):
                getattr(self, "set_" + name)(value)
        if switches:
            raise TypeError(f"not in _SWITCHES: {sorted(switches)}")
        if gloss_decay is not None:
            self.set_gloss_decay(gloss_decay)
        if exact_stream_order:
            self.set_stream_order(True)
        if aov:
            self.set_aov(True)
        self.UpdateScene()

    def close(self):
        h = getattr(self, self._handle, None)
        if h and h.value:
            getattr(self._lib, self._prefix + "destroy")(h)
            setattr(self, self._handle, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_policy(self, **kw):
        p = Policy.from_buffer_copy(self.policy)
        for k, v in kw.items():
            setattr(p, k, int(v))
        self._call("set_policy", C.byref(p))
        self.policy = p                                    # only a policy the library accepted becomes this object's

    def set_gloss_decay(self, decay=None):
        """gloss_decay_table (Renderer.hpp:212) for brdf = 1: decay[b] is mixed into the GGX alpha at bounce b; later bounces use 0.
        None or an empty sequence resets it to zeros.  (A group: on every member.)"""
        d = np.ascontiguousarray([] if decay is None else decay, dtype=np.float32).reshape(-1)
        self._call("set_gloss_decay", _ptr(d) if len(d) else None, len(d))

    def set_stream_order(self, exact: bool = True):
        """True: replay the reference's stream slots (counting sort by material, in-order compaction) and its scalar intersection tail
        (BVH.hpp:270-286) — brute-force traversal, a fidelity mode (mirt_set_stream_order).  False: the default wavefront order.
        (A group: on every member.)"""
        self._call("set_stream_order", int(exact))

    def set_light_ris(self, candidates: int = 8):
        """Next event estimation picks its light among `candidates` uniform draws by resampled importance sampling (the reference's unused
        RIS<count>, Sampling.hpp:25-54): same expectation, less noise where many lights are wasted draws, still one shadow ray per hit.
        0 = off (the default, the uniform draw); at most MAX_LIGHT_RIS; not in exact stream order.  Does not reset the accumulator.
        (A group: on every member.)"""
        self._call("set_light_ris", int(candidates))

    def set_transmission(self, on: bool = True):
        """True: a material with max(transmission) > 0 is glass — a smooth dielectric interface of index 1 + IOR_minus_one (Snell, unpolarised
        Fresnel, total internal reflection; the tint transmission / max is applied once per pass through a ball; mirt.h, mirt_set_transmission).
        False (the default): no kernel reads the two fields, as in the reference.  Shadow rays treat glass as opaque.  Not in exact stream
        order.  Another estimand, and the accumulator is NOT reset: call Reset().  (A group: on every member.)"""
        self._call("set_transmission", int(bool(on)))

    def set_sky_sampling(self, on: bool = True):
        """True: the environment map is one more light of next event estimation, drawn by importance from a table the GPU builds at every
        scene hand-over (mirt.h, mirt_set_sky_sampling); the miss shader's share is MIS-weighted against it.  False (the default): the sky is
        met by extension rays only, as in the reference.  The same expectation with another variance: the accumulator is NOT reset.  No effect
        without ambient light, with mis=False or over a black map.  Not in exact stream order.  (A group: on every member.)"""
        self._call("set_sky_sampling", int(bool(on)))

    def set_ggx_pdf(self, on: bool = True):
        """True: wherever Closure<GGX> shades a hit its pdf is the visible-normal density (Heitz 2018 eq. 17; mirt.h, mirt_set_ggx_pdf) instead of
        the reference's 0 - in next event estimation's MIS weight, at an emitter the sampled ray hits and, under sky sampling, at the sky it
        misses into - so emitters and the sky are weighed two ways on GGX surfaces.  The closure sample, the roulette and the traversal read
        nothing new: rays, terminated and dropped do not change.  False (the default): the reference's 0.  No effect while no material ends up
        GGX.  Formally another estimator, and the accumulator is NOT reset: call Reset().  Not in exact stream order.  (A group: on every member.)"""
        self._call("set_ggx_pdf", int(bool(on)))

    def set_material_closures(self, closures=None):
        """closures[m] = 0 (Lambertian) or 1 (GGX) for material m, so that both kinds share a scene (mirt.h, mirt_set_material_closures); materials
        beyond the list take the policy's brdf.  None or an empty sequence removes the table (the default).  While every material of the scene
        ends up with one closure the kernels of that brdf run; otherwise the MIXED ones (material_closures() tells which).  Not in exact stream
        order.  Another estimand, and the accumulator is NOT reset: call Reset().  (A group: on every member.)"""
        t = _closure_table(closures)
        self._call("set_material_closures", _ptr(t) if len(t) else None, len(t))

    # -- getters: read from "the context to ask", self._asked() — a renderer's own, or member 0 of a group (its setters set every member alike) --
    def _get(self, name, *out):
        """mirt_get_<name> of the context to ask."""
        if getattr(self._lib, "mirt_get_" + name)(self._asked(), *out) < 0:
            raise MirtError(f"mirt_get_{name} failed")

    def material_closures(self):
        """(table, mixed): the table set_material_closures left, and whether the current scene's materials make the next launch a MIXED one."""
        out = np.zeros(MAX_MATERIALS, dtype=np.uint8)
        n, mixed = C.c_uint32(0), C.c_uint32(0)
        self._get("material_closures", _ptr(out), len(out), C.byref(n), C.byref(mixed))
        return [int(v) for v in out[: n.value]], bool(mixed.value)

    def lens(self):
        """(aperture_radius, focus_depth) in effect."""
        a, d = C.c_float(0), C.c_float(0)
        self._get("lens", C.byref(a), C.byref(d))
        return a.value, d.value

    # -- scene hand-over (Application.cpp:230-234) -------------------------------------------------
    def _hand_over_scene(self, nodes=None, prims=None):
        s = self.scene
        self.geometry = np.array(s.geometry, dtype=SPHERE, order="C")        # a copy of this object's own: update_spheres edits it, not the scene
        self.material = np.array(s.material, dtype=MATERIAL, order="C")      # likewise: update_materials edits it
        self.nodes, self.prims = bvh_build(self.geometry)
        if nodes is not None:
            self.nodes = np.ascontiguousarray(nodes, dtype=NODE)
        if prims is not None:
            self.prims = np.array(prims, dtype=SPHERE, order="C")
        self._bvh_of_geometry = geometry_to_bvh_order(self.geometry, self.prims)   # once per hand-over: what update_spheres addresses the BVH order with
        self.lights = light_list(self.geometry, self.material)
        hdri = np.ascontiguousarray(s.hdri, dtype=np.float32)
        amb = np.ascontiguousarray(s.ambient, dtype=np.float32)
        lights = self.lights if len(self.lights) else np.zeros(1, dtype=np.int32)
        self._call("set_scene", _ptr(self.geometry), _ptr(self.prims), len(self.geometry), _ptr(self.nodes), len(self.nodes),
                   _ptr(self.material), len(self.material), _ptr(lights), len(self.lights), _ptr(amb), _ptr(hdri), hdri.shape[1], hdri.shape[0])
        self._ambient = amb.reshape(-1).copy()             # what environment() reports: the library keeps it and has no getter for it
        self.UpdateCamera()

    # -- spheres moved in place (mirt.h "moving spheres in place") ------------------------------------------------------------------
    def update_spheres(self, indices, position=None, radius_sq=None):
        """The reference's SceneUpdate::Geometry for spheres that keep their place (mirt_update_spheres): geometry-order spheres `indices` (what an
        editor holds) take `position` [n, 3] and `radius_sq` [n]; None keeps each sphere's current value.  The traversal tree keeps its topology
        and gets new boxes on the GPU: no rebuild, no re-upload; the BVH order stays the one handed over.  Geometry is part of the estimand and
        the accumulator is NOT reset: call ResetAccumulator().  The temporal history is dropped unless set_history_motion() is on.  self.geometry and self.prims are edited in
        step; the scene object is not written: UpdateScene() hands its own geometry over again.  (A group: on every member.)"""
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        n_spheres = len(self.geometry)
        if len(idx) and (idx.min() < 0 or idx.max() >= n_spheres):
            raise ValueError(f"sphere index out of range: the scene has {n_spheres} spheres")
        g = idx.astype(np.uint32)
        packet = np.empty((len(g), 4), dtype=np.float32)
        packet[:, :3] = self.geometry["position"][g] if position is None else np.asarray(position, dtype=np.float32).reshape(len(g), 3)
        packet[:, 3] = self.geometry["radius_sq"][g] if radius_sq is None else np.asarray(radius_sq, dtype=np.float32).reshape(len(g))
        b = np.ascontiguousarray(self._bvh_of_geometry[g])
        self._call("update_spheres", len(g), _ptr(b) if len(g) else None, _ptr(g) if len(g) else None, _ptr(packet) if len(g) else None)
        for arr, at in ((self.geometry, g), (self.prims, b)):                # only an edit the library accepted becomes this object's
            arr["position"][at] = packet[:, :3]
            arr["radius_sq"][at] = packet[:, 3]

    # -- materials edited in place (mirt.h "updating materials in place") -----------------------------------------------------------
    def update_materials(self, materials=None, sphere_materials=None):
        """The reference's SceneUpdate::Material (mirt_update_materials).  `materials`: material index -> row of the MATERIAL dtype, as a mapping
        or a pair (indices, rows); `sphere_materials`: geometry-order sphere index -> material id, as a mapping or a pair (indices, ids).  Either
        may be None or empty.  No rebuild, no re-upload of the spheres: the material tables are replaced, the ids scattered and the light list
        regenerated on the GPU by the reference's rule; the camera-ray lists and the temporal history stay.  Materials are part of the estimand
        and the accumulator is NOT reset: call ResetAccumulator(), and drop_history() where one is kept.  self.material, self.geometry,
        self.prims and self.lights are edited in step; the scene object is not written.  (A group: on every member.)"""
        m_idx, m_rows = _index_value_pair(materials, MATERIAL, "materials")
        s_idx, s_ids = _index_value_pair(sphere_materials, np.int32, "sphere_materials")
        for what, idx, limit in (("material", m_idx, len(self.material)), ("sphere", s_idx, len(self.geometry))):
            if len(idx) and (idx.min() < 0 or idx.max() >= limit):
                raise ValueError(f"{what} index out of range: the scene has {limit}")
        mi, g = m_idx.astype(np.uint32), s_idx.astype(np.uint32)
        b = np.ascontiguousarray(self._bvh_of_geometry[g])
        opt = lambda a: _ptr(a) if len(a) else None
        self._call("update_materials", len(mi), opt(mi), opt(m_rows), len(g), opt(b), opt(g), opt(s_ids))
        self.material[mi] = m_rows                                             # only an edit the library accepted becomes this object's
        self.geometry["material_ID"][g] = s_ids
        self.prims["material_ID"][b] = s_ids
        self.lights = light_list(self.geometry, self.material)

    def lights_table(self) -> dict:
        """The two per-light tables next event estimation samples, read back from the device (mirt_debug_lights; a group: member 0's): "ids" [n]
        int32 geometry ids, "sphere" [n, 4] and "emit" [n, 4] float32 (emit[:, 3] holds the id's bits), "n_lights", and the compaction's shape
        "block" (spheres per workgroup) and "scan_pass" (workgroup totals per pass of the scan)."""
        info = (C.c_uint32 * 4)()
        ctx = self._asked()
        if self._lib.mirt_debug_lights(ctx, None, None, None, 0, info) < 0:
            raise MirtError("mirt_debug_lights failed: " + self._lib.mirt_last_error(ctx).decode())
        n = int(info[0])
        ids, sphere, emit = np.zeros(n, dtype=np.int32), np.zeros((n, 4), dtype=np.float32), np.zeros((n, 4), dtype=np.float32)
        if n and self._lib.mirt_debug_lights(ctx, _ptr(ids), _ptr(sphere), _ptr(emit), n, info) < 0:
            raise MirtError("mirt_debug_lights failed: " + self._lib.mirt_last_error(ctx).decode())
        return {"ids": ids, "sphere": sphere, "emit": emit, "n_lights": n, "block": int(info[1]), "scan_pass": int(info[2])}

    # -- the environment on its own (mirt.h "replacing the environment map on its own", "analytic sun and sky") -------------------
    sun_sky_defaults = staticmethod(sun_sky_defaults)

    def set_environment(self, ambient=None, hdri=None):
        """The reference's SceneUpdate::Ambient (mirt_set_environment): replaces the ambient colour (None: the scene's) and the environment map
        (`hdri` [h, w, 4] float32; None keeps the map in place) and nothing else — no tree rebuild, the camera-ray lists and the temporal history
        stay.  The environment is part of the estimand and the accumulator is NOT reset: call ResetAccumulator(), and drop_history() where one is
        kept.  The scene object is not written: UpdateScene() hands its own sky over again.  (A group: on every member.)"""
        amb = np.ascontiguousarray(self.scene.ambient if ambient is None else ambient, dtype=np.float32).reshape(-1)
        if amb.size != 3:
            raise ValueError("ambient must hold three floats")
        if hdri is None:
            self._call("set_environment", _ptr(amb), None, 0, 0)
        else:
            m = np.ascontiguousarray(hdri, dtype=np.float32)
            if m.ndim != 3 or m.shape[2] != 4:
                raise ValueError("hdri must be an array of shape (height, width, 4)")
            self._call("set_environment", _ptr(amb), _ptr(m), m.shape[1], m.shape[0])
        self._ambient = amb.copy()

    def set_sun_sky(self, **params):
        """A Preetham daylight sky and a sun disc, baked on the GPU into the environment map under the ambient colour in place (mirt_set_sun_sky);
        keywords: the fields of sun_sky_defaults() (sun_dir towards the sun with y up, turbidity 2..10, sun_radius, sky_scale, sun_scale, ground,
        width, height), each defaulting to that value.  Everything set_environment says holds.  (A group: every member bakes its own map.)"""
        self._call("set_sun_sky", C.byref(_sun_sky_params(params)))

    def environment(self):
        """(ambient, map [h, w, 4] float32, baked): the ambient colour last handed over by this object, the environment map the kernels read, copied
        from the device (a group: member 0's), and whether set_sun_sky baked it (mirt_read_environment)."""
        info = (C.c_uint32 * 4)()
        ctx = self._asked()
        if self._lib.mirt_read_environment(ctx, None, 0, info) < 0:
            raise MirtError("mirt_read_environment failed: " + self._lib.mirt_last_error(ctx).decode())
        m = np.zeros((info[1], info[0], 4), dtype=np.float32)
        if self._lib.mirt_read_environment(ctx, _ptr(m), m.size, info) < 0:
            raise MirtError("mirt_read_environment failed: " + self._lib.mirt_last_error(ctx).decode())
        return self._ambient.copy(), m, bool(info[2])

    def UpdateCamera(self):
        cam: Camera = self.scene.camera
        pos = np.ascontiguousarray(cam.pos, dtype=np.float32)
        ori = np.ascontiguousarray(cam.orient, dtype=np.float32)
        self._call("set_camera", _ptr(pos), _ptr(ori), float(cam.half_width), float(cam.half_height), float(cam.z), float(cam.exposure))
        if self._lens_follows_camera:                      # UpdateLens, Camera.hpp:21-26
            self.set_lens()

    # -- thin lens (mirt.h "thin lens") -------------------------------------------------------------
    def set_lens(self, aperture_radius=None, focus_depth=None):
        """Thin-lens depth of field: lens radius and axial depth of the plane of focus, both in world units; None = the scene camera's
        (focal_length / (2 f_number) / unit_mm, focus_distance).  aperture_radius = 0 is the pinhole path.  Does not reset the accumulator.
        (A group: on every member.)"""
        self._call("set_lens", *_lens_arguments(self.scene.camera, aperture_radius, focus_depth))

    def pick_focus(self, x: int, y: int):
        """The reference's right-click pick (Application.cpp:271-304): the un-jittered pinhole ray of pixel (x, y) -> (distance, depth);
        distance is inf on a miss, depth is the axial depth to hand to set_lens.  Changes no state.  (A group: on the first member.)"""
        dist, depth = C.c_float(0), C.c_float(0)
        self._call("pick_focus", int(x), int(y), C.byref(dist), C.byref(depth))
        return dist.value, depth.value

    # -- the reference interface ---------------------------------------------------------------
    def Resize(self, new_width: int, new_height: int):     # Renderer.hpp:53-63 (+ camera.Resize, Application.cpp:375-376)
        self.width, self.height = int(new_width), int(new_height)
        self.scene.camera.resize(self.width, self.height)
        self.UpdateCamera()
        self._call("resize", self.width, self.height)
        self.framebuffer = np.zeros((self.height, self.width, 4), dtype=np.float32)

    def ResetAccumulator(self):            # Renderer.hpp:64-67
        self._call("reset")

    def Accumulate(self, n_calls: int = 1):   # Renderer.hpp:73-434
        self._call("accumulate", n_calls)

    def AccumulateAsync(self, n_calls: int = 1):
        self._call("accumulate_async", n_calls)

    def Synchronize(self):
        self._call("synchronize")

    def Render(self) -> bool:              # Renderer.hpp:436-478; False = not a multiple of `buckets` yet, frame unchanged
        return self._call("render", _ptr(self.framebuffer)) == MIRT_OK

    def GetFrame(self) -> np.ndarray:      # Renderer.hpp:68 — RGBA32F rows, row 0 = y 0 (bottom on screen)
        return self.framebuffer

    # -- state access ------------------------------------------------------------------------------
    @property
    def accumulations(self) -> int:
        v = C.c_uint32(0)
        self._call("get_accumulations", C.byref(v))
        return v.value

    def _read_slab(self, what: str, *tile_shape) -> np.ndarray:
        """<what>_floats, then read_<what> -> [tile] + tile_shape f32."""
        n = C.c_size_t(0)
        self._call(what + "_floats", C.byref(n))
        out = np.empty(n.value, dtype=np.float32)
        self._call("read_" + what, _ptr(out))
        return out.reshape((n.value // int(np.prod(tile_shape)),) + tile_shape)      # (a context may own no tile at all)

    def _tiles(self) -> int:
        """Tiles of accumulator() and of noise()["tiles"]: the context's own, or the whole image's for a group."""
        n = C.c_size_t(0)
        self._call("accumulator_floats", C.byref(n))
        return n.value // (self.policy.buckets * 768)

    def accumulator(self) -> np.ndarray:
        """[local tile][bucket][rgb][256] f32 — AccumulationTile layout (Renderer.hpp:43-46).  A group: the whole image's slab in
        LaunchIndex order (gathers first)."""
        return self._read_slab("accumulator", self.policy.buckets, 3, 256)

    # -- first-hit AOVs (mirt.h "first-hit AOVs") ---------------------------------------------------------
    def set_aov(self, on: bool = True):
        """True: every accumulation also adds each camera ray's depth, normal and albedo into a slab beside the accumulator
        (the reference's compiled-out FIRST BOUNCE OUTPUTS, Renderer.hpp:216-231).  Only before the first accumulation; not in
        exact stream order.  False: frees the slab.  (A group: on every member.)"""
        self._call("set_aov", int(on))

    def aov(self) -> np.ndarray:
        """[local tile][plane][256] f32 sums over all accumulations: plane 0 depth, 1-3 normal, 4-6 albedo (F0 with brdf = 1).  A group: the
        whole image's sums in LaunchIndex order (gathers first)."""
        return self._read_slab("aov", AOV_PLANES, 256)

    def render_aov(self, which: int, out: np.ndarray = None):
        """One AOV (AOV_DEPTH, AOV_NORMAL, AOV_ALBEDO) resolved over the image, row 0 = y 0: depth (height, width), the others
        (height, width, 3); only this context's tiles are written (a group: the whole frame, gathered first).  None (and `out` untouched)
        before the first accumulation."""
        img = _aov_image(self.height, self.width, which, out)
        return img if self._call("render_aov", int(which), _ptr(img)) == MIRT_OK else None

    # -- denoised resolve (mirt.h "variance-guided à-trous denoised resolve") -----------------------------------
    denoise_defaults = staticmethod(denoise_defaults)

    def render_denoised(self, out: np.ndarray = None, **params):
        """The frame Render() resolves, filtered by an edge-avoiding à-trous wavelet that the first-hit AOVs and each pixel's own bucket variance
        guide (mirt_render_atrous): (height, width, 4) float32, ACES applied last, A = 1.  Keywords are the fields of mirt_denoise_params laid
        over denoise_defaults(): iterations, normal_squarings, demodulate, sigma_lum, sigma_depth, lum_floor, albedo_floor.  Needs AOVs on,
        buckets >= 2 and a context that owns the whole image (a group: gathers first).  None, and `out` untouched, while Render() would return
        False.  Changes no state."""
        shape = (self.height, self.width, 4)
        if out is None:
            out = np.zeros(shape, dtype=np.float32)
        elif out.dtype != np.float32 or out.shape != shape or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous float32 array of shape {shape}")
        p = _denoise_params(params)
        return out if self._call("render_atrous", C.byref(p), _ptr(out)) == MIRT_OK else None

    # -- temporal history (mirt.h "temporal history for the denoised resolve") ---------------------------------------
    temporal_defaults = staticmethod(temporal_defaults)

    def render_temporal(self, out: np.ndarray = None, want_len: bool = False, want_stats: bool = False, **params):
        """render_denoised() through a history that survives Reset() and camera moves (mirt_render_temporal): the last call's pre-filter result
        is reprojected through the first-hit depth into the current view, what fails the depth / normal test is rejected, the rest is blended
        with the new samples by sample count, and the à-trous passes run on the blend.  Keywords: those of render_denoised() plus max_ratio,
        depth_tol, normal_min, update (temporal_defaults()).  Returns the frame; with want_len / want_stats a tuple (frame[, history_len (height,
        width) f32][, stats dict: reprojected, no_history, outside, rejected, unusable]).  None, and nothing written, while Render() would
        return False.  The shading switches do not drop the history: after changing the estimand call drop_history().  (A group: on the
        gather context, after a gather.)"""
        shape = (self.height, self.width, 4)
        if out is None:
            out = np.zeros(shape, dtype=np.float32)
        elif out.dtype != np.float32 or out.shape != shape or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous float32 array of shape {shape}")
        dp, tp = _split_temporal_params(params)
        length = np.zeros(shape[:2], dtype=np.float32) if want_len else None
        st = TemporalStats()
        if self._call("render_temporal", C.byref(dp), C.byref(tp), _ptr(out), _ptr(length) if want_len else None, C.byref(st)) != MIRT_OK:
            return None
        extra = ([length] if want_len else []) + ([st.as_dict()] if want_stats else [])
        return (out, *extra) if extra else out

    def drop_history(self):
        """Forget the history of render_temporal() (mirt_drop_history); the next call starts from the frame's own samples."""
        self._call("drop_history")

    def set_history_motion(self, on: bool = True):
        """True: update_spheres() keeps the temporal history: it carries the id map and the sphere table it was taken under, and render_temporal()
        carries a moved sphere's pixels back to where the sphere was; a tap is taken only where the history shows the same sphere
        (mirt_set_sphere_motion).  False (the default): update_spheres() drops the history.  Any change drops it.  (A group: on every member.)"""
        self._call("set_sphere_motion", int(bool(on)))

    def history_motion(self) -> bool:
        """What set_history_motion left (a group: its members', which all hold the same)."""
        v = C.c_uint32(0)
        self._get("sphere_motion", C.byref(v))
        return bool(v.value)

    def id_map(self, order: str = "bvh"):
        """(prim, distance), each (height, width): per pixel of the whole image the sphere the un-jittered pinhole ray through the pixel centre
        meets first, -1 for none, and how far away, inf on a miss (mirt_id_map): pick_focus() for every pixel in one launch.  order="bvh": ids into
        self.prims, what hit.primID refers to; order="geometry": ids into self.geometry, what update_spheres() takes (translated on the host).
        Changes no state.  (A group: on the context render_temporal() resolves on.)"""
        if order not in ("bvh", "geometry"):
            raise ValueError(f"order must be 'bvh' or 'geometry', not {order!r}")
        prim = np.full((self.height, self.width), -1, dtype=np.int32)
        dist = np.zeros((self.height, self.width), dtype=np.float32)
        if prim.size:
            self._call("id_map", _ptr(prim), _ptr(dist))
        return (prim if order == "bvh" else id_map_to_geometry_order(prim, self._bvh_of_geometry)), dist

    def history_info(self) -> dict:
        """{"valid": a history is held, "bytes": device bytes of its images} (mirt_history_info)."""
        valid, nbytes = C.c_uint32(0), C.c_uint64(0)
        self._call("history_info", C.byref(valid), C.byref(nbytes))
        return {"valid": bool(valid.value), "bytes": int(nbytes.value)}

    # -- noise estimate (mirt.h "per-pixel noise estimate") ----------------------------------------------------
    noise_quantile = staticmethod(noise_quantile)

    def noise(self, floor: float = 0.0, want_map: bool = False, map_out: np.ndarray = None):
        """Per-pixel relative standard error of the mean of the bucket means (mirt_noise) -> {"owned_pixels", "finite_pixels",
        "nonfinite_pixels", "max", "mean", "tiles": (local tiles, 4) f32 {max, mean, usable, non-finite}, "hist": 2048 u32, "map": (height,
        width) f32 or None}; only this context's tiles of the map are written (into `map_out` when given).  None, and nothing written,
        while accumulations is 0 or not a multiple of `buckets`.  Changes no state.  A group: the whole image, without a gather — every
        member reads its own slab; "tiles" is in LaunchIndex order."""
        shape = (self.height, self.width)
        img = None
        if map_out is not None:
            if map_out.dtype != np.float32 or map_out.shape != shape or not map_out.flags.c_contiguous:
                raise ValueError(f"map_out must be a C-contiguous float32 array of shape {shape}")
            img = map_out
        elif want_map:
            img = np.zeros(shape, dtype=np.float32)
        tiles = np.zeros((self._tiles(), 4), dtype=np.float32)
        hist = np.zeros(NOISE_BINS, dtype=np.uint32)
        st = NoiseStats()
        rc = self._call("noise", float(np.float32(floor)), _ptr(img) if img is not None else None, _ptr(tiles) if len(tiles) else None, _ptr(hist), C.byref(st))
        if rc != MIRT_OK:
            return None
        return {**st.as_dict(), "tiles": tiles, "hist": hist, "map": img}

    def accumulate_until(self, target: float, quantile: float = 0.95, floor: float = 0.0, check_every: int = None, max_accumulations: int = 1000):
        """Accumulate `check_every` (default 4 x buckets) at a time until the `quantile` of the per-pixel noise is <= target and no pixel is
        non-finite, or `max_accumulations` is reached (mirt_accumulate_until) -> {"converged", "issued", and the stats of the last check}."""
        rule = StopRule(float(target), float(quantile), float(floor), int(check_every if check_every is not None else 4 * self.policy.buckets), int(max_accumulations))
        st, issued = NoiseStats(), C.c_uint32(0)
        rc = self._call("accumulate_until", C.byref(rule), C.byref(st), C.byref(issued))
        return {"converged": rc == MIRT_OK, "issued": issued.value, **st.as_dict()}

    # -- per-tile adaptive sampling (mirt.h "per-tile adaptive sampling") ----------------------------------------
    adaptive_select = staticmethod(adaptive_select)

    def freeze_tiles(self, mask):
        """Tiles (local order; a group: LaunchIndex order over the image) whose mask entry is non-zero take no more samples until the accumulator is reset or reloaded; there is no
        un-freeze.  Needs accumulations > 0 and a multiple of `buckets`."""
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).reshape(-1)
        self._call("freeze_tiles", _ptr(m) if len(m) else None, len(m))

    def frozen_tiles(self) -> np.ndarray:
        """1 for every frozen tile (a tile frozen at the current count has the count of an active one)."""
        out = np.zeros(self._tiles(), dtype=np.uint8)
        self._call("frozen_tiles", _ptr(out), len(out))
        return out

    def tile_counts(self) -> np.ndarray:
        """Samples per pixel of every local tile: `accumulations` for an active tile, the count it froze at for a frozen one."""
        out = np.zeros(self._tiles(), dtype=np.uint32)
        self._call("tile_counts", _ptr(out), len(out))
        return out

    def noise_above(self, target: float, floor: float = 0.0):
        """Per local tile, the usable pixels whose noise e exceeds `target` (mirt_tile_above); None while noise() would be."""
        out = np.zeros(self._tiles(), dtype=np.uint32)
        rc = self._call("tile_above", float(np.float32(floor)), float(np.float32(target)), _ptr(out), len(out))
        return out if rc == MIRT_OK else None

    def accumulate_adaptive(self, target: float, quantile: float = 0.95, floor: float = 0.0, check_every: int = None, min_accumulations: int = 0,
                            max_accumulations: int = 1000):
        """Accumulate `check_every` (default 4 x buckets) at a time; after each step, once `min_accumulations` is reached, freeze the tiles
        whose `quantile` of the per-pixel noise is <= target (adaptive_select).  Ends when every tile is frozen or at `max_accumulations`
        (mirt_accumulate_adaptive) -> {"converged", "issued", "checks", "frozen_tiles", "owned_tiles", "tile_accumulations", and the stats of
        the last check}.  Stopping on an estimate made from the same samples biases dark; `min_accumulations` is the guard."""
        rule = StopRule(float(target), float(quantile), float(floor), int(check_every if check_every is not None else 4 * self.policy.buckets), int(max_accumulations))
        rep = AdaptiveReport()
        rc = self._call("accumulate_adaptive", C.byref(rule), int(min_accumulations), C.byref(rep))
        return {"converged": rc == MIRT_OK, "issued": int(rep.issued), "checks": int(rep.checks), "frozen_tiles": int(rep.frozen_tiles), "owned_tiles": int(rep.owned_tiles),
                "tile_accumulations": int(rep.tile_accumulations), **rep.last.as_dict()}

    def counters(self) -> dict:
        c = Counters()
        self._call("get_counters", C.byref(c))
        return c.as_dict()


def _switch_getter(name, kind):
    def get(self):
        v = C.c_uint32(0)
        self._get(name, C.byref(v))
        return kind(v.value)
    get.__name__, get.__qualname__, get.__doc__ = name, "_Binding." + name, f"What set_{name} left (a group: its members', which all hold the same)."
    return get


for _name, _kind, _ in _SWITCHES:                          # light_ris() -> int, transmission() -> bool, ...; the table's getter is material_closures()
    if _kind is not list:
        setattr(_Binding, _name, _switch_getter(_name, _kind))


class Renderer(_Binding):
    """Mirror of the reference's ``Renderer<Policy>`` (Renderer.hpp:28-68) over the C-ABI.

    ``Renderer(scene)`` keeps a reference to the scene like the original; call ``UpdateScene`` after
    editing it (the reference rebuilds BVH + light list and resets, Application.cpp:508-510).
    """
    _prefix, _handle = "mirt_", "_ctx"

    def __init__(self, scene: Scene, device: int = 0, max_bounces: int = 16, buckets: int = 5, mis: bool = True,
                 use_bvh: bool = False, count_traffic: bool = False, profile: bool = False, max_batch: int = 0,
                 allow_half_boxes: bool = True, reference_tree: bool = False, streams: int = 0, gpu_build: bool = False, trace_primary_rays: bool = False,
                 brdf: int = 0, gloss_decay=None, exact_stream_order: bool = False, aov: bool = False, lens: bool = False, light_ris: int = 0,
                 transmission: bool = False, sky_sampling: bool = False, material_closures=None, ggx_pdf: bool = False):
        if material_closures is not None:
            _closure_table(material_closures)           # a bad table is refused before the library is loaded or a device touched
        self._lib = load_library()
        self._ctx = C.c_void_p()
        self._lens_follows_camera = bool(lens)          # lens=True: the scene camera's f_number / focus_distance / unit_mm drive a thin lens
        rc = self._lib.mirt_create(device, C.byref(self._ctx))
        if rc != MIRT_OK:
            raise MirtError(f"mirt_create failed ({rc}): {self._lib.mirt_last_error(None).decode()}")
        self.scene = scene
        self.width = self.height = 0
        self.framebuffer = None
        self.policy = Policy(max_bounces, buckets, int(mis), int(use_bvh), int(count_traffic), int(profile), max_batch, int(reference_tree), int(streams), int(gpu_build), int(trace_primary_rays),
                             int(brdf))
        self._call("set_policy", C.byref(self.policy))
        self._call("debug_allow_half_boxes", int(allow_half_boxes))
        self._configure(gloss_decay=gloss_decay, exact_stream_order=exact_stream_order, aov=aov, light_ris=light_ris, transmission=transmission,
                        sky_sampling=sky_sampling, material_closures=material_closures, ggx_pdf=ggx_pdf)

    def _asked(self):
        return self._ctx

    def load_tile_counts(self, counts):
        """After load_accumulator: per-tile counts (positive multiples of `buckets`, at most accumulations); tiles below it are frozen."""
        a = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        self._call("load_tile_counts", _ptr(a) if len(a) else None, len(a))

    def get_policy(self) -> dict:
        """The policy in effect (max_batch / streams resolved where they were left at 0 = auto)."""
        p = Policy()
        self._call("get_policy", C.byref(p))
        return {name: int(getattr(p, name)) for name, _ in Policy._fields_ if not name.startswith("_")}

    @property
    def stream_order(self) -> int:
        v = C.c_uint32(0)
        self._call("get_stream_order", C.byref(v))
        return v.value

    def UpdateScene(self, nodes=None, prims=None):
        """Hands the scene over again (after an edit).  `nodes`: a caller-made tree over the reference-order prims instead of the
        reference builder's (BVH.hpp:18-31 layout, children at first_id / first_id+1, leaves first_id..first_id+prim_count-1).
        `prims`: a caller-made BVH-order array (a permutation of the geometry's rows) instead of the reference builder's."""
        self._hand_over_scene(nodes, prims)

    @staticmethod
    def RequiredTiling() -> int:          # Renderer.hpp:36
        return 16

    # -- sharding / state access -------------------------------------------------------------------
    def SetTileRange(self, first_tile: int, n_tiles: int):
        self._call("set_tile_range", first_tile, n_tiles)

    def SetTileRows(self, first_row: int, row_stride: int):
        """Multi-GPU sharding by interleaved tile rows: this context renders tile rows first_row, first_row + row_stride, ..."""
        self._call("set_tile_rows", first_row, row_stride)

    def accumulator_device(self):
        p, b = C.c_void_p(), C.c_size_t(0)
        self._call("accumulator_device", C.byref(p), C.byref(b))
        return p.value, b.value

    def load_accumulator(self, src, accumulations: int, is_device: bool = False):
        ptr = C.c_void_p(src) if is_device else _ptr(np.ascontiguousarray(src, dtype=np.float32))
        self._call("load_accumulator", ptr, int(is_device), accumulations)

    @property
    def aov_enabled(self) -> bool:
        v = C.c_uint32(0)
        self._call("get_aov", C.byref(v))
        return bool(v.value)

    def aov_device(self):
        p, b = C.c_void_p(), C.c_size_t(0)
        self._call("aov_device", C.byref(p), C.byref(b))
        return p.value, b.value

    def load_aov(self, src, is_device: bool = False):
        ptr = C.c_void_p(src) if is_device else _ptr(np.ascontiguousarray(src, dtype=np.float32))
        self._call("load_aov", ptr, int(is_device))

    def kernel_times(self, reset: bool = True) -> dict:
        t = KernelTimes()
        self._call("get_kernel_times", C.byref(t), int(reset))
        return {k: {"ms": t.ms[i], "launches": int(t.launches[i])} for i, k in enumerate(KERNEL_CLASSES)}

    def debug_info(self) -> dict:
        out = (C.c_uint32 * 8)()
        self._call("debug_info", out)
        keys = ("records", "lds_records", "lds_spheres", "depth", "half_boxes", "trace_lds_bytes", "trace_workgroups_per_cu", "cus")
        d = dict(zip(keys, [int(v) for v in out]))
        d["wide"] = (d["half_boxes"] >> 1) & 1             # 64-B binary16 records of up to four children
        d["half_boxes"] &= 1
        return d

    def debug_tree(self):
        """The records the trace kernels walk, read back from the device: (uint32 words shaped [records, words per record],
        {"records", "record_bytes", "layout" (0 f32 child pairs, 1 binary16 child pairs, 2 4-wide binary16), "depth"})."""
        info = (C.c_uint32 * 4)()
        self._call("debug_tree", None, 0, info)
        n, rec_bytes = int(info[0]), int(info[1])
        words = np.zeros((n, rec_bytes // 4), dtype=np.uint32)
        self._call("debug_tree", _ptr(words), words.nbytes, info)
        return words, dict(zip(("records", "record_bytes", "layout", "depth"), [int(v) for v in info]))

    def debug_sky_table(self) -> dict:
        """The sky sampling table (set_sky_sampling), read back from the device as float32 arrays: "marg" [rows] and "rowsum" [rows], the cell
        edges "tn" and "ts" [rows + 1] (1 - sin el, 1 + sin el), "cond" and "dens" [rows, cols]; "rows", "cols" and "total" (np.float32)."""
        info = (C.c_uint32 * 4)()
        self._call("debug_sky_table", None, 0, info)
        rows, cols, n = int(info[0]), int(info[1]), int(info[3])
        t = np.zeros(n, dtype=np.float32)
        self._call("debug_sky_table", _ptr(t), n, info)
        o = [0, rows, 2 * rows, 3 * rows + 1, 4 * rows + 2, 4 * rows + 2 + rows * cols, n]
        return {"rows": rows, "cols": cols, "total": np.array([info[2]], dtype=np.uint32).view(np.float32)[0], "words": t,
                "marg": t[o[0]:o[1]], "rowsum": t[o[1]:o[2]], "tn": t[o[2]:o[3]], "ts": t[o[3]:o[4]],
                "cond": t[o[4]:o[5]].reshape(rows, cols), "dens": t[o[5]:o[6]].reshape(rows, cols)}

    def debug_primary_lists(self) -> list:
        """hist[n] = pixels whose candidate list holds n spheres (n = 0..7), hist[8] = 8 or more, hist[9] = pixels without a list."""
        out = (C.c_uint32 * 10)()
        self._call("debug_primary_lists", out)
        return [int(v) for v in out]

    def debug_primary_counts(self) -> np.ndarray:
        """[local tile][256] uint32: the length of every local pixel's candidate list; 0xffffffff = a pixel without a list."""
        out = np.zeros((self._tiles(), 256), dtype=np.uint32)
        self._call("debug_primary_counts", _ptr(out), out.size)
        return out

    def stream_handle(self) -> int:
        p = C.c_void_p()
        self._call("get_stream", C.byref(p))
        return p.value

    # -- stage-level (parity tests) ---------------------------------------------------------------
    def debug_raygen(self, accumulations: int):
        n = (self.width // 16) * (self.height // 16) * 256
        p = np.empty((3, n), dtype=np.float32)
        d = np.empty((3, n), dtype=np.float32)
        self._call("debug_raygen", accumulations, _ptr(p), _ptr(d))
        return p, d

    def debug_trace_closest(self, p: np.ndarray, d: np.ndarray):
        p = np.ascontiguousarray(p, dtype=np.float32); d = np.ascontiguousarray(d, dtype=np.float32)
        n = p.shape[1]
        tfar = np.empty(n, dtype=np.float32); prim = np.empty(n, dtype=np.int32)
        self._call("debug_trace_closest", n, _ptr(p), _ptr(d), _ptr(tfar), _ptr(prim))
        return tfar, prim

    def debug_trace_shadow(self, p: np.ndarray, d: np.ndarray, tfar: np.ndarray):
        p = np.ascontiguousarray(p, dtype=np.float32); d = np.ascontiguousarray(d, dtype=np.float32)
        tfar = np.ascontiguousarray(tfar, dtype=np.float32)
        n = p.shape[1]
        occ = np.empty(n, dtype=np.uint8)
        self._call("debug_trace_shadow", n, _ptr(p), _ptr(d), _ptr(tfar), _ptr(occ))
        return occ

    def debug_math(self, fn: int, inputs: np.ndarray, n_out: int) -> np.ndarray:
        inputs = np.ascontiguousarray(inputs, dtype=np.float32)
        n = inputs.shape[-1]
        out = np.empty((n_out, n), dtype=np.float32)
        self._call("debug_math", fn, n, _ptr(inputs), _ptr(out))
        return out


class GroupRenderer(_Binding):
    """The same `Renderer<Policy>` interface on several GPUs of one node, driven by this one process through the library's
    mirt_group_* entry points (include/mirt.h): scene replicated, tile rows interleaved over the devices, one RCCL gather of the
    accumulator slabs to devices[0] when a frame or the accumulator is read.  `devices` may repeat a device (rehearsal on a
    one-GPU box; slabs then move with device copies)."""
    _prefix, _handle = "mirt_group_", "_g"

    def __init__(self, scene: Scene, devices=(0,), max_bounces: int = 16, buckets: int = 5, mis: bool = True, use_bvh: bool = True,
                 count_traffic: bool = False, max_batch: int = 0, streams: int = 0, reference_tree: bool = False, gpu_build: bool = False,
                 brdf: int = 0, gloss_decay=None, exact_stream_order: bool = False, aov: bool = False, lens: bool = False, light_ris: int = 0,
                 transmission: bool = False, sky_sampling: bool = False, material_closures=None, ggx_pdf: bool = False):
        if material_closures is not None:
            _closure_table(material_closures)           # a bad table is refused before the library is loaded or a device touched
        self._lib = load_library()
        self._g = C.c_void_p()
        self._lens_follows_camera = bool(lens)
        dev = (C.c_int * len(devices))(*devices)
        rc = self._lib.mirt_group_create(dev, len(devices), C.byref(self._g))
        if rc != MIRT_OK:
            raise MirtError(f"mirt_group_create failed ({rc}): {self._lib.mirt_group_last_error(None).decode()}")
        self.scene, self.devices = scene, tuple(devices)
        self.width = self.height = 0
        self.framebuffer = None
        self.policy = Policy(max_bounces, buckets, int(mis), int(use_bvh), int(count_traffic), 0, max_batch, int(reference_tree), int(streams), int(gpu_build), 0,
                             int(brdf))
        self._call("set_policy", C.byref(self.policy))
        self._configure(gloss_decay=gloss_decay, exact_stream_order=exact_stream_order, aov=aov, light_ris=light_ris, transmission=transmission,
                        sky_sampling=sky_sampling, material_closures=material_closures, ggx_pdf=ggx_pdf)

    def _asked(self):
        ctx = C.c_void_p()
        self._call("member", 0, C.byref(ctx))
        return ctx

    def UpdateScene(self):
        self._hand_over_scene()

    read_aov = _Binding.aov

    def Gather(self):
        """The one exchange of the path: every member's accumulator slab to devices[0] (implied by accumulator() and Render())."""
        self._call("gather")

    def gather_ms(self) -> float:
        v = C.c_double(0.0)
        self._call("last_gather_ms", C.byref(v))
        return v.value


def rccl_selftest(device: int = 0, n_floats: int = 1 << 20) -> None:
    """mirt_group_rccl_selftest: raises if librccl cannot be loaded or a grouped ncclSend / ncclRecv on `device` does not deliver."""
    lib = load_library()
    rc = lib.mirt_group_rccl_selftest(device, n_floats)
    if rc != MIRT_OK:
        raise MirtError(f"RCCL self-test failed ({rc}): {lib.mirt_group_last_error(None).decode()}")
