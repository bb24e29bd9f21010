"""mirt_update_materials without a GPU: the host-only argument rules, the glass rule and the per-material emit mask
(csrc/scene_update_host.hpp) under sanitizers in a stand-alone program, the mask against mirt_light_list, the Python argument handling,
and the interface at every layer."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("mirt_update_materials", "mirt_group_update_materials", "mirt_debug_lights")
f32 = np.float32


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/native/material_update_check.cpp under -fsanitize=address,undefined.  Nothing here is loaded into Python."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("native") / "material_update_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "native", "material_update_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


# ---- the host check ------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_host_check(checker):
    out = subprocess.run([checker], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "done"
    lines = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines() if " " in line)
    rc = {k: int(re.match(r"rc=(-?\d+)", v).group(1)) for k, v in lines.items()}
    OK, ARG = 0, -1                                                              # as mirt.h numbers them (checked against the header below)
    want = {"ok": OK, "ok_rows_only": OK, "ok_assign_only": OK, "empty": OK,
            "null_material_index": ARG, "null_rows": ARG, "null_bvh": ARG, "null_geometry": ARG, "null_ids": ARG,
            "material_range": ARG, "material_twice": ARG, "bvh_range": ARG, "geometry_range": ARG, "bvh_twice": ARG, "geometry_twice": ARG,
            "id_range": ARG, "id_negative": ARG, "no_spheres_rows": OK, "no_spheres_assign": ARG, "good_rows_bad_assign": ARG,
            # the glass rule: of the resulting table, and only with mirt_set_transmission on
            "transmission_range_on": ARG, "transmission_range_off": OK, "transmission_nan_on": ARG, "ior_on": ARG, "ior_off": OK, "ior_nan_on": ARG,
            "ior_of_an_opaque_row_on": OK, "new_glass_on": OK, "glass_removed_on": OK, "assign_only_on": OK, "glass_rows": ARG}
    assert rc == want
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    assert re.search(r"#define MIRT_ERR_ARG\s+-1\b", header) and re.search(r"#define MIRT_ERR_STATE\s+-3\b", header)
    for k in ("material_twice", "bvh_twice", "geometry_twice"):
        assert "occurs twice" in lines[k], lines[k]
    assert "material_index[1] = 4" in lines["material_range"] and "cannot change" in lines["material_range"]
    assert "material_ID[1] = 4" in lines["id_range"] and "material_ID[1] = -1" in lines["id_negative"] and "material_ID[1] = 9" in lines["good_rows_bad_assign"]
    assert "transmission[0]" in lines["transmission_range_on"] and "IOR_minus_one" in lines["ior_on"] and "IOR_minus_one" in lines["glass_rows"]
    for k in ("null_material_index", "null_rows", "null_bvh", "null_geometry", "null_ids"):
        assert "NULL" in lines[k], lines[k]


# ---- the emit mask ---------------------------------------------------------------------------------------------------------------------
# What the shared expression, (e0 e0 + e1 e1) + e2 e2 > 0 in binary32, says — and both mirt_light_list and the mask are held to it:
#   squares that all underflow to 0 (|e| < 2^-75): NOT a light;   a negative component: a light (its square is positive);
#   a NaN component: NOT a light (no comparison with a NaN holds); an infinite one: a light (inf > 0).
EMISSIONS = [((0.0, 0.0, 0.0), False), ((1.0, 0.0, 0.0), True), ((0.0, 0.0, 20.0), True), ((-0.0, 0.0, 0.0), False),
             ((1e-30, 1e-30, 1e-30), False), ((0.0, 1e-23, 0.0), False), ((0.0, 1e-22, 0.0), True), ((1e-20, 0.0, 0.0), True),
             ((-3.0, 0.0, 0.0), True), ((-1.0, -1.0, -1.0), True), ((-1e-30, 0.0, 0.0), False),
             ((float("nan"), 0.0, 0.0), False), ((1.0, float("nan"), 1.0), False), ((float("inf"), 0.0, 0.0), True), ((float("-inf"), 1.0, 0.0), True),
             ((float("inf"), float("nan"), 0.0), False), ((3e38, 3e38, 0.0), True)]


def test_the_emit_mask_is_what_light_list_decides(mirt, checker):
    mats = np.zeros(len(EMISSIONS), dtype=mirt.scene.MATERIAL)
    mats["emission"] = np.array([e for e, _ in EMISSIONS], dtype=f32)
    geo = np.zeros(len(mats), dtype=mirt.scene.SPHERE)                           # sphere m has material m
    geo["radius_sq"], geo["material_ID"] = 1.0, np.arange(len(mats))
    lights = mirt.light_list(geo, mats)
    args = [f"{w:08x}" for w in mats["emission"].view(np.uint32).reshape(-1)]
    out = subprocess.run([checker] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    mask = int(re.match(r"mask=([0-9a-f]+)", out.stdout.strip()).group(1), 16)
    from_mask = [m for m in range(len(mats)) if (mask >> m) & 1]
    assert from_mask == list(lights), (from_mask, list(lights))
    assert from_mask == [m for m, (_, emits) in enumerate(EMISSIONS) if emits]   # the documented answers
    # 63 materials, the most a scene holds: the top bit of the mask
    many = ["00000000"] * (3 * 62) + ["3f800000", "00000000", "00000000"]
    out = subprocess.run([checker] + many, capture_output=True, text=True, timeout=120)
    assert out.stdout.strip() == f"mask={1 << 62:x}"
    # one statement of the rule
    build = open(os.path.join(mirt.CSRC, "bvh_build.cpp")).read()
    host = open(os.path.join(mirt.CSRC, "scene_update_host.hpp")).read()
    assert "mirt_host::emits(" in build and "mirt_host::emits(" in host and "e[0] * e[0]" not in build


# ---- the Python argument handling --------------------------------------------------------------------------------------------------------
def test_mapping_and_arrays_and_empty_halves(mirt):
    pair = mirt._index_value_pair
    M = mirt.scene.MATERIAL
    mats = np.zeros(4, dtype=M)
    mats["albedo"] = np.arange(12).reshape(4, 3)
    for empty in (None, {}, ([], []), (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=M))):
        idx, val = pair(empty, M, "materials")
        assert idx.shape == (0,) and val.shape == (0,) and val.dtype == M
    idx, val = pair({3: mats[3], 1: mats[1]}, M, "materials")                     # a mapping keeps its order
    assert list(idx) == [3, 1] and val.dtype == M and val.tobytes() == mats[[3, 1]].tobytes() and val.flags.c_contiguous
    idx2, val2 = pair(([3, 1], mats[[3, 1]]), M, "materials")                    # the same as arrays
    assert list(idx2) == [3, 1] and val2.tobytes() == val.tobytes()
    idx3, val3 = pair(([2], [tuple(mats[2])]), M, "materials")                   # a row field by field
    assert val3.tobytes() == mats[[2]].tobytes()
    idx, val = pair({7: 2, 5: np.int32(0)}, np.int32, "sphere_materials")
    assert list(idx) == [7, 5] and val.dtype == np.int32 and list(val) == [2, 0]
    idx, val = pair((np.array([7, 5], dtype=np.uint32), np.array([2, 0], dtype=np.int64)), np.int32, "sphere_materials")
    assert idx.dtype == np.int64 and val.dtype == np.int32 and list(val) == [2, 0]
    with pytest.raises(ValueError):
        pair(([1, 2], [0]), np.int32, "sphere_materials")                        # one value per index
    with pytest.raises(ValueError):
        pair(5, np.int32, "sphere_materials")
    for cls in (mirt.Renderer, mirt.GroupRenderer):
        sig = inspect.signature(cls.update_materials)
        assert list(sig.parameters)[1:] == ["materials", "sphere_materials"] and all(p.default is None for p in list(sig.parameters.values())[1:])
        assert list(inspect.signature(cls.lights_table).parameters) == ["self"]


# ---- interface -----------------------------------------------------------------------------------------------------------------------
def test_update_materials_is_declared_at_every_layer(mirt):
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    declared = set(re.findall(r"^int\s+(mirt_\w+)\s*\(", header, flags=re.M))
    lib = mirt.load_library()
    raw = C.CDLL(mirt.LIB_PATH)
    for n in NEW_NAMES:
        assert n in declared, f"{n} is not declared in include/mirt.h"
        assert hasattr(raw, n), f"{n} is not exported by libmirt.so"
        assert n in lib._declared, f"{n} is not bound in Python"
    for text in ("updating materials in place", "THE LIGHT LIST IS ALWAYS REPLACED BY", "the accumulator is NOT reset", "THE NUMBER OF MATERIALS CANNOT CHANGE",
                 "KEPT: the temporal history", "a refused call leaves every word in place"):
        assert text in header, text
    host = open(os.path.join(mirt.CSRC, "mirt_host.hpp")).read()
    assert "void UpdateMaterials(" in host and "mirt_group_update_materials(" in host
    headless = open(os.path.join(mirt.CSRC, "mirt_headless.cpp")).read()
    assert '"--set-emission"' in headless and '"--sphere-material"' in headless
    launch, capi = open(os.path.join(mirt.CSRC, "mirt_launch.hip")).read(), open(os.path.join(mirt.CSRC, "mirt_capi.hip")).read()
    assert '#include "light_list.hpp"' in launch and "check_materials(" in capi
    kernels = open(os.path.join(mirt.CSRC, "light_list.hpp")).read()
    for name in ("k_assign_materials", "k_light_count", "k_light_scan", "k_light_scatter", "__ballot(", "__popcll("):
        assert name in kernels, name
    assert "atomic" not in kernels.split("#pragma once")[1]                      # no atomic decides a position


def test_help_names_the_flags_and_their_entry_point(mirt):
    exe = os.path.join(mirt.CSRC, "mirt_headless")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", mirt.CSRC, "mirt_headless"], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = subprocess.run([exe, "--help"], capture_output=True, text=True, check=True, timeout=60).stdout
    for flag in ("--set-emission", "--sphere-material"):
        lines = [line for line in text.splitlines() if line.strip().startswith(flag)]
        assert lines and "mirt_update_materials" in lines[0], (flag, lines)
