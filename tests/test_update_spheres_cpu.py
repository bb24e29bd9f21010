"""mirt_update_spheres without a GPU: the geometry-to-BVH-order helper of the Python binding, the host-only argument rules and light-table patch
(csrc/scene_update_host.hpp) under sanitizers in a stand-alone program, and the interface at every layer."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("mirt_update_spheres", "mirt_group_update_spheres")


def spheres(mirt, position, radius_sq, material=0):
    s = np.zeros(len(radius_sq), dtype=mirt.scene.SPHERE)
    s["position"], s["radius_sq"], s["material_ID"] = position, radius_sq, material
    return s


# ---- the permutation helper ------------------------------------------------------------------------------------------------------
def test_order_of_a_shuffled_thousand(mirt):
    rng = np.random.default_rng(7)
    g = spheres(mirt, rng.normal(size=(1000, 3)), rng.uniform(0.1, 2.0, 1000), rng.integers(0, 4, 1000))
    shuffle = rng.permutation(1000)
    prims = g[shuffle]                                            # prims[b] = g[shuffle[b]]
    perm = mirt.geometry_to_bvh_order(g, prims)
    assert perm.dtype == np.uint32 and perm.shape == (1000,)
    assert np.array_equal(np.sort(perm), np.arange(1000))
    assert prims[perm].tobytes() == g.tobytes()
    assert np.array_equal(shuffle[perm], np.arange(1000))         # rows are distinct: the one bijection


def test_order_of_the_reference_builder(mirt):
    for sc in (mirt.scene.default9(), mirt.scene.synthetic(1000)):
        g = np.ascontiguousarray(sc.geometry, dtype=mirt.scene.SPHERE)
        _, prims = mirt.bvh_build(g)
        perm = mirt.geometry_to_bvh_order(g, prims)
        assert np.array_equal(np.sort(perm), np.arange(len(g))) and prims[perm].tobytes() == g.tobytes()


def test_order_with_duplicate_rows_and_a_single_sphere(mirt):
    g = spheres(mirt, [(0, 0, 0), (1, 1, 1), (0, 0, 0), (2, 2, 2), (0, 0, 0), (1, 1, 1)], [1, 4, 1, 9, 1, 4])
    prims = g[[3, 0, 5, 2, 1, 4]]
    perm = mirt.geometry_to_bvh_order(g, prims)
    assert np.array_equal(np.sort(perm), np.arange(6))            # a bijection, although rows repeat
    assert prims[perm].tobytes() == g.tobytes()
    one = spheres(mirt, [(3, 4, 5)], [2.0])
    assert np.array_equal(mirt.geometry_to_bvh_order(one, one.copy()), [0])
    assert mirt.geometry_to_bvh_order(g[:0], g[:0]).shape == (0,)
    # -0.0 and 0.0 are different rows; rows that differ in the material differ
    other = g.copy(); other["material_ID"][3] = 1
    with pytest.raises(ValueError):
        mirt.geometry_to_bvh_order(g, other)
    with pytest.raises(ValueError):
        mirt.geometry_to_bvh_order(g, prims[:5])
    with pytest.raises(ValueError):
        mirt.geometry_to_bvh_order(g, g[[0, 0, 1, 2, 3, 4]])      # same multiset of distinct rows, other multiplicities


# ---- host code under sanitizers ----------------------------------------------------------------------------------------------------
def test_host_code_under_sanitizers(tmp_path):
    """csrc/scene_update_host.hpp with its own main (tests/native/scene_update_check.cpp) under -fsanitize=address,undefined: every refusal of
    mirt.h with its code, arguments before layout, and the light table patched by both search strategies.  Nothing here is loaded into Python."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "scene_update_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "native", "scene_update_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1] == "done"
    lines = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines() if " " in line)
    rc = {k: int(re.match(r"rc=(-?\d+)", v).group(1)) for k, v in lines.items() if v.startswith("rc=")}
    OK, ARG, STATE = 0, -1, -3                                                   # as mirt.h numbers them (checked against the header below)
    want = {"ok": OK, "ok_half": OK, "empty": OK, "null_bvh": ARG, "null_geometry": ARG, "null_values": ARG, "no_spheres": ARG, "bvh_range": ARG,
            "geometry_range": ARG, "bvh_twice": ARG, "geometry_twice": ARG, "nan_centre": ARG, "inf_centre": ARG, "inf_radius": ARG, "negative_radius": ARG,
            "zero_radius_f32": OK, "zero_radius_half": STATE, "far_f32": OK, "far_half": STATE, "thin_f32": OK, "thin_half": STATE, "thick_half": OK,
            "arg_before_state": ARG}
    assert rc == want
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    assert re.search(r"#define MIRT_ERR_ARG\s+-1\b", header) and re.search(r"#define MIRT_ERR_STATE\s+-3\b", header)
    for k in ("zero_radius_half", "far_half", "thin_half"):
        assert "mirt_set_scene" in lines[k], lines[k]
    assert "occurs twice" in lines["bvh_twice"] and "occurs twice" in lines["geometry_twice"]
    patched = "patched=2 0 1 2 3 -1 -1 -1 -1 0 1 2 3 -1 -1 -1 -1"            # lights 5, 1, 5, 9 with sphere 5 edited: rows 0 and 2
    assert lines["lights_2"] == patched and lines["lights_2000"] == patched and lines["lights_none"] == "patched=0"


# ---- interface -----------------------------------------------------------------------------------------------------------------
def test_update_spheres_is_declared_at_every_layer(mirt):
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    declared = set(re.findall(r"^int\s+(mirt_\w+)\s*\(", header, flags=re.M))
    lib = mirt.load_library()
    raw = C.CDLL(mirt.LIB_PATH)
    for n in NEW_NAMES:
        assert n in declared, f"{n} is not declared in include/mirt.h"
        assert hasattr(raw, n), f"{n} is not exported by libmirt.so"
        assert n in lib._declared, f"{n} is not bound in Python"
    for text in ("moving spheres in place", "THE CALLER'S BVH ORDER IS KEPT", "the accumulator is NOT reset", "a refit does not change layouts", "occurs twice in one call"):
        assert text in header, text
    for cls in (mirt.Renderer, mirt.GroupRenderer):
        assert list(inspect.signature(cls.update_spheres).parameters)[1:] == ["indices", "position", "radius_sq"]
    assert list(inspect.signature(mirt.Renderer.UpdateScene).parameters)[1:] == ["nodes", "prims"]
    assert inspect.signature(mirt.Renderer.UpdateScene).parameters["prims"].default is None
    host = open(os.path.join(mirt.CSRC, "mirt_host.hpp")).read()
    assert "void UpdateSpheres(" in host and "mirt_group_update_spheres(" in host
    headless = open(os.path.join(mirt.CSRC, "mirt_headless.cpp")).read()
    assert '"--move-sphere"' in headless
    launch, capi = open(os.path.join(mirt.CSRC, "mirt_launch.hip")).read(), open(os.path.join(mirt.CSRC, "mirt_capi.hip")).read()
    assert '#include "refit.hpp"' in launch and '#include "scene_update_host.hpp"' in capi
    # the leaf box is stated once on the device and shared by the builder and the refit
    for name in ("lbvh_build.hip", "refit.hpp"):
        text = open(os.path.join(mirt.CSRC, name)).read()
        assert "sphere_leaf_box(" in text and "kPadRel *" not in text, name


def test_help_names_the_flag_and_its_entry_point(mirt):
    exe = os.path.join(mirt.CSRC, "mirt_headless")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", mirt.CSRC, "mirt_headless"], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = subprocess.run([exe, "--help"], capture_output=True, text=True, check=True, timeout=60).stdout
    lines = [line for line in text.splitlines() if line.strip().startswith("--move-sphere")]
    assert lines and "mirt_update_spheres" in lines[0], lines
