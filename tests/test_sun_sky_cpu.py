"""The analytic sun and sky and the environment update without a GPU: the interface at every layer, the refusals that need no context, the
defaults, the float64 definition's own properties, the binary32 twin against it within the derived bound, and the host
code under sanitizers in a stand-alone program."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sky_definitions as sd
import sun_sky_definitions as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
MIRT_ERR_ARG = -1
NEW_NAMES = ("mirt_set_environment", "mirt_read_environment", "mirt_sun_sky_defaults", "mirt_set_sun_sky", "mirt_group_set_environment", "mirt_group_set_sun_sky")
# the sweep of the issue: three map sizes, the sun at the zenith, at 35 degrees and on the horizon, both ends of the turbidity range, with and
# without the disc.  sun_radius 0.1: at these map sizes the default disc (0.00465 rad) falls between the sub-samples; DISC_CASE aims it at one.
SWEEP = [(w, h, el, az, T, sc) for (w, h) in ((9, 5), (65, 33), (130, 47)) for (el, az) in ((90.0, 0.0), (35.0, 40.0), (0.0, -60.0)) for T in (2.0, 10.0) for sc in (0.0, 0.1)]


def sweep_params(w, h, el, az, T, sc):
    return ss.params(sun_dir=ss.sun_from_angles(el, az), turbidity=T, sun_scale=sc, sun_radius=0.1, width=w, height=h)


def disc_case():
    """130 x 47 with the default radius and the sun on the third sub-sample of cell (14, 80): the disc is seen by that texel alone, on its limb."""
    phi, sin_el = ss.sub_sample_directions(130, 47)
    s = sin_el[14, 2]
    c = np.sqrt(1.0 - s * s)
    a = phi[80, 2] + 0.0044 / c                                   # 0.0044 rad from the sub-sample: between 0.9 and 1 radius
    return ss.params(sun_dir=(c * np.cos(a), s, c * np.sin(a)), width=130, height=47)


def report(name, **figures):
    print(f"[sun_sky] {name}: " + ", ".join(f"{k} = {v}" for k, v in figures.items()))


# ---- interface -----------------------------------------------------------------------------------------------------------------
def test_sun_sky_interface_is_declared_at_every_layer(mirt):
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    declared = set(re.findall(r"^int\s+(mirt_\w+)\s*\(", header, flags=re.M))
    lib = mirt.load_library()
    raw = C.CDLL(mirt.LIB_PATH)
    for n in NEW_NAMES:
        assert n in declared, f"{n} is not declared (on one line) in include/mirt.h"
        assert hasattr(raw, n), f"{n} is not exported by libmirt.so"
        assert n in lib._declared, f"{n} is not bound in Python"
        assert not any(word in n for word in ("aov", "noise", "until", "temporal", "history", "atrous")), n
    assert C.sizeof(mirt.SunSkyParams) == 48 and mirt.SunSkyParams.ground.offset == 28 and mirt.SunSkyParams.width.offset == 40
    for text in ("SceneUpdate::Ambient", "0.1787 T - 1.4630", "(0.11693, -0.21196, 0.06052, 0.25886)", "0.50572 (96.07995", "fast_atan2(z, x) is the angle", "mirt_drop_history where it keeps"):
        assert text in header, text
    for cls in (mirt.Renderer, mirt.GroupRenderer):
        for method in ("set_environment", "environment", "set_sun_sky", "sun_sky_defaults"):
            assert callable(getattr(cls, method))
        assert list(inspect.signature(cls.set_environment).parameters)[1:] == ["ambient", "hdri"]
    host = open(os.path.join(mirt.CSRC, "mirt_host.hpp")).read()
    for member in ("void SetEnvironment(", "void SetSunSky(", "Environment ReadEnvironment("):
        assert member in host
    headless = open(os.path.join(mirt.CSRC, "mirt_headless.cpp")).read()
    for option in ("--sun-sky", "--env-size", "--env-out", "--sun-orbit"):
        assert f'"{option}"' in headless


def test_help_names_the_flags_and_their_entry_points(mirt):
    exe = os.path.join(mirt.CSRC, "mirt_headless")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", mirt.CSRC, "mirt_headless"], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = subprocess.run([exe, "--help"], capture_output=True, text=True, check=True, timeout=60).stdout
    for flag, entry in (("--sun-sky", "mirt_set_sun_sky"), ("--env-size", "mirt_sun_sky_defaults"), ("--env-out", "mirt_read_environment"), ("--sun-orbit", "mirt_set_sun_sky")):
        lines = [line for line in text.splitlines() if line.strip().startswith(flag)]
        assert lines and entry in lines[0], (flag, lines)


def test_refusals_that_need_no_context(mirt):
    lib = mirt.load_library()
    amb = (C.c_float * 3)(1, 1, 1)
    p = mirt.SunSkyParams()
    assert lib.mirt_sun_sky_defaults(None) == MIRT_ERR_ARG
    assert lib.mirt_sun_sky_defaults(C.byref(p)) == 0
    assert lib.mirt_set_environment(None, amb, None, 0, 0) == MIRT_ERR_ARG
    assert lib.mirt_read_environment(None, None, 0, (C.c_uint32 * 4)()) == MIRT_ERR_ARG
    assert lib.mirt_set_sun_sky(None, C.byref(p)) == MIRT_ERR_ARG
    assert lib.mirt_group_set_environment(None, amb, None, 0, 0) == MIRT_ERR_ARG
    assert lib.mirt_group_set_sun_sky(None, C.byref(p)) == MIRT_ERR_ARG
    with pytest.raises(TypeError):
        mirt._sun_sky_params({"sun_radios": 1.0})


def test_defaults(mirt):
    d = mirt.sun_sky_defaults()
    assert set(d) == set(ss.DEFAULTS)
    for k, v in ss.DEFAULTS.items():
        assert np.array_equal(np.asarray(d[k], dtype=f32), np.asarray(v, dtype=f32)), k
    assert mirt.Renderer.sun_sky_defaults() == d


# ---- the definition's own properties ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(9, 5), (65, 33), (130, 47), (4, 4)])
def test_sub_samples_map_back_into_their_cell(w, h):
    """Every sub-sample direction, through the float64 form of sky_eval's index arithmetic, names the cell it was made for."""
    phi, sin_el = ss.sub_sample_directions(w, h)
    rows, cols = h - 1, w - 1
    ce = np.sqrt(1.0 - sin_el * sin_el)
    d = np.stack(np.broadcast_arrays(ce[:, :, None, None] * np.cos(phi)[None, None], sin_el[:, :, None, None], ce[:, :, None, None] * np.sin(phi)[None, None]), axis=-1)
    r, c = sd.cell_of(d.reshape(-1, 3), w, h)
    want_r, want_c = np.broadcast_arrays(np.arange(rows)[:, None, None, None], np.arange(cols)[None, None, :, None])
    want_r, want_c = np.broadcast_to(want_r, d.shape[:-1]), np.broadcast_to(want_c, d.shape[:-1])
    assert np.array_equal(r, want_r.reshape(-1)) and np.array_equal(c, want_c.reshape(-1))
    assert abs(ss.cell_solid_angles(w, h).sum() * cols - 4.0 * np.pi) < 1e-12


def test_disc_quadrature_against_the_closed_form():
    """At the default parameters (1025 x 513, radius 0.00465) the 4 x 4 grid's sum of texel_sun x Omega(cell) against L 2 pi int ramp sin.
    Measured on the definition alone: +2.30 % (the grid is 0.0015 rad, a third of the radius); asserted with a factor 2 of headroom."""
    p = ss.params()
    got = (ss.sun_weights(p) * ss.cell_solid_angles(p["width"], p["height"])[:, None]).sum()
    want = (ss.sun_closed_form(p) / ss.host_terms(p)["L"])[0]
    gap = got / want - 1.0
    report("disc quadrature 1025x513", summed=got, closed_form=want, gap=gap)
    assert abs(gap) < 2 * 0.0230


def test_zenith_under_a_zenith_sun_is_the_zenith_colour():
    for T in (2.0, 3.0, 10.0):
        t = ss.host_terms(ss.params(sun_dir=(0, 1, 0), turbidity=T))
        Y, x, y = t["zenith"]
        want = np.maximum(ss.M_RGB @ np.array([x / y * Y, Y, (1 - x - y) / y * Y]), 0.0)
        got = ss.sky_rgb_of_direction(t, np.array([0.0, 1.0, 0.0]))
        assert np.allclose(got, want, rtol=1e-13, atol=0) and (want > 0).all()
        assert Y > 0 and 0.2 < x < 0.5 and 0.2 < y < 0.5


def test_lower_hemisphere_is_the_tinted_horizon_ring():
    p = ss.params(sun_dir=ss.sun_from_angles(35, 40), ground=(0.1, 0.2, 0.3), sun_scale=0.0, width=65, height=33)
    d, t = ss.definition(p), ss.host_terms(p)
    phi, _ = ss.sub_sample_directions(65, 33)
    ring = ss.sky_rgb_of_direction(t, np.stack([np.cos(phi), np.zeros_like(phi), np.sin(phi)], axis=-1)).mean(axis=1) * t["sky_scale"]      # [cols, 3]
    for r in range(16, 32):
        assert np.allclose(d["map"][r, :64, :3], ring * t["ground"], rtol=1e-12, atol=0)
    assert not np.allclose(d["map"][15, :64, :3], ring, rtol=1e-3)


def test_turning_the_sun_by_one_cell_shifts_the_map_by_one_column():
    w, h = 65, 33
    for el in (35.0, 0.0):
        a = ss.definition(ss.params(sun_dir=ss.sun_from_angles(el, 40.0), sun_radius=0.1, width=w, height=h))["map"]
        b = ss.definition(ss.params(sun_dir=ss.sun_from_angles(el, 40.0 + 360.0 / (w - 1)), sun_radius=0.1, width=w, height=h))["map"]
        # sun_dir is held as binary32 words: the turn is exact to 1e-7 rad, the sky's slope is O(1) per rad, the limb's 1 / (0.095 x 0.1) per rad
        shifted = np.roll(a[:, :w - 1], 1, axis=1)
        scale = np.abs(a[..., :3]).max()
        assert np.abs(b[:, :w - 1] - shifted).max() < 2e-5 * scale
        assert np.abs(b[:, :w - 1] - a[:, :w - 1]).max() > 1e-3 * scale


# ---- the binary32 twin against the definition ---------------------------------------------------------------------------------------
def check_against_definition(got, p, label):
    """`got` [h, w, 4] binary32 against the float64 definition, every texel within the derived bound; duplicates and alpha exact."""
    d = ss.definition(p, want_bound=True)
    err = np.abs(got[..., :3].astype(np.float64) - d["map"][..., :3])
    ratio = float((err / d["bound"]).max())
    report(label, worst_error_over_bound=round(ratio, 4), worst_error=float(err.max()), weight_error_bound=d["weight_error"], sun_texels=int((d["sun"].max(axis=2) > 0).sum()))
    assert np.isfinite(got).all() and (d["bound"] > 0).all()
    assert ratio <= 1.0
    words = got.view(np.uint32)
    assert np.array_equal(words[:, -1], words[:, 0]) and np.array_equal(words[-1], words[-2])
    assert (got[..., 3] == 1.0).all()
    return d


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "%dx%d-el%g-T%g-sun%g" % (c[0], c[1], c[2], c[4], c[5]))
def test_twin_within_the_derived_bound(case):
    p = sweep_params(*case)
    d = check_against_definition(ss.twin(p), p, "twin " + str(case))
    if case[5] > 0 and case[:2] != (9, 5):
        assert (d["sun"] > 0).any()                               # the disc is seen


def test_twin_on_the_limb_of_the_default_disc():
    p = disc_case()
    d = check_against_definition(ss.twin(p), p, "twin, default disc on a sub-sample")
    lit = np.argwhere(d["sun"][:46, :129, 0] > 0)
    assert lit.tolist() == [[14, 80]] and 0 < d["sun"][14, 80, 0] < ss.host_terms(p)["L"][0] / 16


# ---- host code under sanitizers ----------------------------------------------------------------------------------------------------
def test_host_code_under_sanitizers(mirt, tmp_path):
    """csrc/sun_sky_host.hpp with its own main (tests/native/sun_sky_check.cpp) under -fsanitize=address,undefined: the argument rules, and the
    float64 precomputation word for word against host_args.  Nothing here is loaded into Python."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "sun_sky_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "native", "sun_sky_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines() if " " in line)
    assert lines["null"] == "rc=-1" and lines["defaults"] == "rc=0" and lines["check_null"] == "rc=-1"
    for label in ("nan_dir", "inf_ground", "zero_dir", "twilight", "turbidity_low", "turbidity_high", "radius_zero", "radius_large", "sky_scale_negative",
                  "sun_scale_negative", "width_1", "height_0", "width_large"):
        assert lines[label] == "rc=-1", label
    cases = {"default": ss.params(), "zenith_t2": ss.params(sun_dir=(0, 1, 0), turbidity=2.0), "horizon_t10": ss.params(sun_dir=(1, 0, 0), turbidity=10.0, sun_scale=0.0),
             "tiny_dir": ss.params(sun_dir=(3e-20, 4e-20, 0), width=2, height=2)}
    for label, p in cases.items():
        fields = lines[label].split()
        assert fields[0] == "rc=0" and len(fields) == 1 + 33 + 2 and fields[-2:] == [str(p["width"]), str(p["height"])]
        got = np.array([int(x, 16) for x in fields[1:34]], dtype=np.uint32).view(f32)
        a = ss.host_args(p)
        want = np.concatenate([a["perez"].reshape(-1), a["inv_f0"], a["zenith"], a["sun"], a["sun_rgb"], [a["ramp_edge"], a["ramp_inv"], a["sky_scale"]], a["ground"]]).astype(f32)
        # two float64 libraries (libm, numpy) may differ in the last place of exp / pow / tan: one binary32 step at most
        assert np.all(np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)) <= 1), label
    assert out.stdout.strip().endswith("done")
