"""The noise estimate without a GPU: the interface at every layer, mirt_noise_quantile (host code) against the twin's binning, the binary32
twin (noise_twin.py) against the float64 definition with its derived bound (noise_definitions.py), and the host code under sanitizers in a
stand-alone program."""
import ctypes as C
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import noise_definitions as nd
import noise_twin as nt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
MIRT_NOT_READY, MIRT_ERR_ARG = 1, -1
NEW_NAMES = ("mirt_noise", "mirt_noise_quantile", "mirt_accumulate_until", "mirt_group_noise", "mirt_group_accumulate_until")


def report(name, **figures):
    print(f"[noise] {name}: " + ", ".join(f"{k} = {v}" for k, v in figures.items()))


# ---- interface -----------------------------------------------------------------------------------------------------------------
def test_noise_interface_is_declared_at_every_layer(mirt):
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    declared = set(re.findall(r"^int\s+(mirt_\w+)\s*\(", header, flags=re.M))
    lib = mirt.load_library()
    raw = C.CDLL(mirt.LIB_PATH)
    for n in NEW_NAMES:
        assert n in declared, f"{n} is not declared (on one line) in include/mirt.h"
        assert hasattr(raw, n), f"{n} is not exported by libmirt.so"
        assert n in lib._declared, f"{n} is not bound in Python"
    assert {n for n in declared if "noise" in n or "until" in n} == set(NEW_NAMES)
    for text in ("#define MIRT_NOISE_BINS 2048u", "#define MIRT_NOT_CONVERGED 2", "0.2126f * r_j + 0.7152f * g_j) + 0.0722f * b_j", "not of the median", "0x7f800000"):
        assert text in header
    assert C.sizeof(mirt.Policy) == 48                                          # mirt_policy keeps its layout
    assert C.sizeof(mirt.NoiseStats) == 40 and mirt.NoiseStats.mean.offset == 32 and mirt.NoiseStats.max.offset == 24
    assert C.sizeof(mirt.StopRule) == 20
    assert (mirt.NOISE_BINS, mirt.MIRT_NOT_CONVERGED) == (2048, 2)
    for cls in (mirt.Renderer, mirt.GroupRenderer):
        for method in ("noise", "accumulate_until", "noise_quantile"):
            assert callable(getattr(cls, method))
        assert list(inspect.signature(cls.noise).parameters)[1:3] == ["floor", "want_map"]
    host = open(os.path.join(mirt.CSRC, "mirt_host.hpp")).read()
    for member in ("NoiseResult Noise(", "static float NoiseQuantile(", "UntilResult AccumulateUntil("):
        assert member in host
    headless = open(os.path.join(mirt.CSRC, "mirt_headless.cpp")).read()
    for option in ("--until-noise", "--noise-quantile", "--noise-floor", "--check-every", "--max-accumulations", "--noise-out"):
        assert f'"{option}"' in headless


def test_noise_calls_fail_without_a_context(mirt):
    lib = mirt.load_library()
    assert lib.mirt_noise(None, 0.0, None, None, None, None) < 0
    assert lib.mirt_accumulate_until(None, None, None, None) < 0
    assert lib.mirt_group_noise(None, 0.0, None, None, None, None) < 0 and lib.mirt_group_accumulate_until(None, None, None, None) < 0


# ---- mirt_noise_quantile against the twin's binning --------------------------------------------------------------------------------
def crafted_histograms():
    """name -> (histogram, [q, ...])"""
    out = {}
    h = np.zeros(nt.BINS, dtype=np.uint32); h[1000] = 7
    out["single bin"] = (h, [1e-9, 0.5, 1.0])
    h = np.zeros(nt.BINS, dtype=np.uint32); h[1000] = 50; h[1010] = 50
    out["two bins"] = (h, [0.5, 0.51, 0.49, 1.0, 0.01])                         # q = 0.5: rank 50, exactly the last value of the lower bin
    h = np.zeros(nt.BINS, dtype=np.uint32); h[0] = 1; h[0x7F7] = 1; h[nt.BINS - 1] = 1
    out["both ends"] = (h, [0.01, 0.5, 1.0])
    rng = np.random.default_rng(7)
    out["random"] = (rng.integers(0, 1000, nt.BINS).astype(np.uint32), [0.001, 0.25, 0.5, 0.95, 0.999, 1.0])
    out["full words"] = (np.full(nt.BINS, 0xFFFFFFFF, dtype=np.uint32), [0.5, 1.0])
    return out


def test_quantile_equals_the_twin_on_crafted_histograms(mirt):
    for name, (hist, qs) in crafted_histograms().items():
        for q in qs:
            got, want = mirt.noise_quantile(hist, q), nt.quantile(hist, q)
            assert got == want, f"{name}, q = {q}: {got} vs the twin's {want}"
    h, _ = crafted_histograms()["two bins"]
    assert mirt.noise_quantile(h, 0.5) == nt.bin_upper_edge(1000) and mirt.noise_quantile(h, 0.51) == nt.bin_upper_edge(1010)
    assert mirt.noise_quantile(h, 1.0) == nt.bin_upper_edge(1010)
    assert math.isinf(mirt.noise_quantile(crafted_histograms()["both ends"][0], 0.5))   # bin 0x7f7 ends at +infinity
    # the edge is the value whose word is (bin + 1) << 20: eight sub-bins per octave, at most 12.5 % above anything in the bin
    lo, hi = f32(nt.bin_upper_edge(999)), f32(nt.bin_upper_edge(1000))
    assert hi.view(np.uint32) == 1001 << 20 and 1.0 < float(hi) / float(lo) <= 1.125


def test_quantile_statuses(mirt):
    lib = mirt.load_library()
    empty = np.zeros(nt.BINS, dtype=np.uint32)
    v = C.c_float(-5.0)
    assert lib.mirt_noise_quantile(empty.ctypes.data_as(C.c_void_p), 0.5, C.byref(v)) == MIRT_NOT_READY and v.value == -5.0
    assert mirt.noise_quantile(empty, 0.5) is None and nt.quantile(empty, 0.5) is None
    one = empty.copy(); one[5] = 1
    for bad in (0.0, -0.1, 1.0000001, float("nan"), float("inf")):
        assert lib.mirt_noise_quantile(one.ctypes.data_as(C.c_void_p), bad, C.byref(v)) == MIRT_ERR_ARG and v.value == -5.0
        with pytest.raises(mirt.MirtError):
            mirt.noise_quantile(one, bad)
    assert lib.mirt_noise_quantile(None, 0.5, C.byref(v)) == MIRT_ERR_ARG and lib.mirt_noise_quantile(one.ctypes.data_as(C.c_void_p), 0.5, None) == MIRT_ERR_ARG


# ---- the twin against the float64 definition -------------------------------------------------------------------------------------
def random_slab(rng, tiles, k, spread):
    """Positive words: a per-pixel level over six decades times a per-bucket factor of relative spread `spread`."""
    level = 10.0 ** rng.uniform(-3, 3, (tiles, 1, 3, 256))
    return (level * np.abs(1.0 + spread * rng.standard_normal((tiles, k, 3, 256))) + 1e-6).astype(f32)


@pytest.mark.parametrize("k", [2, 3, 5, 16])
def test_twin_against_float64_definition(k):
    """|e - E| <= ((k + 10) u Ymax + (1.5 k + 9) u SE) / (M + floor), derived in noise_definitions.py from the format (u = 2^-24) and the
    operation count — not from any measurement.  Slabs: noisy buckets (spread 0.5: the SE term matters), nearly equal buckets (spread 1e-4
    and 1e-6: the cancellation term is all there is), floors 0 and 0.05, accumulations / k = 3 so that the scale is not a power of two.
    The histogram's float64 pin: wherever the bound leaves no doubt about the bin — E - bound and E + bound in the same bin — the twin's
    bin is that bin."""
    rng = np.random.default_rng(100 + k)
    worst = 0.0
    for spread in (0.5, 1e-4, 1e-6):
        for floor in (0.0, 0.05):
            slab = random_slab(rng, 6, k, spread)
            scale = nt.scale_of(1.25, 3 * k, k)
            e = nt.noise_e(slab, scale, floor)
            d = nd.noise_e64(slab, scale, floor)
            assert nt.usable(e).all()
            err, bnd = np.abs(e.astype(np.float64) - d["e"]), nd.bound(d, k)
            ratio = float((err / bnd).max())
            worst = max(worst, ratio)
            assert (err <= bnd).all(), f"k = {k}, spread {spread}, floor {floor}: error / bound up to {ratio:.3f}"
            lo, hi = np.maximum(d["e"] - bnd, 0.0).astype(f32), (d["e"] + bnd).astype(f32)
            sure = (lo.view(np.uint32) >> 20) == (hi.view(np.uint32) >> 20)
            assert sure.mean() > 0.5 or spread < 1e-3
            assert ((e.view(np.uint32) >> 20)[sure] == (lo.view(np.uint32) >> 20)[sure]).all()
    report(f"twin vs float64, k = {k}", worst_error_over_bound=round(worst, 4))
    assert worst > 0.005                                                          # the bound is of the order of what happens, not vacuous


def test_twin_edge_cases():
    """Equal buckets give exactly 0; all zero with floor 0 gives 0 by the 0/0 rule; a non-finite word makes the pixel unusable; a negative
    mean + floor sets the sign bit and is unusable too; -0 (equal negative buckets) as well."""
    k = 5
    slab = np.ones((1, k, 3, 256), dtype=f32) * f32(0.37)
    assert not nt.noise_e(slab, 1.0, 0.0).view(np.uint32).any()
    assert not nt.noise_e(np.zeros((1, k, 3, 256), dtype=f32), 1.0, 0.0).view(np.uint32).any()
    slab[0, 2, 1, 7] = np.nan; slab[0, 4, 0, 9] = np.inf
    e = nt.noise_e(slab, 1.0, 0.0)
    assert np.isnan(e[0, 7]) and not np.isfinite(e[0, 9]) and nt.usable(e).sum() == 254
    t_max, t_mean, n_ok, n_bad = nt.tile_records(e)
    assert (t_max[0], t_mean[0], n_ok[0], n_bad[0]) == (0.0, 0.0, 254, 2) and nt.histogram(e)[0] == 254 and nt.histogram(e).sum() == 254
    neg = -np.ones((1, k, 3, 256), dtype=f32)
    e = nt.noise_e(neg, 1.0, 0.0)
    assert (e.view(np.uint32) == 0x80000000).all() and not nt.usable(e).any() and nt.histogram(e).sum() == 0
    assert nt.stats(e) == {"owned_pixels": 256, "finite_pixels": 0, "nonfinite_pixels": 256, "max": 0.0, "mean": 0.0}


# ---- host code under sanitizers ----------------------------------------------------------------------------------------------------
def test_quantile_under_sanitizers(mirt, tmp_path):
    """csrc/noise_host.cpp compiled with its own main (tests/native/noise_sanitize.cpp) under -fsanitize=address,undefined, run on crafted
    histograms; its answers are the twin's.  Nothing here is loaded into Python."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "noise_sanitize"
    src = [os.path.join(ROOT, "tests", "native", "noise_sanitize.cpp"), os.path.join(mirt.CSRC, "noise_host.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *src, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines() if " " in line)
    word = lambda v: f"{int(np.array([v], dtype=f32).view(np.uint32)[0]):08x}"
    untouched = word(-1.0)
    two = np.zeros(nt.BINS, dtype=np.uint32); two[1000] = 50; two[1010] = 50
    ends = np.zeros(nt.BINS, dtype=np.uint32); ends[0] = 1; ends[0x7F7] = 1; ends[nt.BINS - 1] = 1
    full = np.full(nt.BINS, 0xFFFFFFFF, dtype=np.uint32)
    want = {"empty": f"rc=1 word={untouched}", "single_q0.5": f"rc=0 word={word(nt.bin_upper_edge(1000))}", "single_q1": f"rc=0 word={word(nt.bin_upper_edge(1000))}",
            "bad_q0": f"rc=-1 word={untouched}", "bad_q1.5": f"rc=-1 word={untouched}",
            "two_q0.5": f"rc=0 word={word(nt.quantile(two, 0.5))}", "two_q0.51": f"rc=0 word={word(nt.quantile(two, 0.51))}", "two_q1": f"rc=0 word={word(nt.quantile(two, 1.0))}",
            "ends_q0.01": f"rc=0 word={word(nt.quantile(ends, 0.01))}", "ends_q0.5": f"rc=0 word={word(nt.quantile(ends, 0.5))}", "ends_q1": f"rc=0 word={word(nt.quantile(ends, 1.0))}",
            "full_q0.5": f"rc=0 word={word(nt.quantile(full, 0.5))}", "null": "rc=-1 -1"}
    for label, text in want.items():
        assert lines.get(label) == text, f"{label}: {lines.get(label)!r} vs {text!r}"
    assert out.stdout.strip().endswith("done")
