"""Per-tile adaptive sampling without a GPU: the interface at every layer it is built through, the calls without a context,
mirt_adaptive_select (host code) against the numpy twin of adaptive_twin.py and under sanitizers in a stand-alone program, and the
end-to-end scene of test_adaptive_gpu.py replayed on the CPU oracle so that the GPU test cannot pass vacuously."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_twin as at

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
MIRT_ERR_ARG = -1
NEW_NAMES = ("mirt_freeze_tiles", "mirt_tile_counts", "mirt_frozen_tiles", "mirt_load_tile_counts", "mirt_tile_above", "mirt_adaptive_select", "mirt_accumulate_adaptive",
             "mirt_group_freeze_tiles", "mirt_group_tile_counts", "mirt_group_frozen_tiles", "mirt_group_tile_above", "mirt_group_accumulate_adaptive")


def test_adaptive_interface_is_declared_at_every_layer(mirt):
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    declared = set(re.findall(r"^int\s+(mirt_\w+)\s*\(", header, flags=re.M))
    lib = mirt.load_library()
    raw = C.CDLL(mirt.LIB_PATH)
    for n in NEW_NAMES:
        assert n in declared, f"{n} is not declared (on one line) in include/mirt.h"
        assert hasattr(raw, n), f"{n} is not exported by libmirt.so"
        assert n in lib._declared, f"{n} is not bound in Python"
    for text in ("typedef struct mirt_adaptive_report", "biases the frame dark", "min_accumulations is the guard", "there is no un-freeze"):
        assert text in header
    assert C.sizeof(mirt.AdaptiveReport) == 64 and mirt.AdaptiveReport.tile_accumulations.offset == 16 and mirt.AdaptiveReport.last.offset == 24
    assert C.sizeof(mirt.Policy) == 48 and C.sizeof(mirt.StopRule) == 20           # the existing structures keep their layout
    for cls in (mirt.Renderer, mirt.GroupRenderer):
        for method in ("freeze_tiles", "tile_counts", "frozen_tiles", "noise_above", "accumulate_adaptive", "adaptive_select"):
            assert callable(getattr(cls, method)), f"{cls.__name__}.{method}"
    assert callable(mirt.Renderer.load_tile_counts) and callable(mirt.adaptive_select)
    host = open(os.path.join(mirt.CSRC, "mirt_host.hpp")).read()
    for member in ("void FreezeTiles(", "std::vector<uint32_t> TileCounts(", "std::vector<uint32_t> NoiseAbove(", "static std::vector<uint8_t> AdaptiveSelect(", "AdaptiveResult AccumulateAdaptive("):
        assert member in host, member
    headless = open(os.path.join(mirt.CSRC, "mirt_headless.cpp")).read()
    for option in ("--adaptive", "--min-accumulations", "--counts-out"):
        assert f'"{option}"' in headless and f"[{option} " in headless, option       # parsed, and in the usage text


def test_adaptive_calls_fail_without_a_context(mirt):
    lib = mirt.load_library()
    one = np.zeros(4, dtype=np.uint32)
    p = one.ctypes.data_as(C.c_void_p)
    assert lib.mirt_freeze_tiles(None, p, 1) < 0 and lib.mirt_tile_counts(None, p, 1) < 0 and lib.mirt_load_tile_counts(None, p, 1) < 0
    assert lib.mirt_tile_above(None, 0.0, 0.5, p, 1) < 0
    assert lib.mirt_accumulate_adaptive(None, None, 0, None) < 0
    assert lib.mirt_adaptive_select(None, None, None, 3, 0.5, None) == MIRT_ERR_ARG
    assert lib.mirt_frozen_tiles(None, p, 1) < 0
    assert lib.mirt_group_freeze_tiles(None, p, 1) < 0 and lib.mirt_group_tile_counts(None, p, 1) < 0 and lib.mirt_group_frozen_tiles(None, p, 1) < 0
    assert lib.mirt_group_tile_above(None, 0.0, 0.5, p, 1) < 0 and lib.mirt_group_accumulate_adaptive(None, None, 0, None) < 0


def crafted_cases():
    """name -> (records, above, frozen or None, quantile): usable 0, 1, 255, 256; `above` at, one below and one above the cut."""
    out = {}
    for name, q in (("q1", 1.0), ("q0.95", 0.95), ("q0.95f", float(f32(0.95)))):
        rec, above = [], []
        for usable in (0, 1, 255, 256):
            cut = int(math.floor((1.0 - q) * usable))
            for d in (-1, 0, 1):
                if d < 0 and cut == 0:
                    continue
                rec.append([0.5, 0.25, usable, 0.0]); above.append(cut + d)
        out[name] = (np.array(rec, dtype=f32), np.array(above, dtype=np.uint32), None, q)
    rec = np.array([[0.1, 0.1, 255, 1], [0.1, 0.1, 256, 0], [9, 9, 256, 0], [9, 9, 200, 56]], dtype=f32)
    above = np.array([0, 0, 256, 200], dtype=np.uint32)
    out["nonfinite"] = (rec, above, None, 0.95)
    out["frozen"] = (rec, above, np.array([0, 0, 1, 1], dtype=np.uint8), 0.95)
    return out


def test_adaptive_select_equals_the_twin(mirt):
    for name, (rec, above, frozen, q) in crafted_cases().items():
        got, want = mirt.adaptive_select(rec, above, frozen, q), at.select(rec, above, frozen, q)
        assert np.array_equal(got, want), f"{name}: {got} vs the twin's {want}"
    rec, above, _, _ = crafted_cases()["q0.95"]
    # (1 - 0.95) * 256 = 12.8: twelve pixels of a full tile may sit above the target, the thirteenth keeps it active
    assert list(mirt.adaptive_select([[0, 0, 256, 0]] * 3, [11, 12, 13], None, 0.95)) == [1, 1, 0]
    assert list(mirt.adaptive_select([[0, 0, 256, 0]] * 2, [0, 1], None, 1.0)) == [1, 0]
    assert list(mirt.adaptive_select([[0, 0, 0, 0], [0, 0, 0, 256]], [0, 0], None, 0.95)) == [1, 0]      # nothing usable: 0 <= 0 freezes; all non-finite does not
    assert list(mirt.adaptive_select(crafted_cases()["frozen"][0], crafted_cases()["frozen"][1], [0, 0, 1, 1], 0.95)) == [0, 1, 1, 1]
    for bad in (0.0, -0.5, 1.0000001, float("nan")):
        with pytest.raises(mirt.MirtError):
            mirt.adaptive_select(rec, above, None, bad)


def test_adaptive_select_under_sanitizers(mirt, tmp_path):
    """csrc/noise_host.cpp with its own main (tests/native/adaptive_sanitize.cpp) under -fsanitize=address,undefined on the crafted cases; its
    answers are the twin's.  Nothing here is loaded into Python."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "adaptive_sanitize"
    src = [os.path.join(ROOT, "tests", "native", "adaptive_sanitize.cpp"), os.path.join(mirt.CSRC, "noise_host.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *src, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines() if " " in line)
    for name, (rec, above, frozen, q) in crafted_cases().items():
        want = "rc=0 " + "".join(str(int(v)) for v in at.select(rec, above, frozen, q))
        assert lines.get(name) == want, f"{name}: {lines.get(name)!r} vs {want!r}"
    assert lines["bad_q0"] == "rc=-1 7777" and lines["bad_q1.5"] == "rc=-1 7777" and lines["null"] == "rc=-1" and lines["empty"] == "rc=0"
    assert out.stdout.strip().endswith("done")


def test_end_to_end_scene_freezes_early_and_stays_partly_active(mirt):
    """The scene of the GPU loop test, replayed with the brute-force oracle and the twin: at TARGET some tile freezes at the first check and
    some tile is still active at the last (MIRT_NOT_CONVERGED); at TARGET_ALL_FREEZE every tile freezes at the first check (MIRT_OK)."""
    import oracle_binding as ob
    S = at.SCENE
    sc = mirt.scene.default9()
    o = ob.Oracle(sc, max_bounces=S["max_bounces"], buckets=S["buckets"]); o.Resize(S["width"], S["height"])
    slabs = {}
    for n in range(S["check_every"], S["max_accumulations"] + 1, S["check_every"]):
        o.Accumulate(S["check_every"]); slabs[n] = o.accumulator().copy()
    tiles = (S["width"] // 16) * (S["height"] // 16)
    args = (sc.camera.exposure,), (S["quantile"], S["floor"], S["buckets"], S["check_every"], 0, S["max_accumulations"])
    res = at.replay(lambda n: slabs[n], tiles, *args[0], at.TARGET, *args[1], select_fn=mirt.adaptive_select)      # the library's select beside the twin's
    hist = {int(c): int((res["counts"] == c).sum()) for c in np.unique(res["counts"])}
    print(f"[adaptive] target {at.TARGET}: frozen after each check {[int(m.sum()) for m in res['masks']]}, counts {hist}")
    assert res["masks"][0].sum() >= 1 and res["masks"][-1].sum() < tiles and not res["converged"]
    assert res["checks"] == S["max_accumulations"] // S["check_every"] and int(res["counts"].sum()) < tiles * res["issued"]
    assert hist == {5: 3, 10: 1, 15: 1, 20: 1, 25: 2, 30: 8}                       # the histogram DESIGN.md quotes
    done = at.replay(lambda n: slabs[n], tiles, *args[0], at.TARGET_ALL_FREEZE, *args[1])
    assert done["converged"] and done["checks"] == 1 and (done["counts"] == S["check_every"]).all()
    o.close()
