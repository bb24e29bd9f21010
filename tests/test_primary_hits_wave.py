"""k_primary_hits_wave: the camera rays' list tests with one wave per pixel and the lanes as the batch's accumulations (-m gpu).

Batches of kWaveHitsMinBatch = 32 accumulations and more take it, smaller ones keep k_primary_hits (one lane per pixel); the hit records
must not depend on which.  Yardstick, as in test_camera_lists.py: the same calls on a context with trace_primary_rays=1, where no list
is built or read and every camera ray walks the tree — compared on the raw words.  MIRT_DEBUG_POISON_CONTRIB=1 is set for every context,
so a path whose hit record no kernel wrote reaches the accumulator as a NaN.

The (slot, pixel) <-> lane map of the kernel's staged write-out (csrc/hits_wave_map.hpp) is also checked on the host, without a GPU, by a
stand-alone program built under sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB = 5
OVERFLOW = 0xFFFFFFFF
THRESHOLD = 32          # kWaveHitsMinBatch
CAND_REGS = 3           # kCandRegs


@pytest.fixture(autouse=True)
def poisoned(monkeypatch):
    monkeypatch.setenv("MIRT_DEBUG_POISON_CONTRIB", "1")      # read at mirt_create


def same_bits(got, want, what):
    got = np.ascontiguousarray(got, dtype=f32); want = np.ascontiguousarray(want, dtype=f32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    assert not np.isnan(got).any(), f"{what}: a contribution word was never written"
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} words differ"


def pair(mirt, sc_fn, w, h, setup=None, **kw):
    """Two contexts in the same state: camera rays through the lists, and every camera ray walking the tree."""
    out = []
    for walk in (False, True):
        r = mirt.Renderer(sc_fn(), max_bounces=MB, use_bvh=True, streams=1, trace_primary_rays=walk, **kw)
        r.Resize(w, h)
        if setup:
            setup(r)
        out.append(r)
    return out


def compare(lists, walk, what):
    same_bits(lists.accumulator(), walk.accumulator(), what)
    a, b = lists.counters(), walk.counters()
    for k in ("rays", "terminated"):
        assert a[k] == b[k], f"{what}: {k} {a[k]} vs {b[k]}"


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def s1000(mirt):
    return mirt.scene.synthetic(1000, ambient=0.5)


def sky_and_dust(mirt):
    """S(1000) from its usual eye, looking up 2.9 degrees: the rows around the image centre pass above every sphere (the eye is 10 up and 40 to
    80 from spheres that reach 11) and see sky.  On the view axis, 10 from the eye, a cloud of 600 spheres of radius 0.004 in a cube of side
    1.0 — at 128x64 a pixel is 0.094 wide there, so its cone meets a handful of them, fewer at the cloud's edge — and, centred on the
    cloud's right face, half in the cloud and half against the sky, 600 more in a cube of side 0.15, which puts far more than kCandMax = 31
    into the cones of the few pixels that see it: those get no list.  That face lies 5 pixels right of the image centre, in the middle
    of a tile row: the row holds long lists, short ones, pixels without a list and sky side by side.  A third such cube stands clear of the
    cloud, 13 pixels right of the centre in the same tile row, with sky on both sides."""
    sc = s1000(mirt)
    s = mirt.scene
    sc.camera = s.Camera(eye=tuple(float(v) for v in sc.camera.pos), direction=(0.0, 0.05, -1.0), focal_length=40.0, exposure=1.0)
    d = np.array([0.0, 0.05, -1.0]); d /= np.sqrt((d * d).sum())
    centre = np.asarray(sc.camera.pos, dtype=np.float64) + 10.0 * d
    rng = np.random.default_rng(11)
    dust = np.zeros(1800, dtype=s.SPHERE)
    dust["position"][:600] = (centre + rng.uniform(-0.5, 0.5, size=(600, 3))).astype(f32)
    right = np.cross(d, np.array([0.0, 1.0, 0.0])); right /= np.sqrt((right * right).sum())
    dust["position"][600:1200] = (centre + 0.5 * right + rng.uniform(-0.075, 0.075, size=(600, 3))).astype(f32)
    dust["position"][1200:] = (centre + 1.2 * right + rng.uniform(-0.075, 0.075, size=(600, 3))).astype(f32)
    dust["radius_sq"] = f32(0.004) * f32(0.004)
    dust["material_ID"] = (np.arange(1800) % 16).astype(np.int32)
    sc.geometry = np.concatenate([np.asarray(sc.geometry, dtype=s.SPHERE), dust])
    sc.name = "S(1000) + dust against the sky"
    return sc


# ---- batch sizes around every boundary of the kernel -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("max_batch", [31, 32, 33, 63, 64, 65, 128, 192])
def test_batch_sizes(mirt, max_batch):
    """One full batch of max_batch accumulations and a partial one of 7 (k_primary_hits: below the threshold) in one context: 31 runs
    k_primary_hits twice, 32 and more k_primary_hits_wave and then k_primary_hits; 63 / 64 / 65 one lane short of a group, a full group, a
    group and one lane; 128 and 192 two and three full groups."""
    lists, walk = pair(mirt, lambda: s1000(mirt), 64, 48, max_batch=max_batch)
    for r in (lists, walk):
        assert r.get_policy()["max_batch"] == max_batch
        r.Accumulate(max_batch + 7)
        assert r.accumulations == max_batch + 7
    compare(lists, walk, f"max_batch={max_batch}: lists vs trace_primary_rays=1")
    lists.close(); walk.close()


# ---- every kind of pixel within one run of 16 ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_list_shapes_within_a_run(mirt):
    lists, walk = pair(mirt, lambda: sky_and_dust(mirt), 128, 64, max_batch=63)
    cnt = lists.debug_primary_counts()
    assert cnt.shape == (32, 256)
    runs = cnt.reshape(-1, 16)                                     # a tile's 256 pixels are 16 rows of 16: a run of the kernel
    listed = runs != OVERFLOW
    kinds = np.stack([(runs == 0).any(axis=1), (listed & (runs >= 1) & (runs <= CAND_REGS)).any(axis=1),
                      (listed & (runs > CAND_REGS)).any(axis=1), (~listed).any(axis=1)])
    print("runs with an empty list / 1-3 entries / more than 3 / a pixel without a list:", kinds.sum(axis=1), "all four:", int(kinds.all(axis=0).sum()),
          "longest list:", int(runs[listed].max()))
    # The three kinds of list within single runs, and pixels without a list in runs that also hold listed pixels (the run is not skipped as a whole,
    # and its write-out must leave those pixels' records alone).  (On an MI355X: 291 / 206 / 197 / 4 of the 512 runs hold the four kinds; no single
    # run holds all four — the pixels beside one without a list see the dense dust too.)
    assert kinds[:3].all(axis=0).any(), "no run of 16 pixels holds an empty list, a short one and a long one together"
    assert ((~listed).any(axis=1) & listed.any(axis=1) & (kinds[0] | kinds[1])).any(), "no run holds a pixel without a list beside empty or short lists"
    assert (runs[listed] <= 31).all()
    hist = lists.debug_primary_lists()
    assert hist[9] == int((~listed).sum()) and hist[0] == int((runs == 0).sum())
    for r in (lists, walk):
        r.Accumulate(63)
    compare(lists, walk, "sky and dust, batch 63")
    for r in (lists, walk):
        r.Accumulate(5)                                            # the same lists through k_primary_hits
    compare(lists, walk, "sky and dust, batch 63 + batch 5")
    lists.close(); walk.close()


# ---- a tile subset: n_pix is not the image, runs start at a tile other than 0 ------------------------------------------------------
@pytest.mark.gpu
def test_tile_rows(mirt):
    lists, walk = pair(mirt, lambda: s1000(mirt), 64, 64, setup=lambda r: r.SetTileRows(1, 2), max_batch=64)
    for r in (lists, walk):
        r.Accumulate(64 + 3)
    assert lists.accumulator().shape[0] == 8                       # tile rows 1 and 3 of 4, 4 tiles each
    compare(lists, walk, "SetTileRows(1, 2)")
    lists.close(); walk.close()


# ---- counters -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_count_traffic_equal_on_both_sides_of_the_threshold(mirt):
    """count_traffic: a sample adds its pixel's list length to `spheres` in either kernel.  124 accumulations as 4 batches of 31 (k_primary_hits
    every time) and as 3 batches of 32 — through k_primary_hits_wave — and one of 28.  Four batches either way, so the lists' own traversal,
    which a counting pass repeats for every batch, counts four times in both; everything after the camera rays is counted per ray."""
    def run(max_batch):
        r = mirt.Renderer(sky_and_dust(mirt), max_bounces=MB, use_bvh=True, streams=1, count_traffic=True, max_batch=max_batch)
        r.Resize(128, 64)
        r.Accumulate(124)
        c, acc = r.counters(), r.accumulator().copy()
        r.close()
        return c, acc
    c31, a31 = run(31)
    c32, a32 = run(32)
    same_bits(a32, a31, "batches of 32 vs batches of 31")
    print("spheres", c31["spheres"], c32["spheres"], "nodes", c31["nodes"], c32["nodes"])
    for k in ("spheres", "nodes", "rays", "shadow_rays", "shadow_spheres", "terminated"):
        assert c31[k] == c32[k], f"{k}: {c31[k]} in batches of 31, {c32[k]} in batches of 32"


# ---- AOVs read the same hit-record layout ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_aov_slab(mirt):
    lists, walk = pair(mirt, lambda: s1000(mirt), 64, 48, max_batch=63, aov=True)
    for r in (lists, walk):
        r.Accumulate(63)
    compare(lists, walk, "aov on, batch 63")
    same_bits(lists.aov(), walk.aov(), "aov slab")
    lists.close(); walk.close()


# ---- host only: the staging map ------------------------------------------------------------------------------------------------------
def test_staging_map_under_sanitizers(tmp_path):
    """tests/native/hits_wave_map_check.cpp plays the kernel's staging and write-out on heap arrays with the kernel's own index functions, for
    batches of 32, 33, 63, 64, 65, 128, 192 and 256: every record stored exactly once, a slot's 16 records in 16 neighbouring lanes."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "hits_wave_map_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "native", "hits_wave_map_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "hits_wave_map ok" in out.stdout
