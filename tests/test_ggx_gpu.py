"""policy.brdf = 1 (Closure<GGX>, the reference's `#define BRDF 1`) on the GPU, bit for bit against the oracle's GGX closure
(`ob.Oracle(brdf=1)` in its mode-2 traversal, the CPU twin of the HIP kernels'; itself pinned in test_ggx_cpu.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
from oracle_binding import bits, fnv1a
from test_ggx_cpu import mirror_furnace

pytestmark = pytest.mark.gpu

DECAY = [0.0, 0.1, 0.3, 0.6, 1.0]


def assert_same(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, what
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} words differ"


def twin(sc, w, h, spp, brdf=1, decay=None, mb=16, mis=True, tiles=None):
    t = ob.Oracle(sc, brdf=brdf, gloss_decay=decay, max_bounces=mb, mis=mis, trav_mode=ob.TRAV_PER_RAY_BVH)
    t.Resize(w, h, tiles=tiles)
    t.Accumulate(spp)
    return t


def same_counters(r, t, what):
    cg, ct = r.counters(), t.counters()
    for k in ("rays", "shadow_rays", "terminated"):
        assert cg[k] == ct[k], f"{what}: counter {k} {cg[k]} vs twin {ct[k]}"


@pytest.mark.parametrize("use_bvh", [False, True])
def test_mirror_furnace_on_the_gpu(mirt, use_bvh):
    """Analytic known answer: a perfect mirror (alpha = 0, F0 = 1) under a sky of 1 reflects exactly 1.0 into every accumulator word."""
    r = mirt.Renderer(mirror_furnace(mirt), max_bounces=4, use_bvh=use_bvh, brdf=1)
    r.Resize(64, 64); r.Accumulate(5)
    acc = r.accumulator()
    assert np.array_equal(bits(acc), bits(np.ones_like(acc)))
    r.close()


@pytest.mark.parametrize("decay", [None, DECAY], ids=["decay0", "decay"])
@pytest.mark.parametrize("mis", [True, False], ids=["mis", "nomis"])
@pytest.mark.parametrize("scene_name,w,h", [("brdf_test", 160, 96), ("default9", 64, 64)])
def test_ggx_matches_twin(mirt, scene_name, w, h, mis, decay):
    sc = getattr(mirt.scene, scene_name)()
    t = twin(sc, w, h, 10, decay=decay, mis=mis)
    want_acc, want_img = t.accumulator(), t.Render()
    assert want_acc.any() and np.isfinite(want_acc).all()
    for use_bvh in (False, True):
        r = mirt.Renderer(sc, max_bounces=16, mis=mis, use_bvh=use_bvh, brdf=1, gloss_decay=decay)
        r.Resize(w, h); r.Accumulate(10)
        what = f"{scene_name} mis={mis} use_bvh={use_bvh} decay={decay}"
        assert_same(r.accumulator(), want_acc, what + " accumulator")
        assert r.Render()
        assert_same(r.GetFrame(), want_img, what + " frame")
        same_counters(r, t, what)
        r.close()


@pytest.mark.parametrize("streams,max_batch", [(1, 0), (3, 16)])
def test_ggx_full_size_launch_shape(mirt, streams, max_batch):
    """default9 with every material member at 1920x1088 x 64 accumulations (contribution-buffer mode), against the twin on a tile subset."""
    w, h, spp = 1920, 1088, 64
    sc = mirt.scene.default9()
    h_tiles, v_tiles = w // 16, h // 16
    rng = np.random.default_rng(41)
    tiles = np.unique(np.concatenate([[0, h_tiles * v_tiles - 1, (v_tiles // 2) * h_tiles + h_tiles // 2], rng.integers(0, h_tiles * v_tiles, 13)])).astype(np.uint32)
    r = mirt.Renderer(sc, max_bounces=16, use_bvh=True, streams=streams, max_batch=max_batch, brdf=1, gloss_decay=DECAY)
    r.Resize(w, h); r.Accumulate(spp)
    got = r.accumulator()[tiles]
    c = r.counters()
    assert c["terminated"] + c["dropped"] == spp * h_tiles * v_tiles * 256
    r.close()
    t = twin(mirt.scene.default9(), w, h, spp, decay=DECAY, tiles=tiles)
    assert_same(got, t.accumulator(), f"1920x1088x64 streams={streams} max_batch={max_batch}")
    assert got.any()


def test_ggx_deferred_calls_keep_their_decay_table(mirt):
    """mirt_set_gloss_decay launches what AccumulateAsync deferred, with the table those calls were issued under."""
    sc = mirt.scene.brdf_test()
    r = mirt.Renderer(sc, max_bounces=16, use_bvh=True, brdf=1, gloss_decay=DECAY)
    r.Resize(64, 48)
    r.AccumulateAsync(3)
    r.set_gloss_decay([0.5, 0.2])
    r.AccumulateAsync(4)
    r.set_gloss_decay(None)
    r.AccumulateAsync(3)
    r.Synchronize()
    t = ob.Oracle(sc, brdf=1, gloss_decay=DECAY, max_bounces=16, trav_mode=ob.TRAV_PER_RAY_BVH); t.Resize(64, 48)
    t.Accumulate(3); t.set_gloss_decay([0.5, 0.2]); t.Accumulate(4); t.set_gloss_decay(None); t.Accumulate(3)
    assert_same(r.accumulator(), t.accumulator(), "AccumulateAsync with set_gloss_decay between deferred calls")
    same_counters(r, t, "deferred")
    r.close()


def test_switching_back_to_lambertian_leaks_nothing(mirt):
    sc = mirt.scene.default9()
    r = mirt.Renderer(sc, max_bounces=16, use_bvh=True, brdf=1, gloss_decay=DECAY)
    r.Resize(64, 64); r.Accumulate(5)
    ggx = r.accumulator()
    r.set_policy(brdf=0)
    assert r.get_policy()["brdf"] == 0
    r.ResetAccumulator(); r.Accumulate(10)
    o = ob.Oracle(sc, max_bounces=16, trav_mode=ob.TRAV_BRUTE); o.Resize(64, 64); o.Accumulate(10)
    assert_same(r.accumulator(), o.accumulator(), "brdf 1 -> 0 accumulator")
    assert r.Render(); assert_same(r.GetFrame(), o.Render(), "brdf 1 -> 0 frame")
    assert not np.array_equal(bits(ggx), bits(o.accumulator()))          # the GGX run before the switch was a different image
    r.close()


def test_policy_and_decay_are_validated(mirt):
    r = mirt.Renderer(mirt.scene.default9(), brdf=1)
    assert r.get_policy()["brdf"] == 1
    with pytest.raises(mirt.MirtError, match="brdf"):
        r.set_policy(brdf=2)
    assert r.get_policy()["brdf"] == 1
    for bad in ([0.5, -0.1], [np.nan], [1.5], [np.inf], [0.0] * 1025):
        with pytest.raises(mirt.MirtError, match="decay"):
            r.set_gloss_decay(bad)
    r.set_gloss_decay([0.0] * 1024)
    r.set_gloss_decay([])
    r.close()


def test_group_of_two_members_matches_one_context(mirt):
    sc = mirt.scene.brdf_test()
    r = mirt.Renderer(sc, max_bounces=16, use_bvh=True, brdf=1, gloss_decay=DECAY)
    r.Resize(160, 96); r.Accumulate(10)
    g = mirt.GroupRenderer(sc, devices=(0, 0), max_bounces=16, use_bvh=True, brdf=1, gloss_decay=DECAY)
    g.Resize(160, 96); g.Accumulate(10)
    assert_same(g.accumulator(), r.accumulator(), "group of 2 on device 0 vs one context")
    assert r.Render() and g.Render()
    assert_same(g.GetFrame(), r.GetFrame(), "group frame")
    assert g.counters()["rays"] == r.counters()["rays"]
    g.close(); r.close()


def test_headless_host_writes_the_python_frame(mirt, tmp_path):
    """mirt_headless --scene brdf_test --brdf 1 --gloss-decay ... (the C++ host over mirt_host.hpp) renders what the Python Renderer renders."""
    exe = os.path.join(mirt.CSRC, "mirt_headless")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", mirt.CSRC, "mirt_headless"], check=True)
    pfm = tmp_path / "frame.pfm"
    out = subprocess.run([exe, "--scene", "brdf_test", "--brdf", "1", "--gloss-decay", ",".join(str(d) for d in DECAY), "--size", "160x96",
                          "--spp", "10", "--out", str(pfm)], check=True, timeout=120, capture_output=True, text=True).stdout
    rep = json.loads(out)
    r = mirt.Renderer(mirt.scene.brdf_test(), max_bounces=16, use_bvh=True, brdf=1, gloss_decay=DECAY)
    r.Resize(160, 96); r.Accumulate(10); assert r.Render()
    assert rep["accumulations"] == 10 and rep["frame_ready"] and rep["rays"] == r.counters()["rays"]
    assert rep["accumulator_fnv1a"] == fnv1a(r.accumulator())
    assert rep["last_frame_fnv1a"] == fnv1a(r.GetFrame())
    rgb = np.fromfile(pfm, dtype=np.float32, offset=len(b"PF\n160 96\n-1.0\n")).reshape(96, 160, 3)
    assert_same(rgb, r.GetFrame()[:, :, :3], "mirt_headless PFM frame")
    r.close()
