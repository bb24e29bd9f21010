"""The later bounces of the plain and the GGX form run as k_shade<ShadeWaves8, ...> - 8 waves per SIMD, four 512-thread workgroups per CU - and k_shade's grid
follows the launched form (kernels.hpp shade_waves, launch_batch's shade_grid).  The parity suites mostly run one or two workgroups, so:

1. 48 x 32, default9 and S(1000), 5 buckets, max_bounces 5, MIS on, batches of 1, 3 and 64 accumulations (a partial batch, a candidate-list batch,
   a wave-per-pixel batch), the plain form, the GGX form and light RIS: every accumulator word is the oracle's, and so are the counters - rays and
   terminated both oracle modes', shadow_rays the mode's that casts none for a last-bounce hit (Q5), dropped = paths - terminated (the oracle
   counts no dropped paths);
2. S(1000) at 1024 x 1024 x 3: the bounce-1 stream has more 512-ray pieces than 4 workgroups per CU, so every workgroup takes several
   (the grid-stride loop) - against the same context with trace_primary_rays = 1, and against one whose k_shade grids are one workgroup per CU,
   word for word;
3. 16 x 16, one accumulation, max_bounces 9: the last launch holds a single ray - every wave of its one workgroup but one has no hit to shade,
   no survivor and no shadow record to write."""
import numpy as np
import pytest

import oracle_binding as ob

pytestmark = pytest.mark.gpu
DECAY = [0.0, 0.3, 0.6, 0.8]
W, H = 48, 32
COUNTS = (1, 3, 64)
SCENES = {"default9": lambda m: m.scene.default9(), "S1000": lambda m: m.scene.synthetic(1000)}
FORMS = {"plain": {}, "ggx": dict(brdf=1, gloss_decay=DECAY), "ris": dict(light_ris=4)}
_oracle = {}


def same_words(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape, what
    diff = a.view(np.uint32) != b.view(np.uint32)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} words differ"


def oracle_states(mirt, scene, form, w, h, counts, max_bounces):
    """Accumulator and counters of the brute-force oracle after each of `counts` accumulations, and the counters of its per-ray tree mode, whose
    words must be the same.  Computed once per key and left unchanged."""
    key = (scene, form, w, h, counts, max_bounces)
    if key not in _oracle:
        out = {}
        for mode in (ob.TRAV_BRUTE, ob.TRAV_PER_RAY_BVH):
            o = ob.Oracle(SCENES[scene](mirt), max_bounces=max_bounces, buckets=5, mis=True, trav_mode=mode, **FORMS[form])
            o.Resize(w, h)
            done = 0
            for n in counts:
                o.Accumulate(n - done); done = n
                if mode == ob.TRAV_BRUTE:
                    out[n] = dict(acc=o.accumulator().copy(), counters=o.counters())
                else:
                    same_words(o.accumulator(), out[n]["acc"], f"oracle, {scene}, {form}, {n}: the tree mode against brute force")
                    out[n]["twin"] = o.counters()
            o.close()
        _oracle[key] = out
    return _oracle[key]


def check(r, want, paths, what):
    same_words(r.accumulator(), want["acc"], f"{what}: accumulator")
    got = r.counters()
    for k in ("rays", "terminated"):
        assert got[k] == want["counters"][k] == want["twin"][k], (what, k, got[k], want["counters"][k], want["twin"][k])
    assert got["shadow_rays"] == want["twin"]["shadow_rays"] <= want["counters"]["shadow_rays"], (what, got["shadow_rays"], want["twin"]["shadow_rays"])
    assert got["dropped"] == paths - want["counters"]["terminated"], (what, got["dropped"])


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("scene", list(SCENES))
def test_batches_are_the_oracle(mirt, scene, form, n):
    want = oracle_states(mirt, scene, form, W, H, COUNTS, 5)[n]
    r = mirt.Renderer(SCENES[scene](mirt), max_bounces=5, buckets=5, mis=True, use_bvh=True, **FORMS[form])
    r.Resize(W, H); r.Accumulate(n)
    check(r, want, n * W * H, f"{scene}, {form}, one batch of {n}")
    r.close()


def test_grid_stride_over_more_pieces_than_workgroups(mirt, monkeypatch):
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    sc = SCENES["S1000"](mirt)
    got = {}
    # "one per CU": the same kernels over a grid a quarter the size (MIRT_TUNE_SHADE_WGS is read when the context is created), so every workgroup
    # takes other pieces than it does in the default run - a piece skipped or taken twice by the stride shows as a difference between the two
    for label, traced, wgs in (("lists", False, None), ("traced", True, None), ("one per CU", False, "1")):
        if wgs is not None:
            monkeypatch.setenv("MIRT_TUNE_SHADE_WGS", wgs)
        r = mirt.Renderer(sc, max_bounces=5, buckets=5, mis=True, use_bvh=True, trace_primary_rays=traced)
        monkeypatch.delenv("MIRT_TUNE_SHADE_WGS", raising=False)
        r.Resize(1024, 1024); r.Accumulate(3)
        got[label] = (r.accumulator().copy(), r.counters())
        r.close()
    # the premise of the case: the four later bounces read these rays, bounce 1 the most of them - at least a quarter, and that is more than the
    # 512 x 4 x n_cu rays a grid of four workgroups per CU covers in one pass
    assert (got["lists"][1]["rays"] - 3 * 1024 * 1024) // 4 > 512 * 4 * n_cu
    for other in ("traced", "one per CU"):
        same_words(got["lists"][0], got[other][0], f"S(1000), 1024 x 1024 x 3: candidate lists against {other}")
        for k in ("rays", "shadow_rays", "terminated", "dropped"):
            assert got["lists"][1][k] == got[other][1][k], (other, k, got["lists"][1][k], got[other][1][k])


def test_a_launch_with_a_single_ray(mirt):
    want = oracle_states(mirt, "default9", "plain", 16, 16, (1,), 9)[1]
    assert want["counters"]["terminated"] == 255                    # the premise of the case: one path of the 256 is still alive in the last launch
    r = mirt.Renderer(SCENES["default9"](mirt), max_bounces=9, buckets=5, mis=True, use_bvh=True)
    r.Resize(16, 16); r.Accumulate(1)
    check(r, want, 256, "default9, 16 x 16 x 1, 9 bounces")
    r.close()
