"""mirt_set_material_closures on the GPU: Lambertian and GGX materials in one scene.  Every comparison is on raw accumulator words.
 1  the pure ends through the MIXED kernels, against the oracle;   2  a uniform table launches the pure kernels;   3  the first hit decides;
 4  the flag that travels with the sampled ray (Q8's pdf_in);   5  a mixed white furnace;   6  the words do not depend on the route, and the
 AOV colour;   7  with transmission and with sky sampling;   8  statuses."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
from oracle_binding import bits
from test_material_closures_cpu import scene_x, X_W, X_H, X_SPP

pytestmark = pytest.mark.gpu

DECAY = [0.0, 0.1, 0.3, 0.6, 1.0]
ERR_ARG, ERR_STATE = -1, -3


def same_words(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, what
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} words differ"


def with_unused_material(mirt, sc, k, at_front):
    """The scene with one more material that no sphere uses, and the table that gives every authored material closure k and the new one 1 - k:
    the material LIST then holds both kinds, so the MIXED kernels run, and every hit is one of closure k."""
    s = mirt.scene
    extra = np.array([s._material(albedo=(0.3, 0.6, 0.9), F0=(0.9, 0.6, 0.3), roughness=0.5)], dtype=s.MATERIAL)
    geo = sc.geometry.copy()
    if at_front:
        mats = np.concatenate([extra, sc.material]); geo["material_ID"] += 1
        table = [1 - k] + [k] * len(sc.material)
    else:
        mats = np.concatenate([sc.material, extra])
        table = [k] * len(sc.material) + [1 - k]
    return s.Scene(geometry=geo, material=mats, camera=sc.camera, ambient=sc.ambient, hdri=sc.hdri, name=sc.name + "+1"), table


def oracle_run(sc, k, w, h, spp, mb=16, buckets=5, light_ris=0):
    """The oracle's policy.brdf = k run, in its mode-2 traversal: the twin whose shadow_rays counter is the product's (the brute-force mode also
    counts the light samples of last-bounce hits, whose paths it then drops: Q5; the accumulators of the two modes are the same words)."""
    o = ob.Oracle(sc, brdf=k, gloss_decay=DECAY if k else None, max_bounces=mb, buckets=buckets, light_ris=light_ris, trav_mode=ob.TRAV_PER_RAY_BVH)
    o.Resize(w, h); o.Accumulate(spp)
    return o


def gpu_run(mirt, sc, w, h, spp, table=None, keep=False, setup=None, accumulate=None, **kw):
    r = mirt.Renderer(sc, **{"max_bounces": 16, "use_bvh": True, "gloss_decay": DECAY, "material_closures": table, **kw})
    r.Resize(w, h)
    if setup:
        setup(r)
    (accumulate or (lambda q: q.Accumulate(spp)))(r)
    if keep:
        return r
    acc = r.accumulator()
    r.close()
    return acc


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "light_ris", "extra_first"])
@pytest.mark.parametrize("k", [0, 1], ids=["lambertian", "ggx"])
@pytest.mark.parametrize("scene_name", ["default9", "brdf_test"])
def test_pure_ends_through_the_mixed_kernels(mirt, scene_name, k, variant):
    W, H, SPP = 64, 32, 10
    sc, table = with_unused_material(mirt, getattr(mirt.scene, scene_name)(), k, at_front=variant == "extra_first")
    ris = 1 if variant == "light_ris" else 0
    o = oracle_run(sc, k, W, H, SPP, light_ris=ris)
    # policy.brdf is the OTHER closure: the table, which names every material, decides
    r = gpu_run(mirt, sc, W, H, SPP, table=table, keep=True, brdf=1 - k, light_ris=ris)
    got_table, mixed = r.material_closures()
    assert got_table == table and mixed is True
    what = f"{scene_name}, closure {k}, {variant}"
    same_words(r.accumulator(), o.accumulator(), what + ": accumulator")
    assert r.Render(); same_words(r.GetFrame(), o.Render(), what + ": frame")
    cg, co = r.counters(), o.counters()
    for name in ("rays", "shadow_rays", "terminated"):
        assert cg[name] == co[name], f"{what}: counter {name} {cg[name]} vs the oracle's {co[name]}"
    assert o.accumulator().any()
    r.close()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------
def test_uniform_table_launches_the_pure_kernels(mirt):
    W, H, SPP = 64, 32, 10
    sc = mirt.scene.default9()
    n = len(sc.material)
    ggx, lam = gpu_run(mirt, sc, W, H, SPP, brdf=1), gpu_run(mirt, sc, W, H, SPP, brdf=0)
    assert (bits(ggx) != bits(lam)).any()
    r = gpu_run(mirt, sc, W, H, SPP, table=[1] * n, keep=True, brdf=0)
    assert r.material_closures() == ([1] * n, False)
    same_words(r.accumulator(), ggx, "table [1] * n on a brdf = 0 context")
    same_words(ggx, oracle_run(sc, 1, W, H, SPP).accumulator(), "brdf = 1 against the oracle")
    r.set_material_closures(None)
    assert r.material_closures() == ([], False)
    r.ResetAccumulator(); r.Accumulate(SPP)
    same_words(r.accumulator(), lam, "table removed: brdf = 0 again")
    # a table shorter than the material list: the rest takes policy.brdf
    r.set_material_closures([0, 0]); assert r.material_closures() == ([0, 0], False)
    r.set_policy(brdf=1); assert r.material_closures() == ([0, 0], True)          # the table survives mirt_set_policy
    r.UpdateScene(); assert r.material_closures() == ([0, 0], True)                # ... and mirt_set_scene
    r.set_material_closures([1, 1]); assert r.material_closures() == ([1, 1], False)
    r.ResetAccumulator(); r.Accumulate(SPP)
    same_words(r.accumulator(), ggx, "table [1, 1] under brdf = 1")
    r.close()


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------
def first_hit_materials(r, spp):
    """[acc - 1][tile * 256 + px] -> material of the sphere the camera ray of Accumulate() call `acc` meets first (-1: none), by the product's own
    ray generation and traversal."""
    out = []
    for acc in range(1, spp + 1):
        p, d = r.debug_raygen(acc)
        prim = r.debug_trace_closest(p, d)[1]
        out.append(np.where(prim >= 0, r.prims["material_ID"][np.maximum(prim, 0)], -1))
    return np.array(out)


def sample_words(acc, spp):
    """[tile][bucket][rgb][256] with buckets = spp accumulations -> [acc - 1][tile * 256 + px][rgb] words: bucket acc % buckets holds call acc alone."""
    tiles = acc.shape[0]
    per = bits(acc).transpose(1, 0, 3, 2).reshape(spp, tiles * 256, 3)            # [bucket]
    return per[[a % spp for a in range(1, spp + 1)]]


@pytest.mark.parametrize("mb", [1, 2])
def test_first_hit_decides_exactly(mirt, mb):
    """max_bounces = 1 is the case the issue names; there every hit is the last bounce's and is dropped (Q5), so all words are +0 and the case
    shows little.  max_bounces = 2 is where the first hit's closure makes the word: its light sample, its emission, and whether the ray it
    sampled meets a sphere (the word goes back to +0) or leaves the scene."""
    W, H, SPP = 64, 64, 16
    sc = mirt.scene.default9()
    table = [m % 2 for m in range(len(sc.material))]
    kw = dict(max_bounces=mb, buckets=SPP)
    r = gpu_run(mirt, sc, W, H, SPP, table=table, keep=True, **kw)
    assert r.material_closures() == (table, True)
    mat = first_hit_materials(r, SPP)
    mixed = sample_words(r.accumulator(), SPP)
    r.close()
    pure = [sample_words(gpu_run(mirt, sc, W, H, SPP, brdf=k, **kw), SPP) for k in (0, 1)]
    assert mat.size == mixed.shape[0] * mixed.shape[1] == 65536
    closure = np.where(mat >= 0, np.array(table)[np.maximum(mat, 0)], -1)
    compared = 0
    for k in (0, 1):
        sel = closure == k
        assert sel.sum() > 0
        bad = (mixed[sel] != pure[k][sel]).any(axis=1)
        assert not bad.any(), f"max_bounces {mb}: {int(bad.sum())} of {int(sel.sum())} samples that first hit a closure-{k} material differ from the brdf = {k} run"
        compared += int(sel.sum())
    miss = closure < 0
    assert not (mixed[miss] != pure[0][miss]).any() and not (mixed[miss] != pure[1][miss]).any()
    assert compared + int(miss.sum()) == 65536                                     # none is left out
    differ = [(pure[0][closure == k] != pure[1][closure == k]).any(axis=1).mean() for k in (0, 1)]
    print(f"max_bounces {mb}: the two pure runs differ on {differ[0]:.1%} / {differ[1]:.1%} of the samples of closure 0 / 1")
    if mb == 2:
        assert min(differ) > 0.0                                                   # the comparison above could tell the closures apart


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb", [2, 3])
@pytest.mark.parametrize("k", [0, 1])
def test_the_flag_travels_with_the_sampled_ray(mirt, k, mb):
    """Scene X, table [k, 1 - k]: the ball is closure k, the emitter's material the other kind.  A ray the ball sampled carries pdf_in of closure k
    to the emitter it hits; taken from the emitter's material instead, the weight of that hit is the other closure's.
    max_bounces = 2 is the case the issue names; a hit at bounce 1 is then dropped (Q5) and never weighed, so the flag is first read at
    max_bounces = 3 (test_material_closures_cpu.py counts those hits on the oracle's paths): both run."""
    sc = scene_x(mirt)
    kw = dict(max_bounces=mb, buckets=X_SPP, mis=True)
    r = gpu_run(mirt, sc, X_W, X_H, X_SPP, table=[k, 1 - k], keep=True, brdf=0, **kw)
    assert np.array_equal(r.prims["position"], r.geometry["position"]) and list(r.lights) == [1]      # geometry order = BVH order: Q11 suppresses the emitter's NEE onto itself
    assert r.material_closures() == ([k, 1 - k], True)
    mat = first_hit_materials(r, X_SPP)
    mixed = sample_words(r.accumulator(), X_SPP)
    r.close()
    pure = sample_words(gpu_run(mirt, sc, X_W, X_H, X_SPP, brdf=k, **kw), X_SPP)
    other = sample_words(gpu_run(mirt, sc, X_W, X_H, X_SPP, brdf=1 - k, **kw), X_SPP)
    ball = mat == 0
    assert ball.sum() >= 0.25 * ball.size
    bad = (mixed[ball] != pure[ball]).any(axis=1)
    print(f"closure {k}, max_bounces {mb}: {int(ball.sum())} ball-first samples, {int(bad.sum())} differ; the other pure run differs on {(other[ball] != pure[ball]).any(axis=1).mean():.1%}")
    assert not bad.any(), f"{int(bad.sum())} of {int(ball.sum())} ball-first samples differ from the policy.brdf = {k} run"
    assert pure[ball].any()


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------
def test_mixed_white_furnace(mirt):
    """Four balls under a sky of 1, alternately Lambertian with albedo 1 and a perfect mirror (F0 = 1, roughness 0): every bucket word is
    exactly 1.0, what test_white_furnace_gpu and test_mirror_furnace_on_the_gpu demand of theirs."""
    s = mirt.scene
    mats = [s._material(albedo=(1, 1, 1)), s._material(albedo=(0, 0, 0), F0=(1, 1, 1), roughness=0.0)]
    geo = [s._sphere((x, y, 0.0), 0.3 * 0.3, i % 2) for i, (x, y) in enumerate(((-0.35, -0.35), (0.35, -0.35), (0.35, 0.35), (-0.35, 0.35)))]
    sc = s.Scene(geometry=np.array(geo, dtype=s.SPHERE), material=np.array(mats, dtype=s.MATERIAL),
                 camera=s.Camera(eye=(0, 0, 3), direction=(0, 0, -1), focal_length=50.0), ambient=np.ones(3, dtype=np.float32), name="mixed_furnace")
    for use_bvh in (False, True):
        r = gpu_run(mirt, sc, 32, 32, 5, table=[0, 1], keep=True, max_bounces=9, use_bvh=use_bvh, gloss_decay=None)
        assert r.material_closures() == ([0, 1], True)
        mat = first_hit_materials(r, 5)
        assert (mat == 0).sum() > 100 and (mat == 1).sum() > 100
        acc = r.accumulator()
        assert np.array_equal(bits(acc), bits(np.ones_like(acc)))
        assert r.Render() and np.ptp(r.GetFrame()[..., :3].reshape(-1, 3), axis=0).max() == 0.0
        r.close()


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------
def test_words_do_not_depend_on_the_route(mirt):
    W, H, N = 48, 32, 10
    sc = mirt.scene.default9()
    table = [1, 0, 1, 0, 1, 0, 1, 0, 1]

    def run(**kw):
        return gpu_run(mirt, sc, W, H, N, **{"table": table, "max_batch": 3, "buckets": 5, **kw})

    base = run()
    assert (bits(base) != bits(run(table=None, brdf=0))).any() and (bits(base) != bits(run(table=None, brdf=1))).any()
    routes = {
        "max_batch 1": dict(max_batch=1), "max_batch 5": dict(max_batch=5), "max_batch 0": dict(max_batch=0), "streams 1": dict(streams=1), "streams 3": dict(streams=3),
        "10 x async(1)": dict(accumulate=lambda r: [r.AccumulateAsync(1) for _ in range(N)]),
        "brute force": dict(use_bvh=False), "tree built on the device": dict(gpu_build=True), "traced camera rays": dict(trace_primary_rays=True),
        "set after construction": dict(table=None, setup=lambda r: r.set_material_closures(table)),
    }
    for label, kw in routes.items():
        same_words(run(**kw), base, label)
    h_tiles, v_tiles = W // 16, H // 16
    merged = np.zeros((v_tiles, h_tiles) + base.shape[1:], dtype=np.float32)
    for rank in range(2):
        merged[rank::2] = run(setup=lambda q: q.SetTileRows(rank, 2)).reshape((-1, h_tiles) + base.shape[1:])
    same_words(merged.reshape(base.shape), base, "two contexts with interleaved tile rows")
    g = mirt.GroupRenderer(sc, devices=[0, 0], max_bounces=16, buckets=5, use_bvh=True, max_batch=3, gloss_decay=DECAY, material_closures=table)
    assert g.material_closures() == (table, True)
    g.Resize(W, H); g.Accumulate(N)
    same_words(g.accumulator(), base, "a group of the same device twice")
    g.close()
    lens = dict(setup=lambda q: q.set_lens(0.05, 4.0))
    with_lens = run(**lens)
    assert (bits(with_lens) != bits(base)).any()
    same_words(run(use_bvh=False, **lens), with_lens, "lens on against lens on: tree against brute force")
    same_words(run(max_batch=1, **lens), with_lens, "lens on against lens on: batches of 1")
    # the AOV albedo plane: the colour of the first hit's closure, summed in accumulation order
    r = run(keep=True, aov=True)
    same_words(r.accumulator(), base, "AOVs on")
    mat = first_hit_materials(r, N)
    colour = np.array([sc.material["F0"][m] if table[m] else sc.material["albedo"][m] for m in range(len(table))], dtype=np.float32)
    want = np.zeros((mat.shape[1], 3), dtype=np.float32)
    for a in range(N):
        hit = mat[a] >= 0
        want[hit] = want[hit] + colour[mat[a][hit]]
    got = r.aov()[:, 4:7, :].transpose(0, 2, 1).reshape(-1, 3)
    same_words(got, want, "AOV albedo plane")
    r.close()


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------
def lit_default9(mirt):
    """default9 under a small environment map with one bright cell, so that sky sampling changes the launches."""
    sc = mirt.scene.default9()
    hdri = np.full((5, 9, 4), 0.05, dtype=np.float32); hdri[..., 3] = 1.0
    hdri[1, 6, :3] = (40.0, 35.0, 30.0)
    sc.hdri, sc.ambient = hdri, np.full(3, 0.5, dtype=np.float32)
    return sc


@pytest.mark.parametrize("switch", [dict(transmission=True), dict(sky_sampling=True), dict(transmission=True, sky_sampling=True, light_ris=4)],
                         ids=["transmission", "sky_sampling", "all_three"])
@pytest.mark.parametrize("k", [0, 1])
def test_pure_ends_with_the_other_switches(mirt, k, switch):
    W, H, SPP = 64, 32, 10
    plain = lit_default9(mirt)
    want = gpu_run(mirt, plain, W, H, SPP, brdf=k, **switch)
    assert (bits(want) != bits(gpu_run(mirt, plain, W, H, SPP, brdf=k))).any()    # the switch does something here
    for at_front in (False, True):
        sc, table = with_unused_material(mirt, plain, k, at_front)
        r = gpu_run(mirt, sc, W, H, SPP, table=table, keep=True, brdf=1 - k, **switch)
        assert r.material_closures() == (table, True)
        same_words(r.accumulator(), want, f"closure {k}, {sorted(switch)}, extra material {'first' if at_front else 'last'}")
        r.close()


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------
def test_statuses(mirt):
    lib = mirt.load_library()
    W, H = 48, 32
    sc = mirt.scene.default9()
    table = [1, 0, 1, 0, 1, 0, 1, 0, 1]
    r = gpu_run(mirt, sc, W, H, 0, table=table, keep=True, accumulate=lambda q: None, max_batch=16, streams=1)

    def raw_set(values):
        a = np.ascontiguousarray(values, dtype=np.uint8)
        return lib.mirt_set_material_closures(r._ctx, a.ctypes.data_as(C.c_void_p), len(a))

    for bad in ([2], [0, 1, 255], [0] * 64):
        assert raw_set(bad) == ERR_ARG and r.material_closures() == (table, True)          # ... and changes nothing
    assert raw_set([0] * 63) == 0 and r.material_closures() == ([0] * 63, False)
    n, mixed = C.c_uint32(9), C.c_uint32(9)
    small = np.zeros(4, dtype=np.uint8)
    assert lib.mirt_get_material_closures(r._ctx, small.ctypes.data_as(C.c_void_p), 4, C.byref(n), C.byref(mixed)) == ERR_ARG and n.value == 63
    assert lib.mirt_get_material_closures(r._ctx, None, 0, C.byref(n), C.byref(mixed)) == 0 and (n.value, mixed.value) == (63, 0)
    r.set_material_closures(table)
    # exact stream order and a non-empty table exclude each other, both ways
    assert lib.mirt_set_stream_order(r._ctx, 1) == ERR_STATE and r.stream_order == 0
    with pytest.raises(mirt.MirtError, match="mirt_set_material_closures"):
        r.set_stream_order(True)
    r.set_material_closures([]); r.set_stream_order(True)
    assert raw_set(table) == ERR_STATE and r.material_closures() == ([], False)
    with pytest.raises(mirt.MirtError, match="mirt_set_stream_order"):
        r.set_material_closures(table)
    r.set_material_closures(None)                                                          # removing it is always accepted
    r.set_stream_order(False)
    # the accumulator is not reset, and a deferred AccumulateAsync keeps the table it was issued under
    other = [0, 1, 1, 0, 0, 1, 0, 1, 0]
    r.set_material_closures(table)
    r.AccumulateAsync(3)
    r.set_material_closures(other)
    assert r.accumulations == 3
    r.AccumulateAsync(2)
    r.Synchronize()
    q = gpu_run(mirt, sc, W, H, 3, table=table, keep=True, max_batch=16, streams=1)
    q.set_material_closures(other); q.Accumulate(2)
    same_words(r.accumulator(), q.accumulator(), "deferred calls under the table they were issued under")
    assert (bits(q.accumulator()) != bits(gpu_run(mirt, sc, W, H, 5, table=other, max_batch=16, streams=1))).any()
    q.close(); r.close()
