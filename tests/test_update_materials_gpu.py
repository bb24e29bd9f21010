"""mirt_update_materials on the GPU: the regenerated light tables are the documented ones at every size at which a wave edge, a workgroup edge,
an empty output or the totals scan can go wrong; accumulator, frame, AOVs and path counters equal, word for word, those of a fresh context handed
the edited arrays; the order with mirt_update_spheres does not matter; what is kept is kept; every refusal leaves every word in place; a group
equals the single context.

The tolerance is none: the tables are data, and a context that holds the same tables renders the same words."""
import ctypes as C

import numpy as np
import pytest

from test_tree_audit_gpu import read_tree

pytestmark = pytest.mark.gpu
f32 = np.float32
W = H = 64
N_ACC, BUCKETS = 5, 5
ERR_ARG, ERR_STATE = -1, -3
LAYOUTS = (("f32", False, True), ("half", True, True), ("pair", True, False))      # as test_update_spheres_gpu


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_words(a, b, what):
    assert a.shape == b.shape and np.array_equal(words(a), words(b)), what


def expected_tables(mirt, geometry, material):
    """What flatten_tables (mirt_set_scene) writes for lights = mirt_light_list(geometry, material): (ids, light_sphere rows, light_emit rows)."""
    ids = mirt.light_list(geometry, material).astype(np.int32)
    sphere = np.empty((len(ids), 4), dtype=f32)
    sphere[:, :3], sphere[:, 3] = geometry["position"][ids], geometry["radius_sq"][ids]
    emit = np.empty((len(ids), 4), dtype=f32)
    emit[:, :3] = material["emission"][geometry["material_ID"][ids]]
    emit[:, 3] = ids.view(f32)
    return ids, sphere, emit


def tables_are(mirt, r, what):
    ids, sphere, emit = expected_tables(mirt, r.geometry, r.material)
    t = r.lights_table()
    assert t["n_lights"] == len(ids), (what, t["n_lights"], len(ids))
    assert np.array_equal(t["ids"], ids), what
    same_words(t["sphere"], sphere, f"{what}: light_sphere"); same_words(t["emit"], emit, f"{what}: light_emit")
    assert np.array_equal(r.lights, ids), what
    return t


# ---- 1. the light tables are the documented ones ----------------------------------------------------------------------------------------------
def cloud(mirt, n):
    """n spheres of material 0 (dark); material 1 emits, material 2 emits another colour."""
    S = mirt.scene
    rng = np.random.default_rng(n)
    geo = np.zeros(n, dtype=S.SPHERE)
    geo["position"] = rng.uniform(-6.0, 6.0, (n, 3)).astype(f32)
    geo["radius_sq"] = (rng.uniform(0.5, 1.2, n) ** 2).astype(f32)
    mats = np.zeros(3, dtype=S.MATERIAL)
    mats["albedo"] = 0.5
    mats["emission"][1], mats["emission"][2] = (1.0, 2.0, 3.0), (0.0, 0.0, 0.5)
    cam = S.Camera(eye=(0.0, 0.0, 14.0), direction=(0.0, 0.0, -1.0), focal_length=50.0, exposure=1.0)
    return S.Scene(geo, mats, cam, np.full(3, 0.3, dtype=f32), name=f"cloud{n}")


def patterns(n, block):
    """name -> material id per sphere (0 dark, 1 and 2 emitting)."""
    idx = np.arange(n)
    edge = block if n > block else 64 if n > 64 else n // 2
    run = (idx >= max(edge - 3, 0)) & (idx < edge + 3)
    rng = np.random.default_rng(17)
    one_percent = np.zeros(n, dtype=bool)
    one_percent[rng.permutation(n)[: max(n // 100, 1)]] = True
    out = {"none": np.zeros(n, dtype=bool), "all": np.ones(n, dtype=bool), "only the first": idx == 0, "only the last": idx == n - 1,
           "alternating": (idx & 1) == 1, "one run straddling an edge": run, "1 % at random": one_percent}
    return {k: np.where(v, 1 + (idx % 2), 0).astype(np.int32) for k, v in out.items()}


def compaction_shape(mirt):
    r = mirt.Renderer(cloud(mirt, 2), use_bvh=False)
    t = r.lights_table()
    r.close()
    return t["block"], t["scan_pass"]


SIZES = ["1", "2", "63", "64", "65", "255", "256", "257", "B-1", "B", "B+1", "2B+37", "BP+1"]


@pytest.mark.parametrize("size", SIZES)
def test_the_light_tables_are_the_documented_ones(mirt, size):
    B, P = compaction_shape(mirt)
    assert B >= 64 and B % 64 == 0 and P >= 1
    n = int(eval(size.replace("2B", "2*B").replace("BP", "B*P"), {"B": B, "P": P}))
    r = mirt.Renderer(cloud(mirt, n), use_bvh=True)
    assert r.lights_table()["n_lights"] == 0
    everyone = np.arange(n)
    for k, (name, ids) in enumerate(patterns(n, B).items()):
        emission = f32([0.25 * (k + 1), 1.0, 3.0 - 0.125 * k])
        row = r.material[1].copy(); row["emission"] = emission
        r.update_materials({1: row}, (everyone, ids))
        assert np.array_equal(r.geometry["material_ID"], ids) and np.array_equal(r.prims["material_ID"][r._bvh_of_geometry], ids)
        t = tables_are(mirt, r, f"n = {n}, {name}")
        assert t["n_lights"] == int((ids > 0).sum())
        r.update_materials(None, (everyone, ids))                                  # again: the same words
        u = r.lights_table()
        same_words(u["sphere"], t["sphere"], f"n = {n}, {name}: a second run"); same_words(u["emit"], t["emit"], f"n = {n}, {name}: a second run")
    r.close()


# ---- 2. word for word against a fresh context -------------------------------------------------------------------------------------------------
def default9(mirt, variant=""):
    """default9 under an ambient sky: materials 1, 2, 3 emit (spheres 1, 2, 3), 5 and 7 are glass."""
    sc = mirt.scene.default9()
    sc.ambient = np.asarray((0.4, 0.5, 0.6), dtype=f32)
    if variant == "no glass":
        sc.material["transmission"] = 0.0
    elif variant == "one glass":
        sc.material["transmission"][7] = 0.0
    return sc


def s300(mirt, variant=""):
    """synthetic(300) under an ambient sky: material 16 emits (spheres 63, 127, 191, 255).  "dark": nothing emits."""
    sc = mirt.scene.synthetic(300, ambient=0.5)
    sc.material["F0"][:16] = 0.04
    sc.material["roughness"] = 0.6
    if variant == "dark":
        sc.material["emission"] = 0.0
    elif variant == "one glass":
        sc.material["transmission"][3], sc.material["IOR_minus_one"][3] = 0.9, 0.5
    return sc


def row(material, m, **fields):
    out = material[m].copy()
    for k, v in fields.items():
        out[k] = v
    return out


def edits_default9(mat):
    return {
        "a recolour": ("", {2: row(mat, 2, emission=(5.0, 40.0, 10.0))}, None),
        "b dark emits": ("", {6: row(mat, 6, emission=(3.0, 2.0, 1.0))}, None),
        "c lights out": ("", {m: row(mat, m, emission=(0.0, 0.0, 0.0)) for m in (1, 2, 3)}, None),
        "d reassign": ("", None, {2: 4, 6: 3}),
        "e surface only": ("", {0: row(mat, 0, albedo=(0.9, 0.3, 0.2), F0=(0.5, 0.6, 0.7), roughness=0.4), 4: row(mat, 4, albedo=(0.2, 0.7, 0.3), roughness=0.3)}, None),
        "f first glass": ("no glass", {5: row(mat, 5, transmission=(0.9, 0.9, 0.9), IOR_minus_one=0.5)}, None),
        "g last glass": ("one glass", {5: row(mat, 5, transmission=(0.0, 0.0, 0.0))}, None),
    }


def edits_s300(mat):
    return {
        "a recolour": ("", {16: row(mat, 16, emission=(5.0, 40.0, 10.0))}, None),
        "b dark emits": ("dark", {16: row(mat, 16, emission=(20.0, 20.0, 20.0))}, None),             # the scene's first lights: the MIS guard flips
        "c lights out": ("", {16: row(mat, 16, emission=(0.0, 0.0, 0.0))}, None),
        "d reassign": ("", None, {63: 1, 10: 16}),
        "e surface only": ("", {m: row(mat, m, albedo=(0.9, 0.1 * m, 0.2), F0=(0.5, 0.6, 0.7), roughness=0.2 + 0.1 * m) for m in range(4)}, None),
        "f first glass": ("", {3: row(mat, 3, transmission=(0.9, 0.9, 0.9), IOR_minus_one=0.5)}, None),
        "g last glass": ("one glass", {3: row(mat, 3, transmission=(0.0, 0.0, 0.0))}, None),
    }


SCENES = {"default9": (default9, edits_default9), "S300": (s300, edits_s300)}
CONFIGS = {"brdf 0": dict(use_bvh=True), "brdf 1": dict(use_bvh=True, brdf=1),
           "mixed": dict(use_bvh=True, material_closures=[0, 1] * 4), "transmission": dict(use_bvh=True, transmission=True),
           "sky sampling": dict(use_bvh=True, sky_sampling=True), "light ris 4": dict(use_bvh=True, light_ris=4),
           "ggx pdf": dict(use_bvh=True, brdf=1, ggx_pdf=True), "exact stream order": dict(exact_stream_order=True, aov=False)}
EDITS = ("a recolour", "b dark emits", "c lights out", "d reassign", "e surface only")
CASES = [(s, c, e) for s in SCENES for c in CONFIGS for e in EDITS + (("f first glass", "g last glass") if c == "transmission" else ())]


def outputs(r):
    assert r.Render()
    c, base = r.counters(), getattr(r, "counters_at_reset", {})                       # the counters run on over a reset: those since the last one
    out = dict(acc=r.accumulator(), frame=r.GetFrame().copy(), counters={k: c[k] - base.get(k, 0) for k in ("rays", "shadow_rays", "terminated", "dropped")})
    if r.aov_on:
        out["aov"] = r.aov()
    return out


def same_outputs(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if k == "counters":
            assert a[k] == b[k], (what, a[k], b[k])
        else:
            same_words(a[k], b[k], f"{what}: {k}")


def make(mirt, sc, cls=None, **kw):
    kw = dict(dict(max_bounces=6, buckets=BUCKETS, aov=True), **kw)
    r = (cls or mirt.Renderer)(sc, **kw)
    r.aov_on = kw["aov"]
    r.Resize(W, H)
    return r


def fresh_like(mirt, a, sc, **kw):
    """A fresh context handed a's edited arrays in a's order with a's nodes; its lights are mirt_light_list of them."""
    sc.geometry, sc.material = a.geometry.copy(), a.material.copy()
    b = make(mirt, sc, **kw)
    b.UpdateScene(nodes=a.nodes, prims=a.prims)
    assert b.prims.tobytes() == a.prims.tobytes() and b.geometry.tobytes() == a.geometry.tobytes() and b.material.tobytes() == a.material.tobytes()
    assert np.array_equal(a.lights, b.lights)
    return b


def edited_then_fresh(mirt, scene, edit, **kw):
    build, edits = SCENES[scene]
    variant, materials, spheres = edits(build(mirt).material)[edit]
    a = make(mirt, build(mirt, variant), **kw)
    a.Accumulate(BUCKETS)                                                             # the old scene is rendered first: its camera-ray lists exist
    lights_before = len(a.lights)
    a.update_materials(materials, spheres)
    a.ResetAccumulator(); a.counters_at_reset = a.counters()
    a.Accumulate(N_ACC)
    b = fresh_like(mirt, a, build(mirt, variant), **kw)
    b.Accumulate(N_ACC)
    return a, b, lights_before


@pytest.fixture(scope="module")
def unedited(mirt):
    out = {}
    for name, (build, _) in SCENES.items():
        r = make(mirt, build(mirt), use_bvh=True)
        r.Accumulate(N_ACC)
        out[name] = outputs(r)
        r.close()
    return out


@pytest.mark.parametrize("scene,config,edit", CASES, ids=[f"{s}-{c}-{e}" for s, c, e in CASES])
def test_word_for_word_against_a_fresh_context(mirt, unedited, scene, config, edit):
    a, b, lights_before = edited_then_fresh(mirt, scene, edit, **CONFIGS[config])
    tables_are(mirt, a, f"{scene}, {config}, {edit}")
    oa = outputs(a)
    same_outputs(oa, outputs(b), f"{scene}, {config}, {edit}")
    if config == "mixed":
        assert a.material_closures()[1], "the table ends MIXED"
    if edit[0] == "b":
        assert len(a.lights) > lights_before and (scene != "S300" or lights_before == 0)
    if edit[0] == "c":
        assert len(a.lights) == 0 and lights_before > 0
    if edit[0] == "d":
        assert len(a.lights) == lights_before and not np.array_equal(a.lights, mirt.light_list(SCENES[scene][0](mirt).geometry, a.material))
    if config == "brdf 0" and edit[0] in "acde":
        assert not np.array_equal(words(oa["acc"]), words(unedited[scene]["acc"])), "the control: the edit changes the picture"
    a.close(); b.close()


def test_all_three_record_layouts(mirt, monkeypatch):
    _, materials, spheres = edits_default9(default9(mirt).material)["d reassign"]
    for key, allow_half, wide in LAYOUTS:
        with monkeypatch.context() as m:
            if not wide:
                m.setenv("MIRT_TUNE_WIDE", "0")                                     # read in mirt_create
            kw = dict(use_bvh=True, allow_half_boxes=allow_half)
            a = make(mirt, default9(mirt), **kw)
            a.Accumulate(BUCKETS)
            tree = read_tree(a)
            a.update_materials(materials, spheres)
            a.ResetAccumulator(); a.counters_at_reset = a.counters(); a.Accumulate(N_ACC)
            b = fresh_like(mirt, a, default9(mirt), **kw)
            b.Accumulate(N_ACC)
        assert read_tree(a)[1]["layout"] == (0 if not allow_half else 2 if wide else 1)
        same_words(read_tree(a)[0], tree[0], f"{key}: the records are not touched")
        same_outputs(outputs(a), outputs(b), key)
        a.close(); b.close()


# ---- 3. the order with the sibling update ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("materials_first", [True, False])
def test_order_with_update_spheres(mirt, materials_first):
    """Sphere 6 becomes a light and is moved and grown; sphere 2, moved too, stops being one.  update_spheres patches the rows of the lights it
    knows by the ids read back; update_materials regenerates the rows from the geometry-order table update_spheres keeps current."""
    move = ([6, 2], [(-0.1, 0.05, 0.1), (0.25, 0.45, 0.6)], [0.04 * 0.04, 0.09 * 0.09])
    a = make(mirt, default9(mirt), use_bvh=True)
    a.Accumulate(BUCKETS)
    if materials_first:
        a.update_materials(None, {2: 4, 6: 3}); a.update_spheres(*move)
    else:
        a.update_spheres(*move); a.update_materials(None, {2: 4, 6: 3})
    tables_are(mirt, a, "after both updates")
    assert 6 in a.lights and 2 not in a.lights
    a.ResetAccumulator(); a.counters_at_reset = a.counters(); a.Accumulate(N_ACC)
    b = fresh_like(mirt, a, default9(mirt), use_bvh=True)
    b.Accumulate(N_ACC)
    same_outputs(outputs(a), outputs(b), f"materials first = {materials_first}")
    a.close(); b.close()


# ---- 4. what is kept ---------------------------------------------------------------------------------------------------------------------------
def test_lists_tree_history_and_accumulator_are_kept(mirt):
    r = make(mirt, default9(mirt), use_bvh=True)
    r.Accumulate(N_ACC)
    assert r.render_temporal(iterations=1) is not None and r.history_info()["valid"]
    hist, tree = r.debug_primary_lists(), read_tree(r)[0]
    acc, aov, count = r.accumulator(), r.aov(), r.accumulations
    _, materials, spheres = edits_default9(r.material)["d reassign"]
    r.update_materials({6: row(r.material, 6, emission=(3.0, 2.0, 1.0))}, spheres)
    same_words(r.accumulator(), acc, "the accumulator is not reset"); same_words(r.aov(), aov, "nor the AOVs")
    assert r.accumulations == count == N_ACC
    assert r.history_info()["valid"], "the history is kept: surfaces did not move"
    assert r.debug_primary_lists() == hist
    same_words(read_tree(r)[0], tree, "the records")
    r.update_materials(None, None)                                                      # both counts 0: nothing
    r.update_materials({}, ([], []))
    r.close()


def test_deferred_accumulations_render_under_the_old_materials(mirt):
    edit = ({6: row(default9(mirt).material, 6, emission=(3.0, 2.0, 1.0))}, {2: 4})
    a = make(mirt, default9(mirt), use_bvh=True)
    a.AccumulateAsync(3)                                                              # deferred (below a batch): launched by the update, under the old materials
    a.update_materials(*edit)
    a.AccumulateAsync(7)
    b = make(mirt, default9(mirt), use_bvh=True)
    b.Accumulate(3)
    b.update_materials(*edit)
    b.Accumulate(7)
    same_outputs(outputs(a), outputs(b), "asynchronous against two synchronous halves")
    c = fresh_like(mirt, a, default9(mirt), use_bvh=True)
    c.Accumulate(10)
    assert not np.array_equal(words(a.accumulator()), words(c.accumulator()))         # the first three did see the old materials
    a.close(); b.close(); c.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------
def raw_update(mirt, r, mi, rows, b, g, ids):
    """mirt_update_materials itself, past the binding's own checks: (code, message).  None = a NULL array; the count is the longest array's."""
    arr = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)
    mi, rows, b, g, ids = arr(mi, np.uint32), arr(rows, mirt.scene.MATERIAL), arr(b, np.uint32), arr(g, np.uint32), arr(ids, np.int32)
    n_rows = max([len(x) for x in (mi, rows) if x is not None], default=0)
    n_assign = max([len(x) for x in (b, g, ids) if x is not None], default=0)
    ptr = lambda a: None if a is None or len(a) == 0 else a.ctypes.data_as(C.c_void_p)
    rc = r._lib.mirt_update_materials(r._ctx, n_rows, ptr(mi), ptr(rows), n_assign, ptr(b), ptr(g), ptr(ids))
    return rc, r._lib.mirt_last_error(r._ctx).decode()


@pytest.mark.parametrize("transmission", [False, True])
def test_refusals_leave_every_word_in_place(mirt, transmission):
    lib = mirt.load_library()
    ctx = C.c_void_p()
    assert lib.mirt_create(0, C.byref(ctx)) == 0
    one, info = (C.c_uint32 * 1)(0), (C.c_uint32 * 4)()
    blank = np.zeros(1, dtype=mirt.scene.MATERIAL)
    assert lib.mirt_update_materials(ctx, 1, one, blank.ctypes.data_as(C.c_void_p), 0, None, None, None) == ERR_STATE and b"mirt_set_scene" in lib.mirt_last_error(ctx)
    assert lib.mirt_debug_lights(ctx, None, None, None, 0, info) == ERR_STATE
    lib.mirt_destroy(ctx)

    kw = dict(use_bvh=True, transmission=transmission)
    r, control = make(mirt, default9(mirt), **kw), make(mirt, default9(mirt), **kw)
    for x in (r, control):
        x.Accumulate(N_ACC)
    before, tree = r.lights_table(), read_tree(r)[0]
    mat = r.material
    ok_rows, two = [mat[0], mat[4]], [mat[0], mat[4]]
    refused = [((None, ok_rows, None, None, None), "NULL"), (([0, 4], None, None, None, None), "NULL"),
               ((None, None, None, [1, 2], [0, 0]), "NULL"), ((None, None, [1, 2], None, [0, 0]), "NULL"), ((None, None, [1, 2], [1, 2], None), "NULL"),
               (([0, 9], two, None, None, None), "material_index[1] = 9"), (([4, 4], two, None, None, None), "material_index 4 occurs twice"),
               ((None, None, [1, 9], [1, 2], [0, 0]), "bvh_index[1] = 9"), ((None, None, [1, 2], [1, 9], [0, 0]), "geometry_index[1] = 9"),
               ((None, None, [3, 3], [1, 2], [0, 0]), "bvh_index 3 occurs twice"), ((None, None, [1, 2], [4, 4], [0, 0]), "geometry_index 4 occurs twice"),
               ((None, None, [1, 2], [1, 2], [0, 9]), "material_ID[1] = 9"), ((None, None, [1, 2], [1, 2], [0, -1]), "material_ID[1] = -1"),
               # a good half does not carry a bad one: nothing of the call is applied
               (([2], [row(mat, 2, emission=(9.0, 9.0, 9.0))], [1, 2], [1, 2], [0, 9]), "material_ID[1] = 9")]
    glass = [(([5], [row(mat, 5, transmission=(1.5, 0.0, 0.0))], None, None, None), "transmission[0]"),
             (([2, 5], [row(mat, 2, emission=(9.0, 9.0, 9.0)), row(mat, 5, IOR_minus_one=-1.0)], None, None, None), "IOR_minus_one"),
             (([0], [row(mat, 0, transmission=(0.5, 0.5, 0.5), IOR_minus_one=float("nan"))], None, None, None), "IOR_minus_one")]
    for args, text in refused + (glass if transmission else []):
        rc, msg = raw_update(mirt, r, *args)
        assert rc == ERR_ARG and text in msg, (args, rc, msg)
    assert raw_update(mirt, r, None, None, None, None, None)[0] == 0                  # both counts 0
    small = np.zeros(2, dtype=np.int32)
    assert r._lib.mirt_debug_lights(r._ctx, small.ctypes.data_as(C.c_void_p), None, None, 2, info) == ERR_ARG and info[0] == 3
    with pytest.raises(ValueError):
        r.update_materials({9: mat[0]})
    with pytest.raises(ValueError):
        r.update_materials(None, {9: 0})
    after = r.lights_table()
    for k in ("ids", "sphere", "emit"):
        same_words(after[k], before[k], f"the light tables after the refusals: {k}")
    same_words(read_tree(r)[0], tree, "the records after the refusals")
    assert r.material.tobytes() == control.material.tobytes() and r.geometry.tobytes() == control.geometry.tobytes()
    for x in (r, control):
        x.Accumulate(N_ACC)                                                           # on top of the accumulator in place
    same_outputs(outputs(r), outputs(control), "a further accumulation and a render after the refusals")
    if not transmission:                                                              # with the switch off glass is not asked about
        for args, _ in glass:
            rc, msg = raw_update(mirt, r, *args)
            assert rc == 0, msg
    r.close(); control.close()


# ---- 6. a group ----------------------------------------------------------------------------------------------------------------------------------
def test_a_group_equals_the_single_context(mirt):
    kw = dict(use_bvh=True, material_closures=[0, 1] * 4)                             # MIXED: the gather context's AOV colour follows the edited rows
    r = make(mirt, default9(mirt), **kw)
    g = make(mirt, default9(mirt), cls=mirt.GroupRenderer, devices=(0, 0), **kw)
    edit = ({6: row(r.material, 6, emission=(3.0, 2.0, 1.0)), 0: row(r.material, 0, albedo=(0.9, 0.3, 0.2), F0=(0.5, 0.6, 0.7))}, {2: 4})
    for x in (r, g):
        x.Accumulate(BUCKETS); x.update_materials(*edit); x.ResetAccumulator(); x.Accumulate(N_ACC)
    same_words(g.accumulator(), r.accumulator(), "group: accumulator"); same_words(g.aov(), r.aov(), "group: AOVs")
    cg, cr = g.counters(), r.counters()
    assert all(cg[k] == cr[k] for k in ("rays", "shadow_rays", "terminated", "dropped"))
    assert g.Render() and r.Render()
    same_words(g.GetFrame(), r.GetFrame(), "group: frame")
    same_words(g.render_aov(mirt.AOV_ALBEDO), r.render_aov(mirt.AOV_ALBEDO), "group: the albedo plane resolved on the gather context")
    tg, tr = g.lights_table(), r.lights_table()
    for k in ("ids", "sphere", "emit"):
        same_words(tg[k], tr[k], f"group: light tables, {k}")
    assert g.material.tobytes() == r.material.tobytes() and g.geometry.tobytes() == r.geometry.tobytes() and np.array_equal(g.lights, r.lights)
    twice = np.array([4, 4], dtype=np.uint32)
    rows = np.ascontiguousarray([r.material[4], r.material[4]], dtype=mirt.scene.MATERIAL)
    with pytest.raises(mirt.MirtError, match="occurs twice"):
        g._call("update_materials", 2, twice.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p), 0, None, None, None)
    g.close(); r.close()
