"""mirt_update_spheres on the GPU: after an edit the records are the documented tree of the moved spheres over the old topology (tree_audit, with
equality), and accumulator, frame, AOVs and path counters equal, word for word, those of a fresh context handed the edited arrays in the same
order; repeated refits are exact; the lifetime rules; every refusal leaves every word in place; a group equals the single context.

The scenes are the smallest at which the refit can go wrong: the single-leaf record with its empty slot, 2 and 3 spheres (a wide record with
three used slots), default9, the 1000-unit ground beside unit spheres, a tree 31 levels deep, and 300 spheres (more than one 256-thread block)."""
import ctypes as C

import numpy as np
import pytest

import tree_audit as ta
import views_and_scales as views
from test_tree_audit_gpu import BUILDERS, read_tree

pytestmark = pytest.mark.gpu
f32 = np.float32
W = H = 64
N_ACC, BUCKETS = 5, 5
ERR_ARG, ERR_STATE = -1, -3
LAYOUTS = (("f32", False, True), ("half", True, True), ("pair", True, False))      # as test_tree_audit_gpu.three_layouts


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_words(a, b, what):
    assert a.shape == b.shape and np.array_equal(words(a), words(b)), what


def deep(mirt):
    p = ta.deep_cloud()
    sc = views.scaled_cloud(mirt, n=len(p))
    sc.geometry["position"], sc.geometry["radius_sq"] = p["position"], p["radius_sq"]
    return sc


SCENES = {"n1": lambda m: views.scaled_cloud(m, n=1), "n2": lambda m: views.scaled_cloud(m, n=2), "n3": lambda m: views.scaled_cloud(m, n=3),
          "default9": lambda m: m.scene.default9(), "S1000": lambda m: m.scene.synthetic(1000), "deep": deep}


def renderer(mirt, monkeypatch, sc, allow_half, wide, **kw):
    with monkeypatch.context() as m:
        if not wide:
            m.setenv("MIRT_TUNE_WIDE", "0")                                         # read in mirt_create
        return mirt.Renderer(sc, allow_half_boxes=allow_half, **kw)


def half_ulp(x):
    """Spacing of binary16 at magnitude x (bvh_layout.hpp half_ulp_at)."""
    return 2.0 ** -24 if x < 2.0 ** -14 else 2.0 ** (np.frexp(x)[1] - 11)


def fits_binary16(position, radius_sq):
    """mirt.h: a coordinate beyond 60000 or a diameter under 8 binary16 steps at its magnitude does not fit (the rule of the GPU-build branch:
    magnitude max|c| + 1.0001 r, in binary32)."""
    for c, q in zip(np.asarray(position, dtype=f32).reshape(-1, 3), np.asarray(radius_sq, dtype=f32).reshape(-1)):
        r = np.sqrt(q)
        amax = f32(np.abs(c).max() + r * f32(1.0001))
        if amax > 60000.0 or f32(2.0) * r < 8.0 * half_ulp(float(amax)):
            return False
    return True


def edits_of(geometry):
    """The five edits of the issue as (name, geometry indices, positions, radius_sq), each applied on top of the one before."""
    pos, rsq = geometry["position"].astype(f32), geometry["radius_sq"].astype(f32)
    n, r = len(rsq), np.sqrt(rsq)
    ordinary = np.nonzero(r < 100.0)[0]
    ground = int(np.argmax(r))
    big = int(ordinary[np.argmax(r[ordinary])])
    rest = ordinary[ordinary != big] if len(ordinary) > 1 else ordinary             # (the one moved far away is the worst candidate for a small radius)
    near = int(rest[np.argmin(np.abs(pos[rest]).max(axis=1))])
    rng = np.random.default_rng(11)
    one = n // 2
    out = [("one sphere", [one], pos[[one]] + f32([0.25, -0.5, 0.125]) * r[one], None)]
    out.append(("every sphere", np.arange(n), pos + (rng.uniform(-1, 1, (n, 3)) * r[:, None]).astype(f32), None))
    out.append(("only the ground", [ground], pos[[ground]] + f32([0.0, -0.75, 0.0]) * min(r[ground], f32(4.0)), None))
    top = (pos[:, 1] + r).max()
    out.append(("well outside the old root box", [big], f32([[pos[big, 0], top + 8 * r[big] + 5, pos[big, 2]]]), None))
    out.append(("a radius shrunk by 100", [near], None, (rsq[[near]] / f32(10000.0)).astype(f32)))
    return out


# ---- 1. the records are the documented tree of the moved spheres -----------------------------------------------------------------------------
@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", list(SCENES))
def test_records_are_the_documented_tree_of_the_moved_spheres(mirt, monkeypatch, name, builder):
    for key, allow_half, wide in LAYOUTS:
        sc = SCENES[name](mirt)
        r = renderer(mirt, monkeypatch, sc, allow_half, wide, use_bvh=True, **BUILDERS[builder])
        words0, info0 = read_tree(r)
        t0 = ta.decode(words0, info0)
        ta.audit(words0, info0, r.prims)
        for what, idx, position, radius_sq in edits_of(r.geometry.copy()):
            idx = np.asarray(idx)
            new_pos = r.geometry["position"][idx] if position is None else position
            new_rsq = r.geometry["radius_sq"][idx] if radius_sq is None else radius_sq
            before, _ = read_tree(r)
            if info0["layout"] != 0 and not fits_binary16(new_pos, new_rsq):
                with pytest.raises(mirt.MirtError, match="mirt_set_scene"):
                    r.update_spheres(idx, position, radius_sq)
                same_words(read_tree(r)[0], before, f"{name} {builder} {key} {what}: a refused edit leaves the records")
                print(f"{name} {builder} {key} {what}: refused under binary16 records, as documented")
                continue
            r.update_spheres(idx, position, radius_sq)
            got, info = read_tree(r)
            assert info == info0, (name, builder, key, what)
            assert np.array_equal(r.geometry["position"][idx], new_pos) and np.array_equal(r.geometry["radius_sq"][idx], new_rsq)
            assert r.prims[r._bvh_of_geometry].tobytes() == r.geometry.tobytes()                 # both arrays edited in step
            ta.audit(got, info, r.prims, child_order=False)                                       # order is a build heuristic, not a condition
            t = ta.decode(got, info)
            assert np.array_equal(t.ref, t0.ref) and np.array_equal(t.is_unused, t0.is_unused), f"{name} {builder} {key} {what}: the topology changed"
            assert not np.array_equal(got, before), f"{name} {builder} {key} {what}: nothing was refitted"
        r.close()


# ---- 2. word for word against a fresh scene in the same order ----------------------------------------------------------------------------------
def lit_scene(mirt):
    sc = mirt.scene.default9()
    sc.ambient = np.asarray((0.4, 0.5, 0.6), dtype=f32)
    return sc


# default9: spheres 1, 2, 3 are emissive (the NEE table), 0 and 4 the large ones, 5 .. 8 the small ones
EDITS = {"emissive": ([2], [(0.25, 0.45, 0.6)], [0.09 * 0.09]),
         "plain": ([6], [(-0.1, 0.05, 0.1)], None),
         "both": ([3, 6, 0, 1], [(-0.4, 0.1, -0.3), (-0.1, 0.05, 0.1), (0.35, -1.5, 0.05), (0.2, 0.12, 0.1)], [0.07 * 0.07, 0.03 * 0.03, 1.45 * 1.45, 0.04 * 0.04])}
POLICIES = {"brute force": dict(use_bvh=False), "bvh": dict(use_bvh=True), "gpu_build": dict(use_bvh=True, gpu_build=True),
            "reference_tree": dict(use_bvh=True, reference_tree=True), "traced camera rays": dict(use_bvh=True, trace_primary_rays=True),
            "exact stream order": dict(exact_stream_order=True, aov=False), "ggx": dict(use_bvh=True, brdf=1), "light ris": dict(use_bvh=True, light_ris=4)}
CASES = [(p, e) for p in POLICIES for e in (("emissive", "plain", "both") if p == "bvh" else ("both",))]


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


def make(mirt, sc, **kw):
    kw = dict(dict(max_bounces=6, buckets=BUCKETS, aov=True), **kw)
    r = mirt.Renderer(sc, **kw)
    r.aov_on = kw["aov"]
    r.Resize(W, H)
    return r


def edited_then_fresh(mirt, edit, **kw):
    """(a, b): a renders the old scene first (so the old view's camera-ray lists exist), takes the edit and is reset; b is a fresh context handed a's
    edited arrays in a's order with a's nodes."""
    idx, position, radius_sq = EDITS[edit]
    a = make(mirt, lit_scene(mirt), **kw)
    a.Accumulate(BUCKETS)
    a.update_spheres(idx, position, radius_sq)
    a.ResetAccumulator(); a.counters_at_reset = a.counters()
    a.Accumulate(N_ACC)
    sc = lit_scene(mirt)
    sc.geometry = a.geometry.copy()
    b = make(mirt, sc, **kw)
    b.UpdateScene(nodes=a.nodes, prims=a.prims)
    b.Accumulate(N_ACC)
    assert b.prims.tobytes() == a.prims.tobytes() and b.geometry.tobytes() == a.geometry.tobytes() and np.array_equal(a.lights, b.lights)
    return a, b


@pytest.fixture(scope="module")
def unedited(mirt):
    r = make(mirt, lit_scene(mirt), use_bvh=True)
    r.Accumulate(N_ACC)
    out = outputs(r)
    r.close()
    return out


@pytest.mark.parametrize("policy,edit", CASES, ids=[f"{p}-{e}" for p, e in CASES])
def test_word_for_word_against_a_fresh_scene_in_the_same_order(mirt, unedited, policy, edit):
    a, b = edited_then_fresh(mirt, edit, **POLICIES[policy])
    oa = outputs(a)
    same_outputs(oa, outputs(b), f"{policy}, {edit}")
    if policy == "bvh":
        assert not np.array_equal(words(oa["acc"]), words(unedited["acc"])), "the control: the edit changes the picture"
    if policy in ("bvh", "gpu_build", "reference_tree"):
        rng = np.random.default_rng(3)
        n = 4096
        p = rng.uniform(-1.0, 1.0, (3, n)).astype(f32)
        d = rng.normal(size=(3, n)); d = (d / np.linalg.norm(d, axis=0)).astype(f32)
        ta_, pa = a.debug_trace_closest(p, d); tb_, pb = b.debug_trace_closest(p, d)
        same_words(ta_, tb_, "closest hits: distance"); assert np.array_equal(pa, pb)
        assert (pa >= 0).any() and len(np.unique(pa)) > 4, "the probe rays see several spheres"
        tfar = rng.uniform(0.05, 3.0, n).astype(f32)
        assert np.array_equal(a.debug_trace_shadow(p, d, tfar), b.debug_trace_shadow(p, d, tfar))
    a.close(); b.close()


# ---- 3. exactness of repeated refits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["sah", "gpu_build"])
def test_repeated_refits_are_exact(mirt, monkeypatch, builder):
    for key, allow_half, wide in LAYOUTS:
        sc = views.scaled_cloud(mirt, n=300)                                         # two 256-thread blocks of prims
        r = renderer(mirt, monkeypatch, sc, allow_half, wide, use_bvh=True, **BUILDERS[builder])
        q = renderer(mirt, monkeypatch, views.scaled_cloud(mirt, n=300), allow_half, wide, use_bvh=True, **BUILDERS[builder])
        words0, info0 = read_tree(r)
        rng = np.random.default_rng(5)
        idx = rng.permutation(300)[:120]
        home, home_rsq = r.geometry["position"][idx].copy(), r.geometry["radius_sq"][idx].copy()
        away = (home + rng.uniform(-3, 3, home.shape)).astype(f32)
        r.update_spheres(idx, away, home_rsq * f32(1.21))
        moved, _ = read_tree(r)
        assert not np.array_equal(moved, words0)
        ta.audit(moved, info0, r.prims)
        q.update_spheres(idx[:50], away[:50], home_rsq[:50] * f32(1.21))             # two calls ...
        q.update_spheres(idx[50:], away[50:], home_rsq[50:] * f32(1.21))
        same_words(read_tree(q)[0], moved, f"{builder} {key}: two calls equal the one combined call")
        r.update_spheres(idx, home, home_rsq)
        same_words(read_tree(r)[0], words0, f"{builder} {key}: away and back gives the original words")
        r.close(); q.close()


# ---- 4. lifetimes ------------------------------------------------------------------------------------------------------------------------------
def test_accumulator_stays_and_the_history_is_dropped(mirt):
    r = make(mirt, lit_scene(mirt), use_bvh=True)
    r.Accumulate(N_ACC)
    assert r.render_temporal(iterations=1) is not None and r.history_info()["valid"]
    acc, aov, count = r.accumulator(), r.aov(), r.accumulations
    r.update_spheres(*EDITS["both"])
    same_words(r.accumulator(), acc, "the accumulator is not reset"); same_words(r.aov(), aov, "nor the AOVs")
    assert r.accumulations == count == N_ACC
    assert not r.history_info()["valid"]
    r.update_spheres([], None, None)                                                  # n = 0: nothing
    r.close()


def test_deferred_accumulations_render_under_the_old_geometry(mirt):
    a = make(mirt, lit_scene(mirt), use_bvh=True)
    a.AccumulateAsync(3)                                                              # deferred (below a batch): launched by the update, under the old geometry
    a.update_spheres(*EDITS["both"])
    a.AccumulateAsync(7)
    b = make(mirt, lit_scene(mirt), use_bvh=True)
    b.Accumulate(3)
    b.update_spheres(*EDITS["both"])
    b.Accumulate(7)
    same_outputs(outputs(a), outputs(b), "asynchronous against two synchronous halves")
    sc = lit_scene(mirt); sc.geometry = a.geometry.copy()
    c = make(mirt, sc, use_bvh=True)
    c.UpdateScene(nodes=a.nodes, prims=a.prims); c.Accumulate(10)
    assert not np.array_equal(words(a.accumulator()), words(c.accumulator()))         # the first three did see the old geometry
    a.close(); b.close(); c.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------
def raw_update(r, bvh, geo, values):
    """mirt_update_spheres itself, past the binding's own checks: (code, message)."""
    b = None if bvh is None else np.ascontiguousarray(bvh, dtype=np.uint32)
    g = None if geo is None else np.ascontiguousarray(geo, dtype=np.uint32)
    v = None if values is None else np.ascontiguousarray(values, dtype=f32)
    n = max(len(x) for x in (b, g) if x is not None)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = r._lib.mirt_update_spheres(r._ctx, n, ptr(b), ptr(g), ptr(v))
    return rc, r._lib.mirt_last_error(r._ctx).decode()


def test_refusals_leave_every_word_in_place(mirt, monkeypatch):
    lib = mirt.load_library()
    ctx = C.c_void_p()
    assert lib.mirt_create(0, C.byref(ctx)) == 0
    one, v = (C.c_uint32 * 1)(0), (C.c_float * 4)(0, 0, 0, 1)
    assert lib.mirt_update_spheres(ctx, 1, one, one, v) == ERR_STATE and b"mirt_set_scene" in lib.mirt_last_error(ctx)
    lib.mirt_destroy(ctx)
    nan, inf = float("nan"), float("inf")
    ok = [(0.1, 0.2, 0.3, 0.01), (0.2, 0.3, 0.4, 0.01)]
    for key, allow_half, wide in LAYOUTS:
        r = renderer(mirt, monkeypatch, lit_scene(mirt), allow_half, wide, use_bvh=True, max_bounces=6, buckets=BUCKETS, aov=True)
        r.aov_on = True
        r.Resize(W, H); r.Accumulate(N_ACC)
        before, tree = outputs(r), read_tree(r)[0]
        refused = [((None, [1, 2], ok), ERR_ARG, "NULL"), (([1, 2], None, ok), ERR_ARG, "NULL"), (([1, 2], [1, 2], None), ERR_ARG, "NULL"),
                   (([1, 9], [1, 2], ok), ERR_ARG, "bvh_index[1] = 9"), (([1, 2], [1, 9], ok), ERR_ARG, "geometry_index[1] = 9"),
                   (([3, 3], [1, 2], ok), ERR_ARG, "bvh_index 3 occurs twice"), (([1, 2], [4, 4], ok), ERR_ARG, "geometry_index 4 occurs twice"),
                   (([1, 2], [1, 2], [ok[0], (nan, 0, 0, 1)]), ERR_ARG, "finite"), (([1, 2], [1, 2], [ok[0], (0, inf, 0, 1)]), ERR_ARG, "finite"),
                   (([1, 2], [1, 2], [ok[0], (0, 0, 0, inf)]), ERR_ARG, "finite"), (([1, 2], [1, 2], [ok[0], (0, 0, 0, -1.0)]), ERR_ARG, "radius_sq >= 0")]
        # binary16: a centre beyond 60000; a radius under 8 binary16 steps at its magnitude (at 100 a step is 1/16: a diameter of 0.4 < 0.5)
        for values in ([ok[0], (60001.0, 0, 0, 1)], [ok[0], (100.0, 0, 0, 0.04)]):
            assert not fits_binary16([v[:3] for v in values], [v[3] for v in values])
            if allow_half:
                refused.append((([1, 2], [1, 2], values), ERR_STATE, "mirt_set_scene"))
        for args, code, text in refused:
            rc, msg = raw_update(r, *args)
            assert rc == code and text in msg, (key, args, rc, msg)
        assert r._lib.mirt_update_spheres(r._ctx, 0, None, None, None) == 0
        same_words(read_tree(r)[0], tree, f"{key}: the records after the refusals")
        r.ResetAccumulator(); r.counters_at_reset = r.counters(); r.Accumulate(N_ACC)
        same_outputs(outputs(r), before, f"{key}: a render after the refusals")
        if not allow_half:                                                             # f32 records take the same edits
            assert read_tree(r)[1]["layout"] == 0
            for values in ([ok[0], (60001.0, 0, 0, 1)], [ok[0], (100.0, 0, 0, 0.04)]):
                rc, msg = raw_update(r, [1, 2], [1, 2], values)
                assert rc == 0, msg
                prims = r.prims.copy()
                prims["position"][[1, 2]] = [v[:3] for v in values]; prims["radius_sq"][[1, 2]] = [v[3] for v in values]
                words_, info = read_tree(r)
                ta.audit(words_, info, prims)
        else:
            assert read_tree(r)[1]["layout"] == (2 if wide else 1)
        with pytest.raises(ValueError):
            r.update_spheres([9], [(0, 0, 0)], [1.0])
        r.close()


# ---- 6. a group ----------------------------------------------------------------------------------------------------------------------------------
def test_three_member_group_equals_the_single_context(mirt):
    r = make(mirt, lit_scene(mirt), use_bvh=True)
    g = mirt.GroupRenderer(lit_scene(mirt), devices=(0, 0, 0), max_bounces=6, buckets=BUCKETS, aov=True)
    g.Resize(W, 48)                                                                     # three tile rows: one per member
    r.Resize(W, 48)
    for x in (r, g):
        x.Accumulate(BUCKETS); x.update_spheres(*EDITS["both"]); x.ResetAccumulator(); x.Accumulate(N_ACC)
    same_words(g.accumulator(), r.accumulator(), "group: accumulator"); same_words(g.aov(), r.aov(), "group: AOVs")
    cg, cr = g.counters(), r.counters()
    assert all(cg[k] == cr[k] for k in ("rays", "shadow_rays", "terminated", "dropped"))
    assert g.Render() and r.Render()
    same_words(g.GetFrame(), r.GetFrame(), "group: frame")
    assert g.geometry.tobytes() == r.geometry.tobytes() and g.prims.tobytes() == r.prims.tobytes()
    twice, pair, zeros = np.array([1, 1], dtype=np.uint32), np.array([1, 2], dtype=np.uint32), np.zeros(8, dtype=f32)
    with pytest.raises(mirt.MirtError, match="occurs twice"):
        g._call("update_spheres", 2, twice.ctypes.data_as(C.c_void_p), pair.ctypes.data_as(C.c_void_p), zeros.ctypes.data_as(C.c_void_p))
    g.close(); r.close()
