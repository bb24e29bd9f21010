"""The records the trace kernels walk, read back from the device (Renderer.debug_tree) and audited by tests/tree_audit.py: for the host SAH
builder, the caller's tree (reference_tree) and the Morton-order builder of lbvh_build.hip, in the f32 child-pair, binary16 child-pair and
4-wide binary16 layouts.  Every condition is exact (tree_audit.audit); the GPU-built tree is also held to a numpy twin of its builder, set for
set.  The scenes are the smallest at which each thing can go wrong: one leaf, wide records with unused slots, the builders' 256-thread
block edge, a sphere of 1000 units among small ones, equal centres, a flat cloud, binary16 refused or near its limit, more records than the
u16 stack and one CU's LDS hold, and a tree 31 levels deep."""
import functools

import numpy as np
import pytest

import tree_audit as ta
import views_and_scales as views

pytestmark = pytest.mark.gpu
f32 = np.float32
BUILDERS = {"sah": {}, "reference_tree": {"reference_tree": True}, "gpu_build": {"gpu_build": True}}


def cloud_n(mirt, n):
    return views.scaled_cloud(mirt, n=n)


def equal_centres(mirt):
    sc = views.scaled_cloud(mirt, n=300)
    sc.geometry["position"][:] = f32([1.5, -2.0, 0.25])
    return sc


def coplanar(mirt):
    sc = views.scaled_cloud(mirt, n=300)
    sc.geometry["position"][:, 1] = f32(0.75)
    return sc


def deep(mirt):
    p = ta.deep_cloud()
    sc = views.scaled_cloud(mirt, n=len(p))
    sc.geometry["position"], sc.geometry["radius_sq"] = p["position"], p["radius_sq"]
    return sc


SCENES = {f"n{n}": functools.partial(cloud_n, n=n) for n in (1, 2, 3, 4, 5, 255, 256, 257)}
SCENES.update({"S1000": lambda mirt: mirt.scene.synthetic(1000), "default9": lambda mirt: mirt.scene.default9(), "n40000": functools.partial(cloud_n, n=40000),
               "equal_centres": equal_centres, "coplanar": coplanar, "deep": deep})
for _name, (_k, _offset) in views.TRANSFORMS.items():               # binary16 subnormal, coarse, near +-60000, refused (offset70000: f32 records)
    SCENES[f"scaled {_name}"] = functools.partial(lambda mirt, k, offset: views.transformed(views.scaled_cloud(mirt), k=k, offset=offset), k=_k, offset=_offset)
# where the rule of bvh_layout.hpp half_box_adequate is not borderline, the layout is known beforehand
HALF_EXPECTED = {name: 1 for name in SCENES if name.startswith("n") or name in ("equal_centres", "coplanar", "deep")}
HALF_EXPECTED.update({f"scaled {k}": v for k, v in views.HALF_BOXES_FIXED.items()})

_scene_cache, _twin_cache = {}, {}


def scene_of(mirt, name):
    if name not in _scene_cache:
        _scene_cache[name] = SCENES[name](mirt)
    return _scene_cache[name]


def twin_of(name, prims):
    """lbvh_twin over the BVH-order prims (the same array for every renderer of a scene), computed once."""
    if name not in _twin_cache:
        _twin_cache[name] = (prims.copy(), ta.lbvh_twin(prims))
    kept, tw = _twin_cache[name]
    assert np.array_equal(kept["position"], prims["position"]) and np.array_equal(kept["radius_sq"], prims["radius_sq"])
    return tw


def read_tree(r):
    """debug_tree(), with `info` held to debug_info()."""
    words, info = r.debug_tree()
    d = r.debug_info()
    assert info["records"] == d["records"] == len(words) and info["depth"] == d["depth"]
    assert int(info["layout"] >= 1) == d["half_boxes"] and int(info["layout"] == 2) == d["wide"]
    assert info["record_bytes"] == (64, 32, 64)[info["layout"]] == 4 * words.shape[1]
    return words, info


def three_layouts(mirt, monkeypatch, sc, builder, nodes=None):
    """{"f32" | "half" | "pair": (words, info, BVH-order prims, debug_info)}: binary16 refused, allowed, and allowed without wide records (MIRT_TUNE_WIDE=0, read in mirt_create)."""
    out = {}
    for key, allow_half, wide in (("f32", False, True), ("half", True, True), ("pair", True, False)):
        with monkeypatch.context() as m:
            if not wide:
                m.setenv("MIRT_TUNE_WIDE", "0")
            r = mirt.Renderer(sc, use_bvh=True, allow_half_boxes=allow_half, **BUILDERS[builder])
        if nodes is not None:
            r.UpdateScene(nodes=nodes(r))
        words, info = read_tree(r)
        out[key] = (words, info, r.prims.copy(), r.debug_info())
        r.close()
    return out


def check_scene(mirt, monkeypatch, name, builder, nodes=None, sc=None):
    sc = scene_of(mirt, name) if sc is None else sc
    n = len(sc.geometry)
    lbvh = builder == "gpu_build" and n >= 2                         # (one sphere: the host lays out the single-leaf record)
    trees = three_layouts(mirt, monkeypatch, sc, builder, nodes)
    levels = {}
    for key, (words, info, prims, dbg) in trees.items():
        print(f"{name} {builder} {key}: layout {info['layout']} records {info['records']} depth {info['depth']}")
        levels[key] = ta.audit(words, info, prims, child_order=lbvh)                              # 1
    f32_words, f32_info, prims, _ = trees["f32"]
    assert f32_info["layout"] == 0 and f32_info["records"] == max(n - 1, 1)
    depth = f32_info["depth"]
    expect_half = HALF_EXPECTED.get(name)
    if expect_half is None and views.predicted_half_boxes(sc, pad=True) == views.predicted_half_boxes(sc, pad=False):
        expect_half = views.predicted_half_boxes(sc)
    for key in ("half", "pair"):
        info = trees[key][1]
        assert info["depth"] == depth, (key, info, depth)                                         # 2: one tree, whatever the layout
        if expect_half is not None:
            assert int(info["layout"] >= 1) == expect_half, (key, info)
        if info["layout"] >= 1:                                      # 5: wide records whenever binary16 is in use and three entries per wide level fit the stack
            assert (info["layout"] == 2) == (key == "half" and 3 * (depth // 2) < 64), (key, info)
    sets32, level32 = ta.leaf_sets_by_record(f32_words, f32_info)
    for key in ("half", "pair"):
        words, info = trees[key][:2]
        sets, _ = ta.leaf_sets_by_record(words, info)
        if info["layout"] == 2:                                                                   # 2: the wide records are the odd levels of the child-pair tree
            assert set(sets) == {s for s, lv in zip(sets32, level32) if lv % 2 == 1}
            assert len(sets) == int((level32 % 2 == 1).sum())
        else:
            assert sets == sets32
    if lbvh:                                                                                      # 3: the tree is the radix tree of the twin's keys
        tw = twin_of(name, prims)
        assert set(sets32) == tw["sets"]
        assert depth == tw["depth"]
    return trees


SMALL = [name for name in SCENES if name != "n40000"]


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("name", SMALL)
def test_records_are_the_documented_tree(mirt, monkeypatch, name, builder):
    trees = check_scene(mirt, monkeypatch, name, builder)
    if name == "deep" and builder == "gpu_build":
        assert trees["f32"][1]["depth"] == 31 and trees["half"][1]["layout"] == 2 and trees["pair"][1]["layout"] == 1
    if name == "S1000" and builder == "gpu_build":                   # the 1000-unit ground sphere is split off at the root
        tw = twin_of(name, trees["f32"][2])
        large = {int(k & np.uint64(0xFFFFFFFF)) for k in tw["keys"] if int(k >> np.uint64(62)) == 1}
        assert int(np.argmax(trees["f32"][2]["radius_sq"])) in large and len(large) < 10
        assert frozenset(set(range(1000)) - large) in ta.leaf_sets(*trees["f32"][:2])      # a child of the root: bit 62 is the keys' highest


@pytest.mark.parametrize("builder", list(BUILDERS))
def test_records_of_40000_spheres(mirt, monkeypatch, builder):
    """More than 32768 records and spheres: the u32-stack plan; LDS holds only the top of the tree; about 157 workgroups of k_inner_boxes
    whose climbs meet across workgroups."""
    trees = check_scene(mirt, monkeypatch, "n40000", builder)
    for key, (words, info, prims, dbg) in trees.items():
        assert dbg["lds_records"] < dbg["records"], (key, dbg)
    assert trees["f32"][1]["records"] == 39999 > 32768 and trees["pair"][1]["records"] == 39999 and trees["pair"][1]["layout"] == 1


def test_caller_tree_with_leaves_of_several_prims(mirt, monkeypatch):
    """split_multi_prim_leaves: a caller's tree with up to five prims per leaf (the tree of test_caller_tree_with_multi_prim_leaves)."""
    sc = mirt.scene.synthetic(300, ambient=0.5)

    def nodes(r):
        n, out = len(r.prims), []

        def fill(i, a, b):
            if b - a <= 5:
                out[i] = (a, b - a)
                return
            k = len(out); out.extend([None, None])                   # children adjacent: first_id, first_id + 1
            out[i] = (k, 0)
            fill(k, a, (a + b) // 2); fill(k + 1, (a + b) // 2, b)
        out.append(None); fill(0, 0, n)
        arr = np.zeros(len(out), dtype=mirt.scene.NODE)
        arr["first_id"], arr["prim_count"] = [f for f, _ in out], [c for _, c in out]
        assert arr["prim_count"].max() == 5
        return arr
    trees = check_scene(mirt, monkeypatch, "S300 multi", "reference_tree", nodes, sc=sc)
    assert trees["f32"][1]["records"] == 299                         # every leaf of k prims became a subtree of k one-prim leaves


def test_gpu_build_is_deterministic(mirt):
    """The same bytes from every build: three UpdateScene() on one context, and a second context (the arrival protocol of k_inner_boxes and
    the integer atomics of the bounds and the histogram leave nothing to timing)."""
    sc = scene_of(mirt, "n40000")
    for allow_half in (True, False):
        r = mirt.Renderer(sc, use_bvh=True, gpu_build=True, allow_half_boxes=allow_half)
        first, info = read_tree(r)
        assert info["layout"] == (2 if allow_half else 0)
        for _ in range(3):
            r.UpdateScene()
            words, again = read_tree(r)
            assert again == info and words.tobytes() == first.tobytes()
        r.close()
        r2 = mirt.Renderer(sc, use_bvh=True, gpu_build=True, allow_half_boxes=allow_half)
        words, again = read_tree(r2)
        assert again == info and words.tobytes() == first.tobytes()
        r2.close()


def test_debug_tree_arguments(mirt):
    import ctypes as C
    r = mirt.Renderer(scene_of(mirt, "n5"), use_bvh=True)
    info = (C.c_uint32 * 4)()
    assert r._lib.mirt_debug_tree(r._ctx, None, 0, info) == 0 and info[0] >= 1 and info[1] in (32, 64)
    buf = np.zeros(info[0] * info[1] // 4, dtype=np.uint32)
    assert r._lib.mirt_debug_tree(r._ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes - 1, info) < 0
    assert b"capacity" in r._lib.mirt_last_error(r._ctx)
    assert not buf.any()
    assert r._lib.mirt_debug_tree(r._ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes, None) < 0
    assert r._lib.mirt_debug_tree(r._ctx, buf.ctypes.data_as(C.c_void_p), buf.nbytes, info) == 0 and buf.any()
    r.close()
