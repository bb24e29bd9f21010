"""tests/tree_audit.py must be able to fail.  Median-split trees over a seeded cloud are laid out here in the three record layouts by a numpy
restatement of the layout comments at the top of bvh_layout.hpp (an encoder written apart from tree_audit's decoder); the audit passes on them
and names every seeded defect.  lbvh_twin is held to hand-derived keys and trees, and the directed binary16 rounding that the GPU test
compares the builders' conversions against is checked over all 65 536 binary16 patterns and their binary32 neighbours.  No GPU."""
import numpy as np
import pytest

import tree_audit as ta

f32, f16 = np.float32, np.float16
LEAF = 0x80000000
SPHERE = np.dtype([("position", f32, 3), ("radius_sq", f32)])


def make_cloud(n, seed=3):
    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=SPHERE)
    p["position"] = rng.uniform(-6.0, 6.0, (n, 3)).astype(f32)
    p["radius_sq"] = (rng.uniform(0.5, 1.2, n) ** 2).astype(f32)
    return p


def spheres(centres, radii):
    p = np.zeros(len(centres), dtype=SPHERE)
    p["position"] = np.asarray(centres, dtype=f32)
    p["radius_sq"] = np.asarray(radii, dtype=f32) ** 2
    return p


# ---- encoder: bvh_layout.hpp's layout comments -----------------------------------------------------------------------------------------
def median_tree(prims, seed=4):
    """Binary nodes in breadth-first order over a seeded permutation of the prims, split at the median of the range:
    (kids[i] = two of ("L", prim) / ("I", node), level[i] (root = 1), lo32[i], hi32[i] = the node's binary32 box, leaf boxes)."""
    n = len(prims)
    perm = np.random.default_rng(seed).permutation(n)
    llo, lhi = ta.expected_leaf_boxes(prims["position"], prims["radius_sq"])
    ranges, level, kids = [(0, n)], [1], []
    i = 0
    while i < len(ranges):
        a, b = ranges[i]
        m = (a + b) // 2
        pair = []
        for x, y in ((a, m), (m, b)):
            if y - x == 1:
                pair.append(("L", int(perm[x])))
            else:
                ranges.append((x, y)); level.append(level[i] + 1)
                pair.append(("I", len(ranges) - 1))
        kids.append(pair)
        i += 1
    lo = [llo[perm[a:b]].min(axis=0) for a, b in ranges]
    hi = [lhi[perm[a:b]].max(axis=0) for a, b in ranges]
    return kids, level, lo, hi, (llo, lhi)


def slot_of(kid, tree, ref_of_inner):
    kids, level, lo, hi, (llo, lhi) = tree
    if kid[0] == "L":
        return llo[kid[1]], lhi[kid[1]], LEAF | kid[1]
    return lo[kid[1]], hi[kid[1]], ref_of_inner(kid[1])


def pack(layout, records):
    """records: per record a list of (lo32[3], hi32[3], ref) slots, None = unused (the empty box, slot 0's reference)."""
    n = len(records)
    words = np.zeros((n, (16, 8, 16)[layout]), dtype=np.uint32)
    for r, slots in enumerate(records):
        for k, s in enumerate(slots):
            if s is None:
                lo_b = hi_b = [0x7F7FFFFF if layout == 0 else 0x7C00] * 3
                ref = slots[0][2]
            else:
                lo, hi, ref = s
                if layout == 0:
                    lo_b, hi_b = np.asarray(lo, dtype=f32).view(np.uint32), np.asarray(hi, dtype=f32).view(np.uint32)
                else:
                    lo_b, hi_b = ta.half_down(lo).view(np.uint16), ta.half_up(hi).view(np.uint16)
            for a in range(3):
                set_plane(words, layout, r, k, 0, a, int(lo_b[a]))
                set_plane(words, layout, r, k, 1, a, int(hi_b[a]))
            words[r, ((12, 6, 12)[layout]) + k] = ref
    return words


def plane_at(layout, slot, is_hi, axis):
    """(word, shift, mask) of a plane inside its record."""
    if layout == 0:
        return axis * 4 + 2 * is_hi + slot, 0, 0xFFFFFFFF                             # q_axis = (lo0, lo1, hi0, hi1)
    if layout == 1:
        return axis * 2 + is_hi, 16 * slot, 0xFFFF                                    # (lo0 | lo1 << 16, hi0 | hi1 << 16)
    return axis * 4 + 2 * is_hi + slot // 2, 16 * (slot % 2), 0xFFFF                  # (lo k0|k1, lo k2|k3, hi k0|k1, hi k2|k3)


def get_plane(words, layout, rec, slot, is_hi, axis):
    w, sh, mask = plane_at(layout, slot, is_hi, axis)
    return (int(words[rec, w]) >> sh) & mask


def set_plane(words, layout, rec, slot, is_hi, axis, bits):
    w, sh, mask = plane_at(layout, slot, is_hi, axis)
    words[rec, w] = (int(words[rec, w]) & ~(mask << sh) & 0xFFFFFFFF) | ((bits & mask) << sh)


def lay_out(prims, layout):
    """(words, info) of the median tree over `prims` in `layout`."""
    n = len(prims)
    if n == 1:                                                   # single-leaf tree: one record, the second child empty
        llo, lhi = ta.expected_leaf_boxes(prims["position"], prims["radius_sq"])
        records = [[(llo[0], lhi[0], LEAF | 0), None] + ([None, None] if layout == 2 else [])]
        return pack(layout, records), {"records": 1, "record_bytes": (64, 32, 64)[layout], "layout": layout, "depth": 2}
    tree = median_tree(prims)
    kids, level = tree[0], tree[1]
    depth = 1 + max(level)
    if layout != 2:
        records = [[slot_of(k, tree, lambda i: i) for k in pair] for pair in kids]
    else:                                                        # a wide record: an inner node at an odd level and its inner children
        order, wide_of = [0], {0: 0}
        records = []
        for node in order:                                       # grows while it is walked: breadth-first
            flat = []
            for kid in kids[node]:
                flat += [kid] if kid[0] == "L" else kids[kid[1]]
            for kid in flat:
                if kid[0] == "I":
                    wide_of[kid[1]] = len(order); order.append(kid[1])
            slots = [slot_of(k, tree, lambda i: wide_of[i]) for k in flat]
            records.append(slots + [None] * (4 - len(slots)))
    return pack(layout, records), {"records": len(records), "record_bytes": (64, 32, 64)[layout], "layout": layout, "depth": depth}


N_CLOUD = 50
LAYOUTS = (0, 1, 2)


@pytest.fixture(scope="module")
def cloud():
    return make_cloud(N_CLOUD)


@pytest.fixture(scope="module")
def laid_out(cloud):
    return {layout: lay_out(cloud, layout) for layout in LAYOUTS}


def fresh(laid_out, layout):
    words, info = laid_out[layout]
    return words.copy(), dict(info)


def ulp_step(layout, bits, up):
    """The plane one step up / down in its own format."""
    if layout == 0:
        v = np.array(bits, dtype=np.uint32).view(f32)
        return int(np.nextafter(v, f32(np.inf if up else -np.inf)).view(np.uint32))
    v = np.array(bits, dtype=np.uint16).view(f16)
    return int(np.nextafter(v, f16(np.inf if up else -np.inf)).view(np.uint16))


def find_slot(words, info, want_leaf, skip=0):
    """(rec, slot) of the skip-th used leaf / inner slot."""
    t = ta.decode(words, info)
    rec, slot = np.nonzero((t.is_leaf == want_leaf) & ~t.is_unused)
    return int(rec[skip]), int(slot[skip])


# ---- the audit passes on sound trees ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 33, N_CLOUD])
def test_audit_passes_on_median_trees(n, layout):
    prims = make_cloud(n, seed=20 + n)
    words, info = lay_out(prims, layout)
    level = ta.audit(words, info, prims)
    assert level[0] == 1 and len(level) == info["records"]
    sets = ta.leaf_sets(words, info)
    assert frozenset(range(n)) in sets and len(sets) == info["records"]


def test_layouts_describe_the_same_tree(cloud, laid_out):
    """The wide records are the odd levels of the child-pair tree; the two child-pair layouts hold the same sets."""
    s0, l0 = ta.leaf_sets_by_record(*laid_out[0])
    s1, _ = ta.leaf_sets_by_record(*laid_out[1])
    s2, l2 = ta.leaf_sets_by_record(*laid_out[2])
    assert s0 == s1
    assert set(s2) == {s for s, lv in zip(s0, l0) if lv % 2 == 1}
    assert laid_out[2][1]["depth"] == laid_out[0][1]["depth"] and l2.max() == laid_out[0][1]["depth"] // 2
    t = ta.decode(*laid_out[2])
    used = (~t.is_unused).sum(axis=1)
    assert {2, 3, 4} >= set(used.tolist()) and (used == 3).any() and (used == 4).any()      # the seeded defects below need unused slots


# ---- every seeded defect is named -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("is_hi", (0, 1))
def test_leaf_plane_moved_inward(cloud, laid_out, layout, is_hi):
    words, info = fresh(laid_out, layout)
    rec, slot = find_slot(words, info, True, skip=5)
    bits = get_plane(words, layout, rec, slot, is_hi, 1)
    set_plane(words, layout, rec, slot, is_hi, 1, ulp_step(layout, bits, up=not is_hi))
    with pytest.raises(ta.AuditError, match="leaf box (moved inward|rounded to nearest)"):
        ta.audit(words, info, cloud)


@pytest.mark.parametrize("layout", (1, 2))
def test_half_plane_rounded_to_nearest(cloud, laid_out, layout):
    words, info = fresh(laid_out, layout)
    t = ta.decode(words, info)
    llo, lhi = ta.expected_leaf_boxes(cloud["position"], cloud["radius_sq"])
    seeded = 0
    for rec, slot in np.argwhere(t.is_leaf & ~t.is_unused):
        prim = int(t.ref[rec, slot]) & ~LEAF
        for is_hi, src, outward in ((0, llo, ta.half_down), (1, lhi, ta.half_up)):
            for a in range(3):
                near = int(ta.half_nearest(src[prim, a]).view(np.uint16))
                if near == int(outward(src[prim, a]).view(np.uint16)):
                    continue
                w = words.copy()
                set_plane(w, layout, rec, slot, is_hi, a, near)
                with pytest.raises(ta.AuditError, match="leaf box rounded to nearest, not outward"):
                    ta.audit(w, info, cloud)
                seeded += 1
    assert seeded > N_CLOUD                                     # about half of the 6 n planes round inward under round-to-nearest


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("is_hi", (0, 1))
def test_inner_box_smaller_than_the_union(cloud, laid_out, layout, is_hi):
    words, info = fresh(laid_out, layout)
    rec, slot = find_slot(words, info, False, skip=3)
    bits = get_plane(words, layout, rec, slot, is_hi, 2)
    set_plane(words, layout, rec, slot, is_hi, 2, ulp_step(layout, bits, up=not is_hi))
    with pytest.raises(ta.AuditError, match="inner box is not the union"):
        ta.audit(words, info, cloud)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_prim_referenced_twice_another_missing(cloud, laid_out, layout):
    words, info = fresh(laid_out, layout)
    (r0, s0), (r1, s1) = find_slot(words, info, True, skip=2), find_slot(words, info, True, skip=9)
    base = (12, 6, 12)[layout]
    missing = int(words[r0, base + s0]) & ~LEAF
    words[r0, base + s0] = words[r1, base + s1]
    with pytest.raises(ta.AuditError, match=rf"exactly one leaf: referenced more than once \[{int(words[r1, base + s1]) & ~LEAF}\], missing \[{missing}\]"):
        ta.audit(words, info, cloud)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_unreachable_record(cloud, laid_out, layout):
    words, info = fresh(laid_out, layout)
    words = np.concatenate([words, words[-1:]])
    info["records"] += 1
    with pytest.raises(ta.AuditError, match=f"record {info['records'] - 1} is unreachable"):
        ta.audit(words, info, cloud)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("step", (-1, 1, 2))
def test_depth_off(cloud, laid_out, layout, step):
    words, info = fresh(laid_out, layout)
    info["depth"] += step
    if layout == 2 and (info["depth"] // 2) == (laid_out[2][1]["depth"] // 2):
        ta.audit(words, info, cloud)                            # the wide condition pins depth // 2 (an odd depth one up is the same wide tree)
        return
    with pytest.raises(ta.AuditError, match=f"depth {info['depth']} is wrong"):
        ta.audit(words, info, cloud)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_depth_beyond_the_stack(cloud, laid_out, layout):
    words, info = fresh(laid_out, layout)
    info["depth"] = 64
    with pytest.raises(ta.AuditError, match="depth 64 does not fit"):
        ta.audit(words, info, cloud)


def wide_record_with(laid_out, used):
    words, info = fresh(laid_out, 2)
    t = ta.decode(words, info)
    return words, info, int(np.argmax((~t.is_unused).sum(axis=1) == used))


def test_unused_wide_slot_with_a_finite_plane(cloud, laid_out):
    for is_hi, axis in ((0, 0), (1, 2)):
        words, info, rec = wide_record_with(laid_out, 3)
        set_plane(words, 2, rec, 3, is_hi, axis, 0x3C00)
        with pytest.raises(ta.AuditError, match="unused slot with a finite plane"):
            ta.audit(words, info, cloud)
    words, info, rec = wide_record_with(laid_out, 3)
    words[rec, 12 + 3] ^= 1
    with pytest.raises(ta.AuditError, match="does not repeat slot 0's reference"):
        ta.audit(words, info, cloud)


def test_unused_slot_before_a_used_one(cloud, laid_out):
    words, info, rec = wide_record_with(laid_out, 3)
    for is_hi in (0, 1):
        for a in range(3):
            x, y = get_plane(words, 2, rec, 2, is_hi, a), get_plane(words, 2, rec, 3, is_hi, a)
            set_plane(words, 2, rec, 2, is_hi, a, y); set_plane(words, 2, rec, 3, is_hi, a, x)
    words[rec, [14, 15]] = words[rec, [15, 14]]
    with pytest.raises(ta.AuditError, match=f"unused slot before a used one: record {rec} slot 2"):
        ta.audit(words, info, cloud)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_child_index_below_its_parent(cloud, laid_out, layout):
    words, info = fresh(laid_out, layout)
    t = ta.decode(words, info)
    rec, slot = [(r, s) for r, s in np.argwhere(~t.is_leaf & ~t.is_unused) if r >= 2][0]
    words[rec, (12, 6, 12)[layout] + slot] = rec - 1
    with pytest.raises(ta.AuditError, match="child index not greater than its parent's"):
        ta.audit(words, info, cloud)
    words[rec, (12, 6, 12)[layout] + slot] = info["records"]
    with pytest.raises(ta.AuditError, match="reference out of range"):
        ta.audit(words, info, cloud)


@pytest.mark.parametrize("layout", (0, 1))
def test_records_out_of_breadth_first_order(layout):
    """Five prims, four records: 0 -> (1, 2), 1 -> (leaf, 3).  With records 2 and 3 exchanged every child still follows its parent, but a
    record of level 3 precedes one of level 2."""
    prims = make_cloud(5, seed=30)
    llo, lhi = ta.expected_leaf_boxes(prims["position"], prims["radius_sq"])
    leaf = lambda p: (llo[p], lhi[p], LEAF | p)
    box = lambda ps, ref: (llo[ps].min(axis=0), lhi[ps].max(axis=0), ref)
    info = {"records": 4, "record_bytes": (64, 32)[layout], "layout": layout, "depth": 4}
    good = pack(layout, [[box([0, 1, 2], 1), box([3, 4], 2)], [leaf(0), box([1, 2], 3)], [leaf(3), leaf(4)], [leaf(1), leaf(2)]])
    ta.audit(good, info, prims)
    bad = pack(layout, [[box([0, 1, 2], 1), box([3, 4], 3)], [leaf(0), box([1, 2], 2)], [leaf(1), leaf(2)], [leaf(3), leaf(4)]])
    with pytest.raises(ta.AuditError, match="not in breadth-first order: record 2 is at level 3, record 3 at level 2"):
        ta.audit(bad, info, prims)


def test_single_leaf_empty_child():
    prims = make_cloud(1, seed=21)
    for layout in LAYOUTS:
        words, info = lay_out(prims, layout)
        ta.audit(words, info, prims)
        w = words.copy()
        set_plane(w, layout, 0, 1, 0, 1, 0x3C00 if layout else 0x3F800000)
        with pytest.raises(ta.AuditError, match="unused slot with a finite plane"):
            ta.audit(w, info, prims)
        for depth in (1, 3) if layout != 2 else (1, 4):
            with pytest.raises(ta.AuditError, match=f"depth {depth} is wrong"):
                ta.audit(words, dict(info, depth=depth), prims)


def test_child_order_is_checked(cloud, laid_out):
    """The median trees are not ordered by half area: the order check must notice; records with the larger child first must pass it."""
    for layout in LAYOUTS:
        with pytest.raises(ta.AuditError, match="child order"):
            ta.audit(*laid_out[layout], cloud, child_order=True)
    prims = spheres([(0, 0, 0), (5, 0, 0)], [2.0, 1.0])
    llo, lhi = ta.expected_leaf_boxes(prims["position"], prims["radius_sq"])
    for layout in LAYOUTS:
        pad = [None, None] if layout == 2 else []
        good = pack(layout, [[(llo[0], lhi[0], LEAF | 0), (llo[1], lhi[1], LEAF | 1)] + pad])
        bad = pack(layout, [[(llo[1], lhi[1], LEAF | 1), (llo[0], lhi[0], LEAF | 0)] + pad])
        info = {"records": 1, "record_bytes": (64, 32, 64)[layout], "layout": layout, "depth": 2}
        ta.audit(good, info, prims, child_order=True)
        ta.audit(bad, info, prims)
        with pytest.raises(ta.AuditError, match="child order"):
            ta.audit(bad, info, prims, child_order=True)


# ---- the leaf pad ----------------------------------------------------------------------------------------------------------------------------
def test_leaf_pad_of_the_wrong_sign_or_missing_is_noticed(cloud):
    """Records laid out with the pad subtracted instead of added, or left out, fail the audit in every layout where the planes can tell:
    always in binary32; in binary16 only where a binary16 value lies between the two boxes (the pad is a hundredth of a binary16 step
    here, so the outward rounding swallows most of the differences: at least one pair of this cloud must still be caught)."""
    c, r = cloud["position"], np.sqrt(cloud["radius_sq"])
    pad = f32(2.0 ** -18) * (np.abs(c).max(axis=1) + r)
    for sign in (-1.0, 0.0):
        p = (f32(sign) * pad)[:, None]
        lo = np.nextafter((c - r[:, None]) - p, f32(-np.inf)); hi = np.nextafter((c + r[:, None]) + p, f32(np.inf))
        for layout in LAYOUTS:
            pad_slots = [None, None] if layout == 2 else []
            caught = 0
            for k in range(0, N_CLOUD - 1, 2):
                two = cloud[k:k + 2]
                words = pack(layout, [[(lo[k], hi[k], LEAF | 0), (lo[k + 1], hi[k + 1], LEAF | 1)] + pad_slots])
                info = {"records": 1, "record_bytes": (64, 32, 64)[layout], "layout": layout, "depth": 2}
                try:
                    ta.audit(words, info, two)
                except ta.AuditError as e:
                    assert "leaf box moved inward" in str(e) or "rounded to nearest" in str(e)
                    caught += 1
            assert caught == N_CLOUD // 2 if layout == 0 else caught >= 1, (sign, layout, caught)


# ---- binary16 directed rounding, exhaustively ----------------------------------------------------------------------------------------
def test_directed_rounding_over_every_half():
    bits = np.arange(65536, dtype=np.uint16)
    h = bits.view(f16)
    finite = np.isfinite(h)
    values = np.unique(h[finite].astype(np.float64))            # every finite binary16 value, ascending (+-0 once)
    assert len(values) == 2 * 31 * 1024 - 1
    grid = np.concatenate([[-np.inf], values, [np.inf]])
    x0 = h[finite].astype(f32)
    for x in (x0, np.nextafter(x0, f32(np.inf)), np.nextafter(x0, f32(-np.inf)),
              np.nextafter(np.nextafter(x0, f32(np.inf)), f32(np.inf)), (x0 * f32(1.0004883)).astype(f32), (x0 * f32(0.99951)).astype(f32)):
        x64 = x.astype(np.float64)
        want_down = grid[np.searchsorted(grid, x64, side="right") - 1]                # largest grid value <= x
        want_up = grid[np.searchsorted(grid, x64, side="left")]                       # smallest grid value >= x
        assert np.array_equal(ta.half_down(x).astype(np.float64), want_down)
        assert np.array_equal(ta.half_up(x).astype(np.float64), want_up)
    # beyond the largest half, and the signs of zero
    big = np.array([65504.0, 65505.0, 65519.0, 65520.0, 65536.0, 1e9, 3.4e38], dtype=f32)
    assert np.array_equal(ta.half_down(big).astype(np.float64), np.full(7, 65504.0))
    assert np.array_equal(ta.half_up(big).astype(np.float64), [65504.0] + [np.inf] * 6)
    assert np.array_equal(ta.half_up(-big).astype(np.float64), np.full(7, -65504.0))
    assert np.array_equal(ta.half_down(-big).astype(np.float64), [-65504.0] + [-np.inf] * 6)
    tiny = np.array([1e-10, -1e-10], dtype=f32)                                       # below the smallest subnormal 2^-24
    assert np.array_equal(ta.half_down(tiny).astype(np.float64), [0.0, -2.0 ** -24])
    assert np.array_equal(ta.half_up(tiny).astype(np.float64), [2.0 ** -24, 0.0])


# ---- lbvh_twin: known answers --------------------------------------------------------------------------------------------------------
X1023, Y1023, Z1023 = 0x24924924, 0x12492492, 0x09249249         # a coordinate of 1023 spread over every third bit, per axis


def codes_of(prims):
    return (ta.lbvh_keys(prims) >> np.uint64(32)).astype(np.int64).tolist()


def test_twin_two_spheres():
    p = spheres([(0, 0, 0), (1, 1, 1)], [0.1, 0.1])
    assert ta.lbvh_keys(p).tolist() == [0, (0x3FFFFFFF << 32) | 1]             # cell = 1: u = 0 and 1024, clamped to 1023 on the three axes
    tw = ta.lbvh_twin(p)
    assert tw["sets"] == {frozenset({0, 1})} and tw["depth"] == 2


def test_twin_three_spheres():
    p = spheres([(0, 0, 0), (2, 0, 0), (1, 0, 0)], [0.1, 0.1, 0.1])            # cell = 2: qx = 0, 1023, 512
    assert codes_of(p) == [0, X1023, 1 << 29]
    assert ta.lbvh_keys(p).tolist() == [0, (X1023 << 32) | 1, (1 << 61) | 2]
    tw = ta.lbvh_twin(p)
    assert (tw["keys"] & np.uint64(0xFFFFFFFF)).tolist() == [0, 2, 1]
    assert tw["sets"] == {frozenset({0, 1, 2}), frozenset({1, 2})} and tw["depth"] == 3     # bit 29 separates sphere 0; bit 26 the other two


def test_twin_four_spheres():
    p = spheres([(0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 4)], [0.5] * 4)
    assert codes_of(p) == [0, X1023, Y1023, Z1023]
    tw = ta.lbvh_twin(p)
    assert (tw["keys"] & np.uint64(0xFFFFFFFF)).tolist() == [0, 3, 2, 1]
    assert tw["sets"] == {frozenset({0, 1, 2, 3}), frozenset({0, 2, 3}), frozenset({0, 3})} and tw["depth"] == 4
    # quantisation truncates: 4 x 0.3 / 4 x 1024 = 307.2 -> 307 = 0b100110011
    q = spheres([(0, 0, 0), (4, 0, 0), (0, 0, f32(4.0) * f32(0.3))], [0.5] * 3)
    u = int(f32(f32(f32(4.0) * f32(0.3)) / f32(4.0)) * f32(1024.0))
    assert u == 307
    want = sum(1 << (3 * b) for b in range(10) if (u >> b) & 1)
    assert codes_of(q)[2] == want


def test_twin_equal_centres():
    """cell == 0: every code is 0, ties are broken by the index, the tree is the radix tree of 0 .. n-1."""
    p = spheres([(1.5, -2.0, 0.25)] * 5, [0.5, 0.6, 0.7, 0.8, 0.9])
    assert ta.lbvh_keys(p).tolist() == [0, 1, 2, 3, 4]
    tw = ta.lbvh_twin(p)
    assert tw["sets"] == {frozenset(range(5)), frozenset({0, 1, 2, 3}), frozenset({0, 1}), frozenset({2, 3})} and tw["depth"] == 4
    p = spheres([(1.5, -2.0, 0.25)] * 300, np.linspace(0.5, 1.2, 300))
    tw = ta.lbvh_twin(p)
    assert tw["depth"] == 10 and frozenset(range(256)) in tw["sets"] and frozenset(range(256, 300)) in tw["sets"]


def test_twin_large_sphere():
    """A radius of 32 x the others or more: key bit 30, outside the grid's bounds, a child of the root."""
    small = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1)]
    for big_r, is_large in ((100.0, True), (3.2, True), (1.9, False)):             # radii 0.1: exponent 2^-4, threshold 2^(-4 + 1) x 16 = 2
        p = spheres(small[:2] + [(1000, -1000, 1000)] + small[2:], [0.1, 0.1, big_r, 0.1, 0.1])
        assert float(ta.large_threshold(p["radius_sq"])) == 2.0
        codes = codes_of(p)
        assert [c >> 30 for c in codes] == [0, 0, int(is_large), 0, 0]
        tw = ta.lbvh_twin(p)
        if is_large:
            assert codes[4] == 0x3FFFFFFF and codes[2] == (1 << 30) | X1023 | Z1023          # the grid spans the four small spheres only; the large one is clamped into it
            assert int(tw["keys"][-1] & np.uint64(0xFFFFFFFF)) == 2
            assert frozenset({0, 1, 3, 4}) in tw["sets"]                                    # the root's other child
            lv2 = tw["level"] == 2
            assert lv2.sum() == 1 and tw["first"][lv2][0] == 0 and tw["last"][lv2][0] == 3
        else:
            assert codes[4] < 0x3FFFFFFF                                                    # an ordinary sphere stretches the grid


def test_twin_coplanar_cloud():
    rng = np.random.default_rng(8)
    c = rng.uniform(-6, 6, (200, 3)); c[:, 2] = 2.0
    p = spheres(c, rng.uniform(0.5, 1.2, 200))
    codes = np.asarray(codes_of(p))
    assert (codes & Z1023 == 0).all() and (codes & X1023).any() and (codes & Y1023).any()
    tw = ta.lbvh_twin(p)
    assert len(tw["sets"]) == 199 and frozenset(range(200)) in tw["sets"]
    # brute force: every node's set is a maximal run of sorted keys sharing a prefix
    keys = tw["keys"]
    for a, b in zip(tw["first"][:50], tw["last"][:50]):
        d = int(keys[a] ^ keys[b]).bit_length()
        assert (a == 0 or int(keys[a - 1] ^ keys[a]).bit_length() > d) and (b == 199 or int(keys[b] ^ keys[b + 1]).bit_length() > d)


def test_twin_speed_and_shape_at_40000():
    import time
    p = make_cloud(40000, seed=12)
    t0 = time.perf_counter()
    tw = ta.lbvh_twin(p)
    assert time.perf_counter() - t0 < 10.0
    assert len(tw["sets"]) == 39999 and 16 <= tw["depth"] < 64


def test_twin_deep_tree():
    p = ta.deep_cloud()
    assert sorted(codes_of(p)) == [0] + [1 << b for b in range(30)] + [0x3FFFFFFF]
    for seed in (None, 1, 2):
        q = p if seed is None else p[np.random.default_rng(seed).permutation(len(p))]
        tw = ta.lbvh_twin(q)
        assert tw["depth"] == 31 >= 28
        assert 3 * (tw["depth"] // 2) < 64                       # still shallow enough for wide records
