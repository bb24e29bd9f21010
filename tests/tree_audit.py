"""Decoder and checker of the traversal records (Renderer.debug_tree), and a numpy twin of the Morton-order builder.  No GPU needed.

decode()      the three layouts of bvh_layout.hpp (f32 child pairs, binary16 child pairs, 4-wide binary16) as one form: slots of
              (lo[3], hi[3] decoded exactly to float64, ref, is_leaf, is_unused) per record.
audit()       walks the records from record 0 and raises AuditError unless they are the conservative tree bvh_layout.hpp promises.  Every
              condition is exact: the build is compiled with -ffp-contract=off and correctly rounded sqrt / divide, so binary32 numpy
              reproduces the builders' arithmetic and equality is the right assertion.
leaf_sets()   the set of prims below every record.
lbvh_twin()   lbvh_build.hip's k_leaf_boxes .. k_karras restated: Morton keys in binary32 numpy, then the binary radix tree over the
              sorted keys (split every range at its highest differing bit).  Independent of the device sort: keys are unique.
"""
import numpy as np

f32, f16 = np.float32, np.float16
LEAF_BIT = 0x80000000
HALF_INF = 0x7C00
FLT_MAX_BITS = 0x7F7FFFFF
STACK = 64                                                    # MIRT_BVH_STACK
LAYOUT_NAMES = ("f32 child-pair", "binary16 child-pair", "4-wide binary16")
AXES = "xyz"


class AuditError(AssertionError):
    pass


# ---- binary16 with directed rounding, from np.float16 and np.nextafter alone ---------------------------------------------------------
def half_down(x):
    """Largest binary16 <= x (x: binary32 array, no NaN)."""
    x = np.asarray(x, dtype=f32)
    with np.errstate(over="ignore"):
        h = x.astype(f16)
        return np.where(h.astype(f32) > x, np.nextafter(h, f16(-np.inf)), h).astype(f16)


def half_up(x):
    """Smallest binary16 >= x."""
    x = np.asarray(x, dtype=f32)
    with np.errstate(over="ignore"):
        h = x.astype(f16)
        return np.where(h.astype(f32) < x, np.nextafter(h, f16(np.inf)), h).astype(f16)


def half_nearest(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=f32).astype(f16)


# ---- the leaf box of build_records / k_leaf_boxes, binary32 ------------------------------------------------------------------------------
def expected_leaf_boxes(position, radius_sq):
    """r = sqrt(radius_sq), pad = 2^-18 (max|c| + r), one step outward of (c - r) - pad and (c + r) + pad: (lo[n, 3], hi[n, 3]) binary32."""
    c = np.ascontiguousarray(position, dtype=f32).reshape(-1, 3)
    r = np.sqrt(np.ascontiguousarray(radius_sq, dtype=f32).reshape(-1))
    pad = f32(2.0 ** -18) * (np.abs(c).max(axis=1) + r)
    lo = np.nextafter((c - r[:, None]) - pad[:, None], f32(-np.inf))
    hi = np.nextafter((c + r[:, None]) + pad[:, None], f32(np.inf))
    assert lo.dtype == f32 and hi.dtype == f32
    return lo, hi


def half_area(lo, hi):
    """(dx dy + dy dz) + dz dx in binary32 (lbvh_build.hip half_area)."""
    d = (hi - lo).astype(f32)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    with np.errstate(over="ignore", invalid="ignore"):
        return ((dx * dy + dy * dz) + dz * dx).astype(f32)


# ---- decoder -------------------------------------------------------------------------------------------------------------------------
class Tree:
    """layout, n, slots (2 or 4); lo_bits / hi_bits [n, slots, 3] raw planes (u32 of the binary32, or the binary16 pattern);
    lo / hi the same decoded to float64; ref [n, slots]; is_leaf, is_unused [n, slots]."""


def decode(words, info):
    words = np.ascontiguousarray(words, dtype=np.uint32)
    layout, n = int(info["layout"]), int(info["records"])
    want_words = (16, 8, 16)[layout]
    if words.shape != (n, want_words) or int(info["record_bytes"]) != 4 * want_words:
        raise AuditError(f"records shaped {words.shape} with {info['record_bytes']} bytes each: {LAYOUT_NAMES[layout]} records are [{n}, {want_words}]")
    t = Tree()
    t.layout, t.n, t.slots = layout, n, (2, 2, 4)[layout]
    if layout == 0:
        planes = words[:, :12].reshape(n, 3, 4)                                       # [rec, axis, (lo0, lo1, hi0, hi1)]
        t.lo_bits = planes[:, :, 0:2].transpose(0, 2, 1).copy()
        t.hi_bits = planes[:, :, 2:4].transpose(0, 2, 1).copy()
        t.lo = t.lo_bits.view(f32).astype(np.float64)
        t.hi = t.hi_bits.view(f32).astype(np.float64)
        t.ref = words[:, 12:14].copy()
        empty = FLT_MAX_BITS
    else:
        if layout == 1:
            planes = words[:, :6].reshape(n, 3, 2)                                    # [rec, axis, (lo0 | lo1 << 16, hi0 | hi1 << 16)]
            lo_w, hi_w = planes[:, :, 0:1], planes[:, :, 1:2]
            t.ref = words[:, 6:8].copy()
        else:
            planes = words[:, :12].reshape(n, 3, 4)                                   # [rec, axis, (lo k0|k1, lo k2|k3, hi k0|k1, hi k2|k3)]
            lo_w, hi_w = planes[:, :, 0:2], planes[:, :, 2:4]
            t.ref = words[:, 12:16].copy()
        split = lambda w: np.stack([w & 0xFFFF, w >> 16], axis=-1).reshape(n, 3, -1).transpose(0, 2, 1).astype(np.uint16)
        t.lo_bits, t.hi_bits = split(lo_w), split(hi_w)
        t.lo = t.lo_bits.view(f16).astype(np.float64)
        t.hi = t.hi_bits.view(f16).astype(np.float64)
        empty = HALF_INF
    t.empty_bits = empty
    # a slot is unused when any of its planes carries the layout's empty marker (no box of a sphere has one: audit() then asks for all six)
    t.is_unused = ((t.lo_bits == empty) | (t.hi_bits == empty)).any(axis=2)
    t.is_leaf = (t.ref & LEAF_BIT) != 0
    return t


def _where(rec, slot):
    return f"record {int(rec)} slot {int(slot)}"


def _walk(t):
    """Levels of the records (root = 1) by a breadth-first walk from record 0, one numpy step per level; raises on structural defects."""
    n = t.n
    level = np.zeros(n, dtype=np.int64)
    if n == 0:
        raise AuditError("no records")
    level[0] = 1
    frontier = np.array([0], dtype=np.int64)
    inner = ~t.is_leaf & ~t.is_unused
    depth = 1
    while len(frontier):
        rec, slot = np.nonzero(inner[frontier])
        parent = frontier[rec]
        child = t.ref[parent, slot].astype(np.int64)
        bad = child >= n
        if bad.any():
            k = np.argmax(bad)
            raise AuditError(f"reference out of range: {_where(parent[k], slot[k])} points at record {child[k]} of {n}")
        bad = child <= parent
        if bad.any():
            k = np.argmax(bad)
            raise AuditError(f"child index not greater than its parent's: {_where(parent[k], slot[k])} points at record {child[k]}")
        uniq, counts = np.unique(child, return_counts=True)
        if (counts > 1).any() or (level[uniq] != 0).any():
            k = uniq[np.argmax((counts > 1) | (level[uniq] != 0))]
            raise AuditError(f"record {k} is reached more than once")
        depth += 1
        level[child] = depth
        frontier = np.sort(child)
    if (level == 0).any():
        raise AuditError(f"record {int(np.argmax(level == 0))} is unreachable from record 0 ({int((level == 0).sum())} of {n} are)")
    if (np.diff(level) < 0).any():
        k = int(np.argmax(np.diff(level) < 0))
        raise AuditError(f"records are not in breadth-first order: record {k} is at level {level[k]}, record {k + 1} at level {level[k + 1]}")
    return level


def record_levels(words, info):
    return _walk(decode(words, info))


def _check_unused(t):
    un = t.is_unused
    if not un.any():
        return
    rec, slot = np.nonzero(un)
    full = (t.lo_bits[rec, slot] == t.empty_bits).all(axis=1) & (t.hi_bits[rec, slot] == t.empty_bits).all(axis=1)
    if not full.all():
        k = np.argmax(~full)
        raise AuditError(f"unused slot with a finite plane: {_where(rec[k], slot[k])} carries lo {t.lo[rec[k], slot[k]]} hi {t.hi[rec[k], slot[k]]}, "
                         f"not the empty box in all six planes")
    if un[:, 0].any():
        raise AuditError(f"record {int(np.argmax(un[:, 0]))}: slot 0 is unused")
    before = un[:, :-1] & ~un[:, 1:]
    if before.any():
        r, s = np.argwhere(before)[0]
        raise AuditError(f"unused slot before a used one: {_where(r, s)}")
    bad = t.ref[rec, slot] != t.ref[rec, 0]
    if bad.any():
        k = np.argmax(bad)
        raise AuditError(f"unused slot does not repeat slot 0's reference: {_where(rec[k], slot[k])}")
    if t.layout != 2:                                          # child pairs: only the empty second child of a single-leaf tree
        if t.n != 1 or not t.is_leaf[0, 0]:
            raise AuditError(f"unused slot in a child-pair record that is not a single-leaf tree: {_where(rec[0], slot[0])}")


def _half_encode(layout, lo32, hi32):
    """The planes as the layout stores them: (lo bits, hi bits) of binary32 boxes rounded outward."""
    if layout == 0:
        return lo32.view(np.uint32), hi32.view(np.uint32)
    return half_down(lo32).view(np.uint16), half_up(hi32).view(np.uint16)


def _plane_name(is_hi, axis):
    return ("hi." if is_hi else "lo.") + AXES[axis]


def _check_leaves(t, position, radius_sq):
    n_prims = len(radius_sq)
    used_leaf = t.is_leaf & ~t.is_unused
    rec, slot = np.nonzero(used_leaf)
    prim = (t.ref[rec, slot] & ~np.uint32(LEAF_BIT)).astype(np.int64)
    bad = prim >= n_prims
    if bad.any():
        k = np.argmax(bad)
        raise AuditError(f"reference out of range: {_where(rec[k], slot[k])} is leaf of prim {prim[k]} of {n_prims}")
    counts = np.bincount(prim, minlength=n_prims)
    if (counts != 1).any():
        twice, missing = np.nonzero(counts > 1)[0], np.nonzero(counts == 0)[0]
        raise AuditError(f"every prim must be exactly one leaf: referenced more than once {twice[:5].tolist()}, missing {missing[:5].tolist()}")
    lo32, hi32 = expected_leaf_boxes(position, radius_sq)
    want_lo, want_hi = _half_encode(t.layout, lo32[prim], hi32[prim])
    got_lo, got_hi = t.lo_bits[rec, slot], t.hi_bits[rec, slot]
    for is_hi, got, want, src in ((0, got_lo, want_lo, lo32), (1, got_hi, want_hi, hi32)):
        bad = got != want
        if bad.any():
            k, a = np.argwhere(bad)[0]
            dec = (lambda b: float(np.array(b, dtype=got.dtype).view(f32 if t.layout == 0 else f16)))
            g, w = dec(got[k, a]), dec(want[k, a])
            if t.layout != 0 and got[k, a] == half_nearest(src[prim[k], a]).view(np.uint16):
                kind = "rounded to nearest, not outward"
            elif (g > w) if not is_hi else (g < w):
                kind = "moved inward"
            else:
                kind = "wider than the documented box"
            raise AuditError(f"leaf box {kind}: {_where(rec[k], slot[k])} (prim {prim[k]}) plane {_plane_name(is_hi, a)} stores {g!r}, "
                             f"the documented box has {w!r} (binary32 {float(src[prim[k], a])!r})")
    # independently, in float64: the stored box contains the sphere
    c = np.asarray(position, dtype=np.float64).reshape(-1, 3)[prim]
    r = np.sqrt(np.asarray(radius_sq, dtype=np.float64).reshape(-1))[prim]
    out = (t.lo[rec, slot] > c - r[:, None]) | (t.hi[rec, slot] < c + r[:, None])
    if out.any():
        k, a = np.argwhere(out)[0]
        raise AuditError(f"leaf box does not contain its sphere: {_where(rec[k], slot[k])} (prim {prim[k]}) axis {AXES[a]}: "
                         f"[{t.lo[rec[k], slot[k], a]!r}, {t.hi[rec[k], slot[k], a]!r}] vs [{c[k, a] - r[k]!r}, {c[k, a] + r[k]!r}]")
    return lo32, hi32


def _check_inner(t):
    used = ~t.is_unused
    lo = np.where(used[:, :, None], t.lo, np.inf).min(axis=1)                       # the union of every record's used slots
    hi = np.where(used[:, :, None], t.hi, -np.inf).max(axis=1)
    rec, slot = np.nonzero(~t.is_leaf & used)
    child = t.ref[rec, slot].astype(np.int64)
    for is_hi, got, want in ((0, t.lo[rec, slot], lo[child]), (1, t.hi[rec, slot], hi[child])):
        bad = got != want
        if bad.any():
            k, a = np.argwhere(bad)[0]
            raise AuditError(f"inner box is not the union of its children: {_where(rec[k], slot[k])} plane {_plane_name(is_hi, a)} stores {got[k, a]!r}, "
                             f"the used slots of record {child[k]} give {want[k, a]!r}")


def _check_depth(t, level, depth):
    deepest = int(level.max())
    if depth >= STACK:
        raise AuditError(f"depth {depth} does not fit the {STACK}-entry traversal stack")
    if t.layout == 2:
        if deepest != depth // 2:
            raise AuditError(f"depth {depth} is wrong: the wide records have {deepest} levels, depth // 2 = {depth // 2}")
        if 3 * deepest >= STACK:
            raise AuditError(f"depth: {deepest} wide levels can leave {3 * deepest} stack entries, the stack holds {STACK}")
    elif depth != 1 + deepest:
        raise AuditError(f"depth {depth} is wrong: the deepest record is at level {deepest}, so the tree is {1 + deepest} levels deep")


def _slot_boxes32(t, level, lo32, hi32):
    """The binary32 box of every used slot, from the documented leaf boxes upward (unions are exact): lo, hi [n, slots, 3]."""
    used = ~t.is_unused
    slo = np.full((t.n, t.slots, 3), np.inf, dtype=f32); shi = np.full((t.n, t.slots, 3), -np.inf, dtype=f32)
    leaf = t.is_leaf & used
    prim = (t.ref & ~np.uint32(LEAF_BIT)).astype(np.int64)
    slo[leaf], shi[leaf] = lo32[prim[leaf]], hi32[prim[leaf]]
    for lv in range(int(level.max()), 0, -1):                   # a record's union is complete before its parent's slot reads it
        recs = np.nonzero(level == lv)[0]
        rec, slot = np.nonzero((~t.is_leaf & used)[recs])
        child = t.ref[recs[rec], slot].astype(np.int64)
        slo[recs[rec], slot] = slo[child].min(axis=1)
        shi[recs[rec], slot] = shi[child].max(axis=1)
    return slo, shi


def _check_order(t, level, lo32, hi32):
    """lbvh_build.hip: of two siblings, the one with the larger half area is stored first."""
    slo, shi = _slot_boxes32(t, level, lo32, hi32)
    area = half_area(slo, shi)
    def union_area(a, b):
        return half_area(np.minimum(slo[:, a], slo[:, b]), np.maximum(shi[:, a], shi[:, b]))
    def fail(mask, what):
        raise AuditError(f"child order: record {int(np.argmax(mask))}: {what} (half areas {area[int(np.argmax(mask))].tolist()})")
    used = (~t.is_unused).sum(axis=1)
    if t.layout != 2:
        bad = (used == 2) & (area[:, 0] < area[:, 1])
        if bad.any():
            fail(bad, "the child with the smaller half area is first")
        return
    bad = (used == 2) & (area[:, 0] < area[:, 1])
    if bad.any():
        fail(bad, "the child with the smaller half area is first")
    bad = (used == 4) & ((area[:, 0] < area[:, 1]) | (area[:, 2] < area[:, 3]) | (union_area(0, 1) < union_area(2, 3)))
    if bad.any():
        fail(bad, "a half of the wide record, or the two halves, have the smaller half area first")
    leaf_first = ~(area[:, 0] < union_area(1, 2)) & ~(area[:, 1] < area[:, 2])          # {s0} {s1 s2}
    leaf_last = ~(area[:, 0] < area[:, 1]) & ~(union_area(0, 1) < area[:, 2])           # {s0 s1} {s2}
    bad = (used == 3) & ~leaf_first & ~leaf_last
    if bad.any():
        fail(bad, "neither split of its three slots into a child and a pair of grandchildren has the larger half area first")


def audit(words, info, prims, child_order=False):
    """Raises AuditError unless the records are the tree bvh_layout.hpp documents over `prims` (BVH order: the `position` / `radius_sq` that
    hit.primID indexes).  child_order: also the larger-half-area-first order of lbvh_build.hip.  Returns the records' levels."""
    t = decode(words, info)
    position, radius_sq = np.asarray(prims["position"], dtype=f32), np.asarray(prims["radius_sq"], dtype=f32)
    level = _walk(t)
    _check_unused(t)
    lo32, hi32 = _check_leaves(t, position, radius_sq)
    _check_inner(t)
    _check_depth(t, level, int(info["depth"]))
    if child_order:
        _check_order(t, level, lo32, hi32)
    return level


def leaf_sets_by_record(words, info):
    """(list of the frozen prim set below each record, the records' levels)."""
    t = decode(words, info)
    level = _walk(t)
    used = ~t.is_unused
    below = [None] * t.n
    for r in range(t.n - 1, -1, -1):                              # children have larger indices
        s = set()
        for k in range(t.slots):
            if not used[r, k]:
                continue
            ref = int(t.ref[r, k])
            if ref & LEAF_BIT:
                s.add(ref & ~LEAF_BIT)
            else:
                s |= below[ref]
        below[r] = frozenset(s)
    return below, level


def leaf_sets(words, info):
    """The set of frozen prim sets, one per record."""
    return set(leaf_sets_by_record(words, info)[0])


# ---- lbvh_build.hip, restated ------------------------------------------------------------------------------------------------------
def _spread10(v):
    v = v.astype(np.uint64)
    M = np.uint64(0xFFFFFFFF)
    v = ((v * np.uint64(0x00010001)) & M) & np.uint64(0xFF0000FF)
    v = ((v * np.uint64(0x00000101)) & M) & np.uint64(0x0F00F00F)
    v = ((v * np.uint64(0x00000011)) & M) & np.uint64(0xC30C30C3)
    v = ((v * np.uint64(0x00000005)) & M) & np.uint64(0x49249249)
    return v


def large_threshold(radius_sq):
    """k_large_threshold: 2^(median exponent + 5 - 127) of the radii, +inf when that exponent reaches 255."""
    r = np.sqrt(np.asarray(radius_sq, dtype=f32).reshape(-1))
    hist = np.bincount((r.view(np.uint32) >> 23) & 0xFF, minlength=256)
    e = int(np.argmax(2 * np.cumsum(hist) >= len(r)))
    te = e + 5
    return f32(np.inf) if te >= 255 else np.array(te << 23, dtype=np.uint32).view(f32)[()]


def lbvh_keys(prims):
    """k_leaf_boxes' histogram .. k_morton: the 64-bit keys (code << 32 | i), unsorted, in binary32 arithmetic."""
    c = np.asarray(prims["position"], dtype=f32).reshape(-1, 3)
    rsq = np.asarray(prims["radius_sq"], dtype=f32).reshape(-1)
    r = np.sqrt(rsq)
    threshold = large_threshold(rsq)
    ordinary = r < threshold
    lo, hi = c[ordinary].min(axis=0), c[ordinary].max(axis=0)
    cell = f32(max(f32(0.0), (hi - lo).astype(f32).max()))                         # one cell size for the three axes
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        u = ((c - lo) / cell).astype(f32) if cell > 0 else np.zeros_like(c)
        u = np.minimum(np.maximum((u * f32(1024.0)).astype(f32), f32(0.0)), f32(1023.0))
    q = u.astype(np.uint32)                                                         # truncation
    code = ((~ordinary).astype(np.uint64) << np.uint64(30)) | (_spread10(q[:, 0]) << np.uint64(2)) | (_spread10(q[:, 1]) << np.uint64(1)) | _spread10(q[:, 2])
    return (code << np.uint64(32)) | np.arange(len(r), dtype=np.uint64)


def _bit_length64(x):
    """Position of the highest set bit + 1 of uint64 x > 0 (exact: each 32-bit half fits a float64)."""
    hi, lo = (x >> np.uint64(32)).astype(np.float64), (x & np.uint64(0xFFFFFFFF)).astype(np.float64)
    return np.where(hi > 0, np.frexp(hi)[1] + 32, np.frexp(lo)[1]).astype(np.int64)


def radix_tree(sorted_keys):
    """The binary radix tree over unique sorted 64-bit keys: every range [first, last] of two or more keys is split at the highest bit in
    which its first and last key differ.  Returns (first, last, level) of the inner nodes, level by level (root = 1)."""
    keys = np.ascontiguousarray(sorted_keys, dtype=np.uint64)
    assert (keys[1:] > keys[:-1]).all(), "keys must be sorted and unique"
    first, last = np.array([0], dtype=np.int64), np.array([len(keys) - 1], dtype=np.int64)
    out_f, out_l, out_d = [], [], []
    depth = 0
    while len(first):
        depth += 1
        out_f.append(first); out_l.append(last); out_d.append(np.full(len(first), depth, dtype=np.int64))
        d = (_bit_length64(keys[first] ^ keys[last]) - 1).astype(np.uint64)        # the highest differing bit
        t = (keys[last] >> d) << d                                                 # the first key of the upper half
        gamma = np.searchsorted(keys, t, side="left") - 1                          # last key of the lower half
        assert ((gamma >= first) & (gamma < last)).all()
        nf = np.concatenate([first, gamma + 1]); nl = np.concatenate([gamma, last])
        keep = nl > nf
        first, last = nf[keep], nl[keep]
    return np.concatenate(out_f), np.concatenate(out_l), np.concatenate(out_d)


def lbvh_twin(prims):
    """{"keys": the sorted keys, "sets": the frozen prim set of every inner node, "depth": levels including the leaf level,
    "first" / "last" / "level": the inner nodes as ranges of the sorted order}."""
    keys = np.sort(lbvh_keys(prims))
    first, last, level = radix_tree(keys)
    order = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    sets = {frozenset(order[a:b + 1].tolist()) for a, b in zip(first.tolist(), last.tolist())}
    return {"keys": keys, "sets": sets, "depth": int(level.max()) + 1, "first": first, "last": last, "level": level}


def deep_cloud():
    """Centres on the Morton grid (cell = 1024 / 1024: a coordinate is its own quantised value): sphere 0 at the origin, one sphere per code
    bit b whose code is exactly 1 << b, one sphere at (1024, 1024, 1024) that pins the grid.  Sorted, the codes are 0, 1, 2, 4, .. 2^29,
    2^30 - 1: the root separates the two largest, then every split peels one key off the top: 30 inner levels, whatever order the spheres
    come in."""
    centres = [(0.0, 0.0, 0.0)]
    for b in range(30):
        c = [0.0, 0.0, 0.0]
        c[2 - b % 3] = float(1 << (b // 3))                      # code bit 3 j + 2 is bit j of x, 3 j + 1 of y, 3 j of z
        centres.append(tuple(c))
    centres.append((1024.0, 1024.0, 1024.0))
    p = np.zeros(len(centres), dtype=[("position", f32, 3), ("radius_sq", f32)])
    p["position"], p["radius_sq"] = np.asarray(centres, dtype=f32), f32(64.0)   # radius 8: sixteen binary16 steps at 1024, so binary16 is not refused
    return p
