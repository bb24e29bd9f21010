"""Binary32 numpy twin of the noise estimate (include/mirt.h, "per-pixel noise estimate"; resolve.hpp k_noise), restated here:

for a pixel with bucket words r_j, g_j, b_j (j = 0 .. k-1, k >= 2) and scale = exposure / (float)(accumulations / k), every operation
binary32, one rounding each, in this order:

    y_j  = scale * ((0.2126f * r_j + 0.7152f * g_j) + 0.0722f * b_j)
    mean = (((y_0 + y_1) + y_2) + ...) / (float)k
    var  = (((d_0*d_0 + d_1*d_1) + d_2*d_2) + ...) / (float)(k - 1),     d_j = y_j - mean
    se   = sqrt(var / (float)k)
    e    = (mean + floor == 0) ? 0 : se / (mean + floor)

A pixel is usable when the word of e is below 0x7f800000 (finite, sign bit clear); its histogram bin is word >> 20 (2048 bins); only usable
pixels enter the tile maximum, the tile mean, the image statistics and the histogram.  numpy evaluates every array operation on float32
arrays with one rounding and never fuses two, which is the arithmetic the definition asks for."""
import math

import numpy as np

f32 = np.float32
BINS = 2048
USABLE_BELOW = 0x7F800000
LUMA = (f32(0.2126), f32(0.7152), f32(0.0722))


def scale_of(exposure, accumulations, k):
    """exposure / (float)(accumulations / k): the integer quotient, converted, then one binary32 division."""
    return f32(exposure) / f32(accumulations // k)


def noise_e(slab, scale, floor):
    """slab [tiles][k][3][256] f32 -> e [tiles][256] f32."""
    slab = np.asarray(slab, dtype=f32)
    k = slab.shape[1]
    assert slab.ndim == 4 and slab.shape[2:] == (3, 256) and k >= 2
    scale, floor = f32(scale), f32(floor)
    with np.errstate(all="ignore"):
        y = [scale * ((LUMA[0] * slab[:, j, 0] + LUMA[1] * slab[:, j, 1]) + LUMA[2] * slab[:, j, 2]) for j in range(k)]
        s = y[0]
        for j in range(1, k):
            s = s + y[j]
        mean = s / f32(k)
        ss = None
        for j in range(k):
            d = y[j] - mean
            ss = d * d if ss is None else ss + d * d
        var = ss / f32(k - 1)
        se = np.sqrt(var / f32(k))
        denom = mean + floor
        e = np.where(denom == f32(0.0), f32(0.0), se / denom)
    assert e.dtype == f32
    return np.ascontiguousarray(e)


def usable(e):
    return np.asarray(e, dtype=f32).view(np.uint32) < USABLE_BELOW


def histogram(e):
    e = np.asarray(e, dtype=f32).reshape(-1)
    ok = usable(e)
    return np.bincount(e.view(np.uint32)[ok] >> 20, minlength=BINS).astype(np.uint32)


def tile_records(e):
    """e [tiles][256] -> (max [tiles] f32 exact, mean [tiles] float64 of the usable pixels (0 without one), usable counts, unusable counts)."""
    e = np.asarray(e, dtype=f32)
    ok = usable(e)
    masked = np.where(ok, e, f32(0.0))
    n = ok.sum(axis=1)
    mean = np.where(n > 0, masked.astype(np.float64).sum(axis=1) / np.maximum(n, 1), 0.0)
    return masked.max(axis=1), mean, n, 256 - n


def stats(e):
    ok = usable(e)
    vals = np.asarray(e, dtype=f32)[ok]
    return {"owned_pixels": int(ok.size), "finite_pixels": int(ok.sum()), "nonfinite_pixels": int(ok.size - ok.sum()),
            "max": float(vals.max()) if vals.size else 0.0, "mean": float(vals.astype(np.float64).mean()) if vals.size else 0.0}


def bin_upper_edge(b):
    word = USABLE_BELOW if b >= 0x7F7 else (b + 1) << 20
    return float(np.array([word], dtype=np.uint32).view(f32)[0])


def quantile(hist, q):
    """Upper edge of the bin holding the value of rank max(ceil(q * n), 1) among the n binned values; None when n = 0."""
    hist = np.asarray(hist, dtype=np.uint64)
    n = int(hist.sum())
    if n == 0:
        return None
    rank = min(max(int(math.ceil(q * float(n))), 1), n)
    b = int(np.searchsorted(np.cumsum(hist), rank, side="left"))
    return bin_upper_edge(b)


def image(e, tile_ids, width, height, sentinel):
    """e [tiles][256] of the LaunchIndices tile_ids painted into a (height, width) image of `sentinel`."""
    img = np.full((height, width), sentinel, dtype=f32)
    h_tiles = width // 16
    for row, t in zip(np.asarray(e, dtype=f32), tile_ids):
        x0, y0 = 16 * (t % h_tiles), 16 * (t // h_tiles)
        img[y0:y0 + 16, x0:x0 + 16] = row.reshape(16, 16)
    return img
