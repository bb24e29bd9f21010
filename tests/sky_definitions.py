"""Float64 twin of the sky sampling of mirt_set_sky_sampling (include/mirt.h, "sampling the environment map"): cells, their solid angles, the
table, the inverse CDF, the density of a direction through the textbook latitude-longitude map (definitions.equirect_texel), and the two MIS
weights.  Nothing here imports the library: the tests hold the kernels to these functions."""
import numpy as np

import definitions as df

f64 = np.float64
f32 = np.float32
U32 = 2.0 ** -24                      # unit roundoff of binary32
SCAN_BLOCK = 256                      # threads of the scan's workgroup (kernels.hpp kSkyBlock): what the error bound's depth is made of


def cells(width, height):
    """The image seen through truncation by (w - 1, h - 1): -> rows, cols of cells."""
    return max(height - 1, 1), max(width - 1, 1)


def elevation(k, rows):
    """Elevation of cell edge k = 0 .. rows: pi (0.5 - k / rows)."""
    return np.pi * (0.5 - np.asarray(k, dtype=f64) / rows)


def solid_angle(rows, cols):
    """Omega(r), r = 0 .. rows - 1: (2 pi / cols) (sin el(r) - sin el(r + 1)), in the cancellation-free product form."""
    r = np.arange(rows, dtype=f64)
    half = np.pi / (2.0 * rows)
    return (2.0 * np.pi / cols) * 2.0 * np.sin((2.0 * r + 1.0) * half) * np.sin(half)


def importance(hdri, ambient):
    """I[r, c] = max(t.rgb x ambient) x Omega(r) of the texels that own a cell, from the binary32 products the kernels form (each product and the
    x Omega are exact in float64: this is what binary32 rounds)."""
    h, w = hdri.shape[:2]
    rows, cols = cells(w, h)
    t = hdri[:rows, :cols, :3].astype(f32) * np.asarray(ambient, dtype=f32)[None, None, :]        # binary32 products, as the kernel's
    return t.max(axis=2).astype(f64) * solid_angle(rows, cols)[:, None]


def table(hdri, ambient):
    """The table in float64: marginal and conditional running sums, densities (1 / sr), cell probabilities, total."""
    I = importance(hdri, ambient)
    rows, cols = I.shape
    rowsum = I.sum(axis=1)
    total = rowsum.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        dens = I / (solid_angle(rows, cols)[:, None] * total)
        prob = I / total
    return {"rows": rows, "cols": cols, "I": I, "rowsum": rowsum, "marg": np.cumsum(rowsum), "cond": np.cumsum(I, axis=1), "dens": dens, "prob": prob, "total": total}


def scan_depth(n):
    """Additions a running sum of n values goes through at most in the kernels' fixed order: K - 1 within a thread's chunk of K = ceil(n / 256),
    255 over the chunk sums, 1 to join the two."""
    return -(-n // SCAN_BLOCK) - 1 + (SCAN_BLOCK - 1) + 1


def table_bounds(rows, cols):
    """Relative error bounds of the binary32 table against table(): sums of non-negative terms, so n roundings cost at most n u (1 + O(n u)).
    An importance carries 3 roundings beyond its exact binary32 products' maximum (Omega rounded from float64, the product with it) — counted as 2 —
    a conditional running sum scan_depth(cols) more, a marginal one scan_depth(rows) on top of a row sum, a density the division, the product
    Omega x total and the total's own error."""
    i = 2
    cond = i + scan_depth(cols)
    marg = cond + scan_depth(rows)
    dens = i + 2 + 1 + marg
    return {k: v * U32 * 1.01 for k, v in (("cond", cond), ("marg", marg), ("dens", dens))}


def upper(cdf, x):
    """Smallest i with cdf[i] > x (x below cdf[-1])."""
    return np.searchsorted(cdf, x, side="right")


def sample(tab, u0, u1):
    """sky_sample over a table whose running sums are given (the kernels' own binary32 words, or table()'s): the binary32 products u x total are
    part of the definition (x = fl32(u0 x total), clamped below the total); everything after them is float64.
    -> dir (n, 3), row, col, dv, du."""
    marg = np.asarray(tab["marg"]); cond = np.asarray(tab["cond"])
    rows, cols = cond.shape
    if marg.dtype == f32:
        total = marg[-1]
        x = np.minimum(u0.astype(f32) * total, np.nextafter(total, f32(0)))
    else:
        total = marg[-1]
        x = np.minimum(u0.astype(f64) * total, np.nextafter(total, 0.0))
    row = upper(marg, x)
    lo = np.where(row > 0, marg[np.maximum(row, 1) - 1], 0).astype(f64)
    dv = np.minimum((x.astype(f64) - lo) / (marg[row].astype(f64) - lo), 1.0 - U32)
    rs = cond[row, cols - 1]
    if cond.dtype == f32:
        y = np.minimum(u1.astype(f32) * rs, np.nextafter(rs, f32(0)))
    else:
        y = np.minimum(u1.astype(f64) * rs, np.nextafter(rs, 0.0))
    col = np.array([upper(cond[r], v) for r, v in zip(row, y)], dtype=np.int64) if len(row) < 4096 else _upper_rows(cond, row, y)
    lo2 = np.where(col > 0, cond[row, np.maximum(col, 1) - 1], 0).astype(f64)
    du = np.minimum((y.astype(f64) - lo2) / (cond[row, col].astype(f64) - lo2), 1.0 - U32)
    return direction(rows, cols, row, col, dv, du), row, col, dv, du


def _upper_rows(cond, row, y):
    """upper() per sample in its own row, vectorised: running sums are non-decreasing, so count the entries <= y."""
    out = np.empty(len(row), dtype=np.int64)
    for r in np.unique(row):
        m = row == r
        out[m] = np.searchsorted(cond[r], y[m], side="right")
    return out


def direction(rows, cols, row, col, dv, du):
    """The point of cell (row, col) at fractions (dv, du): uniform in sin(elevation) from the upper edge down, uniform in azimuth; the inverse of
    the latitude-longitude map u = 1/2 + atan2(z, x) / 2 pi, v = 1/2 - asin(y) / pi."""
    s_top, s_bot = np.sin(elevation(row, rows)), np.sin(elevation(row + 1, rows))
    y = s_top + dv * (s_bot - s_top)
    # cos(elevation) from the distance to the nearer pole, exact where y itself is ill-conditioned
    half = np.pi / (2.0 * rows)
    north = 2 * row + 1 <= rows
    ta = np.where(north, 2.0 * np.sin(row * half) ** 2, 2.0 * np.sin((rows - row) * half) ** 2)
    tb = np.where(north, 2.0 * np.sin((row + 1) * half) ** 2, 2.0 * np.sin((rows - row - 1) * half) ** 2)
    t = ta + dv * (tb - ta)
    c = np.sqrt(np.maximum(0.0, t * (2.0 - t)))
    phi = 2.0 * np.pi * ((col + du) / cols - 0.5)
    return np.stack([c * np.cos(phi), y, c * np.sin(phi)], axis=1)


def cell_of(d, width, height):
    """The cell a direction lies in by the textbook map (definitions.equirect_texel), the measure-zero last texel row / column folded in."""
    rows, cols = cells(width, height)
    c, r, _, _ = df.equirect_texel(d, width, height)
    if width == 1:
        c = np.zeros_like(c)
    if height == 1:
        r = np.zeros_like(r)
    return np.minimum(r, rows - 1), np.minimum(c, cols - 1)


def pdf(tab, d, width, height):
    """Density (1 / sr) of a direction: its cell's."""
    r, c = cell_of(d, width, height)
    return tab["dens"][r, c]


def nee_weight(sel, p_sky, pdf_closure):
    """MIS weight of a sky sample of next event estimation: the power heuristic of sel x p~ against the closure's pdf of that direction."""
    return df.power_heuristic(sel * p_sky, pdf_closure)


def miss_weight(sel, p_sky, pdf_closure):
    """MIS weight the miss shader gives thr.r x sky for a direction the closure sampled."""
    return df.power_heuristic(pdf_closure, sel * p_sky)


def lambert_pdf(local_z):
    return np.maximum(0.0, local_z) / np.pi


def band_share(tab, bw_phi, bw_lat):
    """Probability, under the table's sampling, of a direction within bw_phi (azimuth) or bw_lat (latitude) of a cell edge: per cell
    1 - (1 - f_phi)(1 - f_lat(r)) — placement is uniform in azimuth and in sin(elevation), and independent in the two."""
    rows, cols = tab["rows"], tab["cols"]
    f_phi = min(1.0, 2.0 * bw_phi / (2.0 * np.pi / cols))
    el = elevation(np.arange(rows + 1), rows)
    f_lat = np.empty(rows)
    for r in range(rows):
        top, bot = el[r], el[r + 1]
        inner_top, inner_bot = top - bw_lat, bot + bw_lat
        free = max(0.0, np.sin(inner_top) - np.sin(inner_bot)) if inner_top > inner_bot else 0.0
        f_lat[r] = 1.0 - free / (np.sin(top) - np.sin(bot))
    per_cell = 1.0 - (1.0 - f_phi) * (1.0 - f_lat)
    return float((tab["prob"].sum(axis=1) * per_cell).sum())


def sun_map(width=65, height=33, sun=(10, 20), power=1e4):
    """The test map: 1 everywhere, one texel of `power`."""
    h = np.ones((height, width, 4), dtype=f32)
    h[sun[0], sun[1], :3] = power
    return h
