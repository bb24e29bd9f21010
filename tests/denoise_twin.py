"""Binary32 numpy twin of the variance-guided à-trous denoised resolve, written from the text of include/mirt.h ("variance-guided à-trous
denoised resolve", THE DEFINITION, steps 1-7), operation for operation; steps 1-2 reuse noise_twin.py where that already states them.  numpy
evaluates every array operation on float32 arrays with one rounding and never fuses two, which is the arithmetic the definition asks for.

Slabs are the library's: accumulator [tile][bucket][rgb][256], AOVs [tile][plane 0..6][256] (depth, normal xyz, albedo rgb), one sample count
per tile, tiles in LaunchIndex order over an image of width x height pixels whose tiles cover 16 (width // 16) x 16 (height // 16) of them."""
import numpy as np

import noise_twin as nt

f32 = np.float32
u32 = np.uint32
FLT_MIN = f32(np.finfo(np.float32).tiny)
H5 = (f32(1 / 16), f32(1 / 4), f32(3 / 8), f32(1 / 4), f32(1 / 16))
G3 = (f32(0.25), f32(0.5), f32(0.25))            # the 3 x 3 kernel is G3[dy] * G3[dx]: exact products
DEFAULTS = {"iterations": 5, "normal_squarings": 5, "demodulate": 1, "sigma_lum": 4.0, "sigma_depth": 0.05, "lum_floor": 1e-4, "albedo_floor": 1.0 / 256.0}


def lum(r, g, b):
    return (nt.LUMA[0] * r + nt.LUMA[1] * g) + nt.LUMA[2] * b


# ---- mirt_render's own operations (resolve.hpp median_k, device_math.hpp tonemapping) -----------------------------------------------------
def _max_sel(a, b):
    return np.where(a < b, b, a)


def _min_sel(a, b):
    return np.where(b < a, b, a)


def _median3(a, b, c):
    return _max_sel(_min_sel(a, b), _min_sel(_max_sel(a, b), c))


def median_k(v):
    """v: list of k float32 arrays -> the median as median_k forms it: the reference's min / max network for k = 5, else an insertion sort on
    `key < v[b]` and the middle word, or (the two middle words added) * 0.5f for an even k."""
    k = len(v)
    if k == 5:
        a, b, c, d, e = v
        return _median3(_max_sel(_min_sel(a, b), _min_sel(c, d)), _min_sel(_max_sel(a, b), _max_sel(c, d)), e)
    v = [np.array(x, dtype=f32) for x in v]
    for a in range(1, k):
        key = v[a].copy()
        moving = np.ones(key.shape, dtype=bool)
        for b in range(a - 1, -1, -1):
            shift = moving & (key < v[b])
            v[b + 1] = np.where(shift, v[b], np.where(moving, key, v[b + 1]))
            moving = shift
        v[0] = np.where(moving, key, v[0])
    return v[k // 2] if k & 1 else (v[k // 2 - 1] + v[k // 2]) * f32(0.5)


def _aces_fit(x):
    return (x * (x + f32(0.0245786)) - f32(0.000090537)) / (x * (f32(0.983729) * x + f32(0.4329510)) + f32(0.238081))


def _clamp01(v):
    m = np.where(f32(0.0) > v, f32(0.0), v)
    return np.where(f32(1.0) < m, f32(1.0), m)


def tonemapping(r, g, b):
    x = _aces_fit((r * f32(0.59719) + g * f32(0.35458)) + b * f32(0.04823))
    y = _aces_fit((r * f32(0.07600) + g * f32(0.90834)) + b * f32(0.01566))
    z = _aces_fit((r * f32(0.02840) + g * f32(0.13383)) + b * f32(0.83777))
    return (_clamp01((x * f32(1.604750) + y * f32(-0.53108)) + z * f32(-0.07367)),
            _clamp01((x * f32(-0.10208) + y * f32(1.10813)) + z * f32(-0.00605)),
            _clamp01((x * f32(-0.00327) + y * f32(-0.07276)) + z * f32(1.07602)))


# ---- layout ----------------------------------------------------------------------------------------------------------------------------------
def to_image(per_tile, width, height):
    """[tiles][256] in LaunchIndex order -> (16 v_tiles, 16 h_tiles), row 0 = y 0."""
    ht, vt = width // 16, height // 16
    a = np.asarray(per_tile)
    assert a.shape == (ht * vt, 256), a.shape
    return np.ascontiguousarray(a.reshape(vt, ht, 16, 16).transpose(0, 2, 1, 3).reshape(vt * 16, ht * 16))


def _frame(r, g, b, width, height):
    out = np.zeros((height, width, 4), dtype=f32)
    h, w = r.shape
    out[:h, :w, 0], out[:h, :w, 1], out[:h, :w, 2], out[:h, :w, 3] = r, g, b, f32(1.0)
    return out


def _scale(exposure, counts, k):
    """[tiles][1]: exposure / (float)(n / k) per tile."""
    n = np.asarray(counts, dtype=np.uint32).reshape(-1, 1)
    return f32(exposure) / (n // k).astype(f32)


def signal(acc, counts, exposure):
    """Step 1: s_c [tiles][256] for c = r, g, b."""
    acc = np.asarray(acc, dtype=f32)
    k = acc.shape[1]
    scale = _scale(exposure, counts, k)
    with np.errstate(all="ignore"):
        return [scale * median_k([acc[:, j, c] for j in range(k)]) for c in range(3)]


def render_frame(acc, counts, exposure, width, height):
    """The twin of mirt_render: tonemapping(s), A = 1."""
    with np.errstate(all="ignore"):
        s = signal(acc, counts, exposure)
        r, g, b = tonemapping(*s)
    return _frame(*(to_image(c, width, height) for c in (r, g, b)), width, height)


# ---- steps 1-5 ---------------------------------------------------------------------------------------------------------------------------------
def prepare(acc, aov, counts, exposure, params, width, height, force_unusable=None):
    """-> state: images x (3), v, z, N (3), m (3), s (3) and the boolean `usable`.  force_unusable: an image mask of pixels to treat as absent."""
    acc, aov = np.asarray(acc, dtype=f32), np.asarray(aov, dtype=f32)
    k = acc.shape[1]
    counts = np.asarray(counts, dtype=np.uint32).reshape(-1)
    assert aov.shape == (acc.shape[0], 7, 256) and len(counts) == acc.shape[0] and k >= 2
    with np.errstate(all="ignore"):
        s = signal(acc, counts, exposure)
        scale = _scale(exposure, counts, k)
        y = [scale * lum(acc[:, j, 0], acc[:, j, 1], acc[:, j, 2]) for j in range(k)]          # step 2, as noise_twin.noise_e
        tot = y[0]
        for j in range(1, k):
            tot = tot + y[j]
        mean = tot / f32(k)
        ss = None
        for j in range(k):
            d = y[j] - mean
            ss = d * d if ss is None else ss + d * d
        var = ss / f32(k - 1)
        v = var / f32(k)
        n = counts.astype(f32).reshape(-1, 1)                                                     # step 3
        z = aov[:, 0] / n
        nx, ny, nz = aov[:, 1], aov[:, 2], aov[:, 3]
        dot = (nx * nx + ny * ny) + nz * nz
        inv = f32(1.0) / np.sqrt(dot)
        zero = dot == f32(0.0)
        N = [np.where(zero, f32(0.0), c * inv) for c in (nx, ny, nz)]
        m, x = [], []
        for c in range(3):                                                                         # step 4
            a = aov[:, 4 + c] / n
            mc = np.where(a >= f32(params["albedo_floor"]), a, f32(1.0)) if params["demodulate"] else np.ones_like(a)
            m.append(mc.astype(f32))
            x.append(s[c] / m[c])
        lm = lum(m[0], m[1], m[2])
        v = v / (lm * lm)
        usable = np.isfinite(v) & (v >= f32(0.0)) & np.isfinite(z)                               # step 5
        for c in range(3):
            usable &= np.isfinite(x[c]) & np.isfinite(N[c])
    img = lambda a: to_image(a, width, height)
    st = {"x": [img(c) for c in x], "v": img(v), "z": img(z), "N": [img(c) for c in N], "m": [img(c) for c in m], "s": [img(c) for c in s], "usable": img(usable)}
    if force_unusable is not None:
        st["usable"] = st["usable"] & ~np.asarray(force_unusable, dtype=bool)
    for a in st["x"] + [st["v"]] + st["m"] + st["s"]:
        assert a.dtype == f32
    return st


# ---- step 6 ------------------------------------------------------------------------------------------------------------------------------------
def _shifted(a, dx, dy, fill):
    """b[y, x] = a[y + dy, x + dx] inside the image, `fill` outside."""
    h, w = a.shape
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if abs(dy) < h and abs(dx) < w:
        b[yd, xd] = a[ys, xs]
    return b


def _add(total, started, taken, term):
    """Each sum starts from the first term taken."""
    return np.where(taken, np.where(started, total + term, term), total)


def atrous_pass(st, step, params):
    """One iteration at `step`: new x (3) and v images; the other fields of the state do not change."""
    x, v, z, N, ok = st["x"], st["v"], st["z"], st["N"], st["usable"]
    sigma_lum, sigma_depth, lum_floor = f32(params["sigma_lum"]), f32(params["sigma_depth"]), f32(params["lum_floor"])
    zero_f = np.zeros_like(v)
    with np.errstate(all="ignore"):
        G, K, started = zero_f.copy(), zero_f.copy(), np.zeros(v.shape, dtype=bool)
        p_zero = (N[0] == 0) & (N[1] == 0) & (N[2] == 0)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                taken = _shifted(ok, dx, dy, False)
                if dx or dy:
                    Nq = [_shifted(c, dx, dy, f32(0.0)) for c in N]
                    nn = (N[0] * Nq[0] + N[1] * Nq[1]) + N[2] * Nq[2]
                    taken = taken & ((p_zero & (Nq[0] == 0) & (Nq[1] == 0) & (Nq[2] == 0)) | (nn > f32(0.0)))
                g = G3[dy + 1] * G3[dx + 1]
                G = _add(G, started, taken, g * _shifted(v, dx, dy, f32(0.0)))
                K = _add(K, started, taken, g)
                started = started | taken
        gv = G / K
        sd = sigma_lum * np.sqrt(gv) + lum_floor
        l_p = lum(*x)
        p_zero = (N[0] == 0) & (N[1] == 0) & (N[2] == 0)
        W, V, X = zero_f.copy(), zero_f.copy(), [zero_f.copy() for _ in range(3)]
        started = np.zeros(v.shape, dtype=bool)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ox, oy = dx * step, dy * step
                taken = _shifted(ok, ox, oy, False)
                xq = [_shifted(c, ox, oy, f32(0.0)) for c in x]
                vq = _shifted(v, ox, oy, f32(0.0))
                if dx == 0 and dy == 0:
                    w = np.full_like(v, f32(9 / 64))
                else:
                    Nq = [_shifted(c, ox, oy, f32(0.0)) for c in N]
                    zq = _shifted(z, ox, oy, f32(0.0))
                    nn = (N[0] * Nq[0] + N[1] * Nq[1]) + N[2] * Nq[2]
                    wn = np.where(nn > f32(0.0), nn, f32(0.0)).astype(f32)
                    for _ in range(int(params["normal_squarings"])):
                        wn = wn * wn
                    both_zero = p_zero & (Nq[0] == 0) & (Nq[1] == 0) & (Nq[2] == 0)
                    wn = np.where(both_zero, f32(1.0), wn)
                    dist = f32(step * max(abs(dx), abs(dy)))
                    tz = np.abs(z - zq) / (sigma_depth * (np.where(z < zq, zq, z) * dist) + FLT_MIN)
                    tl = np.abs(l_p - lum(*xq)) / sd
                    w = (((H5[dy + 2] * H5[dx + 2]) * wn) * (f32(1.0) / (f32(1.0) + tz * tz))) * (f32(1.0) / (f32(1.0) + tl * tl))
                assert w.dtype == f32
                W = _add(W, started, taken, w)
                for c in range(3):
                    X[c] = _add(X[c], started, taken, w * xq[c])
                V = _add(V, started, taken, (w * w) * vq)
                started = started | taken
        new_x = [np.where(ok, X[c] / W, x[c]) for c in range(3)]
        new_v = np.where(ok, V / (W * W), v)
    return new_x, new_v


def run(acc, aov, counts, exposure, params, width, height, force_unusable=None):
    """Steps 1-6 -> the state after the last iteration (x, v filtered)."""
    p = dict(DEFAULTS)
    p.update(params)
    st = prepare(acc, aov, counts, exposure, p, width, height, force_unusable)
    for i in range(int(p["iterations"])):
        st["x"], st["v"] = atrous_pass(st, 1 << i, p)
    return st


def finish(st, width, height):
    """Step 7; an unusable pixel is tonemapping(s)."""
    with np.errstate(all="ignore"):
        out = [np.where(st["usable"], st["x"][c] * st["m"][c], st["s"][c]) for c in range(3)]
        r, g, b = tonemapping(*out)
    return _frame(r, g, b, width, height)


def denoise(acc, aov, counts, exposure, params, width, height, force_unusable=None):
    """-> the frame mirt_render_atrous writes, (height, width, 4) float32 (pixels no tile covers stay 0)."""
    return finish(run(acc, aov, counts, exposure, params, width, height, force_unusable), width, height)
