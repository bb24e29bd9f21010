"""The analytic sun and sky of mirt_set_sun_sky (include/mirt.h, "analytic sun and sky") in float64, written from the formulas and not from the
kernel: cell geometry, Perez, colour conversion, the disc, the 4 x 4 mean.  Beside it `twin`, binary32 numpy in the kernel's operation order, and
`bound`, the rounding bound of the binary32 chain evaluated with the float64 magnitudes (derivation: DESIGN.md section 2).

A parameter set is a dict with the fields of mirt_sun_sky_params; every float field is taken as the binary32 word the struct holds."""
import numpy as np

f32 = np.float32
U = 2.0 ** -24                                       # half an ulp, relative: one binary32 rounding
DEFAULTS = dict(sun_dir=(0.3, 0.9, 0.3), turbidity=3.0, sun_radius=0.00465, sky_scale=0.1, sun_scale=0.1, ground=(0.1, 0.1, 0.1), width=1025, height=513)
M_RGB = np.array([[3.2404542, -1.5371385, -0.4985314], [-0.9692660, 1.8760108, 0.0415560], [0.0556434, -0.2040259, 1.0572252]])
# the device library's documented limits (OpenCL full profile, which it conforms to), in ulp: 1 ulp is at most 2 U relative
ULP_SINCOS, ULP_EXP, ULP_ATAN2 = 4, 3, 6


def params(**kw):
    p = dict(DEFAULTS)
    unknown = set(kw) - set(p)
    assert not unknown, unknown
    p.update(kw)
    return p


def sun_from_angles(elevation_deg, azimuth_deg):
    el, az = np.radians(elevation_deg), np.radians(azimuth_deg)
    d = np.array([np.cos(el) * np.cos(az), np.sin(el), np.cos(el) * np.sin(az)])
    d[np.abs(d) < 1e-16] = 0.0                       # elevation 90 and 0 exactly
    return tuple(float(v) for v in d)


def _words(p):
    """The float fields as the binary32 words of the struct, in float64."""
    g = lambda v: np.asarray(v, dtype=f32).astype(np.float64)
    return g(p["sun_dir"]), float(g(p["turbidity"])), float(g(p["sun_radius"])), float(g(p["sky_scale"])), float(g(p["sun_scale"])), g(p["ground"])


def perez_coefficients(T):
    return np.array([[0.1787 * T - 1.4630, -0.3554 * T + 0.4275, -0.0227 * T + 5.3251, 0.1206 * T - 2.5771, -0.0670 * T + 0.3703],
                     [-0.0193 * T - 0.2592, -0.0665 * T + 0.0008, -0.0004 * T + 0.2125, -0.0641 * T - 0.8989, -0.0033 * T + 0.0452],
                     [-0.0167 * T - 0.2608, -0.0950 * T + 0.0092, -0.0079 * T + 0.2102, -0.0441 * T - 1.6537, -0.0109 * T + 0.0529]])


def perez(c, cos_theta, gamma):
    return (1.0 + c[0] * np.exp(c[1] / cos_theta)) * (1.0 + c[2] * np.exp(c[3] * gamma) + c[4] * np.cos(gamma) ** 2)


def host_terms(p):
    """Everything that depends on the sun alone, float64."""
    sd, T, alpha, sky_scale, sun_scale, ground = _words(p)
    sun = sd / np.sqrt(np.dot(sd, sd))
    theta_s = float(np.arccos(min(sun[1], 1.0)))
    coef = perez_coefficients(T)
    mx = np.array([[0.00166, -0.00375, 0.00209, 0.0], [-0.02903, 0.06377, -0.03202, 0.00394], [0.11693, -0.21196, 0.06052, 0.25886]])
    my = np.array([[0.00275, -0.00610, 0.00317, 0.0], [-0.04214, 0.08970, -0.04153, 0.00516], [0.15346, -0.26756, 0.06670, 0.26688]])
    tv, th = np.array([T * T, T, 1.0]), np.array([theta_s ** 3, theta_s ** 2, theta_s, 1.0])
    chi = (4.0 / 9.0 - T / 120.0) * (np.pi - 2.0 * theta_s)
    zenith = np.array([(4.0453 * T - 4.9710) * np.tan(chi) - 0.2155 * T + 2.4192, tv @ mx @ th, tv @ my @ th])
    f0 = np.array([perez(coef[k], 1.0, theta_s) for k in range(3)])
    m = 1.0 / (np.cos(theta_s) + 0.50572 * (96.07995 - np.degrees(theta_s)) ** -1.6364)
    lam = np.array([0.68, 0.55, 0.44])
    tau = 0.008735 * lam ** -4.08 + (0.04608 * T - 0.04586) * lam ** -1.3
    return dict(sun=sun, theta_s=theta_s, coef=coef, zenith=zenith, f0=f0, L=sun_scale * 1.9e6 * np.exp(-tau * m), alpha=alpha,
                cos_a=np.cos(alpha), cos_09a=np.cos(0.9 * alpha), sky_scale=sky_scale, ground=ground, T=T)


def cell_solid_angles(w, h):
    rows, cols = h - 1, w - 1
    s = np.sin(np.pi * (0.5 - np.arange(rows + 1) / rows))
    return (2.0 * np.pi / cols) * (s[:-1] - s[1:])            # [rows]


def sub_sample_directions(w, h):
    """-> phi [cols, 4], sin_el [rows, 4]: the midpoints of the 4 x 4 grid of every cell, equal solid angle each."""
    rows, cols = h - 1, w - 1
    s = np.sin(np.pi * (0.5 - np.arange(rows + 1) / rows))
    s[0], s[-1] = 1.0, -1.0
    f = (2.0 * np.arange(4) + 1.0) / 8.0
    sin_el = s[:-1, None] + f[None, :] * (s[1:, None] - s[:-1, None])
    phi = 2.0 * np.pi * (np.arange(cols)[:, None] / cols - 0.5) + f[None, :] * (2.0 * np.pi / cols)
    return phi, sin_el


def sky_rgb_of_direction(t, e, want_bound=False, d_err=0.0):
    """Sky radiance (before sky_scale and the tint) along unit vectors e [..., 3], float64.  With want_bound also the absolute rounding bound of
    the binary32 chain for an absolute error d_err per component of e."""
    sun, coef = t["sun"], t["coef"]
    ct = np.maximum(e[..., 1], 1.0 / 64.0)
    cg = e @ sun
    gamma = np.arctan2(np.linalg.norm(np.cross(e, sun), axis=-1), cg)
    v = [t["zenith"][k] * perez(coef[k], ct, gamma) / t["f0"][k] for k in range(3)]
    Y, x, y = v
    X, Z = x / y * Y, (1.0 - x - y) / y * Y
    xyz = np.stack([X, Y, Z], axis=-1)
    rgb = np.maximum(xyz @ M_RGB.T, 0.0)
    if not want_bound:
        return rgb
    # --- the bound: per operation half-ulps and the functions' ulp limits, carried through the condition numbers ---
    sq3 = np.sqrt(3.0)
    d_len = sq3 * (d_err + U) + 3 * U * 2.0                                   # |e -+ sun|: the components' errors, the sun's rounding, dot3 and sqrt
    d_gamma = 2.0 * (2.0 * np.sqrt(2.0) * d_len / 4.0) + 2 * ULP_ATAN2 * U * np.pi + U * np.pi    # lm^2 + lp^2 = 4; atan2f; the doubling is exact
    d_cg = sq3 * (d_err + U) + 4 * U
    d_ct = np.where(e[..., 1] > 1.0 / 64.0, d_err, 0.0)
    rho = []
    for k in range(3):
        A, B, C, D, E = coef[k]
        ex = B / ct
        e1, e2 = np.exp(ex), np.exp(D * gamma)
        term1, term2 = 1.0 + A * e1, 1.0 + C * e2 + E * cg * cg
        d1 = np.abs(A) * e1 * (np.abs(ex) * (2 * U + d_ct / ct) + 2 * ULP_EXP * U + 2 * U) + U * np.abs(term1)
        d2 = (np.abs(C) * e2 * (np.abs(D * gamma) * 2 * U + np.abs(D) * d_gamma + 2 * ULP_EXP * U + 2 * U) + np.abs(E) * (2 * np.abs(cg) * d_cg + 2 * U * cg * cg)
              + 2 * U * (1.0 + np.abs(C) * e2 + np.abs(E) * cg * cg))
        F = term1 * term2
        rho.append((d1 * np.abs(term2) + d2 * np.abs(term1)) / np.abs(F) + U + 4 * U)
    rY, rx, ry = rho
    dX = np.abs(X) * (rY + rx + ry + 2 * U)
    dY = np.abs(Y) * rY
    dZ = np.abs(Y / y) * (x * rx + y * ry + 2 * U * (1.0 + x + y)) + np.abs(Z) * (ry + rY + 2 * U)
    dxyz, axyz = np.stack([dX, dY, dZ], axis=-1), np.abs(xyz)
    d_rgb = dxyz @ np.abs(M_RGB).T + 4 * U * (axyz @ np.abs(M_RGB).T)         # the constants' rounding, three products, two sums
    return rgb, d_rgb


def direction_error(rows):
    """Absolute error bound of a component of the binary32 direction d ("the direction")."""
    arg = 2.47                                            # PI_F is 0.47 U off pi; one division, one product
    d_cs = (arg * np.pi + 2 * ULP_SINCOS) * U             # cosf / sinf of phi, |phi| <= pi
    r_edge = 2 * (arg + 2 * ULP_SINCOS) + 1               # edge = 2 h h, h = sinf(x): x cot x <= 1
    r_t = r_edge + 3                                      # the blend ta + f (tb - ta) of two edges of one sign
    t_max = 1.0 if rows % 2 == 0 else 1.0 + np.sin(np.pi / (2 * rows))
    r_ce = (r_t * (1.0 + t_max / (2.0 - t_max)) + 2) / 2 + 1
    return max(r_ce * U + d_cs + U, (r_t * t_max + 1) * U)


def definition(p, want_bound=False):
    """-> dict: "map" [h, w, 4] float64, "sky" and "sun" [h, w, 3] its two parts; with want_bound also "bound" [h, w, 3]."""
    t = host_terms(p)
    w, h = int(p["width"]), int(p["height"])
    rows, cols = h - 1, w - 1
    phi, sin_el = sub_sample_directions(w, h)
    cos_el = np.sqrt(np.maximum(0.0, 1.0 - sin_el * sin_el))
    cs, sn = np.cos(phi), np.sin(phi)
    # [rows, 4 (i), cols, 4 (j), 3]
    d = np.stack(np.broadcast_arrays(cos_el[:, :, None, None] * cs[None, None], sin_el[:, :, None, None], cos_el[:, :, None, None] * sn[None, None]), axis=-1)
    below = d[..., 1] < 0.0
    foot = np.stack(np.broadcast_arrays(cs[None, None], 0.0, sn[None, None]), axis=-1) + 0.0 * d
    e = np.where(below[..., None], foot, d)
    if want_bound:
        d_err = direction_error(rows)
        sky, d_sky = sky_rgb_of_direction(t, e, True, d_err)
    else:
        sky = sky_rgb_of_direction(t, e)
    tint = np.where(below[..., None], t["ground"], 1.0) * t["sky_scale"]
    sky = sky * tint
    cos_g = d @ t["sun"]
    ramp = t["cos_09a"] - t["cos_a"]
    limb = (cos_g - t["cos_a"]) / ramp
    wgt = np.clip(limb, 0.0, 1.0)
    sun = wgt[..., None] * t["L"]
    mean = lambda a: a.sum(axis=(1, 3)) / 16.0
    out = {}
    sky_t, sun_t = mean(sky), mean(sun)
    if want_bound:
        # the disc: |d - sun| <= 1.05 alpha wherever the weight is not pinned at 0 on both sides; 1 - cos g = |d - sun|^2 / 2
        a = t["alpha"]
        d_x = 1.05 * a * np.sqrt(3.0) * (d_err + 2 * U) + 3 * U * a * a
        e_w = d_x / ramp + 2 * U * (1.0 - t["cos_a"]) / ramp + 3 * U
        live = (limb > -e_w) & (limb < 1.0 + e_w)
        d_sun = (np.where(live, e_w, 0.0) + 3 * U * wgt)[..., None] * t["L"]
        b = mean(d_sky * tint * (1.0 + 2 * U) + 2 * U * sky) + mean(d_sun) + 17 * U * (sky_t + sun_t)
        out["bound"] = _with_duplicates(b, rows, cols)
        out["weight_error"] = float(e_w)
    out["sky"], out["sun"] = _with_duplicates(sky_t, rows, cols), _with_duplicates(sun_t, rows, cols)
    rgb = out["sky"] + out["sun"]
    out["map"] = np.concatenate([rgb, np.ones(rgb.shape[:2] + (1,))], axis=-1)
    return out


def _with_duplicates(a, rows, cols):
    """[rows, cols, ...] cells -> [rows + 1, cols + 1, ...] texels: column w - 1 repeats column 0, row h - 1 repeats row rows - 1."""
    a = np.concatenate([a, a[:, :1]], axis=1)
    return np.concatenate([a, a[-1:]], axis=0)


def sun_weights(p):
    """[rows, cols]: the mean limb weight of every cell, the disc alone (what definition()["sun"] is L times), without the sky's arrays."""
    t = host_terms(p)
    phi, sin_el = sub_sample_directions(int(p["width"]), int(p["height"]))
    cos_el = np.sqrt(np.maximum(0.0, 1.0 - sin_el * sin_el))[:, :, None, None]
    sx, sy, sz = t["sun"]
    cos_g = cos_el * (np.cos(phi) * sx + np.sin(phi) * sz)[None, None] + (sin_el * sy)[:, :, None, None]
    return np.clip((cos_g - t["cos_a"]) / (t["cos_09a"] - t["cos_a"]), 0.0, 1.0).sum(axis=(1, 3)) / 16.0


def sun_closed_form(p):
    """L x the disc's effective solid angle 2 pi int ramp(g) sin g dg = 2 pi (1 - cos 0.9 a + (cos 0.9 a - cos a) / 2)."""
    t = host_terms(p)
    return t["L"] * 2.0 * np.pi * (1.0 - t["cos_09a"] + 0.5 * (t["cos_09a"] - t["cos_a"]))


# ---- binary32 twin, in the kernel's operation order -------------------------------------------------------------------------------------
def host_args(p):
    """What the kernel is launched with: host_terms rounded to binary32 once."""
    t = host_terms(p)
    a = t["alpha"]
    sh, sh9 = np.sin(0.5 * a), np.sin(0.45 * a)
    return dict(perez=t["coef"].astype(f32), inv_f0=(1.0 / t["f0"]).astype(f32), zenith=t["zenith"].astype(f32), sun=t["sun"].astype(f32), sun_rgb=t["L"].astype(f32),
                ramp_edge=f32(2.0 * sh * sh), ramp_inv=f32(1.0 / (2.0 * sh * sh - 2.0 * sh9 * sh9)), sky_scale=f32(t["sky_scale"]), ground=t["ground"].astype(f32))


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def twin(p):
    """[h, w, 4] float32: k_sun_sky's operations, one binary32 rounding each (numpy's sin, cos, exp, arctan2 for the device library's)."""
    a = host_args(p)
    w, h = int(p["width"]), int(p["height"])
    rows, cols = h - 1, w - 1
    PI_F, HALF_PI_F = f32(3.14159265358979323846), f32(1.57079632679489661923)
    one, two, half = f32(1.0), f32(2.0), f32(0.5)
    r = np.minimum(np.arange(h), rows - 1)
    c = np.where(np.arange(w) < cols, np.arange(w), 0)
    north = 2 * r + 1 <= rows

    def edge(k):
        hh = np.sin(HALF_PI_F * (k.astype(f32) / f32(rows)))
        return two * (hh * hh)
    ta = edge(np.where(north, r, rows - r))
    tb = edge(np.where(north, r + 1, rows - (r + 1)))
    n0 = (8 * c + 1 - 4 * cols).astype(np.int64)
    phi = PI_F * ((n0[:, None] + 2 * np.arange(4)[None, :]).astype(f32) / f32(4 * cols))          # [w, 4]
    sn, cs = np.sin(phi), np.cos(phi)
    s = a["sun"]
    total = None
    for i in range(4):
        t = ta + f32(0.125 * (2 * i + 1)) * (tb - ta)                                            # [h]
        y = np.where(north, one - t, t - one)
        ce = np.sqrt(t * (two - t))
        below = (y < 0)[:, None]
        for j in range(4):
            d = [ce[:, None] * cs[None, :, j], np.broadcast_to(y[:, None], (h, w)).astype(f32), ce[:, None] * sn[None, :, j]]
            e = [np.where(below, cs[None, :, j], d[0]), np.where(below, f32(0.0), d[1]), np.where(below, sn[None, :, j], d[2])]
            ct = np.where(e[1] < f32(1.0 / 64.0), f32(1.0 / 64.0), e[1])
            m = [e[k] - s[k] for k in range(3)]
            pp = [e[k] + s[k] for k in range(3)]
            g = two * np.arctan2(np.sqrt(_dot3(m, m)), np.sqrt(_dot3(pp, pp)))
            cg = _dot3(e, s)
            cg2 = cg * cg
            v = []
            for k in range(3):
                A, B, C, D, E = a["perez"][k]
                F = (one + A * np.exp(B / ct)) * ((one + C * np.exp(D * g)) + E * cg2)
                v.append((a["zenith"][k] * F) * a["inv_f0"][k])
            Y = v[0]
            X = (v[1] / v[2]) * Y
            Z = (((one - v[1]) - v[2]) / v[2]) * Y
            M = M_RGB.astype(f32)
            rgb = [(M[q, 0] * X + M[q, 1] * Y) + M[q, 2] * Z for q in range(3)]
            rgb = [np.where(f32(0.0) < x_, x_, f32(0.0)) * a["sky_scale"] for x_ in rgb]
            rgb = [np.where(below, rgb[q] * a["ground"][q], rgb[q]) for q in range(3)]
            u = [d[k] - s[k] for k in range(3)]
            limb = (a["ramp_edge"] - half * _dot3(u, u)) * a["ramp_inv"]
            wgt = np.minimum(np.maximum(f32(0.0), limb), one)
            val = np.stack([rgb[q] + wgt * a["sun_rgb"][q] for q in range(3)], axis=-1)
            assert val.dtype == f32
            total = val if total is None else total + val
    out = np.ones((h, w, 4), dtype=f32)
    out[..., :3] = total * f32(0.0625)
    return out
