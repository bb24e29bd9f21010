"""Float64 definitions of the dielectric interface (mirt_set_transmission), written from the textbook statements, beside tests/definitions.py.

There is no oracle for this feature: the reference carries `transmission` and `IOR_minus_one` and no closure of it reads them.  The pins are
  A  Snell's law and the unpolarised Fresnel reflectance (Born & Wolf, Principles of Optics, 1.5.1-1.5.2; Hecht, Optics, 4.6),
  B  an error model of the binary32 `dielectric_interface` derived from the operation order device_math.hpp writes down,
  C  the deterministic expectation of a pixel that sees ONE glass sphere in front of a piecewise-constant sky (and, optionally, one small emitter):
     the reflect / refract tree to depth max_bounces with weights F and 1 - F.
Named departures from the textbook, never folded silently into a formula:
  G1  radiance is not scaled by 1 / eta^2 on refraction (it cancels for every path that enters the ball and leaves it);
  G2  the tint transmission / max(transmission) multiplies the throughput once, where the ray ENTERS (a surface tint, no absorption along the chord);
  G3  a hit from outside takes the interface with probability tmax = max(transmission) and the material's opaque lobe otherwise;
  Q5  a path still alive after the last bounce is dropped;  Q10  the miss shader scales all three channels by throughput.r;
  Q8  (only with `carrier=False`) an emitter reached by an extension ray weighs powerHeuristic(max(0, D.z) / pi, light pdf) - the weight the path
      would use if it did not know that the ray left an interface; with the carrier bit the weight is 1.
Every function takes and returns float64 arrays; `u` is definitions.u, the binary32 unit roundoff."""
import numpy as np

import definitions as d
from definitions import u

OFFSET = d.OFFSET


# ---- A. Snell and Fresnel --------------------------------------------------------------------------------------------------------
def snell(r, c):
    """r = n_incident / n_transmitted, c = cos(theta_i) -> sin^2(theta_t) = r^2 (1 - c^2), cos(theta_t) (nan under total internal reflection)."""
    sin2_t = r * r * (1.0 - c * c)
    with np.errstate(invalid="ignore"):
        return sin2_t, np.sqrt(1.0 - sin2_t)


def fresnel(r, c):
    """Unpolarised reflectance (rs^2 + rp^2) / 2 of a smooth interface, r = n_i / n_t; 1 under total internal reflection."""
    sin2_t, c_t = snell(r, c)
    with np.errstate(invalid="ignore", divide="ignore"):
        rs = (r * c - c_t) / (r * c + c_t)
        rp = (c - r * c_t) / (c + r * c_t)
        F = 0.5 * (rs * rs + rp * rp)
    return np.where(sin2_t >= 1.0, 1.0, F)


def interface(Vl, n, entering, s1):
    """The library's interface in float64, in the hit's frame (normal +z facing the ray, Vl the direction back along it):
    -> local direction (m, 3), F, reflected, tir.  n == 1: F = 0 and the ray goes straight on."""
    Vl = np.asarray(Vl, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)
    r = np.where(entering, 1.0 / n, n)
    c = Vl[:, 2]
    sin2_t, c_t = snell(r, c)
    tir = (sin2_t >= 1.0) & (n != 1.0)
    F = np.where(n == 1.0, 0.0, fresnel(r, c))
    reflected = tir | (s1 < F)
    mirror = np.stack([-Vl[:, 0], -Vl[:, 1], c], axis=1)
    t = np.stack([-r * Vl[:, 0], -r * Vl[:, 1], -np.where(tir, 0.0, c_t)], axis=1)
    with np.errstate(invalid="ignore"):
        t = t / np.linalg.norm(t, axis=1, keepdims=True)
    t = np.where((n == 1.0)[:, None], -Vl, t)
    return np.where(reflected[:, None], mirror, t), F, reflected, tir


# ---- B. error model of the binary32 dielectric_interface ---------------------------------------------------------------------------
def interface_error_model(Vl, n, entering):
    """Bounds of the binary32 rounding error of dielectric_interface from the float64 magnitudes, following device_math.hpp's operation order;
    e = u (1 + O(u)), taken as 1.01 u.  Every input (Vl, n) is a binary32 number, exact.
      r = 1 / n (entering: one rounding, relative e) or n (exact)                                             rel(r) <= e
      A = 1 - c * c: the product rounds by e c^2, the difference by e |A|                                      E_A = e (c^2 + |A|)
      r * r: relative 3 e;  sin2_t = (r * r) * A                                                               E_s2 = r^2 (E_A + 4 e |A|)
      B = 1 - sin2_t                                                                                           E_B = E_s2 + e |B|
      c_t = sqrt(B): |sqrt(x + h) - sqrt(x)| <= min(sqrt|h|, |h| / sqrt(x)), plus the sqrt's own rounding     E_ct = min(sqrt(E_B), E_B / sqrt(B)) + e c_t
        - ill-conditioned near the critical angle: the bound is a function of B = 1 - sin2_t, it grows like E_B / sqrt(B) and ends at sqrt(E_B).
      rc = r * c: E_rc = 2 e rc;  rct = r * c_t: E_rct = r E_ct + 2 e rct
      rs = (rc - c_t) / (rc + c_t):  E_num = E_rc + E_ct + e |num|,  E_den = E_rc + E_ct + e den,
                                     E_rs = (E_num + |rs| E_den) / (den - E_den) + e |rs|            (interval quotient; inf when den <= E_den)
      rp = (c - rct) / (c + rct):    likewise with E_num = E_rct + e |num|, E_den = E_rct + e den
      F = 0.5 (rs^2 + rp^2):         E_F = 0.5 sum(2 |x| E_x + E_x^2 + e x^2) + e F
      refracted direction = normalize3(r D + k N), k = rc - c_t, with D = -Vl and N = +z in fn 11: x and y are r * D.x + k * 0, one product each,
        E_xy = 2 e r |v_xy|; z is -(rc) + fl(rc - c_t) with the SAME rounded rc, i.e. -c_t but for the roundings of k and of the sum,
        E_z = E_ct + e (|rc - c_t| + c_t); normalize3 is a dot product
        (3 e), a sqrt (e + half the dot's), a reciprocal and a product (e each): 5 e on the scale, and d(v / |v|) <= 2 |dv| / |v|     E_dir = 2 |dv| / |v| + 5 e
      the mirror direction D + (2 c) N is exact there (x, y: sign flips; z: -c + 2 c).
    Flags: `tir` can differ only where |B| <= E_s2 (tie_tir); `reflected` (s1 < F) only where |s1 - F| <= E_F (interface_ties forms that).
    Where B < -E_s2 the device reports total internal reflection for certain: F = 1 and the mirror direction, both exact.
    -> dict(E_F, E_dir, tie_tir, B)."""
    e = 1.01 * u
    Vl = np.asarray(Vl, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)
    r = np.where(entering, 1.0 / n, n)
    c = Vl[:, 2]
    A = 1.0 - c * c
    E_A = e * (c * c + np.abs(A))
    E_s2 = r * r * (E_A + 4 * e * np.abs(A))
    B = 1.0 - r * r * A
    E_B = E_s2 + e * np.abs(B)
    Bp = np.maximum(B, 0.0)
    c_t = np.sqrt(Bp)
    with np.errstate(divide="ignore", invalid="ignore"):
        E_ct = np.minimum(np.sqrt(E_B), np.where(c_t > 0, E_B / c_t, np.inf)) + e * c_t
        rc, rct = r * c, r * c_t
        E_rc, E_rct = 2 * e * rc, r * E_ct + 2 * e * rct

        def quotient(num, den, E_num, E_den):
            q = np.abs(num / den)
            return np.where(den > E_den, (E_num + q * E_den) / (den - E_den) + e * q, np.inf), q

        E_rs, rs = quotient(rc - c_t, rc + c_t, E_rc + E_ct + e * np.abs(rc - c_t), E_rc + E_ct + e * (rc + c_t))
        E_rp, rp = quotient(c - rct, c + rct, E_rct + e * np.abs(c - rct), E_rct + e * (c + rct))
        F = 0.5 * (rs * rs + rp * rp)
        E_F = 0.5 * (2 * rs * E_rs + E_rs ** 2 + e * rs * rs + 2 * rp * E_rp + E_rp ** 2 + e * rp * rp) + e * F
        vxy = np.hypot(Vl[:, 0], Vl[:, 1])
        dv = np.hypot(2 * e * r * vxy, E_ct + e * (np.abs(rc - c_t) + c_t))
        E_dir = 2 * dv / np.sqrt(r * r * vxy * vxy + Bp) + 5 * e
    exact = (n == 1.0) | (B < -E_s2)              # index-matched (special-cased), or total internal reflection for certain: F = 1 and the mirror direction, exactly
    return dict(E_F=np.where(exact, 0.0, E_F), E_dir=np.where(exact, 0.0, E_dir), tie_tir=(np.abs(B) <= E_s2) & (n != 1.0), B=B)


def interface_ties(model, F, s1):
    """Inputs whose flags the model cannot decide: the critical angle within the rounding of sin2_t, or the draw within E_F of F where the
    comparison s1 < F is not exact anyway (E_F > 0), or no finite bound at all."""
    return model["tie_tir"] | ((model["E_F"] > 0) & (np.abs(s1 - F) <= model["E_F"])) | ~np.isfinite(model["E_F"])


def fn11_grid():
    """About 4096 inputs of mirt_debug_math fn 11 as binary32: a grid over c, n in {1, 1.0001, 1.44, 1.762, 11}, both senses, four draws s1, and the
    critical angle of every leaving case straddled ulp by ulp.  -> Vl (m, 3), n, entering, s1 (float32 / bool arrays)."""
    f = np.float32
    cs = np.concatenate([np.linspace(0.0, 1.0, 97), [1e-3, 1e-6, 0.999999]])
    ns = np.array([1.0, 1.0001, 1.44, 1.762, 11.0], dtype=f)
    s1s = np.array([0.0, 0.04, 0.5, 1.0], dtype=f)
    C, N, E, S = np.meshgrid(cs, ns, [True, False], s1s, indexing="ij")
    C, N, E, S = C.ravel(), N.ravel().astype(f), E.ravel(), S.ravel().astype(f)
    # the critical angle, leaving: c_crit^2 = 1 - 1 / n^2; 12 values on either side, binary32 neighbours of c_crit and a few coarser steps
    for n in ns[1:]:
        cc = f(np.sqrt(1.0 - 1.0 / float(n) ** 2))
        steps = np.array([0, 1, 2, 3, 8, 64, 1024, 16384], dtype=np.int64)
        bits = np.array([cc], dtype=f).view(np.int32)[0]
        vals = np.concatenate([(bits + steps).astype(np.int32).view(f), (bits - steps[1:]).astype(np.int32).view(f)])
        C = np.concatenate([C, vals.astype(np.float64)]); N = np.concatenate([N, np.full(len(vals), n, dtype=f)])
        E = np.concatenate([E, np.zeros(len(vals), dtype=bool)]); S = np.concatenate([S, np.full(len(vals), 0.5, dtype=f)])
    phi = 2.399963 * np.arange(len(C))                                              # golden-angle azimuths
    sin_t = np.sqrt(np.maximum(0.0, 1.0 - C * C))
    Vl = np.stack([sin_t * np.cos(phi), sin_t * np.sin(phi), C], axis=1).astype(f)
    return Vl, N, E, S


# ---- C. one glass sphere in front of a piecewise-constant sky ------------------------------------------------------------------------
def quadrant_sky(colours):
    """An HDRI of 3 x 3 texels that is piecewise constant over FOUR regions under D2 (scale width - 1 = 2 and truncation): column 0 for
    atan2(z, x) < 0 (z < 0), column 1 for z >= 0, row 0 for y > 0, row 1 for y <= 0; column 2 and row 2 are reached at u = 1 / v = 1 only and
    repeat their neighbours.  colours: ((row 0: z < 0, z >= 0), (row 1: z < 0, z >= 0)) RGB -> (3, 3, 4) float32."""
    h = np.zeros((3, 3, 4), dtype=np.float32)
    for row in range(3):
        for col in range(3):
            h[row, col, :3] = colours[min(row, 1)][min(col, 1)]
            h[row, col, 3] = 1.0
    return h


def sky_lookup(D, colours):
    """The quadrant of a direction, and its margin to the nearest texel border (the planes y = 0 and z = 0) as min(|y|, |z|)."""
    col = (D[:, 2] >= 0).astype(int)
    row = (D[:, 1] <= 0).astype(int)
    return np.asarray(colours, dtype=np.float64)[row, col], np.minimum(np.abs(D[:, 1]), np.abs(D[:, 2]))


def _hit_sphere(O, D, centre, radius):
    """Smallest non-negative root of |O + t D - centre| = radius (the larger one when the origin is inside), inf on a miss."""
    oc = centre[None, :] - O
    b = np.einsum("ij,ij->i", oc, D)
    disc = b * b - np.einsum("ij,ij->i", oc, oc) + radius * radius
    s = np.sqrt(np.maximum(disc, 0.0))
    t = np.where(b - s >= 0, b - s, b + s)
    return np.where((disc >= 0) & (t >= 0), t, np.inf)


def glass_ball_radiance(O, D, n, transmission, max_bounces, sky, emitter=None, carrier=True, border=0.02):
    """Expected radiance (m, 3) of the paths that start as the rays (O, D) towards ONE glass sphere of radius 1 about the origin (opaque lobe
    black: albedo 0, no emission), index n, tint `transmission`, in front of `sky` (quadrant colours, or None for a black sky) and, optionally, one
    emitter (centre, radius, emission) that is the scene's only light.  The reflect / refract tree to depth max_bounces: a hit from outside
    continues with probability tmax (G3) as the interface, reflects with F (weight 1) or refracts with 1 - F (weight transmission / tmax entering,
    1 leaving: G2, no eta^2: G1); total internal reflection continues with probability 1; a branch alive after bounce max_bounces - 1 is dropped (Q5);
    a miss adds weight * thr.r * sky (Q10); an emitter hit at bounce > 0 adds weight * thr * emission * w, w = 1 with the carrier bit, else the
    power heuristic of (max(0, D.z) / pi, cone pdf) (Q8), and the path ends there (the emitter is black: albedo 0).  An emitter hit at bounce 0 adds
    its emission (Q9).  -> radiance (m, 3), dropped (m,): the probability that the path is dropped, slack (m, 3): weight * thr.r * the largest
    difference between two sky colours, summed over the leaves whose direction lies within `border` of a texel border."""
    t3 = np.asarray(transmission, dtype=np.float64)
    tmax = t3.max()
    m = len(O)
    out, dropped, slack = np.zeros((m, 3)), np.zeros(m), np.zeros((m, 3))
    centre = np.zeros(3)
    spread = 0.0 if sky is None else np.ptp(np.asarray(sky, dtype=np.float64).reshape(-1, 3), axis=0)

    def walk(idx, O, D, w, thr, bounce, after_interface):
        if len(idx) == 0:
            return
        t_ball = _hit_sphere(O, D, centre, 1.0)
        t_em = _hit_sphere(O, D, emitter[0], emitter[1]) if emitter is not None else np.full(len(idx), np.inf)
        miss = ~np.isfinite(t_ball) & ~np.isfinite(t_em)
        if sky is not None and miss.any():
            colour, margin = sky_lookup(D[miss], sky)
            np.add.at(out, idx[miss], (w[miss] * thr[miss, 0])[:, None] * colour)
            near = margin < border
            np.add.at(slack, idx[miss][near], (w[miss][near] * thr[miss, 0][near])[:, None] * spread)
        last = bounce == max_bounces - 1
        em = np.isfinite(t_em) & (t_em < t_ball)
        if em.any():
            if last:
                np.add.at(dropped, idx[em], w[em])
            elif bounce == 0:
                np.add.at(out, idx[em], w[em][:, None] * emitter[2][None, :])
            else:
                if carrier and after_interface:
                    weight = 1.0
                else:
                    sin2 = emitter[1] ** 2 / np.sum((emitter[0][None, :] - O[em]) ** 2, axis=1)
                    weight = d.power_heuristic(np.maximum(0.0, D[em, 2]) / np.pi, d.cone_pdf(sin2)[0])[:, None]
                np.add.at(out, idx[em], w[em][:, None] * thr[em] * emitter[2][None, :] * weight)
        hit = np.isfinite(t_ball) & ~em
        if not hit.any():
            return
        if last:
            np.add.at(dropped, idx[hit], w[hit])
            return
        idx, O, D, w, thr, t = idx[hit], O[hit], D[hit], w[hit], thr[hit], t_ball[hit]
        P = O + D * t[:, None]
        N = P / np.linalg.norm(P, axis=1, keepdims=True)
        inside = np.einsum("ij,ij->i", N, D) >= 0
        N = np.where(inside[:, None], -N, N)
        c = -np.einsum("ij,ij->i", N, D)
        r = np.where(inside, n, 1.0 / n)
        w = np.where(inside, w, w * tmax)                                           # G3: the opaque lobe is black
        if n == 1.0:
            F = np.zeros(len(idx)); refr = D
        else:
            F = fresnel(r, c)
            _, c_t = snell(r, c)
            refr = r[:, None] * D + (r * c - np.nan_to_num(c_t))[:, None] * N
            refr = refr / np.linalg.norm(refr, axis=1, keepdims=True)
        refl = D + 2 * c[:, None] * N
        keep = F > 0
        walk(idx[keep], P[keep] + OFFSET * N[keep], refl[keep], (w * F)[keep], thr[keep], bounce + 1, True)
        keep = F < 1
        thr_in = np.where(inside[:, None], thr, thr * (t3 / tmax)[None, :])            # G2
        walk(idx[keep], P[keep] - OFFSET * N[keep], refr[keep], (w * (1 - F))[keep], thr_in[keep], bounce + 1, True)

    walk(np.arange(m), np.asarray(O, dtype=np.float64), np.asarray(D, dtype=np.float64), np.ones(m), np.ones((m, 3)), 0, False)
    return out, dropped, slack


def camera_rays(width, height, focal_length, eye_z, sub=4):
    """A pinhole at (0, 0, eye_z) looking down -z (identity orientation): `sub` x `sub` stratified sub-pixel positions of every pixel (the path
    jitters uniformly over the pixel) -> O (m, 3), D (m, 3), pixel index y * width + x (m,)."""
    z = d.lens_z(height, focal_length)
    k = (np.arange(sub) + 0.5) / sub
    px, py, sx, sy = np.meshgrid(np.arange(width), np.arange(height), k, k, indexing="ij")
    v = np.stack([(px + sx - width * 0.5).ravel(), (py + sy - height * 0.5).ravel(), np.full(px.size, z)], axis=1)
    D = v / np.linalg.norm(v, axis=1, keepdims=True)
    O = np.tile(np.array([0.0, 0.0, eye_z]), (len(D), 1))
    return O, D, (py * width + px).ravel()


def pixel_expectation(width, height, focal_length, eye_z, n, transmission, max_bounces, sky, emitter=None, carrier=True, sub=4):
    """Per-pixel means of glass_ball_radiance over the sub-pixel positions: radiance (height, width, 3), dropped (height, width),
    slack (height, width, 3), and `spread` (height, width, 3): the largest minus the smallest sub-pixel value, a bound of what the stratified mean
    can miss when the integrand jumps inside the pixel."""
    O, D, pix = camera_rays(width, height, focal_length, eye_z, sub)
    rad, drop, slack = glass_ball_radiance(O, D, n, transmission, max_bounces, sky, emitter, carrier)
    cnt = sub * sub
    order = np.argsort(pix, kind="stable")
    rad, drop, slack = rad[order].reshape(height * width, cnt, 3), drop[order].reshape(height * width, cnt), slack[order].reshape(height * width, cnt, 3)
    return (rad.mean(axis=1).reshape(height, width, 3), drop.mean(axis=1).reshape(height, width), slack.mean(axis=1).reshape(height, width, 3),
            (rad.max(axis=1) - rad.min(axis=1)).reshape(height, width, 3))


def acc_pixels(acc, width):
    """The accumulator [tile][bucket][rgb][256] as (bucket, height, width, 3) sums."""
    acc = np.asarray(acc, dtype=np.float64)
    tiles, k = acc.shape[0], acc.shape[1]
    x, y = d.pixel_of_slot(np.arange(tiles * 256), width)
    height = int(y.max()) + 1
    out = np.zeros((k, height, width, 3))
    out[:, y, x, :] = np.transpose(acc, (1, 0, 3, 2)).reshape(k, tiles * 256, 3)
    return out
