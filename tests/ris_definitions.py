"""Resampled importance sampling of the light sample, in float64 numpy: what `mirt_set_light_ris` must compute, stated apart from the kernels.

One path from a Lambertian point of albedo rho under black sphere lights (albedo 0: a path that reaches one ends there), max_bounces >= 3,
MIS on - the setting of definitions.direct_lambert, whose conventions (uniform cone sampling, Malley's cosine sampling, the power
heuristic with its floor, the world-space pdf of the closure sample, the 1e-4 offset) are taken from definitions.py.  Its own generator.

Light sample, M candidates.  Candidate i: a light k_i uniform among the n lights, a direction w_i uniform in the cone it subtends,
    f_i = Le rho cos+(w_i.n) / pi * w_l(w_i) / (cone_pdf / n)        the integrand times its MIS weight over the density it was drawn with
    v_i = max over the channels of f_i                                (0 when the point is inside the light or w_i is below the horizon)
one candidate s is kept with probability v_s / sum v (a weighted reservoir; none when every v_i = 0), and the light sample contributes
    f_s * (sum v) / (M v_s) * V(w_s)
so its expectation is (1 / M) sum_i E[f_i V] = the plain light sample's, whatever M.  Closure sample: unchanged, independent of the above.

Switches, each a misreading that the tests must be able to tell from the estimator:
    no_one_over_m        the factor 1 / M left out
    count_positive       M replaced by the number of candidates with v_i > 0
    mean_of_candidates   f_s replaced by the candidates' mean (1 / M) sum f_i
"""
import numpy as np

import definitions as df


def _cone_sample(P, centre, radius_sq, u, phi):
    """Uniform in the cone the sphere subtends from P: direction (k, 3), its pdf (k,), distance to the surface (k,), inside (k,) flag."""
    wc = centre - P
    d2 = (wc * wc).sum(axis=1)
    inside = d2 <= radius_sq
    d = np.sqrt(np.where(inside, 1.0, d2))
    wc = wc / d[:, None]
    sin2 = np.where(inside, 0.5, np.minimum(radius_sq / np.where(inside, 1.0, d2), 1.0))
    pdf, omc = df.cone_pdf(sin2)
    cos_t = 1.0 - u * omc
    sin_t = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
    t, b = df.basis_about(wc)
    w = sin_t[:, None] * (np.cos(phi)[:, None] * t + np.sin(phi)[:, None] * b) + cos_t[:, None] * wc
    reach = d * cos_t - np.sqrt(np.maximum(0.0, radius_sq - (d * sin_t) ** 2))
    return w, pdf, reach, inside


def _nearest(P, w, centre, radius_sq, skip):
    """Distance to the nearest sphere along w, the sphere `skip` (k,) left out; inf without one."""
    oc = centre[None, :, :] - P[:, None, :]
    b = (oc * w[:, None, :]).sum(axis=2)
    disc = b * b - (oc * oc).sum(axis=2) + radius_sq[None, :]
    s = np.sqrt(np.maximum(disc, 0.0))
    t = np.where(b - s >= 0.0, b - s, b + s)
    t = np.where((disc >= 0.0) & (t >= 0.0), t, np.inf)
    t[np.arange(len(P)), skip] = np.inf
    return t.min(axis=1)


def shadow_share(x, n, lights, candidates, n_u=16, n_phi=32):
    """Probability that the light sample casts a shadow ray, without sampling.  One candidate casts when its direction lies above the horizon
    (its weight is then positive): p = (1 / n_lights) sum over the lights of the share of the light's cone above the horizon, by
    definitions.cone_quadrature - what direct_lambert calls `shadow`.  The candidates are independent given the hit, so M of them leave nothing
    selected with probability (1 - p)^M.  x, n: (m, 3), or (m, q, 3) for q points that share a row -> (m,): the rows' mean of 1 - (1 - p)^M."""
    x, n = np.asarray(x, dtype=np.float64), np.asarray(n, dtype=np.float64)
    if x.ndim == 2:
        x, n = x[:, None, :], n[:, None, :]
    m, q = x.shape[:2]
    pts, nrm = x.reshape(-1, 3), n.reshape(-1, 3)
    P = pts + df.OFFSET * nrm
    p = np.zeros(len(P))
    for c, r2, _ in lights:
        for lo in range(0, len(P), 2048):
            dirs = df.cone_quadrature(P[lo:lo + 2048], np.asarray(c, dtype=np.float64), float(r2), n_u, n_phi)[0]
            p[lo:lo + 2048] += ((dirs * nrm[lo:lo + 2048, None, :]).sum(axis=2) > 0.0).mean(axis=1) / len(lights)
    return (1.0 - (1.0 - p) ** int(candidates)).reshape(m, q).mean(axis=1)


def ris_direct(x, n, rho, lights, candidates, n_paths, rng, no_one_over_m=False, count_positive=False, mean_of_candidates=False, chunk=1 << 16):
    """x, n: (m, 3) points and unit normals, or (m, q, 3): q points that share a row (a pixel's footprint; the row's figures are those of
    the mixture).  Every point starts n_paths paths.  lights: [(centre (3,), radius_sq, emission (3,))].  candidates >= 1.
    -> dict E, var (m, 3): mean and variance of one path's contribution; shadow (m,): probability that the light sample casts a shadow ray;
    samples: paths per row."""
    x, n, rho = (np.asarray(a, dtype=np.float64) for a in (x, n, rho))
    if x.ndim == 2:
        x, n = x[:, None, :], n[:, None, :]
    m, q = x.shape[:2]
    per_row = q * n_paths
    centre = np.array([l[0] for l in lights], dtype=np.float64).reshape(-1, 3)
    r2 = np.array([float(l[1]) for l in lights], dtype=np.float64)
    Le = np.array([l[2] for l in lights], dtype=np.float64).reshape(-1, 3)
    nl, M, p = len(lights), int(candidates), rho.max()
    s1, s2, cast_sum = np.zeros((m, 3)), np.zeros((m, 3)), np.zeros(m)
    rows_per_chunk = max(1, chunk // per_row)
    for lo in range(0, m, rows_per_chunk):
        hi = min(m, lo + rows_per_chunk)
        nrm = np.repeat(n[lo:hi].reshape(-1, 3), n_paths, axis=0)
        P = np.repeat(x[lo:hi].reshape(-1, 3), n_paths, axis=0) + df.OFFSET * nrm
        N = len(P)
        total, v_sum, f_sum, positive = np.zeros((N, 3)), np.zeros(N), np.zeros((N, 3)), np.zeros(N)
        f_s, v_s, w_s, reach_s, k_s = np.zeros((N, 3)), np.zeros(N), np.zeros((N, 3)), np.zeros(N), np.zeros(N, dtype=np.int64)
        for _ in range(M):
            k = rng.integers(0, nl, N)
            w, pdf_c, reach, inside = _cone_sample(P, centre[k], r2[k], rng.random(N), 2.0 * np.pi * rng.random(N))
            cos_n = (w * nrm).sum(axis=1)
            p_l, p_b = pdf_c / nl, np.maximum(0.0, cos_n) / np.pi
            f = Le[k] * rho[None, :] * (p_b * df.power_heuristic(p_l, p_b) / p_l)[:, None]
            f = np.where((inside | (cos_n < 0.0))[:, None], 0.0, f)
            v = f.max(axis=1)
            v_sum += v
            f_sum += f
            positive += v > 0.0
            take = (v > 0.0) & (rng.random(N) * v_sum < v)
            f_s[take], v_s[take], w_s[take], reach_s[take], k_s[take] = f[take], v[take], w[take], reach[take], k[take]
        cast = v_s > 0.0
        c = np.flatnonzero(cast)
        count = positive[c] if count_positive else (1.0 if no_one_over_m else float(M))
        carried = (f_sum[c] / M) if mean_of_candidates else f_s[c]
        seen = ~(_nearest(P[c], w_s[c], centre, r2, k_s[c]) < reach_s[c])
        total[c] = carried * (v_sum[c] / (count * v_s[c]))[:, None] * seen[:, None]
        # the closure sample: survives the roulette with p, cosine-distributed, carries rho / p, weighs a light it finds against the light sample
        live = np.flatnonzero(rng.random(N) < p)
        r_, phi = np.sqrt(rng.random(len(live))), 2.0 * np.pi * rng.random(len(live))
        t, b = df.basis_about(nrm[live])
        w = (r_ * np.cos(phi))[:, None] * t + (r_ * np.sin(phi))[:, None] * b + np.sqrt(np.maximum(0.0, 1.0 - r_ * r_))[:, None] * nrm[live]
        oc = centre[None, :, :] - P[live][:, None, :]
        bq = (oc * w[:, None, :]).sum(axis=2)
        d2 = (oc * oc).sum(axis=2)
        disc = bq * bq - d2 + r2[None, :]
        s = np.sqrt(np.maximum(disc, 0.0))
        th = np.where(bq - s >= 0.0, bq - s, bq + s)
        th = np.where((disc >= 0.0) & (th >= 0.0), th, np.inf)
        kk = th.argmin(axis=1)
        found = np.isfinite(th[np.arange(len(live)), kk])
        g = df.cone_pdf(np.minimum(r2[kk] / d2[np.arange(len(live)), kk], 1.0))[0] / nl
        pdf_in = np.maximum(0.0, w[:, 2]) / np.pi
        total[live] += np.where(found[:, None], (rho / p)[None, :] * df.power_heuristic(pdf_in, g)[:, None] * Le[kk], 0.0)
        rows = total.reshape(hi - lo, per_row, 3)
        s1[lo:hi], s2[lo:hi] = rows.sum(axis=1), (rows * rows).sum(axis=1)
        cast_sum[lo:hi] = cast.reshape(hi - lo, per_row).sum(axis=1)
    E = s1 / per_row
    return dict(E=E, var=s2 / per_row - E * E, shadow=cast_sum / per_row, samples=per_row)
