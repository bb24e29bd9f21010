"""Float64 helpers of the GGX-pdf tests (mirt_set_ggx_pdf): two independent quadratures around definitions.ggx_vndf_pdf_of_direction, the function-level
error model, and the scenes and bucket statistics the GPU tests share.  No backend is imported here."""
import math

import numpy as np

import definitions as df

f32, f64 = np.float32, np.float64
u = df.u

ALPHAS = (0.02, 0.1, 0.3, 0.7, 1.0)
VIEW_DEGREES = (0.0, 45.0, 80.0)
# Both quadratures are midpoint rules on a polar grid whose polar angle is theta = theta_max s^2, s uniform: the nodes crowd towards the pole, where
# the lobe of a small alpha lives (alpha = 0.02: its width 2 alpha = 0.04 rad of L is s < 0.11, some eighty rings at 768).  Both integrands jump
# at the horizon, so the rule converges like the cell size there, not its square; QUAD_N is the grid at which doubling both ways moves every one of
# the 15 sums by less than QUAD_TOL / 10 (test_ggx_pdf_cpu.test_normalisation asserts it and prints the largest move).
QUAD_N = (768, 384)                       # rings, sectors
QUAD_TOL = 1e-3


def view(degrees):
    t = math.radians(degrees)
    return np.array([math.sin(t), 0.0, math.cos(t)])


def _polar_grid(axis, theta_max, n_s, n_phi):
    """Midpoint nodes about `axis` (3,) -> unit directions (n_s * n_phi, 3) and their solid-angle weights."""
    s = (np.arange(n_s) + 0.5) / n_s
    phi = (np.arange(n_phi) + 0.5) * (2.0 * np.pi / n_phi)
    theta = theta_max * s * s
    w_ring = np.sin(theta) * (2.0 * theta_max * s / n_s) * (2.0 * np.pi / n_phi)
    t_, b_ = df.basis_about(axis[None, :])
    st, ct = np.sin(theta)[:, None, None], np.cos(theta)[:, None, None]
    d = st * (np.cos(phi)[None, :, None] * t_[0] + np.sin(phi)[None, :, None] * b_[0]) + ct * axis
    return d.reshape(-1, 3), np.repeat(w_ring, n_phi)


def pdf_mass_over_directions(alpha, V, n=QUAD_N):
    """The integral of ggx_vndf_pdf_of_direction(alpha, L, V) over the sphere of L (it is 0 below the surface), on a polar grid about the MIRROR
    direction of V."""
    L, w = _polar_grid(np.array([-V[0], -V[1], V[2]]), np.pi, n[0], n[1])
    return float((df.ggx_vndf_pdf_of_direction(alpha, L, np.broadcast_to(V, L.shape)) * w).sum())


def vndf_mass_over_normals(alpha, V, n=QUAD_N):
    """The integral of ggx_vndf(alpha, V, H) over the upper hemisphere of H, on a polar grid about the NORMAL -> (all of it, the part whose
    reflection 2 (V.H) H - V lies at or below the surface)."""
    H, w = _polar_grid(np.array([0.0, 0.0, 1.0]), 0.5 * np.pi, n[0], n[1])
    d = df.ggx_vndf(alpha, V, H) * w
    below = 2.0 * (H @ V) * H[:, 2] - V[2] <= 0.0
    return float(d.sum()), float(d[below].sum())


# ---- function level --------------------------------------------------------------------------------------------------------------
# check_ggx_eval's model for the D term carried over to G1 D / (4 V.z): relative GGX_EVAL_K / k + GGX_EVAL_REL, k = 1 + (alpha^2 - 1) cos^2(theta_h)
# from float64 — D divides by k^2, and k is a difference of numbers near 1 that carries 3 roundings of u, so D is off by 2 x 3u / k; the 24u / k of
# the eval has that four times over for the half vector's own rounding (cos^2(theta_h) to ~8u).  G1 (a square root of a ratio, two adds, a
# division: each well conditioned for V.z >= 1e-3) and the final product and quotient stay inside the eval's 64u, which there covers F, G2 and
# the same product.
def pdf_sweep(seed=41, n=6000):
    """alpha (n,), L, V (n, 3) in binary32: alpha from 0 to 1 with 0 and values whose square is below the 1e-5 floor; V and L from the normal to
    grazing (cos down to 1e-3), a quarter of the L near the mirror direction (the lobe); then the rows that must give exactly 0."""
    rng = np.random.default_rng(seed)

    def upper(m, z_min=1e-3):
        z = np.exp(rng.uniform(np.log(z_min), 0.0, m)); phi = rng.uniform(0, 2 * np.pi, m)
        rho = np.sqrt(1.0 - z * z)
        d = np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1).astype(f32)
        return d / np.linalg.norm(d.astype(f64), axis=1, keepdims=True).astype(f32)

    alpha = np.exp(rng.uniform(np.log(1e-4), 0.0, n)).astype(f32)
    alpha[:10] = [0.0, 1e-4, 1e-3, 3.1e-3, 3.2e-3, 1e-2, 0.1, 0.3, 0.5, 1.0]         # 3.1e-3^2 < 1e-5 < 3.2e-3^2
    alpha[10:40] = 0.0
    L, V = upper(n), upper(n)
    q = n // 4
    near = V[:q] * f32([-1, -1, 1]) + rng.normal(size=(q, 3)).astype(f32) * np.maximum(alpha[:q, None], f32(1e-3))
    L[:q] = (near / np.linalg.norm(near.astype(f64), axis=1, keepdims=True)).astype(f32)
    L[:, 2] = np.abs(L[:, 2])
    L[0], V[0] = (0, 0, 1), (0, 0, 1)                                              # the mirror at normal incidence
    zero = np.zeros(n, dtype=bool)
    zero[-60:-40] = True; L[-60:-40, 2] *= -1                                      # L below the surface
    zero[-40:-30] = True; L[-40:-30, 2] = 0.0                                      # L on the horizon
    zero[-30:-10] = True; V[-30:-10, 2] = 0.0                                      # V.z = 0
    zero[-10:] = True; V[-10:, 2] *= -1                                            # V below the surface
    alpha[-5:] = 0.0; alpha[-35:-30] = 0.0; alpha[-25:-20] = 0.0                   # ... also for the mirror (G1 would be 0 / 0)
    return alpha, L, V, zero


def pdf_reference(alpha, L, V):
    """ggx_vndf_pdf_of_direction in float64 on the binary32 inputs, 0 where V.z <= 0 (the definition's own guard covers L) -> value, k."""
    a, L, V = alpha.astype(f64), L.astype(f64), V.astype(f64)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.where(V[:, 2] > 0.0, df.ggx_vndf_pdf_of_direction(a, L, V), 0.0)
        H = L + V
        H = H / np.linalg.norm(H, axis=1, keepdims=True)
    k = df.ggx_d(np.maximum(a * a, 1e-5), np.maximum(np.nan_to_num(H[:, 2]), 0.0))[1]
    return np.nan_to_num(want), k


# ---- image statistics --------------------------------------------------------------------------------------------------------------
def bucket_variance(acc, n_acc, buckets):
    """Per-pixel variance ACROSS BUCKETS of the per-bucket mean image, averaged over pixels and channels, straight from the accumulator
    [tile][bucket][rgb][256]: an estimate of (per-path variance) / (n_acc / buckets), with buckets - 1 degrees of freedom a pixel."""
    a = acc.astype(f64) / (n_acc / buckets)
    return float(a.var(axis=1, ddof=1).mean())


def bucket_mean_and_se(acc, n_acc, buckets, tile_mask=None):
    """Mean over a set of pixels, per channel, and its standard error from the spread of the bucket means."""
    a = acc.astype(f64) / (n_acc / buckets)                                          # [tile][bucket][rgb][256]
    a = a.transpose(1, 2, 0, 3).reshape(buckets, 3, -1)                              # [bucket][rgb][tile * 256 + px]
    if tile_mask is not None:
        a = a[:, :, tile_mask]
    m = a.mean(axis=2)                                                               # [bucket][rgb]
    return m.mean(axis=0), m.std(axis=0, ddof=1) / math.sqrt(buckets)


# ---- the low-roughness cap ---------------------------------------------------------------------------------------------------------
_rough_cache = {}


def rough_sampler(rough, lights, max_bounces, per_pixel, seed, closure_pdf="zero"):
    """test_definitions_cpu.g_sampler with the unit sphere's roughness as an argument: definitions.path_sampler's GGX closure from jittered first
    hits of the F frame -> per-pixel mean and sample variance (h * w, 3), dropped share, shadow and ray counts per path; once a process."""
    import test_definitions_cpu as cpu
    key = (rough, repr(lights), max_bounces, per_pixel, seed, closure_pdf)
    if key not in _rough_cache:
        rng = np.random.default_rng(seed)
        jit = rng.random((cpu.F_H, cpu.F_W, per_pixel, 2))
        xs, ys = np.arange(cpu.F_W)[None, :, None] + jit[..., 0], np.arange(cpu.F_H)[:, None, None] + jit[..., 1]
        pts = df.sphere_depth_normal(xs, ys, cpu.F_W / 2.0, cpu.F_H / 2.0, df.lens_z(cpu.F_H, cpu.F_FOCAL), cpu.F_EYE)[1].reshape(-1, 3)
        scene = cpu.sampler_scene(lights)
        scene["F0"] = np.array([cpu.G_F0] + [(0, 0, 0)] * len(lights), dtype=f64)
        scene["roughness"] = np.array([float(f32(rough))] + [0.0] * len(lights))
        out = df.path_sampler(scene, pts, pts, 1, max_bounces, rng, brdf=1, view=cpu.g_view(pts), closure_pdf=closure_pdf)
        x = out["sum"].reshape(cpu.F_H * cpu.F_W, per_pixel, 3)
        mean = x.mean(axis=1)
        _rough_cache[key] = dict(E=mean, var=(x * x).mean(axis=1) - mean * mean, dropped=float(out["dropped"].mean()), shadow=float(out["shadow"].mean()),
                                 rays=float(out["rays"].mean()))
    return _rough_cache[key]
