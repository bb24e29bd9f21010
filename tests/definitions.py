"""Float64 definitions of the operations on the path, written from their textbook statements.

A third statement beside oracle/oracle.cpp (CPU) and csrc/kernels.hpp (GPU): plain numpy, float64 throughout, no fast-math
polynomials, no operation ordering, no fused multiply-adds.  tests/test_definitions_cpu.py holds the oracle to it,
tests/test_definitions_gpu.py the kernels.  Where the reference deliberately departs from the textbook (the Q rows,
plus the few listed here) the departure is a NAMED argument or a named expectation in the tests, never folded silently into a formula:

  D1  ray-sphere roots are those of  t^2 - 2 b t + (|oc|^2 - r^2) = 0  with the leading coefficient taken as 1 whatever |D| is
      (BVH.hpp:251-286 never divides by |D|^2; exact for unit directions, a "fat" sphere for stretched ones).
  D2  the sky image is addressed with (width - 1, height - 1) as scale and truncation (Application.cpp:230-231, Primitives.hpp:35-46),
      so the last column / row is reached only at u = 1 / v = 1 exactly.
  D3  GGX D takes max(alpha^2, 1e-5) while the masking term takes alpha^2 itself (Sampling.hpp:295).
  D4  the cone pdf divides by max(1 - cos(theta_max), 1e-6) (Sampling.hpp:192-194).
  D7  the visible-normal sample warps the disk along the second axis of the branch-free basis (Duff et al. 2017) about the stretched view
      direction, not along the axis in the plane of that direction and the normal (Sampling.hpp:261), and clamps the normals this puts
      below the surface onto the horizon (Sampling.hpp:268): `axis` and `clamp` of ggx_visible_normal.

Every function takes and returns float64 arrays; `u` is the binary32 unit roundoff the error models are written in."""
import numpy as np

u = 2.0 ** -24                                     # binary32 unit roundoff (round to nearest)
CHI2_255_P1E6 = 377.08                             # upper 1e-6 quantile of chi-square with 255 degrees of freedom (16 x 16 cells - 1)


# ---- A. ray / sphere ------------------------------------------------------------------------------------------------------------
def sphere_roots(P, D, centre, radius_sq):
    """Quadratic of |P + t D - c|^2 = r^2 under D1, for rays (n, 3) against spheres (m, 3): -> b, oc2, disc as (n, m) arrays.
    Roots are b -+ sqrt(disc), disc = b^2 - (|oc|^2 - r^2)  (any textbook on ray tracing; e.g. Glassner 1989, ch. 2)."""
    oc = centre[None, :, :] - P[:, None, :]
    b = np.einsum("nmk,nk->nm", oc, D)
    oc2 = np.einsum("nmk,nmk->nm", oc, oc)
    return b, oc2, b * b - oc2 + radius_sq[None, :]


def sphere_error_model(P, D, centre, radius_sq, b, oc2, disc):
    """Bound of the binary32 rounding error of b, disc and of a root b -+ sqrt(disc) as the path evaluates them, from the float64
    magnitudes.  Derivation, e = u(1 + O(u)):
      oc_k = fl(c_k - p_k): relative error e each.
      b = sum of three products d_k oc_k, accumulated (fused or not): at most 3 roundings on top of oc's ->  E_b = 4 e sum|d_k oc_k|.
      disc = r^2 - sum oc_k^2 + b^2 in four accumulation steps, every partial sum bounded by M = r^2 + |oc|^2 + b^2: 4 e M for the
        steps, 2 e |oc|^2 for oc's own rounding, 2|b| E_b + E_b^2 for b's ->  E_disc = 6 e M + 2|b| E_b + E_b^2.
      s = sqrt(disc): |sqrt(x + h) - sqrt(x)| = |h| / (sqrt(x + h) + sqrt(x)) <= min(sqrt|h|, |h| / sqrt(x)), plus e s for the sqrt.
      t = b -+ s: E_t = E_b + E_s + e |t|.
    -> E_b, E_disc, E_root (n, m); E_root is for either root up to the e|t| term, which the caller adds."""
    oc = np.abs(centre[None, :, :] - P[:, None, :])
    sabs = np.einsum("nmk,nk->nm", oc, np.abs(D))
    E_b = 4 * u * sabs
    M = radius_sq[None, :] + oc2 + b * b
    E_disc = 6 * u * M + 2 * np.abs(b) * E_b + E_b * E_b
    s = np.sqrt(np.maximum(disc, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        E_s = np.minimum(np.sqrt(E_disc), np.where(s > 0, E_disc / s, np.inf)) + u * s
    return E_b, E_disc, E_b + E_s


def closest_hit(P, D, centre, radius_sq, chunk=2048):
    """Closest hit in words (BVH.hpp:261-266, 279-285 as shipped with USEBVH false): a sphere is hit when its discriminant is not
    negative; its distance is the smaller root, or the larger one when the smaller is negative (the origin is inside); a distance is
    accepted when it is not negative and strictly below the best so far, spheres taken in array order - so the answer is the
    smallest non-negative root over all spheres, the lowest array index among equals, +inf / -1 when there is none.

    -> dict of per-ray arrays: t, prim; E (error bound of t); unsure (bool: some sphere whose own hit / miss / root choice lies within
    its error bound could change the answer); rivals (list of index arrays: spheres whose root is within the summed error bounds of
    the best one, bit-identical copies of the best sphere left out since equal inputs give equal roots and the index decides)."""
    n = len(P)
    out = dict(t=np.full(n, np.inf), prim=np.full(n, -1, dtype=np.int64), E=np.zeros(n), unsure=np.zeros(n, dtype=bool), rivals=[None] * n)
    key = np.concatenate([centre, radius_sq[:, None]], axis=1)
    for lo in range(0, n, chunk):
        p, d = P[lo:lo + chunk], D[lo:lo + chunk]
        b, oc2, disc = sphere_roots(p, d, centre, radius_sq)
        E_b, E_disc, E_root = sphere_error_model(p, d, centre, radius_sq, b, oc2, disc)
        s = np.sqrt(np.maximum(disc, 0.0))
        near, far = b - s, b + s
        t = np.where(near >= 0.0, near, far)
        hit = (disc >= 0.0) & (t >= 0.0)
        E = E_root + u * np.abs(t)
        t_hit = np.where(hit, t, np.inf)
        best = np.argmin(t_hit, axis=1)
        rows = np.arange(len(p))
        t_best, E_best = t_hit[rows, best], np.where(np.isfinite(t_hit[rows, best]), E[rows, best], 0.0)
        # a sphere's own status is in doubt when disc, or either root, is within its error of zero - and it matters only if the
        # distance it could then report is not certainly beyond the best one
        doubt = (np.abs(disc) <= E_disc) | (np.abs(near) <= E) | (np.abs(far) <= E)
        could_report = np.maximum(np.where(near + E >= 0.0, near, far) - E, 0.0)
        reachable = (far + E >= 0.0) & (disc + E_disc >= 0.0)
        matters = doubt & reachable & (could_report <= (t_best + E_best)[:, None])
        out["unsure"][lo:lo + chunk] = matters.any(axis=1)
        close = hit & (t_hit - E <= (t_best + E_best)[:, None])
        close[rows, best] = False
        same = (key[None, :, :] == key[best][:, None, :]).all(axis=2)
        close &= ~same
        for r in np.flatnonzero(close.any(axis=1)):
            out["rivals"][lo + r] = np.flatnonzero(close[r])
        out["t"][lo:lo + chunk], out["E"][lo:lo + chunk] = t_best, E_best
        out["prim"][lo:lo + chunk] = np.where(np.isfinite(t_best), best, -1)
    return out


def root_of(P, D, centre, radius_sq, prim):
    """The accepted root and its error bound for ray i against sphere prim[i] alone (prim >= 0)."""
    oc = centre[prim] - P
    b = np.einsum("nk,nk->n", oc, D)
    oc2 = np.einsum("nk,nk->n", oc, oc)
    disc = b * b - oc2 + radius_sq[prim]
    sabs = np.einsum("nk,nk->n", np.abs(oc), np.abs(D))
    E_b = 4 * u * sabs
    E_disc = 6 * u * (radius_sq[prim] + oc2 + b * b) + 2 * np.abs(b) * E_b + E_b * E_b
    s = np.sqrt(np.maximum(disc, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        E_s = np.minimum(np.sqrt(E_disc), np.where(s > 0, E_disc / s, np.inf)) + u * s
    near, far = b - s, b + s
    E = E_b + E_s
    return near, far, E + u * np.maximum(np.abs(near), np.abs(far))


def occluded(P, D, tmax, centre, radius_sq, chunk=2048):
    """Any-hit in words (BVH.hpp:294-300): occluded when some sphere's accepted distance (as in closest_hit) lies in [0, tmax).
    -> occ (bool), unsure (bool: no sphere occludes for certain and at least one might, within its error bound)."""
    n = len(P)
    occ, unsure = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for lo in range(0, n, chunk):
        p, d, tm = P[lo:lo + chunk], D[lo:lo + chunk], tmax[lo:lo + chunk, None]
        b, oc2, disc = sphere_roots(p, d, centre, radius_sq)
        E_b, E_disc, E_root = sphere_error_model(p, d, centre, radius_sq, b, oc2, disc)
        s = np.sqrt(np.maximum(disc, 0.0))
        near, far = b - s, b + s
        t = np.where(near >= 0.0, near, far)
        E = E_root + u * np.abs(t)
        yes = (disc >= 0.0) & (t >= 0.0) & (t < tm)
        doubt = (np.abs(disc) <= E_disc) | (np.abs(near) <= E) | (np.abs(far) <= E) | (np.abs(t - tm) <= E + u * tm)
        # certain: the status cannot flip.  possible: it might occlude if an error went the right way
        possible = (disc + E_disc >= 0.0) & (far + E >= 0.0) & (np.where(near + E >= 0, near, far) - E < tm)
        certain = yes & ~doubt
        occ[lo:lo + chunk] = yes.any(axis=1)
        unsure[lo:lo + chunk] = ~certain.any(axis=1) & (doubt & possible).any(axis=1)
    return occ, unsure


# ---- B. frames and sampling -----------------------------------------------------------------------------------------------------
def rotation_of_quaternion(q):
    """3x3 of v -> q v q* for q = (x, y, z, w) (n, 4), NOT normalised: the matrix is |q|^2 times a rotation (Shoemake 1985).
    -> (n, 3, 3)."""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((len(q), 3, 3))
    R[:, 0, 0] = w * w + x * x - y * y - z * z; R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = w * w - x * x + y * y - z * z; R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = w * w - x * x - y * y + z * z
    return R


def frame_defect_bound(N):
    """The shortest-arc quaternion from +z to N is q = (-N.y, N.x, 0, 1 + N.z) / sqrt(2 (1 + N.z)); for an input that is not exactly of
    unit length, |q|^2 - 1 = (|N|^2 - 1) / (2 (1 + N.z)) exactly.  The matrix of q then has R^T R = |q|^4 I, so its defect from
    orthonormality is | |q|^4 - 1 |, and R e_z - N = (0, 0, (1 - |N|^2) / (1 + N.z)).  -> (n,) bound on both, rounding left to the caller."""
    n2 = (N * N).sum(axis=1)
    k = np.abs(n2 - 1.0) / (2.0 * (1.0 + N[:, 2]))
    return 2.0 * k + k * k


def cone_pdf(sin2_theta_max, floor=1e-6):
    """Uniform sampling of the cone of directions that a sphere subtends: 1 / (2 pi (1 - cos theta_max)) (Shirley & Wang 1996;
    PBRT 3rd ed. 14.2.2).  `floor` is D4."""
    one_minus_cos = sin2_theta_max / (1.0 + np.sqrt(1.0 - sin2_theta_max))          # cancellation-free form of 1 - cos
    return 1.0 / (2.0 * np.pi * np.maximum(one_minus_cos, floor)), one_minus_cos


def cosine_upper_share(normal_y):
    """Share of a cosine-weighted hemisphere about a normal that lies in the half space y > 0: (1 + n.y) / 2 (the view factor of a
    small surface patch to a half plane, Nusselt's analogue; checked by quadrature in the tests)."""
    return 0.5 * (1.0 + normal_y)


def cosine_upper_share_quadrature(normal, n_r=400, n_phi=800):
    """The same by midpoint quadrature: cosine-weighted directions about `normal` are a uniform disk (Malley's method), so the share is
    the part of the unit disk whose lifted direction has y > 0."""
    n = normal / np.linalg.norm(normal)
    a = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    t = np.cross(n, a); t /= np.linalg.norm(t)
    b = np.cross(n, t)
    r2 = (np.arange(n_r) + 0.5) / n_r                                               # equal-area rings: r^2 uniform
    phi = 2 * np.pi * (np.arange(n_phi) + 0.5) / n_phi
    r = np.sqrt(r2)[:, None]
    y = r * np.cos(phi)[None, :] * t[1] + r * np.sin(phi)[None, :] * b[1] + np.sqrt(1.0 - r2)[:, None] * n[1]
    return float((y > 0).mean())


# ---- C. GGX ---------------------------------------------------------------------------------------------------------------------
def ggx_lambda(alpha2, cos_theta):
    """Smith Lambda of the GGX distribution (Heitz 2014, eq. 72): (-1 + sqrt(1 + alpha^2 tan^2 theta)) / 2."""
    c2 = cos_theta * cos_theta
    with np.errstate(divide="ignore", invalid="ignore"):
        tan2 = np.where(c2 > 0, (1.0 - c2) / c2, np.inf)
    return 0.5 * (-1.0 + np.sqrt(1.0 + alpha2 * tan2))


def ggx_d(alpha2, cos_h):
    """GGX / Trowbridge-Reitz normal distribution (Walter et al. 2007, eq. 33): alpha^2 / (pi ((alpha^2 - 1) cos^2 + 1)^2)."""
    k = (alpha2 - 1.0) * cos_h * cos_h + 1.0
    return alpha2 / (np.pi * k * k), k


def schlick(F0, cos_hv):
    """Schlick 1994: F0 + (1 - F0)(1 - cos)^5."""
    return F0 + (1.0 - F0) * np.clip(1.0 - cos_hv, 0.0, 1.0)[..., None] ** 5


def ggx_eval_cos(F0, alpha, L, V, d_floor=1e-5):
    """f(L, V) cos(theta_L) of the microfacet BRDF with the height-correlated Smith masking-shadowing (Heitz 2014, eq. 99):
    F D G2 / (4 cos_V),  G2 = 1 / (1 + Lambda(V) + Lambda(L)).  Directions in the local frame (normal = +z), cosines clamped at 0.
    `d_floor` is D3.  -> value (n, 3), k = the cancelling term of D (for the error model)."""
    nl, nv = np.maximum(L[:, 2], 0.0), np.maximum(V[:, 2], 0.0)
    H = L + V
    H = H / np.linalg.norm(H, axis=1, keepdims=True)
    nh, hv = np.maximum(H[:, 2], 0.0), np.maximum((H * V).sum(axis=1), 0.0)
    a2 = alpha * alpha
    D, k = ggx_d(np.maximum(a2, d_floor), nh)
    G2 = 1.0 / (1.0 + ggx_lambda(a2, nv) + ggx_lambda(a2, nl))
    with np.errstate(divide="ignore", invalid="ignore"):
        val = np.where((nl > 0) & (nv > 0), D * G2 / (4.0 * nv), 0.0)
    return schlick(F0, hv) * val[:, None], k


def ggx_vndf_weight(F0, alpha, L, V):
    """Weight of a sample drawn from the distribution of visible normals (Heitz 2018, eq. 19 with the height-correlated G2):
    F G2 / G1(V) = F (1 + Lambda(V)) / (1 + Lambda(V) + Lambda(L)); 0 when L is below the surface.
    -> value (n, 3), the half vector H rebuilt from L + V, the scalar weight, H.V."""
    nl, nv = np.maximum(L[:, 2], 0.0), np.maximum(V[:, 2], 0.0)
    H = L + V
    H = H / np.linalg.norm(H, axis=1, keepdims=True)
    hv = np.maximum((H * V).sum(axis=1), 0.0)
    a2 = alpha * alpha
    lv, ll = ggx_lambda(a2, nv), ggx_lambda(a2, nl)
    w = np.where(nl > 0, (1.0 + lv) / (1.0 + lv + ll), 0.0)
    return schlick(F0, hv) * w[:, None], H, w, hv


def ggx_g1(alpha2, cos_theta):
    """Smith masking of one direction (Heitz 2014, eq. 43): 1 / (1 + Lambda)."""
    return 1.0 / (1.0 + ggx_lambda(alpha2, cos_theta))


def ggx_vndf(alpha, V, H):
    """Density, per solid angle of H, of the normals visible from V (Heitz 2014, eq. 2; Heitz 2018, eq. 1):
    G1(V) max(0, V.H) D(H) / V.z; 0 for H below the surface.  V (3,), H (..., 3), both unit."""
    a2 = alpha * alpha
    D = np.where(H[..., 2] > 0.0, ggx_d(a2, np.maximum(H[..., 2], 0.0))[0], 0.0)
    return ggx_g1(a2, V[2]) * np.maximum(0.0, (H * V).sum(axis=-1)) * D / V[2]


def duff_basis(n):
    """The branch-free orthonormal basis of Duff et al. 2017 (JCGT 6(1), listing 3) about unit vectors n (..., 3):
    s = copysign(1, n.z), a = -1 / (s + n.z), b = n.x n.y a;  b1 = (1 + s n.x^2 a, s b, -s n.x),  b2 = (b, s + n.y^2 a, -n.y)."""
    s = np.copysign(1.0, n[..., 2])
    a = -1.0 / (s + n[..., 2])
    b = n[..., 0] * n[..., 1] * a
    return (np.stack([1.0 + s * n[..., 0] ** 2 * a, s * b, -s * n[..., 0]], axis=-1),
            np.stack([b, s + n[..., 1] ** 2 * a, -n[..., 1]], axis=-1))


def ggx_visible_normal(alpha, V, u, v, axis="reference", clamp=True):
    """A normal sampled from the distribution of visible normals by Heitz 2018's construction (JCGT 7(4), listing 1, with the disk taken
    as r = sqrt(u), phi = 2 pi v): stretch V by alpha, Vh = normalize(alpha V.x, alpha V.y, V.z); a point (t1, t2) of the unit disk;
    t2 <- (1 - s) sqrt(1 - t1^2) + s t2 with s = (1 + Vh.z) / 2; lift, Nh = t1 A1 + t2 A2 + sqrt(1 - t1^2 - t2^2) Vh; unstretch,
    H = normalize(alpha Nh.x, alpha Nh.y, Nh.z).  `axis` names the pair (A1, A2) that spans the disk:
      "heitz"      T1 = normalize(z x Vh) ((1, 0, 0) at Vh = z), T2 = Vh x T1: the warp acts along T2, the axis in the plane of Vh and the
                   surface normal, towards the normal.  The push-forward of the uniform square is then ggx_vndf (checked by quadrature in
                   the tests) and Nh.z >= 0 always.
      "reference"  D7: (A1, A2) = duff_basis(Vh) (Sampling.hpp:116-130, :261), the Heitz pair turned about Vh by psi:
                   A1 = cos(psi) T1 + sin(psi) T2, A2 = -sin(psi) T1 + cos(psi) T2.  With phi_V the azimuth of V, psi = -(phi_V + pi / 2):
                   0 only for V.x = 0 with V.y < 0, pi (the warp pushes AWAY from the normal) for V.x = 0 with V.y > 0.
    `clamp` is the second half of D7: max(0, Nh.z) before the last normalisation (Sampling.hpp:268), which moves the normals that the turned
    warp puts below the surface onto the horizon, H.z = 0 exactly.
    alpha, V[..., 0], u and v broadcast against each other (one view and many samples, or a view per sample); V unit with V.z > 0
    -> H (..., 3), psi in (-pi, pi] of V's own shape (a float for one view)."""
    V, u, v, alpha = np.asarray(V, dtype=np.float64), np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64), np.asarray(alpha, dtype=np.float64)
    Vh = np.stack(np.broadcast_arrays(alpha * V[..., 0], alpha * V[..., 1], V[..., 2]), axis=-1)
    Vh = Vh / np.linalg.norm(Vh, axis=-1, keepdims=True)
    T1 = np.stack([-Vh[..., 1], Vh[..., 0], np.zeros(Vh.shape[:-1])], axis=-1)
    length = np.linalg.norm(T1, axis=-1, keepdims=True)
    T1 = np.where(length > 0.0, T1 / np.where(length > 0.0, length, 1.0), np.array([1.0, 0.0, 0.0]))
    T2 = np.cross(Vh, T1)
    B1, B2 = duff_basis(Vh)
    psi = np.arctan2((B1 * T2).sum(axis=-1), (B1 * T1).sum(axis=-1))
    assert np.abs((B2 * T1).sum(axis=-1) + np.sin(psi)).max() <= 1e-9 and np.abs((B2 * T2).sum(axis=-1) - np.cos(psi)).max() <= 1e-9   # a rotation, not a reflection
    A1, A2 = {"heitz": (T1, T2), "reference": (B1, B2)}[axis]
    r, phi = np.sqrt(u), 2.0 * np.pi * v
    t1, t2 = r * np.cos(phi), r * np.sin(phi)
    s = 0.5 * (1.0 + Vh[..., 2])
    t2 = (1.0 - s) * np.sqrt(np.maximum(0.0, 1.0 - t1 * t1)) + s * t2
    Nh = t1[..., None] * A1 + t2[..., None] * A2 + np.sqrt(np.maximum(0.0, 1.0 - t1 * t1 - t2 * t2))[..., None] * Vh
    H = np.stack(np.broadcast_arrays(alpha * Nh[..., 0], alpha * Nh[..., 1], np.maximum(0.0, Nh[..., 2]) if clamp else Nh[..., 2]), axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        H = H / np.linalg.norm(H, axis=-1, keepdims=True)
    H = np.where(np.isfinite(H), H, np.array([0.0, 0.0, 1.0]))                      # alpha = 0 with the clamp at work: the mirror's normal
    return H, (float(psi) if psi.ndim == 0 else psi)


def frame_about(N):
    """Rotation matrices (m, 3, 3) of the shortest arc that takes +z to the unit vectors N (m, 3): R e_z = N; columns 0 and 1 are the
    tangent axes of the local frame (to_world(v) = R v, to_local(v) = R^T v).  From the quaternion (-N.y, N.x, 0, 1 + N.z), normalised."""
    q = np.stack([-N[:, 1], N[:, 0], np.zeros(len(N)), 1.0 + N[:, 2]], axis=1)
    return rotation_of_quaternion(q / np.linalg.norm(q, axis=1, keepdims=True))


def chi2_upper(dof, p):
    """Upper-p quantile of chi-square with `dof` degrees of freedom: scipy's where it is installed, else Wilson & Hilferty 1931,
    dof (1 - 2 / (9 dof) + z sqrt(2 / (9 dof)))^3 with z the normal quantile (at p = 1e-6: 0.7 % above scipy's at 30 degrees of freedom, 0.16 % at 100, 0.05 % at 255 - the fallback is the looser one, slightly)."""
    try:
        from scipy.stats import chi2
        return float(chi2.isf(p, dof))
    except ImportError:
        from statistics import NormalDist
        z = NormalDist().inv_cdf(1.0 - p)
        return float(dof * (1.0 - 2.0 / (9.0 * dof) + z * np.sqrt(2.0 / (9.0 * dof))) ** 3)


def hemisphere_grid(n_theta, n_phi):
    """Midpoint grid on the upper hemisphere in (theta, phi): -> directions (n, 3), solid-angle weights (n,)."""
    th = (np.arange(n_theta) + 0.5) * (0.5 * np.pi / n_theta)
    ph = (np.arange(n_phi) + 0.5) * (2 * np.pi / n_phi)
    T, Pp = np.meshgrid(th, ph, indexing="ij")
    d = np.stack([np.sin(T) * np.cos(Pp), np.sin(T) * np.sin(Pp), np.cos(T)], axis=-1).reshape(-1, 3)
    w = (np.sin(T) * (0.5 * np.pi / n_theta) * (2 * np.pi / n_phi)).reshape(-1)
    return d, w


# ---- D. camera, sky, resolve ----------------------------------------------------------------------------------------------------
def lens_z(height, focal_length):
    """Pinhole with a 24 mm high sensor: the image plane, in pixels, lies at z = -(height / 2) * focal_length / 12."""
    return -(height * 0.5) * focal_length / 12.0


def project(direction, orient, half_width, half_height, z):
    """Where a world-space direction pierces the image plane of a pinhole looking down -z in its own frame: rotate back by the
    conjugate of the orientation quaternion (x, y, z, w), scale to the plane.  -> pixel coordinates x, y (float)."""
    R = rotation_of_quaternion(np.asarray(orient, dtype=np.float64)[None, :])[0]
    R = R / np.cbrt(np.linalg.det(R))
    local = direction @ R                                                           # R^T d, row-vector form
    s = z / local[:, 2]
    return local[:, 0] * s + half_width, local[:, 1] * s + half_height, local[:, 2]


def pixel_of_slot(index, width):
    """Ray / accumulator slot -> pixel: slots are tile-major, 256 per 16 x 16 tile, tiles row by row, 16 pixels a row in the tile."""
    tile, ID = index // 256, index % 256
    h_tiles = width // 16
    return 16 * (tile % h_tiles) + ID % 16, 16 * (tile // h_tiles) + ID // 16


def equirect_texel(d, width, height):
    """Latitude-longitude lookup (Debevec's convention turned so that u = 1/2 + atan2(z, x) / 2 pi, v = 1/2 - asin(y) / pi) under D2:
    -> column, row (int), and the continuous coordinates ex, ey they were truncated from."""
    ex = (width - 1) * (0.5 + np.arctan2(d[:, 2], d[:, 0]) / (2 * np.pi))
    ey = (height - 1) * (0.5 - np.arcsin(np.clip(d[:, 1], -1.0, 1.0)) / np.pi)
    return np.floor(ex).astype(np.int64), np.floor(ey).astype(np.int64), ex, ey


ACES_IN = np.array([[0.59719, 0.35458, 0.04823], [0.07600, 0.90834, 0.01566], [0.02840, 0.13383, 0.83777]])
ACES_OUT = np.array([[1.60475, -0.53108, -0.07367], [-0.10208, 1.10813, -0.00605], [-0.00327, -0.07276, 1.07602]])


def aces_fitted(rgb):
    """Stephen Hill's published fit of the ACES RRT + ODT (BakingLab ACES.hlsl): input matrix, rational fit, output matrix, saturate."""
    v = rgb @ ACES_IN.T
    v = (v * (v + 0.0245786) - 0.000090537) / (v * (0.983729 * v + 0.4329510) + 0.238081)
    return np.clip(v @ ACES_OUT.T, 0.0, 1.0)


def resolve(acc, accumulations, exposure, width, height):
    """Median of means (Renderer.hpp:436-478) from the accumulator [tile][bucket][rgb][256] alone: per-bucket mean, np.median across the
    buckets (even counts: the mean of the two middle values, numpy's convention), exposure, ACES, alpha 1.  -> (height, width, 4)."""
    acc = np.asarray(acc, dtype=np.float64)
    k = acc.shape[1]
    mean = acc / (accumulations / k)
    med = np.median(mean, axis=1) * exposure                                        # [tile][rgb][256]
    rgb = aces_fitted(np.moveaxis(med, 1, 2).reshape(-1, 3))
    x, y = pixel_of_slot(np.arange(acc.shape[0] * 256), width)
    out = np.zeros((height, width, 4))
    out[y, x, :3] = rgb
    out[y, x, 3] = 1.0
    return out


def sphere_depth_normal(ix, iy, half_width, half_height, z, eye_z, radius=1.0):
    """A pinhole at (0, 0, eye_z) looking down -z (identity orientation) at a sphere about the origin: image-plane point (ix, iy) ->
    distance to the first hit (inf on a miss) and the unit normal there."""
    d = np.stack([ix - half_width, iy - half_height, np.full_like(ix, z)], axis=-1)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    b = -eye_z * d[..., 2]
    disc = b * b - (eye_z * eye_z - radius * radius)
    t = np.where(disc >= 0, b - np.sqrt(np.maximum(disc, 0.0)), np.inf)
    with np.errstate(invalid="ignore"):
        n = (np.array([0.0, 0.0, eye_z]) + d * np.where(np.isfinite(t), t, 0.0)[..., None]) / radius
    return t, n


# ---- F. next-event estimation and multiple importance sampling ------------------------------------------------------------------
# The expectation of the estimator the path implements at a Lambertian point lit by sphere lights, from the textbook forms
# (Veach 1997, ch. 9: multiple importance sampling, the power heuristic with beta = 2; Shirley & Wang 1996: the cone a sphere subtends)
# plus the named departures
#   D5  the closure pdf that the NEXT emissive hit weighs itself with is max(0, w.z) / pi of the WORLD-space direction, not of the
#       direction in the surface's frame (Renderer.hpp:386,401); the light sample's weight uses the local one.
#   D6  the power heuristic is f^2 / max(1e-6, f^2 + g^2) (Sampling.hpp:241-247).
# A light is (centre (3,), radius_sq, emission (3,)); blockers are (centres (k, 3), radius_sq (k,)), k >= 0.  Points x with unit normals n
# are (m, 3).  The light sample and the closure sample of one bounce are drawn from different seeds and are taken as independent.
OFFSET = 1e-4                                      # the shading point is moved by this along the normal before any ray leaves it


def power_heuristic(f, g, floor=1e-6):
    """Veach's power heuristic with beta = 2; `floor` is D6."""
    return f * f / np.maximum(floor, f * f + g * g)


def basis_about(w):
    """Two unit vectors that complete unit vectors w (m, 3) to right-handed orthonormal frames (cross products with the axis w is least along)."""
    a = np.zeros_like(w)
    a[np.arange(len(w)), np.argmin(np.abs(w), axis=1)] = 1.0
    t = np.cross(a, w); t /= np.linalg.norm(t, axis=1, keepdims=True)
    return t, np.cross(w, t)


def cone_quadrature(P, centre, radius_sq, n_u, n_phi):
    """Midpoint rule over the cone that the sphere (centre, radius_sq) subtends from each of the points P (m, 3), in the parameters of
    uniform cone sampling: cos(theta) = 1 - u (1 - cos theta_max) with u and phi / 2 pi at the midpoints of an n_u x n_phi grid.  Every cell
    carries the same solid angle, so the constant pdf cone_pdf integrates to 1 exactly - asserted.
    -> directions (m, q, 3), weight (m,) of one cell, distance (m, q) to the sphere's surface along each direction, sin^2(theta_max) (m,)."""
    wc = centre[None, :] - P
    d2 = (wc * wc).sum(axis=1)
    assert (d2 > radius_sq).all(), "a point inside the sphere sees no cone"
    d = np.sqrt(d2)
    wc = wc / d[:, None]
    sin2 = radius_sq / d2
    pdf, omc = cone_pdf(sin2, floor=0.0)
    uu = (np.arange(n_u) + 0.5) / n_u
    ph = 2.0 * np.pi * (np.arange(n_phi) + 0.5) / n_phi
    cos_t = 1.0 - uu[None, :] * omc[:, None]                                         # (m, n_u)
    sin_t = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
    t, b = basis_about(wc)
    ring = np.cos(ph)[None, :, None] * t[:, None, :] + np.sin(ph)[None, :, None] * b[:, None, :]    # (m, n_phi, 3)
    dirs = (sin_t[:, :, None, None] * ring[:, None, :, :] + cos_t[:, :, None, None] * wc[:, None, None, :]).reshape(len(P), n_u * n_phi, 3)
    weight = 2.0 * np.pi * omc / (n_u * n_phi)
    assert np.abs(pdf * weight * (n_u * n_phi) - 1.0).max() <= 1e-12
    cq, sq = np.repeat(cos_t, n_phi, axis=1), np.repeat(sin_t, n_phi, axis=1)
    dist = d[:, None] * cq - np.sqrt(np.maximum(0.0, radius_sq - (d[:, None] * sq) ** 2))
    return dirs, weight, dist, sin2


def visible(P, dirs, dist, others):
    """V of the rendering equation along dirs (m, q, 3) from P (m, 3) up to dist (m, q): 1 unless `occluded` finds a sphere of `others` on the way."""
    centres, r2 = others
    if len(r2) == 0:
        return np.ones(dist.shape)
    m, q = dist.shape
    occ, _ = occluded(np.repeat(P, q, axis=0), dirs.reshape(-1, 3), dist.reshape(-1), np.asarray(centres, dtype=np.float64), np.asarray(r2, dtype=np.float64), chunk=1 << 16)
    return 1.0 - occ.reshape(m, q)


def _others(lights, k, blockers):
    """Everything that can stand between a point and light k: the blockers and the other lights."""
    c = [np.asarray(blockers[0], dtype=np.float64).reshape(-1, 3)] + [np.asarray(l[0], dtype=np.float64)[None, :] for j, l in enumerate(lights) if j != k]
    r = [np.asarray(blockers[1], dtype=np.float64).reshape(-1)] + [np.array([float(l[1])]) for j, l in enumerate(lights) if j != k]
    return np.concatenate(c), np.concatenate(r)


NO_BLOCKERS = (np.zeros((0, 3)), np.zeros(0))


def direct_lambert(x, n, rho, lights, blockers=NO_BLOCKERS, q8=True, n_u=16, n_phi=32, n_lights_in_light_pdf=None, n_lights_in_hit_weight=None):
    """One path's contribution from a Lambertian point of albedo rho (3,) under black lights (albedo 0: a path that reaches one ends
    there) and black blockers, max_bounces >= 3, MIS on.  Two samples see the light: the light sample, weighted w_l = p_l^2 / (p_l^2 + p_b^2),
    and the cosine-distributed closure sample that survives the roulette with p = max(rho), carries rho / p and finds the light, weighted
    w_b = p_b'^2 / (p_b'^2 + p_l^2);  p_l = cone_pdf / n_lights, p_b = max(0, w.n) / pi, p_b' = max(0, w.z) / pi with q8 (D5), = p_b without.

        E  = sum over lights  Le rho / pi  int_cone cos+(w.n) V(w) [w_l(w) + w_b(w)] dw                 (p cancels)
        M2 = sum over lights  int p_l (Le rho cos+ w_l V / (pi p_l))^2 dw  +  p int cos+ / pi (Le rho w_b V / p)^2 dw  +  2 E_l E_b

    (the last term: the two samples are independent).  Without q8 the weights sum to 1 and E is the form factor of the light.
    `n_lights_in_*` are there for the guards only: what the expectation would be if the number of lights were left out of one pdf.
    -> dict E (m, 3), M2 (m, 3), shadow (m,): the probability that the light sample casts a shadow ray (it lies above the horizon and
    carries a positive contribution), var (m, 3) = M2 - E^2."""
    x, n, rho = (np.asarray(a, dtype=np.float64) for a in (x, n, rho))
    P = x + OFFSET * n
    p = rho.max()
    nl_l = len(lights) if n_lights_in_light_pdf is None else n_lights_in_light_pdf
    nl_b = len(lights) if n_lights_in_hit_weight is None else n_lights_in_hit_weight
    E_l, E_b, M2_l, M2_b, shadow = np.zeros((len(x), 3)), np.zeros((len(x), 3)), np.zeros((len(x), 3)), np.zeros((len(x), 3)), np.zeros(len(x))
    for k, (c, r2, Le) in enumerate(lights):
        c, Le = np.asarray(c, dtype=np.float64), np.asarray(Le, dtype=np.float64)
        dirs, wq, dist, sin2 = cone_quadrature(P, c, float(r2), n_u, n_phi)
        cos_n = np.maximum(0.0, (dirs * n[:, None, :]).sum(axis=2))
        V = visible(P, dirs, dist, _others(lights, k, blockers))
        cone = cone_pdf(sin2)[0][:, None]                                            # D4 inside
        p_l, p_l_hit = cone / nl_l, cone / nl_b
        p_b = cos_n / np.pi
        p_b_hit = np.maximum(0.0, dirs[:, :, 2]) / np.pi if q8 else p_b
        w_l = power_heuristic(p_l, p_b)
        w_b = np.where(cos_n > 0.0, power_heuristic(p_b_hit, p_l_hit), 0.0)
        f_l = (cos_n * V * w_l / np.pi)                                               # per unit Le rho
        f_b = (cos_n * V * w_b / np.pi)
        s_l, s_b = (f_l * wq[:, None]).sum(axis=1), (f_b * wq[:, None]).sum(axis=1)
        E_l += s_l[:, None] * (Le * rho)[None, :]
        E_b += s_b[:, None] * (Le * rho)[None, :]
        pick_pdf = cone / len(lights)                                                 # the density the light sample is really drawn with
        m2_l = ((f_l / pick_pdf) ** 2 * pick_pdf * wq[:, None]).sum(axis=1)
        m2_b = (cos_n / np.pi * (V * w_b) ** 2 * wq[:, None]).sum(axis=1) / p
        M2_l += m2_l[:, None] * (Le * rho)[None, :] ** 2
        M2_b += m2_b[:, None] * (Le * rho)[None, :] ** 2
        shadow += ((cos_n > 0.0) & (w_l > 0.0)).mean(axis=1) / len(lights)
    E = E_l + E_b
    M2 = M2_l + M2_b + 2.0 * E_l * E_b
    return dict(E=E, M2=M2, var=M2 - E * E, shadow=shadow)


def form_factor_sphere(x, n, rho, light):
    """Radiance leaving a Lambertian point towards any direction under one unoccluded sphere light that lies wholly above the horizon:
    rho Le (r / d)^2 cos(theta_c), theta_c between the normal and the centre (the sphere's view factor; Howell's catalogue B-43)."""
    c, r2, Le = light
    P = np.asarray(x, dtype=np.float64) + OFFSET * np.asarray(n, dtype=np.float64)
    wc = np.asarray(c, dtype=np.float64)[None, :] - P
    d2 = (wc * wc).sum(axis=1)
    cos_c = (wc * n).sum(axis=1) / np.sqrt(d2)
    assert (cos_c > np.sqrt(r2 / d2)).all(), "the closed form needs the whole sphere above the horizon"
    return (r2 / d2 * cos_c)[:, None] * (np.asarray(Le, dtype=np.float64) * np.asarray(rho, dtype=np.float64))[None, :]


def direct_no_mis(x, n, rho, lights, blockers=NO_BLOCKERS, n_u=16, n_phi=32):
    """Q9: with MIS off there is no light sample, and an emissive hit adds its RAW emission - no throughput, so neither rho nor the
    roulette's 1 / p.  The closure sample survives with p = max(rho) and is cosine-distributed:  E = p Le int_cone cos+ / pi V dw,
    M2 = p Le^2 int_cone cos+ / pi V dw.  No shadow ray is ever cast."""
    x, n, rho = (np.asarray(a, dtype=np.float64) for a in (x, n, rho))
    P = x + OFFSET * n
    p = rho.max()
    E, M2 = np.zeros((len(x), 3)), np.zeros((len(x), 3))
    for k, (c, r2, Le) in enumerate(lights):
        Le = np.asarray(Le, dtype=np.float64)
        dirs, wq, dist, sin2 = cone_quadrature(P, np.asarray(c, dtype=np.float64), float(r2), n_u, n_phi)
        cos_n = np.maximum(0.0, (dirs * n[:, None, :]).sum(axis=2))
        s = (cos_n / np.pi * visible(P, dirs, dist, _others(lights, k, blockers)) * wq[:, None]).sum(axis=1)
        E += p * s[:, None] * Le[None, :]
        M2 += p * s[:, None] * (Le * Le)[None, :]
    return dict(E=E, M2=M2, var=M2 - E * E, shadow=np.zeros(len(x)))


def ggx_vndf_pdf_of_direction(alpha, L, V):
    """Density, per solid angle of L, of the reflection of V about a visible normal (Heitz 2018, eq. 17): D_V(H) / (4 V.H) =
    G1(V) D(H) / (4 V.z).  What Closure<GGX>::pdf would be had the reference written it; it returns 0 (DataStreams.hpp:196-198)."""
    H = L + V
    H = H / np.linalg.norm(H, axis=-1, keepdims=True)
    a2 = alpha * alpha
    return np.where((L[..., 2] > 0.0) & (H[..., 2] > 0.0), ggx_g1(a2, V[..., 2]) * ggx_d(np.maximum(a2, 1e-5), np.maximum(H[..., 2], 0.0))[0] / (4.0 * V[..., 2]), 0.0)


def path_sampler(scene, x, n, n_paths, max_bounces, rng, mis=True, q5=True, q8=True, prim0=0, brdf=0, view=None, decay=(), axis="reference", clamp=True,
                 closure_pdf="zero"):
    """A plain path tracer in float64 numpy for Lambertian spheres, one light sample and one cosine-distributed closure sample a bounce.
    scene: dict centre (k, 3), radius_sq (k,), albedo (k, 3), emission (k, 3).  Every row of x, n (m, 3) - a first hit on sphere `prim0`
    and its unit normal - starts n_paths paths.  Textbook throughout (cosine sampling by Malley's method, uniform cone sampling,
    sphere_roots for every intersection, its own generator) with the named departures: Q5 (a path that still hits on the last bounce
    is dropped whole; `q5`), Q6 (roulette from bounce 0 with max(throughput), unclamped), Q8 / D5 (`q8`), Q9 (an emissive hit adds its raw
    emission at bounce 0 or without MIS), D4, D6.  The sky is black (Q10 cannot appear).
    brdf = 1 is the GGX closure (part G): scene carries F0 (k, 3) and roughness (k,) as well, `view` (m, 3) the unit directions from the
    first hits back to the eye, `decay` the gloss-decay table (0 beyond its length).  Per bounce alpha = a^2 + (1 - a^2) decay[bounce] with
    a the roughness; the light sample carries Le thr f cos / p_l - ggx_eval_cos, and the closure pdf is 0 as the reference wrote it, so D6's
    floored heuristic p_l / max(1e-6, p_l^2 + 0) is 1 / p_l and an emissive hit past bounce 0 weighs 0; the bounce reflects the view about
    ggx_visible_normal(axis, clamp) (D7) and multiplies the throughput by ggx_vndf_weight BEFORE the roulette takes max(throughput).
    `closure_pdf="vndf"` is a what-if for the guards: the true density ggx_vndf_pdf_of_direction in both MIS weights.
    -> dict sum, sum_sq (m, 3): over the n_paths contributions of each row; shadow, rays (m,): shadow rays cast and rays traced beyond
    the given first hit; dropped (m,)."""
    centre, r2 = np.asarray(scene["centre"], dtype=np.float64), np.asarray(scene["radius_sq"], dtype=np.float64)
    albedo, emission = np.asarray(scene["albedo"], dtype=np.float64), np.asarray(scene["emission"], dtype=np.float64)
    lights = np.flatnonzero((emission * emission).sum(axis=1) > 0.0)
    emissive = emission.max(axis=1) > 0.0
    m = len(x)
    row = np.repeat(np.arange(m), n_paths)
    N = len(row)
    nrm = np.asarray(n, dtype=np.float64)[row]
    ggx = brdf == 1
    if ggx:
        F0, rough, Vw = np.asarray(scene["F0"], dtype=np.float64), np.asarray(scene["roughness"], dtype=np.float64), np.asarray(view, dtype=np.float64)[row].copy()
    P = np.asarray(x, dtype=np.float64)[row] + OFFSET * nrm
    prim = np.full(N, prim0)
    thr, rad = np.ones((N, 3)), np.zeros((N, 3))
    pdf_in, origin = np.zeros(N), np.zeros((N, 3))
    alive = np.arange(N)                                                             # indices of the paths still under way
    out = dict(sum=np.zeros((m, 3)), sum_sq=np.zeros((m, 3)), shadow=np.zeros(m), rays=np.zeros(m), dropped=np.zeros(m))

    def nearest(p, d, skip=None):
        b, oc2, disc = sphere_roots(p, d, centre, r2)
        s = np.sqrt(np.maximum(disc, 0.0))
        t = np.where(b - s >= 0.0, b - s, b + s)
        t = np.where((disc >= 0.0) & (t >= 0.0), t, np.inf)
        if skip is not None:
            t[np.arange(len(p)), skip] = np.inf
        k = np.argmin(t, axis=1)
        return t[np.arange(len(p)), k], k

    for bounce in range(max_bounces):
        if len(alive) == 0:
            break
        a = alive
        if bounce == max_bounces - 1:
            if q5:                                                                   # Q5
                rad[a] = 0.0
                np.add.at(out["dropped"], row[a], 1.0)
            break
        if ggx:
            R = frame_about(nrm[a])
            Vl = np.einsum("nji,nj->ni", R, Vw[a])
            a2r = rough[prim[a]] ** 2
            alpha = a2r + (1.0 - a2r) * (decay[bounce] if bounce < len(decay) else 0.0)
        if mis and len(lights):
            pick = lights[rng.integers(0, len(lights), len(a))]
            wc = centre[pick] - P[a]
            d2 = (wc * wc).sum(axis=1)
            ok = (pick != prim[a]) & (d2 > r2[pick])
            d = np.sqrt(d2)
            wc = wc / d[:, None]
            sin2 = np.minimum(r2[pick] / d2, 1.0)
            pdf_c, omc = cone_pdf(sin2)                                              # D4
            cos_t = 1.0 - rng.random(len(a)) * omc
            sin_t = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
            phi = 2.0 * np.pi * rng.random(len(a))
            t_, b_ = basis_about(wc)
            w = sin_t[:, None] * (np.cos(phi)[:, None] * t_ + np.sin(phi)[:, None] * b_) + cos_t[:, None] * wc
            cos_n = (w * nrm[a]).sum(axis=1)
            p_l = pdf_c / len(lights)
            if ggx:
                Ll = np.einsum("nji,nj->ni", R, w)
                with np.errstate(invalid="ignore", divide="ignore"):
                    f = ggx_eval_cos(F0[prim[a]], alpha, Ll, Vl)[0]
                    p_b = ggx_vndf_pdf_of_direction(alpha, Ll, Vl) if closure_pdf == "vndf" else np.zeros(len(a))
                contrib = emission[pick] * thr[a] * np.nan_to_num(f) * (p_l / np.maximum(1e-6, p_l * p_l + p_b * p_b))[:, None]          # D6
                cos_n = Ll[:, 2]
            else:
                p_b = np.maximum(0.0, cos_n) / np.pi
                contrib = emission[pick] * thr[a] * albedo[prim[a]] * (p_b * p_l / np.maximum(1e-6, p_l * p_l + p_b * p_b))[:, None]     # D6
            cast = ok & (cos_n >= 0.0) & (contrib.max(axis=1) > 0.0)
            reach = d * cos_t - np.sqrt(np.maximum(0.0, r2[pick] - (d * sin_t) ** 2))
            t_near, _ = nearest(P[a], w, skip=pick)
            rad[a] += np.where((cast & ~(t_near < reach))[:, None], contrib, 0.0)
            np.add.at(out["shadow"], row[a], cast.astype(np.float64))
        em = emissive[prim[a]]
        if mis and len(lights) and bounce > 0:
            oc = centre[prim[a]] - origin[a]
            g = cone_pdf(np.minimum(r2[prim[a]] / (oc * oc).sum(axis=1), 1.0))[0] / len(lights)
            rad[a] += np.where(em[:, None], thr[a] * power_heuristic(pdf_in[a], g)[:, None] * emission[prim[a]], 0.0)
        else:
            rad[a] += np.where(em[:, None], emission[prim[a]], 0.0)                  # Q9
        if ggx:
            H = ggx_visible_normal(alpha, Vl, rng.random(len(a)), rng.random(len(a)), axis=axis, clamp=clamp)[0]
            L = 2.0 * (H * Vl).sum(axis=1)[:, None] * H - Vl
            L = L / np.linalg.norm(L, axis=1, keepdims=True)
            with np.errstate(invalid="ignore", divide="ignore"):
                est = np.where((L[:, 2] > 0.0)[:, None], np.nan_to_num(ggx_vndf_weight(F0[prim[a]], alpha, L, Vl)[0]), 0.0)
                pdf_new = ggx_vndf_pdf_of_direction(alpha, L, Vl) if closure_pdf == "vndf" else np.zeros(len(a))
            thr[a] = thr[a] * est
            p = thr[a].max(axis=1)
            live = rng.random(len(a)) < p                                            # Q6, on the estimator
            a = a[live]
            thr[a] = thr[a] / p[live][:, None]
            w = np.einsum("nij,nj->ni", R[live], L[live])
            pdf_in[a] = pdf_new[live]
            Vw[a] = -w
        else:
            thr[a] = thr[a] * albedo[prim[a]]
            p = thr[a].max(axis=1)
            live = rng.random(len(a)) < p                                            # Q6
            a = a[live]
            thr[a] = thr[a] / p[live][:, None]
            r_, phi = np.sqrt(rng.random(len(a))), 2.0 * np.pi * rng.random(len(a))  # Malley: a uniform disk, lifted
            t_, b_ = basis_about(nrm[a])
            w = (r_ * np.cos(phi))[:, None] * t_ + (r_ * np.sin(phi))[:, None] * b_ + np.sqrt(np.maximum(0.0, 1.0 - r_ * r_))[:, None] * nrm[a]
            pdf_in[a] = np.maximum(0.0, w[:, 2] if q8 else (w * nrm[a]).sum(axis=1)) / np.pi                                         # D5
        origin[a] = P[a]
        np.add.at(out["rays"], row[a], 1.0)
        t_hit, k = nearest(P[a], w)
        found = np.isfinite(t_hit)
        a, w, t_hit, k = a[found], w[found], t_hit[found], k[found]
        hit = P[a] + w * t_hit[:, None]
        nn = (hit - centre[k]) / np.sqrt(r2[k])[:, None]
        nn = np.where(((nn * w).sum(axis=1) >= 0.0)[:, None], -nn, nn)
        nrm[a], prim[a] = nn, k
        P[a] = hit + OFFSET * nn
        alive = a
    np.add.at(out["sum"], row, rad)
    np.add.at(out["sum_sq"], row, rad * rad)
    return out
