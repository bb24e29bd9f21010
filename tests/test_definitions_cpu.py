"""The CPU oracle against float64 definitions of each operation (tests/definitions.py), operation by operation.

Every other test compares the HIP path with oracle/oracle.cpp bit for bit; both were written from the same reference lines, so a shared
misreading passes all of them.  Here each operation is held to a statement of what it is meant to compute, in float64 numpy, written from
the textbook formula.  The `check_*` functions take a backend (this file: the oracle through oracle_binding; test_definitions_gpu.py:
the kernels through the debug entry points) so that both sides face the same inputs, the same definitions and the same bounds.

Bounds are never taken from the code under test.  Each is either derived (the derivation is at the constant or in definitions.py) or
measured on the CPU oracle and given a stated margin; the measured figure is in the docstring of the check and in DESIGN.md §2.
Reference departures from the textbook are named expectations (D1-D4 in definitions.py, Q rows of SURVEY.md §8a).

Part F holds next-event estimation and MIS to float64 expectations of the estimator the reference implements (Q8 and Q9 are named
departures there, not reasons to look away) for the Lambertian closure.  Part C holds the GGX closure's sampled normal to its stated
density (D7) by chi-square; part G holds the GGX closure inside the path (light sample, roulette, per-bounce roughness, Q5 under it) to
float64 expectations, G3 from a grazing camera.  Left open: inside the path the axis and the clamp of D7 are not told apart under the
cap of 1 500 accumulations, and Q11 under a differing authoring order; stream order and Q14 (fused body, unfused tail) are
arithmetic, not definitions.  Those rows stay pinned by parity alone."""
import math

import numpy as np
import pytest

import definitions as df
import oracle_binding as ob
from definitions import u

f32, f64 = np.float32, np.float64

# ---- bounds ---------------------------------------------------------------------------------------------------------------------
EXCLUDED_CAP = 0.005                  # part A: share of rays per scene that may be set aside as undecidable in binary32 (set by the issue)
SINCOS_ABS = 2e-6                     # asserted by test_fast_math_properties against float64 sin / cos
ATAN2_ABS, ASIN_ABS = 2e-3, 1e-3      # likewise
# azimuth: sincos bound + rounding of the argument 2 pi s (constant, product: 3 roundings of a value <= 2 pi) + sqrt and product
AZIMUTH_ABS = SINCOS_ABS + 2 * math.pi * 3 * u + 2 * u
# unit length of a sampled direction: |len^2 - 1| <= rho^2 |s^2 + c^2 - 1| <= 2 * 2 * SINCOS_ABS, so |len - 1| <= 2 * SINCOS_ABS; + roundings
UNIT_ABS = 2 * SINCOS_ABS + 8 * u
FRAME_ROUNDING = 24 * u               # q's three components carry <= 3 roundings each: |q|^2 to 6u, |q|^4 to 12u; doubled
CONE_ANGLE_ABS = SINCOS_ABS + 16 * u  # direction components: sincos bound + basis / combination roundings; angle error <= component error
# GGX eval: D's denominator k = 1 + (a^2 - 1) cos^2 cancels.  cos^2 of the normalised half vector carries 7u, the product 9u (value <= 1),
# the sum one more: |dk| <= 10u, D = a^2 / (pi k^2) -> 20u / k relative; 24u / k taken.  The rest (F, G2, H.V, products: about 30 roundings): 64u.
GGX_EVAL_K, GGX_EVAL_REL = 24 * u, 64 * u
GGX_WEIGHT_REL = 64 * u               # measured 1.0e-6 on the oracle where H.V > 0.1 (two G1, their ratio, Schlick), margin x 3.7
# F is a function of H.V, and H.V is known from the binary32 direction only through (H.V)^2 = (1 + L.V) / 2: L's components carry u / 2 each,
# so d(H.V)^2 <= u and d(H.V) <= u / (2 H.V); Schlick's slope is <= 5 -> dF <= 2.5u / (H.V); 10u / (H.V) taken (grazing V: H.V ~ 1e-3)
GGX_HV_COND = 10 * u
GGX_UPPER_ABS = 16 * u                # H.z >= 0 and V.H >= 0 up to the rounding of the reflected direction
RESOLVE_ABS = 32 * u                  # ACES in binary32: fit to ~10u relative, output matrix row sums of |m| <= 2.21 -> < 30u; measured 2.7e-7
PROJECT_REL = 32 * u                  # rotation + normalisation: < 16 roundings of values <= the image-plane distance; doubled
SIGMA = 5.0                           # whole-path closed forms: 5 sigma with the analytic sigma (a bound for the reference itself)


def report(name, **figures):
    print(f"[definitions] {name}: " + ", ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items()))


# ---- the oracle as a backend ----------------------------------------------------------------------------------------------------
class OracleBackend:
    name = "oracle"
    variants = (("brute", dict(trav_mode=ob.TRAV_BRUTE)), ("twin_bvh", dict(trav_mode=ob.TRAV_PER_RAY_BVH)))

    def __init__(self, mirt):
        self.mirt, self.lib = mirt, ob.load()

    @staticmethod
    def _c(a):
        return np.ascontiguousarray(a, dtype=f32)

    def hemisphere(self, t, s):
        out = np.empty((len(t), 3), dtype=f32); base = out.ctypes.data
        for i in range(len(t)):
            self.lib.orc_hemisphere(float(t[i]), float(s[i]), base + 12 * i)
        return out

    def frame(self, N, v):
        N, v = self._c(N), self._c(v)
        q, l, w = (np.empty((len(N), k), dtype=f32) for k in (4, 3, 3))
        nb, vb, qb, lb, wb = (a.ctypes.data for a in (N, v, q, l, w))
        for i in range(len(N)):
            self.lib.orc_tangent_space(nb + 12 * i, qb + 16 * i)
            self.lib.orc_to_local(qb + 16 * i, vb + 12 * i, lb + 12 * i)
            self.lib.orc_to_world(qb + 16 * i, vb + 12 * i, wb + 12 * i)
        return q, l, w

    def sample_sphere(self, Wc, sin2, dist, r2, t, s):
        Wc = self._c(Wc); out = np.empty((len(Wc), 5), dtype=f32); wb, base = Wc.ctypes.data, out.ctypes.data
        for i in range(len(Wc)):
            self.lib.orc_sample_direction_to_sphere(wb + 12 * i, float(sin2[i]), float(dist[i]), float(r2[i]), float(t[i]), float(s[i]), base + 20 * i)
        return out

    def ggx_eval(self, F0, alpha, L, V):
        F0, L, V = self._c(F0), self._c(L), self._c(V); out = np.empty((len(L), 3), dtype=f32)
        fb, lb, vb, base = (a.ctypes.data for a in (F0, L, V, out))
        for i in range(len(L)):
            self.lib.orc_ggx_eval(fb + 12 * i, float(alpha[i]), lb + 12 * i, vb + 12 * i, base + 12 * i)
        return out

    def ggx_sample(self, F0, alpha, V, u0, u1):
        F0, V = self._c(F0), self._c(V); d, e = np.empty((len(V), 3), dtype=f32), np.empty((len(V), 3), dtype=f32)
        fb, vb, db, eb = (a.ctypes.data for a in (F0, V, d, e))
        for i in range(len(V)):
            self.lib.orc_ggx_sample(fb + 12 * i, float(alpha[i]), vb + 12 * i, float(u0[i]), float(u1[i]), db + 12 * i, eb + 12 * i)
        return d, e

    def raygen(self, sc, w, h, acc, max_bounces=16):
        o = ob.Oracle(sc, max_bounces=max_bounces); o.Resize(w, h)
        p, d = o.raygen(acc); o.close()
        return p, d

    def tracers(self, sc):
        for label, kw in self.variants:
            o = ob.Oracle(sc); o.Resize(16, 16)
            mode = kw["trav_mode"]
            yield label, (lambda P, D, o=o, m=mode: o.trace_closest(P, D, m)), (lambda P, D, T, o=o, m=mode: o.trace_shadow(P, D, T, m))
            o.close()

    def render(self, sc, w, h, n_acc, max_bounces, buckets=5, mis=True, variant=0, brdf=0, gloss_decay=None):
        o = ob.Oracle(sc, max_bounces=max_bounces, buckets=buckets, mis=mis, brdf=brdf, gloss_decay=gloss_decay, **self.variants[variant][1])
        o.Resize(w, h); o.Accumulate(n_acc)
        out = dict(acc=o.accumulator(), frame=o.Render() if n_acc % buckets == 0 else None, counters=o.counters())
        o.close()
        return out


@pytest.fixture(scope="module")
def be(mirt):
    return OracleBackend(mirt)


def pcg(mirt, seed, n):
    """n draws of the project's own generator (Random.hpp:20-29 as restated in scene.py), binary32 in [0, 1]."""
    return mirt.scene.pcg_floats(mirt.scene.hash_u32(seed), n)


def unit_f32(v):
    """glm::normalize in binary32: v * (1 / sqrt(dot)) - the way normals reach the frame on the path."""
    v = np.asarray(v, dtype=f32)
    d = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    return v * (f32(1.0) / np.sqrt(d))[:, None]


# ---- A. intersection and occlusion ----------------------------------------------------------------------------------------------
def awkward_scene(mirt):
    """Exact duplicates, a concentric shell, a sphere around the camera, tiny and huge radii, half the centres on one plane."""
    S = mirt.scene
    rng = np.random.default_rng(5)
    n = 65
    geo = np.zeros(n, dtype=S.SPHERE)
    geo["position"] = rng.uniform(-6, 6, (n, 3)).astype(f32)
    geo["radius_sq"] = (rng.uniform(0.05, 1.2, n) ** 2).astype(f32)
    geo["position"][1] = geo["position"][0]; geo["radius_sq"][1] = geo["radius_sq"][0]
    geo["position"][2] = geo["position"][0]; geo["radius_sq"][2] = geo["radius_sq"][0] * 4
    geo["position"][3] = (0.0, 1.0, 14.0); geo["radius_sq"][3] = 4.0
    geo["radius_sq"][4] = 1e-6; geo["radius_sq"][5] = 400.0
    geo["position"][n // 2:, 1] = 0.5
    mats = np.zeros(2, dtype=S.MATERIAL); mats["albedo"] = 0.5; mats["emission"][1] = 15.0
    geo["material_ID"][::16] = 1
    cam = S.Camera(eye=(0.0, 1.0, 14.0), direction=(0.0, -0.05, -1.0), focal_length=35.0, exposure=1.0)
    return S.Scene(geo, mats, cam, np.full(3, 0.3, dtype=f32), name="awkward")


TRACE_SCENES = {"default9": (lambda m: m.scene.default9(), 20000), "S8a": (lambda m: m.scene.synthetic(8, ambient=0.5), 20000),
                "S1000a": (lambda m: m.scene.synthetic(1000, ambient=0.5), 20000), "awkward": (awkward_scene, 20000)}


def ray_mix(sc, n_rays):
    """The ray mix of test_trace_kernels_bit_exact: the 128 x 128 camera rays, then rays from points at 0.5, 1 -+ 1e-3, 1.5 and 3 radii
    off sphere centres in random directions; five axis-parallel; a quarter with non-unit directions (|D| 0.9 ... 1.5, D1).  One change,
    reasoned: that test starts a fifth of its rays ON the surface (factor 1.0).  Such a ray has a root that is zero up to rounding, so whether
    binary32 reports 0, the far root or a miss is undecidable for every one of them - 20 % of the mix against a 0.5 % cap - and they are
    moved to 1e-3 radii either side of the surface."""
    o = ob.Oracle(sc); o.Resize(128, 128)
    cp, cd = o.raygen(1)
    prims = o.bvh()[1]
    o.close()
    rng = np.random.default_rng(3)
    geo = sc.geometry
    pick = rng.integers(0, len(geo), n_rays)
    nrm = rng.normal(size=(n_rays, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    rad = np.sqrt(geo["radius_sq"][pick])[:, None] * rng.choice([0.5, 1.0 - 1e-3, 1.0 + 1e-3, 1.5, 3.0], size=(n_rays, 1))
    p = (geo["position"][pick] + nrm * rad).astype(f32).T
    d = rng.normal(size=(n_rays, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32).T
    d[0, :5] = 0.0
    q = n_rays // 4
    d[:, :q] *= rng.choice(np.array([0.9, 0.999, 1.00001, 1.00004, 1.0002, 1.002, 1.06, 1.125, 1.5], dtype=f32), size=q)[None, :]
    P = np.ascontiguousarray(np.concatenate([cp, p], axis=1)); D = np.ascontiguousarray(np.concatenate([cd, d], axis=1))
    return P, D, prims


_reference_cache = {}


def trace_reference(mirt, scene_name):
    if scene_name not in _reference_cache:
        make, n_rays = TRACE_SCENES[scene_name]
        sc = make(mirt)
        P, D, prims = ray_mix(sc, n_rays)
        centre, r2 = prims["position"].astype(f64), prims["radius_sq"].astype(f64)
        P64, D64 = P.T.astype(f64), D.T.astype(f64)
        ref = df.closest_hit(P64, D64, centre, r2)
        rng = np.random.default_rng(11)
        tmax = np.where(np.isfinite(ref["t"]), ref["t"] * rng.uniform(0.5, 1.5, len(P64)), 10.0).astype(f32)
        occ, occ_unsure = df.occluded(P64, D64, tmax.astype(f64), centre, r2)
        _reference_cache[scene_name] = (sc, P, D, P64, D64, centre, r2, ref, tmax, occ, occ_unsure)
    return _reference_cache[scene_name]


def check_intersection(be, mirt, scene_name):
    """Closest hit and any-hit against the float64 nearest non-negative root over all spheres (definitions.closest_hit states the acceptance
    rule in words).  (1) hit / miss equal, (2) sphere equal, (3) |t - t64| within the per-ray bound derived in
    definitions.sphere_error_model.  Set aside: rays on which some sphere's own status is within its derived error of flipping (1), and rays
    with a second root within the summed bounds of the nearest (2) - those must still report one of the rivals, at that rival's float64
    distance.  Together <= 0.5 % per scene.

    Measured on the oracle (brute force and the twin BVH alike), 36 384 rays a scene: set aside default9 0.005 %, S8a 0.055 %, S1000a 0.21 %,
    awkward 0.21 % (shadow rays 0.05 / 0.20 / 0.07 / 0.23 %); largest |t - t64| / bound 0.27 (awkward); wrong class / sphere / distance among
    the rest: 0.  S1000a shows two sphere disagreements in all (rays 10485 and 15247 of the mix: binary32 reports a grazing hit on a small
    sphere at t = 50.0 / 70.9 where float64 has the ray pass it and reach t = 74.2 / 72.4).  Both are explained by the derived error - the
    small sphere's own discriminant lies inside E_disc - and are set aside under (1), not tolerated by a flat bound."""
    sc, P, D, P64, D64, centre, r2, ref, tmax, occ, occ_unsure = trace_reference(mirt, scene_name)
    n = len(P64)
    has_rival = np.array([r is not None for r in ref["rivals"]])
    aside = ref["unsure"] | has_rival
    assert aside.mean() <= EXCLUDED_CAP, f"{scene_name}: {aside.mean():.4%} of the rays set aside"
    assert occ_unsure.mean() <= EXCLUDED_CAP, f"{scene_name}: {occ_unsure.mean():.4%} of the shadow rays set aside"
    clean = ~aside
    want_hit = ref["prim"] >= 0
    assert want_hit.mean() > 0.2 and (~want_hit).sum() > 100
    for label, closest, shadow in be.tracers(sc):
        t32, id32 = closest(P, D)
        t32 = t32.astype(f64)
        what = f"{be.name}/{label}/{scene_name}"
        wrong_class = clean & ((id32 >= 0) != want_hit)
        assert not wrong_class.any(), f"{what}: hit/miss differs on {wrong_class.sum()} rays, first {np.flatnonzero(wrong_class)[:5]}"
        wrong_prim = clean & (id32 != ref["prim"])
        assert not wrong_prim.any(), f"{what}: sphere differs on {wrong_prim.sum()} rays, first {np.flatnonzero(wrong_prim)[:5]}"
        k = clean & want_hit
        ratio = np.abs(t32[k] - ref["t"][k]) / ref["E"][k]
        assert ratio.max() <= 1.0, f"{what}: |t - t64| is {ratio.max():.3g} x the derived bound"
        # rays with rivals (and no doubtful sphere): one of the rivals, at its own float64 distance
        rv = np.flatnonzero(has_rival & ~ref["unsure"])
        for i in rv:
            allowed = set(ref["rivals"][i].tolist()) | {int(ref["prim"][i])}
            assert int(id32[i]) in allowed, f"{what}: ray {i} reports sphere {id32[i]}, candidates {sorted(allowed)}"
        if len(rv):
            near, far, E = df.root_of(P64[rv], D64[rv], centre, r2, id32[rv])
            t64 = np.where(near >= -E, np.maximum(near, 0.0), far)
            assert (np.minimum(np.abs(t32[rv] - t64), np.abs(t32[rv] - far)) <= E).all(), f"{what}: a rival's distance is off"
        got_occ = shadow(P, D, tmax).astype(bool)
        bad = ~occ_unsure & (got_occ != occ)
        assert not bad.any(), f"{what}: occlusion differs on {bad.sum()} rays, first {np.flatnonzero(bad)[:5]}"
        report(what, rays=n, set_aside=float(aside.mean()), shadow_set_aside=float(occ_unsure.mean()), worst_t_over_bound=float(ratio.max()),
               occluded=float(occ.mean()))


@pytest.mark.parametrize("scene_name", list(TRACE_SCENES))
def test_intersection(be, mirt, scene_name):
    check_intersection(be, mirt, scene_name)


# ---- B. sampling and frames -----------------------------------------------------------------------------------------------------
def check_hemisphere(be, mirt):
    """hemisphere(t, s): unit, z >= 0, z^2 = 1 - t (found from the outputs: t is the squared radius of Malley's disk, not the squared
    cosine), azimuth 2 pi s, cosine-weighted - chi-square on a 16 x 16 grid of equal-probability cells in (z^2, phi), 20 000 inputs from the
    project's own PCG, critical value 377.08 (p = 1e-6, 255 degrees of freedom).
    Measured on the oracle: chi-square 208.8; |len - 1| <= 1.3e-7; x, y within 5.9e-7 of sqrt(t) cos / sin(2 pi s)."""
    n = 20000
    r = pcg(mirt, 2024, 2 * n)
    t = np.concatenate([r[0::2], f32([0.0, 1.0, 1.0, 0.5])]); s = np.concatenate([r[1::2], f32([0.0, 1.0, 0.25, 1.0])])
    out = be.hemisphere(t, s).astype(f64)
    t64, s64 = t.astype(f64), s.astype(f64)
    length = np.linalg.norm(out, axis=1)
    assert np.abs(length - 1.0).max() <= UNIT_ABS
    assert (out[:, 2] >= 0.0).all()
    z2 = out[:, 2] ** 2
    fit_cos, fit_sin = np.abs(z2 - (1.0 - t64)).max(), np.abs(z2 - t64).max()
    assert fit_cos <= 4 * u and fit_sin > 0.5, (fit_cos, fit_sin)             # named: z^2 = 1 - t
    rho = np.sqrt(t64)
    ex = np.abs(out[:, 0] - rho * np.cos(2 * np.pi * s64)).max(); ey = np.abs(out[:, 1] - rho * np.sin(2 * np.pi * s64)).max()
    assert max(ex, ey) <= AZIMUTH_ABS, (ex, ey)
    o = out[:n]
    i = np.minimum((16 * o[:, 2] ** 2).astype(int), 15)
    j = np.minimum((16 * (np.arctan2(o[:, 1], o[:, 0]) % (2 * np.pi)) / (2 * np.pi)).astype(int), 15)
    counts = np.bincount(i * 16 + j, minlength=256).astype(f64)
    chi2 = float(((counts - n / 256.0) ** 2 / (n / 256.0)).sum())
    report(f"{be.name}/hemisphere", chi2=chi2, unit=float(np.abs(length - 1).max()), azimuth=float(max(ex, ey)))
    assert chi2 < df.CHI2_255_P1E6, chi2


def test_hemisphere(be, mirt):
    check_hemisphere(be, mirt)


SMALL_ANGLE = 0.00068523              # sin^2(theta_max) below which the sampler switches to its small-angle form


def check_sample_sphere(be, mirt):
    """sample_direction_to_sphere: of the five outputs the LAST is the pdf (the only column that tracks 1 / (2 pi (1 - cos theta_max)));
    the first three are a unit direction inside the cone about Wc.  pdf bound, derived: cos = sqrt(fl(1 - sin^2)) carries <= u absolute
    (half an ulp of a value in [1/2, 1] through a sqrt of slope <= 0.71, plus the sqrt's own half ulp), 1 - cos is then exact or one more
    rounding, so the relative error is <= 2u / (1 - cos theta_max) + 4u.  Below sin^2 ~ 2e-6 the floor D4 takes over.
    Measured on the oracle, pdf relative error: small-angle side (sin^2 in [1e-5, 0.000685)) max 8.6e-3 at sin^2 = 1.0e-5, where the bound
    is 2.4e-2; just below / above the switch 1.3e-4 / 1.3e-4 (bound 3.5e-4); larger angles <= 5.1e-5; error / bound <= 0.40 throughout.
    Direction: |len - 1| <= 2.7e-7; angle beyond the cone <= 7.3e-8 rad; large-angle branch cos(theta) within 2.5e-7 of 1 - t (1 - cos theta_max)."""
    n = 20000
    rng = np.random.default_rng(17)
    Wc = unit_f32(rng.normal(size=(n, 3)))
    Wc[:3] = [(0, 0, 1), (0, 0, -1), (1, 0, 0)]
    dist = rng.uniform(0.2, 50, n).astype(f32)
    sin2 = rng.uniform(0.001, 0.9, n).astype(f32)
    q = n // 4
    sin2[:q] = np.exp(rng.uniform(np.log(1e-5), np.log(SMALL_ANGLE), q)).astype(f32)
    sin2[q:q + 2000] = (SMALL_ANGLE * (1.0 + rng.uniform(-1e-3, 1e-3, 2000))).astype(f32)
    th = f32(SMALL_ANGLE)
    sin2[q:q + 3] = [np.nextafter(th, f32(0)), th, np.nextafter(th, f32(1))]
    r2 = (sin2 * (dist * dist)).astype(f32)
    r = pcg(mirt, 77, 2 * n); t, s = r[0::2].copy(), r[1::2].copy()
    out = be.sample_sphere(Wc, sin2, dist, r2, t, s).astype(f64)
    s2 = sin2.astype(f64)
    pdf64, omc = df.cone_pdf(s2)
    tracks = [float(np.median(np.abs(out[:, k] / pdf64 - 1.0))) < 1e-2 for k in range(5)]
    assert tracks == [False, False, False, False, True], tracks                 # named: out[4] is the pdf, out[3] the distance
    rel = np.abs(out[:, 4] / pdf64 - 1.0)
    bound = 2 * u / omc + 4 * u
    assert (rel <= bound).all(), f"pdf off by {(rel / bound).max():.3g} x the derived bound"
    small = sin2 < th
    L = out[:, :3]; W = Wc.astype(f64)
    length = np.linalg.norm(L, axis=1)
    assert np.abs(length - 1.0).max() <= UNIT_ABS
    angle = np.arctan2(np.linalg.norm(np.cross(L, W), axis=1), (L * W).sum(axis=1))
    beyond = angle - np.arcsin(np.sqrt(s2))
    assert beyond.max() <= CONE_ANGLE_ABS, beyond.max()
    cos_want = 1.0 - t.astype(f64) * omc
    cos_err = np.abs(np.cos(angle) * 1.0 - cos_want)[~small]
    assert cos_err.max() <= CONE_ANGLE_ABS, cos_err.max()                       # uniform in the cone's solid angle: cos(theta) linear in t
    # D4: the floor
    tiny = np.full(4, 1e-7, dtype=f32)
    o4 = be.sample_sphere(Wc[:4], tiny, dist[:4], tiny * dist[:4] ** 2, t[:4], s[:4]).astype(f64)
    assert np.abs(o4[:, 4] * (2 * np.pi * 1e-6) - 1.0).max() <= 8 * u
    edge = (np.abs(s2 / SMALL_ANGLE - 1.0) < 2e-3)
    report(f"{be.name}/sample_sphere", pdf_rel_small=float(rel[small].max()), at_sin2=float(s2[small][rel[small].argmax()]),
           pdf_rel_below_switch=float(rel[edge & small].max()), pdf_rel_above_switch=float(rel[edge & ~small].max()), pdf_rel_large=float(rel[~small & ~edge].max()),
           worst_over_bound=float((rel / bound).max()), unit=float(np.abs(length - 1).max()), beyond_cone=float(beyond.max()), cos_err=float(cos_err.max()))


def test_sample_direction_to_sphere(be, mirt):
    check_sample_sphere(be, mirt)


def check_frame(be, mirt):
    """tangent_space / to_local / to_world for 20 000 normals, among them (0, 0, +-1) and 4 000 with N.z -> -1.  The quaternion is rebuilt as
    a 3 x 3 in float64.  A REFERENCE PROPERTY, not a bug: the shortest-arc formula never normalises, so for an input of length |N| != 1 it
    has |q|^2 - 1 = (|N|^2 - 1) / (2 (1 + N.z)) exactly, the matrix is |q|^2 times a rotation, and both its defect from orthonormality
    max|R^T R - I| and |R e_z - N| are bounded by B = 2k + k^2, k = | |N|^2 - 1 | / (2 (1 + N.z)) (+ 24u (1 + B)^2 of rounding).  Binary32-normalised
    normals have | |N|^2 - 1 | ~ 1e-7, so the defect grows like 1e-7 / (1 + N.z) towards the pole; below N.z = -1 + 2^-23 the frame of
    (0, 0, -1) is returned outright.  to_world / to_local agree with R v / R^T v within (that bound + 32u) |v|.
    Measured on the oracle, largest defect by 1 + N.z: [1e-7, 1e-6) 2.5, [1e-6, 1e-5) 0.22, [1e-5, 1e-4) 2.0e-2, [1e-4, 1e-3) 2.1e-3,
    [1e-3, 1e-2) 2.0e-4, [1e-2, 0.1) 2.2e-5, [0.1, 2] 2.1e-6; defect / bound <= 1.00 (the bound is the exact algebra, so it is met tightly)."""
    n = 20000
    rng = np.random.default_rng(23)
    eps = np.exp(rng.uniform(np.log(3e-4), np.log(0.3), 4000)); phi = rng.uniform(0, 2 * np.pi, 4000)
    near_pole = np.stack([np.sin(eps) * np.cos(phi), np.sin(eps) * np.sin(phi), -np.cos(eps)], axis=1)
    N = unit_f32(np.concatenate([rng.normal(size=(n - 4000 - 4, 3)), near_pole, [(0, 0, 1), (0, 0, -1), (1e-4, 0, -1), (0, -3e-4, -1)]]))
    v = rng.normal(size=(n, 3)).astype(f32)
    q, l, w = (a.astype(f64) for a in be.frame(N, v))
    N64, v64 = N.astype(f64), v.astype(f64)
    pole = N[:, 2] < f32(-1.0) + f32(2.0 ** -23)
    assert pole.sum() >= 1 and (q[pole] == [0.0, 1.0, 0.0, 0.0]).all()          # named: the pole branch
    k = ~pole
    R = df.rotation_of_quaternion(q[k])
    defect = np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max(axis=(1, 2))
    bound = df.frame_defect_bound(N64[k])
    bound = bound + FRAME_ROUNDING * (1.0 + bound) ** 2                         # the roundings are relative to |q|^4
    assert (defect <= bound).all(), f"defect is {(defect / bound).max():.3g} x the derived bound"
    to_n = np.abs(R[:, :, 2] - N64[k]).max(axis=1)
    assert (to_n <= bound).all(), f"R e_z misses N by {(to_n / bound).max():.3g} x the derived bound"
    vb = (bound + 32 * u) * np.linalg.norm(v64[k], axis=1)
    assert (np.abs(w[k] - np.einsum("nij,nj->ni", R, v64[k])).max(axis=1) <= vb).all()
    assert (np.abs(l[k] - np.einsum("nji,nj->ni", R, v64[k])).max(axis=1) <= vb).all()
    one_plus = 1.0 + N64[k][:, 2]
    edges = [1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 0.1, 2.01]
    table = {f"[{a:g},{b:g})": float(defect[(one_plus >= a) & (one_plus < b)].max()) for a, b in zip(edges, edges[1:]) if ((one_plus >= a) & (one_plus < b)).any()}
    report(f"{be.name}/frame", worst_over_bound=float((defect / bound).max()), **table)
    assert len(table) >= 6                                                       # the sweep reaches the pole


def test_tangent_frame(be, mirt):
    check_frame(be, mirt)


# ---- C. GGX ---------------------------------------------------------------------------------------------------------------------
def upper_dirs(rng, n, z_min=1e-3):
    z = np.exp(rng.uniform(np.log(z_min), 0.0, n)); phi = rng.uniform(0, 2 * np.pi, n)
    rho = np.sqrt(1.0 - z * z)
    return unit_f32(np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1))


def check_ggx_eval(be, mirt):
    """Closure<GGX>::eval = F D G2 cos_L / (4 cos_L cos_V) with Schlick's F, the GGX D and the HEIGHT-CORRELATED Smith G2 (the variant
    Sampling.hpp:287-291 uses, written here from Heitz 2014 eq. 99 with Lambda, not from its Lagarde form), alpha from 1e-4 to 1, V and L
    down to cos = 1e-3.  D3 (D's alpha^2 floored at 1e-5) is a named argument of the definition.  Bound per sample, derived at GGX_EVAL_K:
    24u / k + 64u with k = 1 + (alpha^2 - 1) cos^2(theta_h) from float64.
    Measured on the oracle: error / bound <= 0.33; away from the cancellation (k > 0.1) the relative error is <= 3.5e-6."""
    n = 6000
    rng = np.random.default_rng(31)
    F0 = rng.uniform(0.02, 1.0, (n, 3)).astype(f32)
    alpha = np.exp(rng.uniform(np.log(1e-4), 0.0, n)).astype(f32)
    alpha[:8] = [1e-4, 1e-3, 1e-2, 0.1, 0.3, 1.0, 3.2e-3, 0.5]
    L, V = upper_dirs(rng, n), upper_dirs(rng, n)
    L[: n // 4] = unit_f32(V[: n // 4] * f32([-1, -1, 1]) + rng.normal(size=(n // 4, 3)).astype(f32) * alpha[: n // 4, None])   # near the mirror direction: the lobe
    L[:, 2] = np.abs(L[:, 2])
    got = be.ggx_eval(F0, alpha, L, V).astype(f64)
    want, k = df.ggx_eval_cos(F0.astype(f64), alpha.astype(f64), L.astype(f64), V.astype(f64))
    assert np.isfinite(got).all() and (got >= 0).all() and want.max() > 10.0
    rel = np.abs(got - want).max(axis=1) / np.maximum(want.max(axis=1), 1e-300)
    bound = GGX_EVAL_K / k + GGX_EVAL_REL
    sig = want.max(axis=1) > 1e-30
    assert (rel[sig] <= bound[sig]).all(), f"eval off by {(rel[sig] / bound[sig]).max():.3g} x the derived bound"
    report(f"{be.name}/ggx_eval", worst_over_bound=float((rel[sig] / bound[sig]).max()), rel_where_k_large=float(rel[sig & (k > 0.1)].max()), smallest_k=float(k.min()))


def check_ggx_sample(be, mirt):
    """Closure<GGX>::sample: the direction is the reflection of V about a visible normal - the half vector rebuilt from (V, L) lies in the
    upper hemisphere and faces V - and the estimator is F G2 / G1(V) (Heitz 2018 eq. 19, height-correlated G2), 0 below the surface.
    alpha = 0 is the mirror about the normal with weight F(cos_V).  Bound: 64u relative (measured 1.0e-6 on the oracle where H.V > 0.1, x 3.7)
    + 10u / (H.V) for the conditioning of F on the binary32 direction (derived at GGX_HV_COND) + 1e-7 absolute.
    Measured on the oracle: error / bound <= 0.14; 15 % of the samples (grazing V down to cos = 1e-3) leave below the surface with weight 0."""
    n = 6000
    rng = np.random.default_rng(37)
    F0 = rng.uniform(0.02, 1.0, (n, 3)).astype(f32)
    alpha = np.exp(rng.uniform(np.log(1e-4), 0.0, n)).astype(f32)
    alpha[:6] = [1e-4, 1e-3, 1e-2, 0.1, 1.0, 0.0]
    V = upper_dirs(rng, n)
    V[:2] = [(0, 0, 1), (0.6, 0.0, 0.8)]
    r = pcg(mirt, 99, 2 * n); u0, u1 = r[0::2].copy(), r[1::2].copy()
    d, e = (a.astype(f64) for a in be.ggx_sample(F0, alpha, V, u0, u1))
    V64, a64 = V.astype(f64), alpha.astype(f64)
    mirror = alpha == 0
    assert (d[mirror] == V64[mirror] * [-1, -1, 1]).all()
    assert np.abs(e[mirror] - df.schlick(F0[mirror].astype(f64), V64[mirror][:, 2])).max() <= 16 * u
    k = ~mirror
    assert np.abs(np.linalg.norm(d[k], axis=1) - 1.0).max() <= 16 * u
    want, H, weight, hv = df.ggx_vndf_weight(F0[k].astype(f64), a64[k], d[k], V64[k])
    assert (H[:, 2] >= -GGX_UPPER_ABS).all() and ((H * V64[k]).sum(axis=1) >= -GGX_UPPER_ABS).all()
    err = np.abs(e[k] - want).max(axis=1)
    tol = GGX_WEIGHT_REL * want.max(axis=1) + GGX_HV_COND / np.maximum(hv, 1e-30) * weight + 1e-7
    assert (err <= tol).all(), f"estimator off by {(err / tol).max():.3g} x the bound"
    assert (d[k][:, 2] > 0).mean() > 0.5 and ((e[k] == 0).all(axis=1) == (d[k][:, 2] <= 0)).all()
    well = (hv > 0.1) & (want.max(axis=1) > 1e-3)
    report(f"{be.name}/ggx_sample", worst_over_bound=float((err / tol).max()), rel_where_hv_large=float((err[well] / want.max(axis=1)[well]).max()), below_surface=float((d[k][:, 2] <= 0).mean()))


ENERGY_PAIRS = [(0.15, 0.9), (0.15, 0.3), (0.3, 0.9), (0.3, 0.3), (0.6, 0.9), (0.6, 0.2), (1.0, 0.9), (1.0, 0.3)]       # (alpha, cos_V)


def check_ggx_energy(be, mirt):
    """For F0 = 1 the hemispherical integral of eval (which carries the cosine) is the directional albedo of single scattering, <= 1.
    Midpoint quadrature on 96 x 192 cells in (theta, phi) of the backend's eval; the quadrature error is taken as twice the change of the
    float64 definition's integral between this grid and the 192 x 384 one, + 1e-4.
    Measured on the oracle: integrals 0.33 (alpha 1, cos 0.9) ... 0.97 (alpha 0.15, cos 0.9), each within 1e-5 relative of the definition's on the same grid."""
    d1, w1 = df.hemisphere_grid(96, 192)
    d2, w2 = df.hemisphere_grid(192, 384)
    worst = {}
    for alpha, cv in ENERGY_PAIRS:
        V = np.array([math.sqrt(1 - cv * cv), 0.0, cv])
        one = np.ones((len(d1), 3))
        got = be.ggx_eval(one, np.full(len(d1), alpha), d1, np.tile(V, (len(d1), 1))).astype(f64)[:, 0]
        q_got = float((got * w1).sum())
        q1 = float((df.ggx_eval_cos(one, np.full(len(d1), alpha), d1, np.tile(V, (len(d1), 1)))[0][:, 0] * w1).sum())
        q2 = float((df.ggx_eval_cos(np.ones((len(d2), 3)), np.full(len(d2), alpha), d2, np.tile(V, (len(d2), 1)))[0][:, 0] * w2).sum())
        quad_err = 2 * abs(q1 - q2) + 1e-4
        assert q_got <= 1.0 + quad_err, (alpha, cv, q_got)
        assert abs(q_got - q1) <= 1e-5 * q1, (alpha, cv, q_got, q1)               # binary32 inputs of the grid + the eval bound, summed
        assert q2 > 0.3
        worst[f"a{alpha}_c{cv}"] = q_got
    report(f"{be.name}/ggx_energy", **worst)


def test_ggx_eval(be, mirt):
    check_ggx_eval(be, mirt)


def test_ggx_sample(be, mirt):
    check_ggx_sample(be, mirt)


def test_ggx_energy(be, mirt):
    check_ggx_energy(be, mirt)


# ---- C, the distribution of the sampled normal (D7) -------------------------------------------------------------------------------
# (alpha, cos V, azimuth of V in degrees).  psi = -(azimuth + 90 degrees) is the angle by which the reference turns Heitz's disk axes about
# the stretched V (definitions.ggx_visible_normal): 0 at -90 (V.x = 0, V.y < 0), 180 degrees at +90 (V.x = 0, V.y > 0), V.x != 0 elsewhere.
VN_PAIRS = [(0.05, 0.9, 0.0), (0.05, 0.3, 30.0), (0.3, 0.9, 0.0), (0.3, 0.5, 200.0), (0.3, 0.1, 45.0), (1.0, 0.7, 0.0), (1.0, 0.2, 120.0),
            (0.3, 0.3, -90.0), (1.0, 0.3, 90.0)]
VN_TEXTBOOK = [(0.3, 0.9, 0.0), (1.0, 0.3, 60.0), (0.05, 0.2, 200.0), (0.3, 0.1, -90.0)]     # section-2 pairs: two at cos V <= 0.3
VN_N, VN_P = 20000, 1e-6                  # samples per pair; the level of the chi-square test, fixed beforehand
VN_GRID = 1024                            # (u, v) midpoints a side behind the expected bin probabilities
VN_HORIZON = 16 * u                       # a rebuilt half vector with |H.z| below this was clamped (the clamp gives H.z = 0, L.z = -V.z exactly; the backend's H is
                                          # rebuilt from a binary32 direction + V, the definition's H.z is exactly 0; unclamped mass inside the band: about 1e-6 of a cell)
_vn_cache = {}


def vn_view(cos_v, phi_deg):
    """The binary32 view direction of a pair, as float64; V.x is exactly 0 at +-90 degrees."""
    s, phi = math.sqrt(1.0 - cos_v * cos_v), math.radians(phi_deg)
    v = np.array([0.0 if abs(phi_deg) == 90.0 else s * math.cos(phi), s * math.sin(phi), cos_v]).astype(f32).astype(f64)
    return v / np.linalg.norm(v)


def vn_bin(H, edges):
    """Cell of half vectors H (n, 3): 16 rows in H.z between `edges` x 16 equal sectors of azimuth about the normal, then 16 cells by
    azimuth for the clamped mass at H.z = 0, then one cell for whatever lies below the surface (nothing does under D7)."""
    az = np.minimum((16 * (np.arctan2(H[:, 1], H[:, 0]) % (2 * np.pi)) / (2 * np.pi)).astype(int), 15)
    row = np.searchsorted(edges[1:-1], H[:, 2], side="right")
    return np.where(H[:, 2] < -VN_HORIZON, 272, np.where(H[:, 2] <= VN_HORIZON, 256 + az, 16 * row + az))


def vn_grid_probabilities(alpha, V, edges, n, axis="reference", clamp=True):
    """Probability of each of the 273 cells under the definition: the share of an n x n midpoint grid over (u, v) that lands in it."""
    key = (alpha, tuple(V), tuple(edges), n, axis, clamp)
    if key not in _vn_cache:
        counts = np.zeros(273)
        mid = (np.arange(n) + 0.5) / n
        for lo in range(0, n, 256):
            uu, vv = np.meshgrid(mid[lo:lo + 256], mid, indexing="ij")
            H = df.ggx_visible_normal(alpha, V, uu.reshape(-1), vv.reshape(-1), axis=axis, clamp=clamp)[0]
            counts += np.bincount(vn_bin(H, edges), minlength=273)
        _vn_cache[key] = counts / (n * n)
    return _vn_cache[key]


def vn_edges(alpha, V, axis="reference"):
    """Row edges in H.z: the sixteen-quantiles of the definition's own H.z above the horizon (a 256 x 256 grid), so that a narrow lobe
    (alpha = 0.05: all of it within 1e-3 of H.z = 1) is resolved as well as a wide one.  Fixed by the definition, never by a backend."""
    mid = (np.arange(256) + 0.5) / 256
    uu, vv = np.meshgrid(mid, mid, indexing="ij")
    z = df.ggx_visible_normal(alpha, V, uu.reshape(-1), vv.reshape(-1), axis=axis)[0][:, 2]
    q = np.quantile(z[z > VN_HORIZON], np.arange(1, 16) / 16.0)
    return np.concatenate([[0.0], q, [1.0]])


def vn_density_probabilities(alpha, V, edges, m):
    """The same cells under the closed-form density definitions.ggx_vndf: midpoint rule on m x m points of each cell in (polar angle, azimuth)
    with the solid angle's sine.  The horizon cells carry nothing."""
    out = np.zeros(273)
    s = (np.arange(m) + 0.5) / m
    for row in range(16):
        t0, t1 = math.acos(edges[row + 1]), math.acos(edges[row])
        theta = t0 + s * (t1 - t0)
        for col in range(16):
            phi = (col + s) * (2 * np.pi / 16)
            T, P = np.meshgrid(theta, phi, indexing="ij")
            H = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], axis=-1)
            out[16 * row + col] = (df.ggx_vndf(alpha, V, H) * np.sin(T)).mean() * (t1 - t0) * (2 * np.pi / 16)
    return out


def test_visible_normal_definition():
    """D7's definition against the textbook, no backend: with Heitz's axes and no clamp the push-forward of the uniform square through
    definitions.ggx_visible_normal is the visible-normal density G1(V) max(0, V.H) D(H) / V.z, cell by cell of the 16 x 16 grid (no mass
    below the surface).  Bound on the largest cell difference: twice the change of the grid's cell probabilities from 1024 to 2048 midpoints a
    side, plus twice the change of the density's cell integrals from 32 to 64 points a side, plus 1e-6 - and that bound is itself below 5 % of
    a cell's mean mass, so a turned axis (tens of per cent) cannot hide in it.  The reference axis is Heitz's turned by psi = -(azimuth of V
    + 90 degrees): 0 for V.x = 0 with V.y < 0, where the two agree to rounding; not 0 for V.x != 0; 180 degrees for V.x = 0 with V.y > 0
    (the warp pushes away from the normal).  The mass the clamp moves onto the horizon is reported per pair.
    Measured: largest cell difference / bound 0.16, 0.37, 0.18, 0.42 (bound 2.1e-5 ... 1.6e-4 against a mean cell mass of 3.9e-3); the
    horizon mass under D7 for VN_PAIRS, 0 ... 0.63: DESIGN.md section 2."""
    figures = {}
    for alpha, cv, phi in VN_TEXTBOOK:
        V = vn_view(cv, phi)
        edges = vn_edges(alpha, V, axis="heitz")
        p1, p2 = (vn_grid_probabilities(alpha, V, edges, n, axis="heitz", clamp=False) for n in (VN_GRID, 2 * VN_GRID))
        d1, d2 = (vn_density_probabilities(alpha, V, edges, m) for m in (32, 64))
        assert p2[256:].sum() == 0.0 and abs(d2.sum() - 1.0) <= 1e-3
        bound = 2 * np.abs(p2 - p1).max() + 2 * np.abs(d2 - d1).max() + 1e-6
        worst = float(np.abs(p2 - d2).max())
        figures[f"a{alpha}_c{cv}_p{phi:g}"] = f"{worst:.2e}/{bound:.2e}"
        assert bound <= 0.05 / 256 and worst <= bound, (alpha, cv, phi, worst, bound)
        turned = vn_grid_probabilities(alpha, V, edges, VN_GRID, axis="reference", clamp=False)
        psi = df.ggx_visible_normal(alpha, V, np.array([0.5]), np.array([0.5]))[1]
        assert abs(math.remainder(psi + math.radians(phi + 90.0), 2 * math.pi)) < 1e-6
        if V[0] == 0.0 and V[1] < 0.0:
            assert abs(psi) <= 1e-12 and np.abs(turned - p1).max() <= 1e-12
        else:
            assert abs(psi) > 0.1 and np.abs(turned - p1).max() > 10 * bound
    uv = np.random.default_rng(5).random((2, 4096))
    for alpha, cv, phi in VN_PAIRS:
        V = vn_view(cv, phi)
        Hr, psi = df.ggx_visible_normal(alpha, V, uv[0], uv[1], axis="reference", clamp=False)
        Hh = df.ggx_visible_normal(alpha, V, uv[0], uv[1], axis="heitz", clamp=False)[0]
        if V[0] == 0.0:
            assert abs(psi) <= 1e-12 if V[1] < 0 else abs(abs(psi) - np.pi) <= 1e-12
            assert (np.abs(Hr - Hh).max() <= 1e-12) == (V[1] < 0)
        else:
            assert abs(math.sin(psi)) > 0.1 and np.abs(Hr - Hh).max() > 0.01
        assert (Hh[:, 2] > 0).all()
        figures[f"horizon_a{alpha}_c{cv}_p{phi:g}"] = float(vn_grid_probabilities(alpha, V, vn_edges(alpha, V), VN_GRID)[256:].sum())
    report("definitions/visible_normal", **figures)


def vn_groups(expected):
    """Cells that expect fewer than 5 counts are pooled into one; if the pool still expects fewer than 5 it joins the smallest other cell.
    -> group index per cell, number of groups."""
    small = expected < 5.0
    order = np.flatnonzero(~small)
    group = np.full(len(expected), len(order))
    group[order] = np.arange(len(order))
    if not small.any():
        return group, len(order)
    if expected[small].sum() < 5.0:
        group[small] = group[order[np.argmin(expected[order])]]
        return group, len(order)
    return group, len(order) + 1


def vn_chi2(counts, expected):
    group, k = vn_groups(expected)
    o, e = np.bincount(group, weights=counts, minlength=k), np.bincount(group, weights=expected, minlength=k)
    return float(((o - e) ** 2 / e).sum()), k - 1


def check_ggx_sample_distribution(be, mirt):
    """Closure<GGX>::sample, how the sampled normals are DISTRIBUTED: per pair of VN_PAIRS, 20 000 inputs from the project's own PCG, the half
    vector rebuilt from (V, direction), counted on 16 rows in H.z (the sixteen-quantiles of the definition's H.z) x 16 sectors of azimuth about
    the normal, plus 16 cells by azimuth for the clamped mass at H.z = 0.  Expected cell probabilities: definitions.ggx_visible_normal with
    axis="reference" (D7) on a 1024 x 1024 midpoint grid over (u, v); cells that expect fewer than 5 counts are pooled.  Chi-square against
    the upper p = 1e-6 quantile (fixed beforehand) for the degrees of freedom left, from scipy.stats.chi2.isf where scipy is installed - it
    is where these figures were taken - and from Wilson & Hilferty otherwise (0.05 ... 0.16 % higher at these degrees of freedom: definitions.chi2_upper).
    Measured on the oracle, chi-square / threshold (degrees of freedom), in the order of VN_PAIRS: DESIGN.md section 2."""
    figures = {}
    for k, (alpha, cv, phi) in enumerate(VN_PAIRS):
        V = vn_view(cv, phi)
        r = pcg(mirt, 7000 + k, 2 * VN_N); u0, u1 = r[0::2].copy(), r[1::2].copy()
        d, e = be.ggx_sample(np.ones((VN_N, 3), dtype=f32), np.full(VN_N, alpha, dtype=f32), np.tile(V.astype(f32), (VN_N, 1)), u0, u1)
        H = d.astype(f64) + V
        H = H / np.linalg.norm(H, axis=1, keepdims=True)
        edges = vn_edges(alpha, V)
        counts = np.bincount(vn_bin(H, edges), minlength=273)
        expected = VN_N * vn_grid_probabilities(alpha, V, edges, VN_GRID)
        chi2, dof = vn_chi2(counts, expected)
        limit = df.chi2_upper(dof, VN_P)
        figures[f"a{alpha}_c{cv}_p{phi:g}"] = f"{chi2:.1f}/{limit:.1f}({dof})"
        assert dof >= 15 and chi2 < limit, (alpha, cv, phi, chi2, limit, dof)
        assert counts[272] == 0                                                     # the clamp: no half vector below the surface
        assert abs(counts[256:272].sum() - expected[256:272].sum()) <= SIGMA * math.sqrt(max(expected[256:272].sum(), 1.0))      # the horizon mass as a whole
    report(f"{be.name}/ggx_sample_distribution", **figures)


def test_ggx_sample_distribution(be, mirt):
    check_ggx_sample_distribution(be, mirt)


def test_ggx_sample_distribution_guards():
    """What makes the chi-square a test of D7, no backend: were the samples drawn with Heitz's axis (or without the clamp) while the cells
    expect D7, the statistic's noncentrality n sum (p_alt - p)^2 / p over the pooled cells is at least twice the threshold at every pair with
    V.x != 0 but the nearly symmetric ones (alpha = 0.05, or alpha = 0.3 at cos V = 0.9) - at least three are required.  At psi = 0 the axis
    cannot show, and does not.  Without the clamp the clamped mass keeps its azimuth and leaves the horizon cells for the one below the
    surface, which must stay empty: at every pair whose horizon mass expects 5 counts or more, so does that cell.
    Measured noncentrality / threshold under Heitz's axis, and the horizon mass, per pair: DESIGN.md section 2."""
    figures, told = {}, 0
    for alpha, cv, phi in VN_PAIRS:
        V = vn_view(cv, phi)
        edges = vn_edges(alpha, V)
        p = vn_grid_probabilities(alpha, V, edges, VN_GRID)
        group, k = vn_groups(VN_N * p)
        limit = df.chi2_upper(k - 1, VN_P)
        alt = vn_grid_probabilities(alpha, V, edges, VN_GRID, axis="heitz")
        e, a = np.bincount(group, weights=p, minlength=k), np.bincount(group, weights=alt, minlength=k)
        ratio = float(VN_N * ((a - e) ** 2 / e).sum() / limit)
        horizon = float(p[256:272].sum())
        figures[f"a{alpha}_c{cv}_p{phi:g}"] = f"{ratio:.1f}/{horizon:.4f}"
        assert p[272] == 0.0
        if VN_N * horizon >= 5.0:
            assert VN_N * vn_grid_probabilities(alpha, V, edges, VN_GRID, clamp=False)[272] >= 5.0
        if V[0] != 0.0:
            told += ratio >= 2.0
        elif V[1] < 0.0:
            assert ratio < 0.01 and horizon == 0.0
    report("guards/ggx_sample_distribution", told_apart=told, **figures)
    assert told >= 3


# ---- D. camera, sky, resolve ----------------------------------------------------------------------------------------------------
def turned_camera_scene(mirt):
    """default9 seen through a camera whose orientation is set as a quaternion outright (a roll as well as a turn)."""
    sc = mirt.scene.default9()
    sc.camera.focal_length = 20.0
    q = np.array([0.2, -0.5, 0.3, 0.7]); sc.camera.orient = (q / np.linalg.norm(q)).astype(f32)
    return sc


def check_raygen(be, mirt):
    """Every camera ray, projected through the float64 pinhole (conjugate of the orientation quaternion, image plane at
    z = -(height / 2) focal / 12), lands in the footprint [x, x + 1] x [y, y + 1] of the pixel that its slot stands for (tile-major slots,
    16 x 16 tiles), within 32u of the image-plane distance; it starts at the eye and looks forward.  The jitter fills the footprint: its
    mean is 1/2 within 5 sigma of a uniform variable.
    Measured on the oracle: no ray outside its footprint at all (tolerance 4.7e-4 px at 96 x 64, focal 40)."""
    worst = 0.0
    for make, w, h in ((mirt.scene.default9, 96, 64), (lambda: turned_camera_scene(mirt), 64, 96)):
        for acc in (1, 2, 77):
            sc = make()
            p, d = be.raygen(sc, w, h, acc)
            cam = sc.camera
            z = df.lens_z(h, cam.focal_length)
            assert abs(float(cam.z) - z) <= 4 * u * abs(z)
            assert (p == np.asarray(cam.pos, dtype=f32)[:, None]).all()
            d64 = d.T.astype(f64)
            assert np.abs(np.linalg.norm(d64, axis=1) - 1.0).max() <= 4 * u
            x, y, lz = df.project(d64, cam.orient, w / 2.0, h / 2.0, z)
            px, py = df.pixel_of_slot(np.arange(len(x)), w)
            assert (lz < 0).all()
            tol = PROJECT_REL * math.hypot(abs(z), w)
            out = max((px - x).max(), (x - px - 1).max(), (py - y).max(), (y - py - 1).max())
            assert out <= tol, f"{w}x{h} accumulation {acc}: a ray leaves its pixel by {out:.3g} px (tolerance {tol:.3g})"
            worst = max(worst, out)
            fx, fy = x - px, y - py
            five_sigma = SIGMA * math.sqrt(1.0 / 12.0 / len(x))
            assert abs(fx.mean() - 0.5) <= five_sigma and abs(fy.mean() - 0.5) <= five_sigma
            assert sorted(set(zip(px.tolist(), py.tolist()))) == [(a, b) for a in range(w) for b in range(h)]
    report(f"{be.name}/raygen", worst_excursion_px=float(worst))


def test_raygen(be, mirt):
    check_raygen(be, mirt)


SKY_H, SKY_W = 19, 37
CUBE_FACES = [(0, 0, 0, 1), (0, 1, 0, 0), (0, math.sqrt(0.5), 0, math.sqrt(0.5)), (0, -math.sqrt(0.5), 0, math.sqrt(0.5)),
              (math.sqrt(0.5), 0, 0, math.sqrt(0.5)), (-math.sqrt(0.5), 0, 0, math.sqrt(0.5))]      # orientations (x, y, z, w): -z, +z, -x, +x, +y, -y


def check_sky(be, mirt, variants=(0,)):
    """The sky lookup through the path: six 128 x 128 cameras with a 90 degree field (focal 12) cover the sphere as a cube map - 98 304 unit
    directions - over a 19 x 37 image whose texel (row, column) holds (row + 1, column + 1, id); one bounce, one bucket, one accumulation,
    the only sphere behind the camera, so each accumulator word is the texel its ray picked.  It must be the float64 equirect texel (D2)
    unless the direction lies within the asserted fast_atan2 / fast_asin error (2e-3 / 1e-3 rad) of a texel edge.  Cap: the solid-angle-
    weighted share of set-aside rays (a pixel of a 90 degree pinhole subtends cos^3 of its angle to the axis) <= the share of the sphere
    those bands cover for this image size, computed below, + 10 %.
    Measured on the oracle: 3.48 % set aside against a band area of 3.45 %; wrong texels outside the bands 0 (inside them 16 of 98 304)."""
    S = mirt.scene
    hdri = np.zeros((SKY_H, SKY_W, 4), dtype=f32)
    hdri[..., 0] = np.arange(1, SKY_H + 1)[:, None]; hdri[..., 1] = np.arange(1, SKY_W + 1)[None, :]
    hdri[..., 2] = (np.arange(SKY_H)[:, None] * SKY_W + np.arange(SKY_W)[None, :] + 1); hdri[..., 3] = 1.0
    w = h = 128
    bw_phi = ATAN2_ABS + 1e-4 * 2 * math.pi / (SKY_W - 1)                        # + 1e-4 texel for the binary32 scale-and-add
    bw_lat = ASIN_ABS + 1e-4 * math.pi / (SKY_H - 1)
    for variant in variants:
        n_aside = w_aside = w_all = 0.0
        wrong_inside = 0
        for q in CUBE_FACES:
            cam = S.Camera(eye=(0.0, 0.0, 0.0), direction=(0.0, 0.0, -1.0), focal_length=12.0)
            cam.orient = np.asarray(q, dtype=f32)
            fwd = df.rotation_of_quaternion(np.asarray(q, dtype=f64)[None])[0] @ np.array([0.0, 0.0, -1.0])
            geo = np.array([S._sphere(tuple(-3.0 * fwd), 0.01, 0)], dtype=S.SPHERE)
            sc = S.Scene(geo, np.array([S._material(albedo=(0.5, 0.5, 0.5))], dtype=S.MATERIAL), cam, np.ones(3, dtype=f32), hdri=hdri, name="sky_face")
            res = be.render(sc, w, h, 1, max_bounces=1, buckets=1, variant=variant)
            assert res["counters"]["terminated"] == w * h and res["counters"]["rays"] == w * h
            p, d = be.raygen(sc, w, h, 1, max_bounces=1)
            d64 = d.T.astype(f64)
            acc = res["acc"][:, 0]                                               # [tile][rgb][256]
            row = acc[:, 0].reshape(-1).astype(np.int64) - 1; col = acc[:, 1].reshape(-1).astype(np.int64) - 1
            assert (acc[:, 2].reshape(-1) == row * SKY_W + col + 1).all()        # one texel, all three channels from it
            c64, r64, ex, ey = df.equirect_texel(d64, SKY_W, SKY_H)
            phi = np.arctan2(d64[:, 2], d64[:, 0]); lat = np.arcsin(np.clip(d64[:, 1], -1, 1))
            edge_phi = (np.arange(SKY_W) / (SKY_W - 1) - 0.5) * 2 * np.pi        # ex = k
            edge_lat = (0.5 - np.arange(SKY_H) / (SKY_H - 1)) * np.pi            # ey = k
            d_phi = np.abs((phi[:, None] - edge_phi[None, :] + np.pi) % (2 * np.pi) - np.pi).min(axis=1)
            d_lat = np.abs(lat[:, None] - edge_lat[None, :]).min(axis=1)
            aside = (d_phi <= bw_phi) | (d_lat <= bw_lat)
            wrong = (row != r64) | (col != c64)
            assert not (wrong & ~aside).any(), f"variant {variant} face {q}: {int((wrong & ~aside).sum())} wrong texels away from any edge"
            assert (np.abs(row - r64) <= 1).all() and (np.minimum(np.abs(col - c64), SKY_W - 1 - np.abs(col - c64)) <= 1).all()
            local_z = np.abs(d64 @ fwd)
            weight = local_z ** 3
            n_aside += aside.sum(); w_aside += weight[aside].sum(); w_all += weight.sum(); wrong_inside += int(wrong.sum())
        share_phi = (SKY_W - 1) * 2 * bw_phi / (2 * math.pi)                     # columns 0 and W - 1 share the meridian phi = +-pi
        share_lat = sum(math.sin(min(l + bw_lat, math.pi / 2)) - math.sin(max(l - bw_lat, -math.pi / 2)) for l in edge_lat) / 2.0
        band_area = share_phi + share_lat - share_phi * share_lat                # bands in phi and in latitude are independent sets on the sphere
        report(f"{be.name}/sky/variant{variant}", set_aside=float(w_aside / w_all), band_area=float(band_area), wrong_inside_bands=wrong_inside)
        assert w_aside / w_all <= 1.1 * band_area


def test_sky_lookup(be, mirt):
    check_sky(be, mirt, variants=(0, 1))


def check_resolve(be, mirt, variants=(0,)):
    """Render() against the frame recomputed from the accumulator alone in float64: per-bucket means, np.median across the buckets,
    exposure 1.5, the published ACES fit, alpha 1; k = 3, 4, 5, 16 buckets, two accumulations per bucket.  Even k: the reference has only
    the five-input network (Sampling.hpp:13-21, k = 5 fixed); other k is this project's generalisation (Q19) and even k takes the mean of
    the two middle values, which is np.median's convention.  Bound 32u absolute on outputs in [0, 1] (derived at RESOLVE_ABS).
    Measured on the oracle: largest difference 2.7e-7 (k = 4); the mean instead of the median would move this frame by 0.71 ... 0.98."""
    for variant in variants:
        for k in (3, 4, 5, 16):
            sc = mirt.scene.synthetic(8, ambient=0.5)
            sc.camera.exposure = 1.5
            res = be.render(sc, 64, 64, 2 * k, max_bounces=4, buckets=k, variant=variant)
            want = df.resolve(res["acc"], 2 * k, 1.5, 64, 64)
            got = res["frame"].astype(f64)
            err = np.abs(got - want).max()
            assert err <= RESOLVE_ABS, f"k={k}: frame differs from the float64 resolve by {err:.3g}"
            assert (got[..., 3] == 1.0).all()
            mean_rgb = df.aces_fitted(np.moveaxis(res["acc"].astype(f64).sum(axis=1) / (2 * k) * 1.5, 1, 2).reshape(-1, 3))
            x, y = df.pixel_of_slot(np.arange(len(mean_rgb)), 64)
            by_mean = np.abs(want[y, x, :3] - mean_rgb).max()
            assert by_mean > 0.05                                                # the input tells the median from the mean
            report(f"{be.name}/resolve/variant{variant}/k{k}", err=float(err), mean_instead_of_median=float(by_mean))


def test_resolve(be, mirt):
    check_resolve(be, mirt, variants=(0,))


def one_sphere(mirt, albedo=(0.5, 0.5, 0.5), emission=(0, 0, 0), eye_z=1.25, focal=35.0, ambient=1.0, hdri=None):
    S = mirt.scene
    cam = S.Camera(eye=(0.0, 0.0, eye_z), direction=(0.0, 0.0, -1.0), focal_length=focal, exposure=1.0)
    sc = S.Scene(np.array([S._sphere((0, 0, 0), 1.0, 0)], dtype=S.SPHERE), np.array([S._material(albedo=albedo, emission=emission)], dtype=S.MATERIAL),
                 cam, np.full(3, ambient, dtype=f32), name="one_sphere")
    if hdri is not None:
        sc.hdri = np.asarray(hdri, dtype=f32)
    return sc


def footprint_depth_bounds(w, h, focal, eye_z):
    """Per pixel of a pinhole on the axis of a unit sphere: smallest and largest first-hit distance over the footprint [x, x+1] x [y, y+1].
    The distance grows with the angle to the axis, i.e. with the image-plane distance from the centre, so the extremes sit at the
    footprint's points nearest to and farthest from the centre.  -> lo, hi (h, w); hi = inf where the footprint leaves the silhouette."""
    z = df.lens_z(h, focal)
    xs, ys = np.meshgrid(np.arange(w, dtype=f64), np.arange(h, dtype=f64))
    cx, cy = w / 2.0, h / 2.0
    nx, ny = np.clip(cx, xs, xs + 1), np.clip(cy, ys, ys + 1)
    fx, fy = np.where(np.abs(xs - cx) > np.abs(xs + 1 - cx), xs, xs + 1), np.where(np.abs(ys - cy) > np.abs(ys + 1 - cy), ys, ys + 1)
    lo = df.sphere_depth_normal(nx, ny, cx, cy, z, eye_z)[0]
    hi = df.sphere_depth_normal(fx, fy, cx, cy, z, eye_z)[0]
    return lo, hi


def footprint_root_error(be, sc, w, h, accs, max_bounces=16):
    """Per pixel, the largest part-A bound (definitions.root_of) of the distance along any of its camera rays of accumulations `accs`:
    towards the silhouette the discriminant cancels and the bound grows.  -> (h, w), and the rays per accumulation."""
    E = np.zeros((h, w)); rays = []
    c, r2 = np.zeros((1, 3)), np.ones(1)
    for acc in accs:
        p, d = be.raygen(sc, w, h, acc, max_bounces=max_bounces)
        px, py = df.pixel_of_slot(np.arange(p.shape[1]), w)
        e = df.root_of(p.T.astype(f64), d.T.astype(f64), c, r2, np.zeros(p.shape[1], dtype=np.int64))[2]
        np.maximum.at(E, (py, px), e)
        rays.append((p, d, px, py))
    return E, rays


def check_first_hit_depth(be, mirt):
    """Camera rays of the one-sphere scene (eye (0, 0, 6), 32 x 32) traced by the backend: each sample's distance lies between the float64
    ray-sphere distances at the nearest and farthest points of its pixel's footprint, +- the part-A bound of that ray; a footprint wholly
    outside the silhouette never hits, one wholly inside always does."""
    sc = one_sphere(mirt, eye_z=6.0, focal=50.0)
    w = h = 32
    lo, hi = footprint_depth_bounds(w, h, 50.0, 6.0)
    E, rays = footprint_root_error(be, sc, w, h, (1, 2, 3))
    for p, d, px, py in rays:
        for label, closest, _ in be.tracers(sc):
            t, prim = closest(p, d)
            t = np.where(prim >= 0, t.astype(f64), np.inf)
            assert (t >= lo[py, px] - E[py, px]).all() and (t <= hi[py, px] + E[py, px]).all(), label
            assert np.isfinite(t).sum() > 50 and np.isinf(t).sum() > 50


def test_first_hit_depth(be, mirt):
    check_first_hit_depth(be, mirt)


# ---- E. whole path --------------------------------------------------------------------------------------------------------------
FILLING = [((0.6, 0.6, 0.6), "grey"), ((0.8, 0.4, 0.2), "red"), ((0.2, 0.4, 0.8), "blue")]


def check_filling_sphere(be, mirt, w, h, n_acc, variant=0):
    """Scene 1: a unit sphere fills the frame (eye (0, 0, 1.25), focal 35), unit sky, no light, 8 bounces.  Every path hits, survives the
    roulette with p = max(albedo) (Q6), leaves the convex sphere and meets the sky with throughput albedo / p - of which the miss shader
    takes the RED channel for all three (Q10).  Hence: the three channels are the same words; the mean is p * albedo.r / p = albedo.r;
    `rays` = n (1 + p) in expectation; `terminated` = n exactly; `shadow_rays` = 0 (Q12 guard).  Bounds: 5 sigma, sigma from the Bernoulli
    variance p (1 - p).
    Measured on the oracle, z of the mean = z of `rays` (each survivor is one more ray): 64 x 64 x 50: grey +2.22, red +3.02, blue +3.02;
    256 x 256 x 20: grey +0.002, red +0.90, blue +0.90 (red and blue share every random number).  z does not grow with
    the sample count, so the +3 at the small size is a draw, not a bias of the generator, make_unit_float or the roulette."""
    n = w * h * n_acc
    for albedo, label in FILLING:
        res = be.render(one_sphere(mirt, albedo=albedo), w, h, n_acc, max_bounces=8, variant=variant)
        acc = res["acc"]
        assert np.array_equal(ob.bits(acc[:, :, 0]), ob.bits(acc[:, :, 1])) and np.array_equal(ob.bits(acc[:, :, 0]), ob.bits(acc[:, :, 2]))   # Q10
        p = max(albedo)
        value = albedo[0] / p
        mean = acc[:, :, 0].astype(f64).sum() / n
        z_mean = (mean - p * value) / (value * math.sqrt(p * (1 - p) / n))
        c = res["counters"]
        z_rays = (c["rays"] - n * (1 + p)) / math.sqrt(n * p * (1 - p))
        report(f"{be.name}/filling/{w}x{h}x{n_acc}/{label}", mean=float(mean), z_mean=float(z_mean), rays=c["rays"], z_rays=float(z_rays))
        assert c["terminated"] == n and c["shadow_rays"] == 0
        assert abs(z_mean) <= SIGMA, f"{label}: mean {mean:.6f} is {z_mean:+.2f} sigma from {p * value}"
        assert abs(z_rays) <= SIGMA, f"{label}: rays {c['rays']} is {z_rays:+.2f} sigma from {n * (1 + p)}"


@pytest.mark.parametrize("w,h,n_acc", [(64, 64, 50), (256, 256, 20)])
def test_filling_sphere(be, mirt, w, h, n_acc):
    check_filling_sphere(be, mirt, w, h, n_acc)


def check_two_tone_sky(be, mirt, variant=0):
    """Scene 2: the same grey sphere (0.6), 100 accumulations, under a sky that is 1 above the horizon and 0 below: a 3 x 1 image with rows (1, 0, 0) - under
    D2 a two-row image would show its second row at y = -1 only.  A surviving path leaves along a cosine-weighted direction about the hit
    normal n; the share of those with y > 0 is (1 + n.y) / 2 (checked against quadrature here).  Per pixel the expectation is
    0.6 (1 + n.y) / 2, n averaged over the footprint on a 4 x 4 grid; the upper and the lower half of the image are each held
    to 5 sigma with the analytic variance of the three-valued sample.  Pins hemisphere + tangent frame + sky row together.
    Measured on the oracle: z = +1.6 (upper half), +1.5 (lower half); the halves' expectations are 18 sigma apart."""
    for ny in (-0.7, 0.0, 0.35, 1.0):
        nrm = np.array([0.3, ny, math.sqrt(max(0.0, 1 - 0.09 - ny * ny))]) if abs(ny) < 1 else np.array([0.0, ny, 0.0])
        assert abs(df.cosine_upper_share_quadrature(nrm) - df.cosine_upper_share(nrm[1] / np.linalg.norm(nrm))) <= 2e-3
    w = h = 64; n_acc = 100; rho, A, B = 0.6, 1.0, 0.0
    hdri = np.ones((3, 1, 4), dtype=f32); hdri[1:, :, :3] = B
    res = be.render(one_sphere(mirt, albedo=(rho, rho, rho), hdri=hdri), w, h, n_acc, max_bounces=8, variant=variant)
    sub = (np.arange(4) + 0.5) / 4
    xs = (np.arange(w)[None, :, None, None] + sub[None, None, :, None]) + np.zeros((h, 1, 1, 4))
    ys = (np.arange(h)[:, None, None, None] + sub[None, None, None, :]) + np.zeros((1, w, 4, 1))
    t, nrm = df.sphere_depth_normal(xs, ys, w / 2.0, h / 2.0, df.lens_z(h, 35.0), 1.25)
    assert np.isfinite(t).all()
    F = df.cosine_upper_share(nrm[..., 1]).mean(axis=(2, 3))
    expect = rho * (B + (A - B) * F)
    var = rho * (F * A * A + (1 - F) * B * B) - expect ** 2
    px, py = df.pixel_of_slot(np.arange(w * h), w)
    img = np.zeros((h, w)); img[py, px] = res["acc"][:, :, 0].astype(f64).sum(axis=1).reshape(-1) / n_acc
    zs = {}
    for name, rows in (("upper", slice(h // 2, h)), ("lower", slice(0, h // 2))):
        sigma = math.sqrt(var[rows].sum() / n_acc) / expect[rows].size
        zs[name] = float((img[rows].mean() - expect[rows].mean()) / sigma)
    sep = float((expect[h // 2:].mean() - expect[: h // 2].mean()) / (math.sqrt(var.sum() / n_acc) / (expect.size / 2)))
    report(f"{be.name}/two_tone", z_upper=zs["upper"], z_lower=zs["lower"], halves_apart_in_sigma=sep)
    assert abs(zs["upper"]) <= SIGMA and abs(zs["lower"]) <= SIGMA, zs
    assert sep > 2 * SIGMA                                                        # a swapped sky would fail both halves


def test_two_tone_sky(be, mirt):
    check_two_tone_sky(be, mirt)


def check_emissive_sphere(be, mirt, variant=0):
    """Scene 3: one emissive, black sphere fills the frame, MIS on, black sky.  At bounce 0 the emission is added with throughput 1 (Q9 leaves
    bounce 0 alone); the only light is the sphere just hit, so no shadow ray is cast; nothing else can contribute.  Every bucket word is
    therefore (accumulations in the bucket) x emission exactly, for 2 and for 8 bounces.  With ONE bounce the hit is on the last bounce and
    the path is dropped with its radiance (Q5): all zeros, nothing terminated."""
    em = (2.0, 0.5, 4.0)
    for mb in (2, 8):
        res = be.render(one_sphere(mirt, albedo=(0, 0, 0), emission=em, ambient=0.0), 64, 64, 10, max_bounces=mb, variant=variant)
        acc = res["acc"]
        for c in range(3):
            assert (acc[:, :, c] == f32(2 * em[c])).all(), (mb, c)
        assert res["counters"]["shadow_rays"] == 0 and res["counters"]["terminated"] == 64 * 64 * 10
    res = be.render(one_sphere(mirt, albedo=(0, 0, 0), emission=em, ambient=0.0), 64, 64, 10, max_bounces=1, variant=variant)
    assert not res["acc"].any() and res["counters"]["terminated"] == 0             # Q5


def test_emissive_sphere(be, mirt):
    check_emissive_sphere(be, mirt)


# ---- F. next-event estimation and MIS -------------------------------------------------------------------------------------------
# The unit sphere fills the frame (eye (0, 0, 1.25), focal 35, 64 x 64, black sky); every other sphere has its centre behind the eye plane
# and is seen by no camera ray (guard_first_hits).  The frame shows only the part of the sphere whose normal is within 7 degrees of +z
# (5 at the middle of an edge).  Two consequences for the placing of the lights:
#   * a light that is fully above the horizon in one row and fully below it in another must subtend less than 5 degrees from behind the
#     eye plane, i.e. be small and at least 5.7 away.  Binary32 cannot resolve such a light: its own root along the shadow ray is known
#     to about 2 d^2 u / sqrt(disc) (definitions.sphere_error_model), beyond the 1e-5 by which the reference shortens the shadow ray, and
#     the light shadows itself at random (measured on the oracle with radius 0.18 at distance 7: the image 100 and more sigma too dark,
#     `shadow_rays` within one sigma).  That is arithmetic, not definition, so the lights here are large and near: the error stays
#     below a tenth of the 1e-5 except on a rim that holds less than 1 % of the cone.  The NdotW early-out gets two cases of its own, which
#     need not lie behind the eye plane (the unit sphere hides them from the camera; guard_first_hits asserts it): BELOW, a large light under
#     the horizon of every visible point - nothing may arrive and no shadow ray may be cast - and SUNK, whose centre is below the horizon
#     (NdotW < 0) while a part of it is above: the early-out must NOT be taken.
#   * a light weighs the closure sample noticeably only when it subtends tens of degrees.
#   HIGH  radius 1.5 at (0, 1.75, 2.8): 44 degrees off the axis, half angle 37 - wholly above the horizon everywhere, the closure sample
#         carries 5 - 10 % and D5 shows in it;
#   LOW   radius 0.75 at (0, 1.8, 1.3): 80 degrees off the axis, half angle 24 - cut by the horizon in every pixel, by an amount that
#         changes with the row: the `Ll.z < 0` break, and a `shadow_rays` share strictly between 0 and 1;
#   SIDE  radius 0.434 at (-2.462, 0, 1.434): 80 degrees off the axis along -x, half angle 10 - wholly above the horizon in the left
#         half of the image and cut by it in the right half.
F_W = F_H = 64
F_EYE, F_FOCAL = 1.25, 35.0
F_RHO = (0.8, 0.4, 0.2)
F_SUB = 2                                 # sub-pixel grid of the footprint
F_QUAD = (16, 32)                         # cells of the cone quadrature (a case may ask for more); test_direct_lighting_guards holds it to the refinement condition
HIGH = ((0.0, 1.75, 2.8), 1.5, (3.0, 2.0, 1.0))
LOW = ((0.0, 1.8, 1.3), 0.75, (6.0, 8.0, 12.0))
SIDE = ((-2.462, 0.0, 1.434), 0.434, (10.0, 20.0, 40.0))   # F2's second light: another size and colour
BLOCKER = ((0.0, 0.0, 1.5), 0.12)                          # F3: between the lower rows of the visible cap and the near edge of HIGH
SUNK = ((0.0, 1.811, 0.778), 0.75, (6.0, 8.0, 12.0))       # LOW turned to 97 degrees off the axis: its CENTRE is below the horizon, a part of it above
BELOW = ((0.0, 2.53, -1.12), 1.5, (3.0, 2.0, 1.0))         # HIGH's size, 130 degrees off the axis: wholly below the horizon of every visible point
DIFFUSE = ((0.0, -0.7, 2.01), 0.75, (0.5, 1.0, 0.75))       # F5: a coloured Lambertian sphere that the cap sees and the camera does not


def lit_scene(mirt, lights, blockers=(), diffuse=(), rho=F_RHO):
    """The unit sphere (albedo rho), the lights (albedo 0), the blockers (albedo 0, no emission) and the diffuse spheres, one material each.
    Q11: the reference compares a light's index in the authoring order with the hit's index in the tree's order and skips the light sample
    when they are equal.  The scene is authored in the tree's own order, so the two agree and the comparison is the intended one
    (guard_first_hits asserts it); what Q11 does under a differing order stays pinned by parity alone."""
    S = mirt.scene
    geo, mats = [S._sphere((0, 0, 0), 1.0, 0)], [S._material(albedo=rho)]
    for c, r, Le in lights:
        geo.append(S._sphere(c, r * r, len(mats))); mats.append(S._material(emission=Le))
    for c, r in blockers:
        geo.append(S._sphere(c, r * r, len(mats))); mats.append(S._material())
    for c, r, alb in diffuse:
        geo.append(S._sphere(c, r * r, len(mats))); mats.append(S._material(albedo=alb))
    cam = S.Camera(eye=(0.0, 0.0, F_EYE), direction=(0.0, 0.0, -1.0), focal_length=F_FOCAL, exposure=1.0)
    geo, mats = np.array(geo, dtype=S.SPHERE), np.array(mats, dtype=S.MATERIAL)
    key = geo.tobytes()
    if key not in _tree_order:
        o = ob.Oracle(S.Scene(geo, mats, cam, np.zeros(3, dtype=f32), name="part_f")); _tree_order[key] = o.bvh()[1].copy(); o.close()
    return S.Scene(_tree_order[key].copy(), mats, cam, np.zeros(3, dtype=f32), name="part_f")


_tree_order, _f_cache = {}, {}


def df_lights(lights):
    return [(np.array(c, dtype=f64), float(f32(r * r)), np.array(Le, dtype=f64)) for c, r, Le in lights]


def df_blockers(blockers):
    return (np.array([c for c, r in blockers], dtype=f64).reshape(-1, 3), np.array([float(f32(r * r)) for c, r in blockers]))


def footprint_points(sub=F_SUB, cam=None):
    """First hits of the unit sphere on a sub x sub midpoint grid of every pixel's footprint: x = n, (h * w, sub * sub, 3).  `cam` = (eye_z,
    focal) is another camera on the axis (part G3), under which a footprint may leave the sphere: NaN there."""
    s = (np.arange(sub) + 0.5) / sub
    xs = (np.arange(F_W)[None, :, None, None] + s[None, None, :, None]) + np.zeros((F_H, 1, 1, sub))
    ys = (np.arange(F_H)[:, None, None, None] + s[None, None, None, :]) + np.zeros((1, F_W, sub, 1))
    eye, focal = (F_EYE, F_FOCAL) if cam is None else cam
    t, nrm = df.sphere_depth_normal(xs, ys, F_W / 2.0, F_H / 2.0, df.lens_z(F_H, focal), eye)
    assert cam is not None or np.isfinite(t).all()
    return np.where(np.isfinite(t)[..., None], nrm, np.nan).reshape(F_H * F_W, sub * sub, 3)


# name -> the scene's pieces, MIS, the cells of the cone quadrature, the accumulations (the smallest multiple of 5, from 100, at which
# test_direct_lighting_guards holds), and what the second of the three regions is
F_CASES = {
    "F1_high": dict(lights=[HIGH], n_acc=345, second="lower"),
    "F1_low": dict(lights=[LOW], n_acc=100, second="lower"),
    "F1_sunk": dict(lights=[SUNK], n_acc=135, second="lower"),
    "F1_below": dict(lights=[BELOW], n_acc=100, second="lower"),
    "F2_two_lights": dict(lights=[HIGH, SIDE], n_acc=100, second="horizon"),
    "F3_blocker": dict(lights=[HIGH], blockers=[BLOCKER], n_acc=100, second="shadowed", quad=(32, 64)),
    "F4_no_mis": dict(lights=[HIGH], n_acc=405, second="lower", mis=False),
}
F_LAMBERT = list(F_CASES)
CENTRE16 = np.zeros((F_H, F_W), dtype=bool); CENTRE16[24:40, 24:40] = True
CENTRE8 = np.zeros((F_H, F_W), dtype=bool); CENTRE8[28:36, 28:36] = True


def f_expectation(name, pixels=None, refine=1, blockers=None, **alt):
    """The float64 side of a case per pixel - E, var (k, 3), shadow (k,) - computed once a process and shared by every backend and variant.
    The mean over the sub-pixels; the variance of the mixture (mean of the second moments minus the square of the mean, which adds the
    between-sub-pixel variance).  `pixels`: flat indices (default all); `refine`: factor on the quadrature's cells; `blockers`, `alt`:
    a what-if for a guard (direct_lambert's keywords)."""
    key = (name, None if pixels is None else tuple(pixels), refine, blockers, tuple(sorted(alt.items())))
    if key in _f_cache:
        return _f_cache[key]
    case = F_CASES[name]
    n_u, n_phi = (refine * c for c in case.get("quad", F_QUAD))
    lights, blk = df_lights(case["lights"]), df_blockers(case.get("blockers", ()) if blockers is None else blockers)
    nrm = footprint_points()
    nrm = nrm if pixels is None else nrm[pixels]
    k, q = nrm.shape[:2]
    out = dict(E=np.zeros((k, 3)), var=np.zeros((k, 3)), shadow=np.zeros(k))
    for lo in range(0, k, 512):
        pts = nrm[lo:lo + 512].reshape(-1, 3)
        if case.get("mis", True):
            r = df.direct_lambert(pts, pts, F_RHO, lights, blk, n_u=n_u, n_phi=n_phi, **alt)
        else:
            r = df.direct_no_mis(pts, pts, F_RHO, lights, blk, n_u=n_u, n_phi=n_phi)
        E = r["E"].reshape(-1, q, 3).mean(axis=1)
        out["E"][lo:lo + 512] = E
        out["var"][lo:lo + 512] = r["M2"].reshape(-1, q, 3).mean(axis=1) - E * E
        out["shadow"][lo:lo + 512] = r["shadow"].reshape(-1, q).mean(axis=1)
    _f_cache[key] = out
    return out


def f_regions(name):
    """Three disjoint regions: the central 16 x 16; off it, the lower half / the pixels where SIDE's cone is cut by the horizon / the pixels
    from which the blocker takes more than a thousandth of the light; the rest."""
    second = F_CASES[name]["second"]
    if second == "lower":
        mask = np.zeros((F_H, F_W), dtype=bool); mask[: F_H // 2] = True
    elif second == "horizon":
        nrm = footprint_points()
        wc = np.array(SIDE[0])[None, None, :] - nrm * (1.0 + df.OFFSET)
        d = np.linalg.norm(wc, axis=-1)
        mask = (((wc * nrm).sum(axis=-1) / d) < SIDE[1] / d).any(axis=1).reshape(F_H, F_W)
    else:
        mask = (f_expectation(name)["E"][:, 0] < 0.999 * f_expectation(name, blockers=())["E"][:, 0]).reshape(F_H, F_W)
    mask = mask & ~CENTRE16
    return {"centre": CENTRE16, second: mask, "rest": ~CENTRE16 & ~mask}


def region_stats(exp, mask, n_acc):
    """Mean expectation and standard error of the mean over a region, per channel."""
    k = mask.reshape(-1)
    return exp["E"][k].mean(axis=0), np.sqrt(exp["var"][k].sum(axis=0) / n_acc) / k.sum()


def apart(name, region, **alt):
    """Largest distance over the channels, in standard errors of the region's mean, between a case's expectation and a what-if's."""
    e0, se = region_stats(f_expectation(name), region, F_CASES[name]["n_acc"])
    e1, _ = region_stats(f_expectation(name, **alt), region, F_CASES[name]["n_acc"])
    return float((np.abs(e1 - e0) / se).max())


def backend_image(res, n_acc):
    px, py = df.pixel_of_slot(np.arange(F_W * F_H), F_W)
    img = np.zeros((F_H, F_W, 3))
    img[py, px] = np.moveaxis(res["acc"].astype(f64).sum(axis=1), 1, 2).reshape(-1, 3) / n_acc
    return img


def guard_first_hits(be, sc, max_bounces, kept=None):
    """No camera ray sees anything but the unit sphere (float64 closest hit on the backend's own camera rays), and Q11 cannot bite.  With
    `kept` (h, w; part G3) that holds for every ray of a kept pixel - the regions are drawn from those alone - while rays of the other pixels
    may pass the limb, where they meet the black sky: some must, and none of them may be a kept pixel's."""
    p, d = be.raygen(sc, F_W, F_H, 1, max_bounces=max_bounces)
    geo = sc.geometry
    hit = df.closest_hit(p.T.astype(f64), d.T.astype(f64), geo["position"].astype(f64), geo["radius_sq"].astype(f64))
    unit = int(np.flatnonzero((geo["position"] == 0).all(axis=1))[0])
    if kept is None:
        assert (hit["prim"] == unit).all()
    else:
        px, py = df.pixel_of_slot(np.arange(p.shape[1]), F_W)
        k = kept[py, px]
        assert (hit["prim"][k] == unit).all() and not hit["unsure"][k].any()
        assert (hit["prim"][~k] == -1).sum() >= 64
    o = ob.Oracle(sc); prims = o.bvh()[1]; o.close()
    assert prims.tobytes() == np.ascontiguousarray(geo).tobytes()                   # tree order = authoring order


def check_direct(be, mirt, name, variant=0, **render_kw):
    """One case of F_CASES on a backend, max_bounces = 3: the image's mean over each of three disjoint regions, per channel, within SIGMA
    standard errors of the float64 expectation (the variance is the definition's, never the backend's); `terminated` = n exactly (a black
    light ends the path); `rays` = n (1 + p) at SIGMA Bernoulli sigma; `shadow_rays` within SIGMA of the definition's share.  A region whose
    expectation is 0 with variance 0 (F1_below) must be 0 exactly.  Measured on the oracle: DESIGN.md section 2, rows F."""
    case = F_CASES[name]
    n_acc = case["n_acc"]
    exp, regions = f_expectation(name), f_regions(name)
    sc = lit_scene(mirt, case["lights"], case.get("blockers", ()))
    guard_first_hits(be, sc, 3)
    res = be.render(sc, F_W, F_H, n_acc, max_bounces=3, variant=variant, mis=case.get("mis", True), **render_kw)
    img = backend_image(res, n_acc)
    n = F_W * F_H * n_acc
    zs = {}
    for label, mask in regions.items():
        want, se = region_stats(exp, mask, n_acc)
        got = img[mask].mean(axis=0)
        assert mask.sum() >= 64
        if not want.any() and not se.any():
            assert not got.any(), f"{name}/{label}: light where none can arrive"
            zs[label] = [0.0, 0.0, 0.0]
            continue
        assert (want > 0).all() and (se / want < 0.01).all(), (name, label, se / want)
        zs[label] = [float(v) for v in (got - want) / se]
    c = res["counters"]
    p = max(F_RHO)
    z_rays = (c["rays"] - n * (1 + p)) / math.sqrt(n * p * (1 - p))
    want_sh = n_acc * exp["shadow"].sum()
    sigma_sh = math.sqrt(n_acc * (exp["shadow"] * (1 - exp["shadow"])).sum())
    report(f"{be.name}/{name}/variant{variant}" + "".join(f"/{k}" for k in render_kw), **{f"z_{k}": "/".join(f"{v:+.2f}" for v in z) for k, z in zs.items()},
           z_rays=float(z_rays), shadow_rays=c["shadow_rays"], shadow_expected=float(want_sh), shadow_sigma=float(sigma_sh))
    for label, z in zs.items():
        assert max(abs(v) for v in z) <= SIGMA, f"{name}/{label}: {z} sigma from the expectation"
    assert c["terminated"] == n
    assert abs(z_rays) <= SIGMA, f"{name}: rays {c['rays']} is {z_rays:+.2f} sigma from {n * (1 + p)}"
    assert abs(c["shadow_rays"] - want_sh) <= SIGMA * sigma_sh, f"{name}: {c['shadow_rays']} shadow rays, expected {want_sh:.1f} +- {sigma_sh:.1f}"


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", F_LAMBERT)
def test_direct_lighting(be, mirt, name, variant):
    check_direct(be, mirt, name, variant=variant)


def test_direct_lighting_guards():
    """What makes part F a test, from the definitions alone (no backend).  Measured: DESIGN.md section 2, rows F."""
    figures = {}
    # the quadrature itself: without D5 the two weights sum to 1 and the light's form factor must come out.  The midpoint rule is exact for
    # it (cos(w.n) is linear in the rule's cos(theta) and its azimuthal part sums to zero over equal cells), D6's floor is never reached
    # (p_l^2 > 1), so what is left is rounding: 1536 terms of a few u64 each, 1e-12 taken
    pts = footprint_points().reshape(-1, 3)[:: 997]
    quad = df.direct_lambert(pts, pts, F_RHO, df_lights([HIGH]), q8=False, n_u=F_QUAD[0], n_phi=F_QUAD[1])["E"]
    figures["form_factor_rel"] = float(np.abs(quad / df.form_factor_sphere(pts, pts, F_RHO, df_lights([HIGH])[0]) - 1.0).max())
    assert figures["form_factor_rel"] <= 1e-12
    # the resolution: doubling it moves no pixel by more than a tenth of that pixel's standard error (a subsample of pixels), and - since
    # the bounds are on regional means - their mean over the subsample by no more than a tenth of the standard error of that mean
    some = np.arange(0, F_W * F_H, 61)
    for name in F_LAMBERT:
        n_acc = F_CASES[name]["n_acc"]
        a, b = f_expectation(name, pixels=some), f_expectation(name, pixels=some, refine=2)
        se = np.sqrt(a["var"] / n_acc)
        assert (np.abs(b["E"] - a["E"]) <= 0.1 * se).all(), name
        se_mean = np.sqrt(a["var"].sum(axis=0) / n_acc) / len(some)
        assert (np.abs(b["E"].mean(axis=0) - a["E"].mean(axis=0)) <= 0.1 * se_mean).all(), name
        with np.errstate(divide="ignore", invalid="ignore"):
            figures[f"refine_{name}"] = float(np.nanmax(np.where(se > 0, np.abs(b["E"] - a["E"]) / se, 0.0)))
            figures[f"refine_mean_{name}"] = float(np.nanmax(np.where(se_mean > 0, np.abs(b["E"].mean(axis=0) - a["E"].mean(axis=0)) / se_mean, 0.0)))
    # F1: D5 shows off the centre and not at it
    regs = f_regions("F1_high")
    for label in ("lower", "rest"):
        figures[f"q8_{label}"] = apart("F1_high", regs[label], q8=False)
        assert figures[f"q8_{label}"] > 2 * SIGMA
    figures["q8_centre8"] = apart("F1_high", CENTRE8, q8=False)
    assert figures["q8_centre8"] < 0.5
    # F2: the number of lights in the light sample's pdf and in the emissive hit's weight
    for what in ("n_lights_in_light_pdf", "n_lights_in_hit_weight"):
        figures[what] = apart("F2_two_lights", ~CENTRE16, **{what: 1})
        assert figures[what] > 2 * SIGMA
    # F3: the blocker is seen where it shadows, and there is a region it does not reach
    regs = f_regions("F3_blocker")
    figures["blocker"] = apart("F3_blocker", regs["shadowed"], blockers=())
    assert figures["blocker"] > 2 * SIGMA and regs["rest"].sum() >= 256
    # the horizon: LOW and SUNK are cut in every pixel by an amount that changes over the image, SUNK's centre is below the horizon of every
    # point (so NdotW < 0 there and only the comparison with sin^2 keeps the light), BELOW is wholly below, HIGH wholly above
    for name in ("F1_low", "F1_sunk"):
        sh = f_expectation(name)["shadow"]
        figures[f"{name}_share"] = f"{sh.min():.3f}..{sh.max():.3f}"
        assert 0.05 < sh.min() and sh.max() < 0.95 and sh.max() - sh.min() > 0.1
    pts = footprint_points().reshape(-1, 3)
    assert (((np.array(SUNK[0])[None, :] - pts * (1 + df.OFFSET)) * pts).sum(axis=1) < 0).all()
    below = f_expectation("F1_below")
    assert not below["E"].any() and not below["var"].any() and not below["shadow"].any()
    assert (f_expectation("F1_high")["shadow"] == 1.0).all()
    report("guards/F", **figures)


# ---- F5. several bounces against the float64 path sampler -----------------------------------------------------------------------
F5_ACC, F5_REF = 50, 200                  # accumulations of the backend; paths per pixel of the sampler (at least four times as many)
_sampler_cache = {}


def sampler_scene(lights, diffuse=()):
    spheres = [((0, 0, 0), 1.0, F_RHO, (0, 0, 0))] + [(c, r, (0, 0, 0), Le) for c, r, Le in lights] + [(c, r, alb, (0, 0, 0)) for c, r, alb in diffuse]
    return dict(centre=np.array([s[0] for s in spheres], dtype=f64), radius_sq=np.array([float(f32(s[1] * s[1])) for s in spheres]),
                albedo=np.array([s[2] for s in spheres], dtype=f64), emission=np.array([s[3] for s in spheres], dtype=f64))


def sampler_run(lights, diffuse, max_bounces, per_pixel, seed, **kw):
    """path_sampler from jittered first hits, `per_pixel` paths a pixel, fixed seed -> per-pixel mean and sample variance (h * w, 3), the
    share of dropped paths, computed once a process."""
    key = (repr(lights), repr(diffuse), max_bounces, per_pixel, seed, tuple(sorted(kw.items())))
    if key not in _sampler_cache:
        rng = np.random.default_rng(seed)
        jit = rng.random((F_H, F_W, per_pixel, 2))
        xs, ys = np.arange(F_W)[None, :, None] + jit[..., 0], np.arange(F_H)[:, None, None] + jit[..., 1]
        pts = df.sphere_depth_normal(xs, ys, F_W / 2.0, F_H / 2.0, df.lens_z(F_H, F_FOCAL), F_EYE)[1].reshape(-1, 3)
        out = df.path_sampler(sampler_scene(lights, diffuse), pts, pts, 1, max_bounces, rng, **kw)
        x = out["sum"].reshape(F_H * F_W, per_pixel, 3)
        mean = x.mean(axis=1)
        _sampler_cache[key] = dict(E=mean, var=(x * x).mean(axis=1) - mean * mean, dropped=float(out["dropped"].mean()))
    return _sampler_cache[key]


def test_path_sampler_meets_the_quadrature():
    """The sampler itself against F0, max_bounces = 3, MIS on (HIGH, LOW) and off: its regional means within SIGMA of its own standard error."""
    for name in ("F1_high", "F1_low", "F4_no_mis"):
        ref = sampler_run(F_CASES[name]["lights"], (), 3, 40, 2027, mis=F_CASES[name].get("mis", True))
        exp = f_expectation(name)
        for label, mask in f_regions(name).items():
            k = mask.reshape(-1)
            z = (ref["E"][k].mean(axis=0) - exp["E"][k].mean(axis=0)) / (np.sqrt(ref["var"][k].sum(axis=0) / 40) / k.sum())
            report(f"sampler/{name}/{label}", z="/".join(f"{v:+.2f}" for v in z))
            assert np.abs(z).max() <= SIGMA, (name, label, z)
        assert ref["dropped"] == 0.0


def check_several_bounces(be, mirt, max_bounces, variant=0):
    """F5: F1's HIGH scene plus a coloured diffuse sphere behind the eye plane, so that light reaches the visible cap by one, two and more
    diffuse bounces: `pdf_in` carried from bounce to bounce (D5), the emissive hit's weight past bounce 1, the roulette on coloured throughput
    (Q6) and, at max_bounces = 4, the drop of Q5.  Each region's mean within SIGMA sqrt(s^2 / n_backend + s^2 / n_ref) of the sampler's, s^2
    the SAMPLER's per-pixel sample variance, summed over the region; `terminated` = n - dropped against the sampler's share of dropped paths,
    SIGMA binomial sigma of both counts."""
    sc = lit_scene(mirt, [HIGH], diffuse=[DIFFUSE])
    guard_first_hits(be, sc, max_bounces)
    ref = sampler_run([HIGH], [DIFFUSE], max_bounces, F5_REF, 4242)
    res = be.render(sc, F_W, F_H, F5_ACC, max_bounces=max_bounces, variant=variant)
    img = backend_image(res, F5_ACC)
    zs = {}
    for label, mask in f_regions("F1_high").items():
        k = mask.reshape(-1)
        se = np.sqrt(ref["var"][k].sum(axis=0) * (1.0 / F5_ACC + 1.0 / F5_REF)) / k.sum()
        zs[label] = [float(v) for v in (img[mask].mean(axis=0) - ref["E"][k].mean(axis=0)) / se]
    n, q = F_W * F_H * F5_ACC, ref["dropped"]
    sigma_term = math.sqrt(n * q * (1 - q) * (1.0 + F5_ACC / F5_REF))
    z_term = (res["counters"]["terminated"] - n * (1 - q)) / sigma_term if sigma_term > 0 else float(res["counters"]["terminated"] - n)
    report(f"{be.name}/F5/bounces{max_bounces}/variant{variant}", **{f"z_{k}": "/".join(f"{v:+.2f}" for v in z) for k, z in zs.items()}, dropped_share=q, z_terminated=float(z_term))
    for label, z in zs.items():
        assert max(abs(v) for v in z) <= SIGMA, f"F5/{label}: {z} sigma from the sampler"
    assert abs(z_term) <= SIGMA, z_term


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("max_bounces", [4, 16])
def test_several_bounces(be, mirt, max_bounces, variant):
    check_several_bounces(be, mirt, max_bounces, variant=variant)


def test_several_bounces_guards():
    """From the sampler alone: at max_bounces = 4 the drop of Q5 is what is measured (the sampler without it is more than 2 SIGMA of the
    check's own standard error away in some region), and the second diffuse sphere matters (F1's one-bounce expectation is as far away)."""
    on, off = sampler_run([HIGH], [DIFFUSE], 4, F5_REF, 4242), sampler_run([HIGH], [DIFFUSE], 4, F5_REF, 4242, q5=False)
    direct = f_expectation("F1_high")
    far_q5 = far_direct = 0.0
    for label, mask in f_regions("F1_high").items():
        k = mask.reshape(-1)
        se = np.sqrt(on["var"][k].sum(axis=0) * (1.0 / F5_ACC + 1.0 / F5_REF)) / k.sum()
        far_q5 = max(far_q5, float((np.abs(off["E"][k].mean(axis=0) - on["E"][k].mean(axis=0)) / se).max()))
        far_direct = max(far_direct, float((np.abs(direct["E"][k].mean(axis=0) - on["E"][k].mean(axis=0)) / se).max()))
    report("guards/F5", q5_off_apart=far_q5, one_bounce_apart=far_direct, dropped_share=on["dropped"])
    assert on["dropped"] > 0.0 and off["dropped"] == 0.0
    assert far_q5 > 2 * SIGMA and far_direct > 2 * SIGMA


# ---- G. the GGX closure inside the path -----------------------------------------------------------------------------------------
# Part F's frame and lights with brdf = 1: the unit sphere is a GGX cap (F0 grey-ish 0.5 - 0.8, roughness 0.548 so that alpha = 0.30).  A black
# light still reflects Schlick's (1 - cos)^5 under this closure (F0 = 0, alpha = decay[bounce]), so a path that finds it is not ended there:
# at max_bounces = 2 the only thing that can happen to it is Q5.
G_F0, G_ROUGH = (0.8, 0.65, 0.5), 0.548
G_DIFFUSE_F0, G_DIFFUSE_ROUGH = (0.3, 0.9, 0.6), 0.8                   # G2: DIFFUSE's sphere as a coloured, rougher GGX surface
G_DECAY = (0.0, 0.15, 0.3, 0.45) + (0.5,) * 12                         # G2: the gloss-decay table, non-zero from bounce 1 on
G_QUAD, G_GRID = (16, 32), 24                                          # cells of the cone quadrature; (u, v) midpoints a side for the drop probability
G1_ACC = 100                                                           # smallest multiple of 5 at which test_ggx_path_guards holds (cap 1 500)
G2_ACC, G2_REF = 190, 760                                                # smallest multiple of 5 (sampler: four times as many) at which the decay guard holds
_g_cache = {}


def ggx_scene(mirt, lights, diffuse=(), cam=None, rough=G_ROUGH):
    sc = lit_scene(mirt, lights, diffuse=[(c, r, (0, 0, 0)) for c, r, _ in diffuse], rho=(0, 0, 0))
    if cam is not None:
        sc.camera = mirt.scene.Camera(eye=(0.0, 0.0, cam[0]), direction=(0.0, 0.0, -1.0), focal_length=cam[1], exposure=1.0)
    sc.material["F0"][0], sc.material["roughness"][0] = G_F0, rough
    for k, (_, _, (F0, rough)) in enumerate(diffuse):
        sc.material["F0"][1 + len(lights) + k], sc.material["roughness"][1 + len(lights) + k] = F0, rough
    return sc


def g_view(nrm, eye=F_EYE):
    """Unit directions from points of the unit sphere (x = n) back to the eye."""
    v = np.array([0.0, 0.0, eye]) - nrm
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def g1_expectation(pixels=None, refine=1, axis="reference", clamp=True, closure_pdf="zero", q5=True, cam=None, rough=G_ROUGH, sub=F_SUB):
    """G1 by quadrature, per pixel (mean over the sub-pixels, variance of the mixture): one path's contribution at max_bounces = 2 is
    C S with C the light sample's (Le f cos w / 1 drawn with density p_l, w = p_l / max(1e-6, p_l^2 + p_b^2), p_b = 0) and S = 1 unless Q5
    drops the path, which it does when the closure sample survives the roulette (probability min(1, max(F G2 / G1))) and meets a sphere.
    The two draws are independent:  E = E[C] (1 - P_drop),  M2 = E[C^2] (1 - P_drop).  E[C], E[C^2] by the cone quadrature of part F,
    P_drop and the survival probability by a midpoint grid over the (u, v) square through definitions.ggx_visible_normal.
    -> dict E, var (k, 3), shadow, survive, drop (k,)."""
    key = (None if pixels is None else tuple(pixels), refine, axis, clamp, closure_pdf, q5, cam, rough, sub)
    if key in _g_cache:
        return _g_cache[key]
    c, r2, Le = df_lights([HIGH])[0]
    nrm = footprint_points(sub=sub, cam=cam)
    nrm = nrm if pixels is None else nrm[pixels]
    assert np.isfinite(nrm).all()
    eye = F_EYE if cam is None else cam[0]
    k, q = nrm.shape[:2]
    g = G_GRID * refine
    mid = (np.arange(g) + 0.5) / g
    uu, vv = (a.reshape(-1) for a in np.meshgrid(mid, mid, indexing="ij"))
    F0 = np.array(G_F0)
    alpha = float(f32(rough)) ** 2
    out = dict(E=np.zeros((k, 3)), var=np.zeros((k, 3)), shadow=np.zeros(k), survive=np.zeros(k), drop=np.zeros(k))
    for lo in range(0, k, 1024 // (sub * sub)):
        n = nrm[lo:lo + 1024 // (sub * sub)].reshape(-1, 3)
        m = len(n)
        P, R = n * (1.0 + df.OFFSET), df.frame_about(n)
        Vl = np.einsum("nji,nj->ni", R, g_view(n, eye))
        kc, kd = ("cone", key[0], refine, cam, rough, sub, closure_pdf, lo), ("drop", key[0], refine, cam, rough, sub, axis, clamp, lo)
        if kc not in _g_cache:                                                      # the light sample: shared by the what-ifs on the bounce
            dirs, wq, dist, sin2 = df.cone_quadrature(P, c, r2, G_QUAD[0] * refine, G_QUAD[1] * refine)
            cells = dirs.shape[1]
            Ll = np.einsum("nji,ncj->nci", R, dirs).reshape(-1, 3)
            Vc = np.repeat(Vl, cells, axis=0)
            f = df.ggx_eval_cos(np.tile(F0, (m * cells, 1)), alpha, Ll, Vc)[0]
            p_l = np.repeat(df.cone_pdf(sin2)[0], cells)
            p_b = df.ggx_vndf_pdf_of_direction(alpha, Ll, Vc) if closure_pdf == "vndf" else 0.0
            C = np.where((Ll[:, 2] >= 0.0)[:, None], Le[None, :] * f * (p_l / np.maximum(1e-6, p_l * p_l + p_b * p_b))[:, None], 0.0)
            mass = (np.repeat(wq, cells) * p_l)[:, None]
            _g_cache[kc] = ((C * mass).reshape(m, cells, 3).sum(axis=1), (C * C * mass).reshape(m, cells, 3).sum(axis=1), (C.max(axis=1) > 0.0).reshape(m, cells).mean(axis=1))
        if kd not in _g_cache:                                                      # the bounce: shared by the what-ifs on the light sample
            H = df.ggx_visible_normal(alpha, Vl[:, None, :], uu[None, :], vv[None, :], axis=axis, clamp=clamp)[0]
            Vg = np.broadcast_to(Vl[:, None, :], H.shape)
            L = 2.0 * (H * Vg).sum(axis=-1, keepdims=True) * H - Vg
            L = (L / np.linalg.norm(L, axis=-1, keepdims=True)).reshape(-1, 3)
            with np.errstate(invalid="ignore", divide="ignore"):
                est = np.where((L[:, 2] > 0.0)[:, None], np.nan_to_num(df.ggx_vndf_weight(np.tile(F0, (len(L), 1)), alpha, L, Vg.reshape(-1, 3))[0]), 0.0)
            live = np.minimum(1.0, est.max(axis=1))
            Lw = np.einsum("nij,ngj->ngi", R, L.reshape(m, g * g, 3)).reshape(-1, 3)
            b, oc2, disc = df.sphere_roots(np.repeat(P, g * g, axis=0), Lw, c[None, :], np.array([r2]))
            meets = (disc[:, 0] >= 0.0) & (b[:, 0] + np.sqrt(np.maximum(disc[:, 0], 0.0)) >= 0.0)
            _g_cache[kd] = (live.reshape(m, g * g).mean(axis=1), (live * meets).reshape(m, g * g).mean(axis=1))
        (EC, M2C, shadow), (survive, drop) = _g_cache[kc], _g_cache[kd]
        drop = drop if q5 else np.zeros(m)
        E = (EC * (1.0 - drop)[:, None]).reshape(-1, q, 3).mean(axis=1)
        sl = slice(lo, lo + 1024 // (sub * sub))
        out["E"][sl] = E
        out["var"][sl] = (M2C * (1.0 - drop)[:, None]).reshape(-1, q, 3).mean(axis=1) - E * E
        out["shadow"][sl], out["survive"][sl], out["drop"][sl] = (a.reshape(-1, q).mean(axis=1) for a in (shadow, survive, drop))
    _g_cache[key] = out
    return out


def g_sampler(lights, diffuse, max_bounces, per_pixel, seed, decay=(), **kw):
    """path_sampler with the GGX closure from jittered first hits -> per-pixel mean and sample variance (h * w, 3), dropped share, shadow and
    ray counts per path; once a process."""
    key = ("g", repr(lights), repr(diffuse), max_bounces, per_pixel, seed, tuple(decay), tuple(sorted(kw.items())))
    if key not in _sampler_cache:
        rng = np.random.default_rng(seed)
        jit = rng.random((F_H, F_W, per_pixel, 2))
        xs, ys = np.arange(F_W)[None, :, None] + jit[..., 0], np.arange(F_H)[:, None, None] + jit[..., 1]
        pts = df.sphere_depth_normal(xs, ys, F_W / 2.0, F_H / 2.0, df.lens_z(F_H, F_FOCAL), F_EYE)[1].reshape(-1, 3)
        scene = sampler_scene(lights, [(c, r, (0, 0, 0)) for c, r, _ in diffuse])
        scene["F0"] = np.array([G_F0] + [(0, 0, 0)] * len(lights) + [d[2][0] for d in diffuse], dtype=f64)
        scene["roughness"] = np.array([float(f32(G_ROUGH))] + [0.0] * len(lights) + [float(f32(d[2][1])) for d in diffuse])
        out = df.path_sampler(scene, pts, pts, 1, max_bounces, rng, brdf=1, view=g_view(pts), decay=decay, **kw)
        x = out["sum"].reshape(F_H * F_W, per_pixel, 3)
        mean = x.mean(axis=1)
        _sampler_cache[key] = dict(E=mean, var=(x * x).mean(axis=1) - mean * mean, dropped=float(out["dropped"].mean()), shadow=float(out["shadow"].mean()),
                                   rays=float(out["rays"].mean()))
    return _sampler_cache[key]


def test_ggx_sampler_meets_the_quadrature():
    """G1 stated twice from the float64 map alone: path_sampler's GGX closure (40 paths a pixel, max_bounces = 2) against g1_expectation,
    regional means within SIGMA of the sampler's own standard error, its dropped share within SIGMA binomial sigma of the quadrature's."""
    ref, exp = g_sampler([HIGH], (), 2, 40, 2031), g1_expectation()
    for label, mask in f_regions("F1_high").items():
        k = mask.reshape(-1)
        z = (ref["E"][k].mean(axis=0) - exp["E"][k].mean(axis=0)) / (np.sqrt(ref["var"][k].sum(axis=0) / 40) / k.sum())
        report(f"sampler/G1/{label}", z="/".join(f"{v:+.2f}" for v in z))
        assert np.abs(z).max() <= SIGMA, (label, z)
    n = F_W * F_H * 40
    z_drop = (ref["dropped"] - exp["drop"].mean()) * n / math.sqrt(n * exp["drop"].mean() * (1 - exp["drop"].mean()))
    report("sampler/G1", dropped=ref["dropped"], expected=float(exp["drop"].mean()), z_drop=float(z_drop))
    assert abs(z_drop) <= SIGMA and ref["shadow"] == 1.0


def check_ggx_direct(be, mirt, variant=0, **render_kw):
    """G1: the GGX cap under HIGH, max_bounces = 2, brdf = 1, against g1_expectation: regional means within SIGMA standard errors (the
    definition's variance); `shadow_rays` = n exactly (HIGH is wholly above the horizon and f > 0 there); `rays` = n (1 + P_survive) and
    `terminated` = n (1 - P_drop) (a dropped path is not counted as terminated) within SIGMA of their Bernoulli sums.
    Measured on the oracle: DESIGN.md section 2, row G1."""
    exp, regions = g1_expectation(), f_regions("F1_high")
    sc = ggx_scene(mirt, [HIGH])
    guard_first_hits(be, sc, 2)
    res = be.render(sc, F_W, F_H, G1_ACC, max_bounces=2, variant=variant, brdf=1, **render_kw)
    img = backend_image(res, G1_ACC)
    n, zs = F_W * F_H * G1_ACC, {}
    for label, mask in regions.items():
        want, se = region_stats(exp, mask, G1_ACC)
        assert (want > 0).all() and (se / want < 0.01).all(), (label, se / want)
        zs[label] = [float(v) for v in (img[mask].mean(axis=0) - want) / se]
    c = res["counters"]
    z_rays = (c["rays"] - n - G1_ACC * exp["survive"].sum()) / math.sqrt(G1_ACC * (exp["survive"] * (1 - exp["survive"])).sum())
    z_term = (c["terminated"] - n + G1_ACC * exp["drop"].sum()) / math.sqrt(G1_ACC * (exp["drop"] * (1 - exp["drop"])).sum())
    report(f"{be.name}/G1/variant{variant}" + "".join(f"/{k}" for k in render_kw), **{f"z_{k}": "/".join(f"{v:+.2f}" for v in z) for k, z in zs.items()},
           z_rays=float(z_rays), z_terminated=float(z_term), shadow_rays=c["shadow_rays"])
    for label, z in zs.items():
        assert max(abs(v) for v in z) <= SIGMA, f"G1/{label}: {z} sigma from the expectation"
    assert c["shadow_rays"] == n and (exp["shadow"] == 1.0).all()
    assert abs(z_rays) <= SIGMA and abs(z_term) <= SIGMA, (z_rays, z_term)


@pytest.mark.parametrize("variant", [0, 1])
def test_ggx_direct(be, mirt, variant):
    check_ggx_direct(be, mirt, variant=variant)


def check_ggx_bounces(be, mirt, max_bounces, variant=0):
    """G2: HIGH plus DIFFUSE's sphere as a coloured GGX surface of another roughness, the gloss-decay table G_DECAY, against path_sampler's GGX
    closure with the sampler's own variance (as F5): alpha = a^2 + (1 - a^2) decay[bounce], the roulette on coloured throughput, Q5 under GGX
    (`terminated` against the sampler's dropped share).  Measured on the oracle: DESIGN.md section 2, row G2."""
    diffuse = [(DIFFUSE[0], DIFFUSE[1], (G_DIFFUSE_F0, G_DIFFUSE_ROUGH))]
    sc = ggx_scene(mirt, [HIGH], diffuse)
    guard_first_hits(be, sc, max_bounces)
    ref = g_sampler([HIGH], diffuse, max_bounces, G2_REF, 4343, decay=G_DECAY)
    res = be.render(sc, F_W, F_H, G2_ACC, max_bounces=max_bounces, variant=variant, brdf=1, gloss_decay=G_DECAY)
    img = backend_image(res, G2_ACC)
    zs = {}
    for label, mask in f_regions("F1_high").items():
        k = mask.reshape(-1)
        se = np.sqrt(ref["var"][k].sum(axis=0) * (1.0 / G2_ACC + 1.0 / G2_REF)) / k.sum()
        zs[label] = [float(v) for v in (img[mask].mean(axis=0) - ref["E"][k].mean(axis=0)) / se]
    n, q = F_W * F_H * G2_ACC, ref["dropped"]
    sigma_term = math.sqrt(n * q * (1 - q) * (1.0 + G2_ACC / G2_REF))
    z_term = (res["counters"]["terminated"] - n * (1 - q)) / sigma_term if sigma_term > 0 else float(res["counters"]["terminated"] - n)
    report(f"{be.name}/G2/bounces{max_bounces}/variant{variant}", **{f"z_{k}": "/".join(f"{v:+.2f}" for v in z) for k, z in zs.items()}, dropped_share=q, z_terminated=float(z_term))
    for label, z in zs.items():
        assert max(abs(v) for v in z) <= SIGMA, f"G2/{label}: {z} sigma from the sampler"
    assert abs(z_term) <= SIGMA, z_term


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("max_bounces", [4, 16])
def test_ggx_bounces(be, mirt, max_bounces, variant):
    check_ggx_bounces(be, mirt, max_bounces, variant=variant)


def test_ggx_path_guards():
    """What makes part G a test, from the definitions alone (no backend).  At the chosen counts each alternative lies at least 2 SIGMA from the
    D7 expectation in some region - or is stated here as one these scenes cannot tell apart under the cap of 1 500 accumulations:
      G1 (100 accumulations)  the true visible-normal pdf in the MIS weights; no Q5;
      G2 at 4 bounces (190 against 760 sampler paths; 175 / 700 gave 9.8)  no gloss-decay table;
      NOT told apart: Heitz's axis (under 0.01 SIGMA-units a root-accumulation in G1: 0.3 sigma at 1 500) and the dropped clamp (exactly 0:
      no normal is clamped at alpha = 0.30 within 7 degrees of the normal).  The frame shows only near-normal views; the axis and the clamp
      are held at function level by check_ggx_sample_distribution; G3 (test_ggx_grazing_guards) asks again from a grazing camera.
    Doubling both quadratures moves no pixel by more than 0.1 of its standard error, nor the subsample's mean by 0.1 of the mean's.
    Measured: DESIGN.md section 2, rows G."""
    figures, regs = {}, f_regions("F1_high")
    base = g1_expectation()

    def g1_apart(n_acc, **alt):
        other = g1_expectation(**alt)
        return max(float((np.abs(region_stats(other, m, n_acc)[0] - region_stats(base, m, n_acc)[0]) / region_stats(base, m, n_acc)[1]).max()) for m in regs.values())

    for label, alt in (("true_pdf", dict(closure_pdf="vndf")), ("no_q5", dict(q5=False))):
        figures[f"G1_{label}"] = g1_apart(G1_ACC, **alt)
        assert figures[f"G1_{label}"] >= 2 * SIGMA
    figures["G1_heitz_at_cap"] = g1_apart(1500, axis="heitz")
    figures["G1_no_clamp_at_cap"] = g1_apart(1500, clamp=False)
    assert figures["G1_heitz_at_cap"] < 0.5 and figures["G1_no_clamp_at_cap"] == 0.0          # stated, not hidden: these need a wider view
    some = np.arange(0, F_W * F_H, 61)
    a, b = g1_expectation(pixels=some), g1_expectation(pixels=some, refine=2)
    se = np.sqrt(a["var"] / G1_ACC)
    se_mean = np.sqrt(a["var"].sum(axis=0) / G1_ACC) / len(some)
    figures["G1_refine"] = float((np.abs(b["E"] - a["E"]) / se).max())
    figures["G1_refine_mean"] = float((np.abs(b["E"].mean(axis=0) - a["E"].mean(axis=0)) / se_mean).max())
    assert figures["G1_refine"] <= 0.1 and figures["G1_refine_mean"] <= 0.1
    assert (base["shadow"] == 1.0).all() and 0.01 < base["drop"].min() and base["drop"].max() - base["drop"].min() > 0.1 and base["survive"].max() < 0.9
    diffuse = [(DIFFUSE[0], DIFFUSE[1], (G_DIFFUSE_F0, G_DIFFUSE_ROUGH))]
    on = g_sampler([HIGH], diffuse, 4, G2_REF, 4343, decay=G_DECAY)
    for label, decay, kw in (("no_decay", (), {}), ("no_q5", G_DECAY, dict(q5=False))):
        off = g_sampler([HIGH], diffuse, 4, G2_REF, 4343, decay=decay, **kw)
        far = 0.0
        for mask in regs.values():
            k = mask.reshape(-1)
            se = np.sqrt(on["var"][k].sum(axis=0) * (1.0 / G2_ACC + 1.0 / G2_REF)) / k.sum()
            far = max(far, float((np.abs(off["E"][k].mean(axis=0) - on["E"][k].mean(axis=0)) / se).max()))
        figures[f"G2_{label}"] = far
    figures["G1_drop_share"] = f"{base['drop'].min():.3f}..{base['drop'].max():.3f}"
    report("guards/G", dropped_share_G2=on["dropped"], **figures)
    assert figures["G2_no_decay"] >= 2 * SIGMA and on["dropped"] > 0.0


# ---- G3. the grazing camera -------------------------------------------------------------------------------------------------------
# The eye at (0, 0, 3) with the same lens: the limb lies 19.5 degrees off the axis, inside the frame's corners (25.8), and the image shows
# normals out to the limb's 70.5 degrees.  Kept pixels are those whose whole footprint has normals within 60 degrees of +z; the others -
# the limb, and the black sky past it - are masked out of the regions by guard_first_hits.  V leaves the normal by up to 79 degrees there,
# at every azimuth of the local frame.
G3_CAM = (3.0, 35.0)
G3_SUB = F_SUB                                                         # sub-pixel grid of the footprint (4 x 4 moves no region's z by more than 0.03)
G3_ACC = 100                                                           # smallest multiple of 5, from 100, at which the guards that can hold do


def g3_kept():
    """-> kept (h, w) bool, the flat indices of the kept pixels, and per kept pixel the angle of its mean normal to +z and its azimuth (degrees)."""
    nrm = footprint_points(cam=G3_CAM)
    s = np.array([0.0, 1.0])
    xs, ys = np.arange(F_W)[None, :, None, None] + s[None, None, :, None], np.arange(F_H)[:, None, None, None] + s[None, None, None, :]
    t, corner = df.sphere_depth_normal(xs + np.zeros_like(ys), ys + np.zeros_like(xs), F_W / 2.0, F_H / 2.0, df.lens_z(F_H, G3_CAM[1]), G3_CAM[0])
    kept = (np.isfinite(t) & (corner[..., 2] >= 0.5)).all(axis=(2, 3))
    idx = np.flatnonzero(kept.reshape(-1))
    mean = nrm[idx].mean(axis=1)
    mean = mean / np.linalg.norm(mean, axis=1, keepdims=True)
    return kept, idx, np.degrees(np.arccos(mean[:, 2])), np.degrees(np.arctan2(mean[:, 1], mean[:, 0])) % 360.0


def g3_regions():
    """Seventeen named regions over the kept pixels: the cap within 15 degrees of the axis, and eight sectors of azimuth each of the rings of
    normals 15 - 30 and 30 - 60 degrees off it (a turned axis shows with a sign that changes round the ring, so a whole ring would cancel it)."""
    _, _, ang, az = g3_kept()
    regs = {"inner": ang < 15.0}
    for name, lo, hi in (("mid", 15.0, 30.0), ("outer", 30.0, 61.0)):
        for k in range(8):
            regs[f"{name}{k}"] = (ang >= lo) & (ang < hi) & (az >= 45.0 * k) & (az < 45.0 * k + 45.0)
    return regs


def check_ggx_grazing(be, mirt, variant=0):
    """G3: G1's scene and expectation from the farther eye - normals out to 60 degrees, V tens of degrees off the normal at every azimuth of
    the local frame, HIGH partly or wholly below the horizon of many pixels - over the kept pixels only; each of the seventeen regions within
    SIGMA standard errors.  The counters cover the masked pixels too and are not compared.  Measured on the oracle: DESIGN.md, row G3."""
    kept, idx, ang, _ = g3_kept()
    exp = g1_expectation(pixels=idx, cam=G3_CAM, sub=G3_SUB)
    sc = ggx_scene(mirt, [HIGH], cam=G3_CAM)
    guard_first_hits(be, sc, 2, kept=kept)
    res = be.render(sc, F_W, F_H, G3_ACC, max_bounces=2, variant=variant, brdf=1)
    img = backend_image(res, G3_ACC).reshape(-1, 3)[idx]
    assert ang.max() >= 30.0 and (ang >= 30.0).sum() >= 1024
    zs = {}
    for label, mask in g3_regions().items():
        want, se = region_stats(exp, mask, G3_ACC)
        assert mask.sum() >= 64 and (want > 0).all()
        zs[label] = float(((img[mask].mean(axis=0) - want) / se)[np.argmax(np.abs((img[mask].mean(axis=0) - want) / se))])
    report(f"{be.name}/G3/variant{variant}", **zs)
    assert max(abs(v) for v in zs.values()) <= SIGMA, zs


@pytest.mark.parametrize("variant", [0, 1])
def test_ggx_grazing(be, mirt, variant):
    check_ggx_grazing(be, mirt, variant=variant)


def test_ggx_grazing_guards():
    """G3 from the definitions alone.  At 100 accumulations the true visible-normal pdf in the MIS weights and the missing Q5 lie beyond 2 SIGMA
    in some region.  Heitz's axis and the dropped clamp do NOT, and not at the cap of 1 500 either - stated, with their figures, not raised:
    at max_bounces = 2 the axis reaches the image only through the probability that Q5 drops the path, which the wide light integrates over
    (largest region: the figure below, at the cap), and a normal below the surface reflects V below the surface with or without the clamp
    (weight 0 either way; the difference is exactly 0).  Inside the path these two rest on check_ggx_sample_distribution.
    Doubling both quadratures moves no kept pixel of a subsample by more than 0.1 of its standard error, nor the subsample's mean."""
    kept, idx, ang, _ = g3_kept()
    regs, base, figures = g3_regions(), g1_expectation(pixels=idx, cam=G3_CAM, sub=G3_SUB), {}

    def apart_at(n_acc, **alt):
        other = g1_expectation(pixels=idx, cam=G3_CAM, sub=G3_SUB, **alt)
        return max(float((np.abs(region_stats(other, m, n_acc)[0] - region_stats(base, m, n_acc)[0]) / region_stats(base, m, n_acc)[1]).max()) for m in regs.values())

    for label, alt in (("true_pdf", dict(closure_pdf="vndf")), ("no_q5", dict(q5=False))):
        figures[label] = apart_at(G3_ACC, **alt)
        assert figures[label] >= 2 * SIGMA
    figures["heitz_at_cap"], figures["no_clamp_at_cap"] = apart_at(1500, axis="heitz"), apart_at(1500, clamp=False)
    assert figures["heitz_at_cap"] < 2 * SIGMA and figures["no_clamp_at_cap"] == 0.0
    some = idx[::37]
    a, b = g1_expectation(pixels=some, cam=G3_CAM, sub=G3_SUB), g1_expectation(pixels=some, cam=G3_CAM, sub=G3_SUB, refine=2)
    se = np.sqrt(a["var"] / G3_ACC)
    figures["refine"] = float((np.abs(b["E"] - a["E"]) / se).max())
    figures["refine_mean"] = float((np.abs(b["E"].mean(axis=0) - a["E"].mean(axis=0)) / (np.sqrt(a["var"].sum(axis=0) / G3_ACC) / len(some))).max())
    assert figures["refine"] <= 0.1 and figures["refine_mean"] <= 0.1
    shares = base["shadow"]
    figures["shadow_share"] = f"{shares.min():.3f}..{shares.max():.3f}"
    assert shares.min() < 0.5 and shares.max() == 1.0 and ang.max() >= 55.0
    report("guards/G3", kept=len(idx), **figures)
