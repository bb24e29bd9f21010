"""One float64 path sampler for the whole per-hit text of k_shade (csrc/shade_hit_body.inc with csrc/nee_sample_body.inc), with every switch that
selects an instantiation as an argument: closure per material, light RIS, the dielectric interface, the sampled sky, the GGX closure pdf.

Each switch has a float64 statement of its own (definitions.path_sampler / g1_expectation, sky_definitions, glass_definitions.glass_ball_radiance,
ris_definitions.ris_direct); this file states what the estimator is where they MEET, from those definitions alone - plain numpy, its own generator,
textbook sampling, no device arithmetic and no stream order.  It keeps the named departures definitions.path_sampler keeps (Q5, Q6, Q8 / D5, Q9, D4,
D6), glass_definitions' G1 - G3 and Q10 (the miss shader, and the sky's light sample with it, scale all three channels by throughput.r), and adds
the composition rules, each marked `# rule:` where it is applied.  Q11 is NOT stated: a light sample skips the light that was hit, by sphere; the
scenes held to this sampler are authored in tree order, where Q11 says the same.  `mutate` names ONE deliberate error (MUTATIONS); it switches a single
expression and exists for the guards of tests/test_composed_cpu.py, which show that the GPU test would notice it.

composed_scene() is the scene both test modules render; composed_forms() the 80 forms; the fixture helpers reduce a twin run to what
tests/golden/composed_forms.npz holds."""
import itertools

import numpy as np

import definitions as df
import glass_definitions as gd
import sky_definitions as sd

f32, f64 = np.float32, np.float64
OFFSET = df.OFFSET

MUTATIONS = {
    1: "SKY: the emitter-hit heuristic takes the selection pdf 1 / n_lights",
    2: "SKY, GGX hit, pdf off: miss weight 1",
    3: "GLASS: a light sample is also taken at interface hits",
    4: "GLASS: an emitter hit after an interface is weighed by the heuristic",
    5: "GLASS + SKY: a miss after an interface is weighed by the heuristic",
    6: "MIXED, pdf off: a GGX-sampled ray carries the Lambert pdf to the next emitter",
    7: "MIXED + PDF: a Lambertian-sampled ray carries the vndf pdf of the next hit's alpha",
    8: "PDF: the light sample weighs against a pdf of 0",
    9: "RIS + SKY: the sky is never a candidate, selection still 1 / (n_lights + 1)",
    10: "RIS: the final factor omits 1 / M",
    11: "GLASS: entering does not apply transmission / tmax",
    12: "transmissive material, opaque lobe chosen: throughput divided by (1 - tmax)",
}


def _local(R, w):
    return np.einsum("nji,nj->ni", R, w)


def _world(R, v):
    return np.einsum("nij,nj->ni", R, v)


def composed_sampler(scene, rays, n_paths, max_bounces, rng, *, closures, light_ris=0, transmission=False, sky=None, ggx_pdf=False, decay=(), mutate=None):
    """scene: dict centre (k, 3), radius_sq (k,), material (k,) -> rows of albedo, emission, F0 (m, 3), roughness (m,), transmission (m, 3), ior (m,)
    (the index of refraction, 1 + IOR_minus_one); optional hdri (h, w, >= 3) and ambient (3,): the sky's colour (black without them).
    rays: (p, d), each (n, 3): every ray starts n_paths paths; its first hit is definitions.closest_hit's.  closures[material] is 0 (Lambertian) or
    1 (GGX).  light_ris: candidates of the light sample (0: the plain draw).  transmission: the dielectric interface is on.  sky: None, or
    sky_definitions.table(hdri, ambient): the environment map is light number n_lights.  ggx_pdf: a GGX hit's closure pdf is the vndf pdf, else 0.
    decay: the gloss-decay table (0 beyond its length).
    -> dict sum, sum_sq (n, 3): over the n_paths contributions of each ray; rays, shadow, terminated, dropped (n,): counts per ray, summed over
    its paths (rays counts the given ray too; a path is either terminated or dropped), rays_sq, shadow_sq (n,): sums of their squares per path."""
    centre, r2 = np.asarray(scene["centre"], dtype=f64), np.asarray(scene["radius_sq"], dtype=f64)
    material = np.asarray(scene.get("material", np.arange(len(r2))), dtype=np.int64)
    n_mat = int(material.max()) + 1
    tab = lambda key, width: np.asarray(scene[key], dtype=f64) if key in scene else (np.zeros((n_mat, width)) if width else np.zeros(n_mat))
    albedo, emission, F0, rough, trans = tab("albedo", 3), tab("emission", 3), tab("F0", 3), tab("roughness", 0), tab("transmission", 3)
    ior = np.asarray(scene["ior"], dtype=f64) if "ior" in scene else np.ones(n_mat)
    closures = np.asarray(closures, dtype=np.int64)
    has_sky = "hdri" in scene and np.any(np.asarray(scene.get("ambient", 0.0)) != 0)
    if has_sky:
        hdri, ambient = np.asarray(scene["hdri"], dtype=f64), np.asarray(scene["ambient"], dtype=f64)
        map_h, map_w = hdri.shape[:2]
    lights = np.flatnonzero((emission[material] ** 2).sum(axis=1) > 0.0)             # the emissive spheres, in array order
    n_l = len(lights)
    n_pick = n_l + 1 if sky is not None else n_l                                     # rule: the sky is light number n_lights
    sel = 1.0 / n_pick if n_pick else 0.0                                            # rule: ... and the selection probability is 1 / (n_lights + 1) in both heuristics
    sel_hit = 1.0 / n_l if (mutate == 1 and n_l) else sel
    M = max(1, int(light_ris))

    P0, D0 = np.asarray(rays[0], dtype=f64), np.asarray(rays[1], dtype=f64)
    m = len(P0)
    first = df.closest_hit(P0, D0, centre, r2)
    row = np.repeat(np.arange(m), n_paths)
    N = len(row)
    O, D = P0[row].copy(), D0[row].copy()
    thr, rad = np.ones((N, 3)), np.zeros((N, 3))
    pdf_in, miss_w, after_iface = np.zeros(N), np.ones(N), np.zeros(N, dtype=bool)
    lam_sampled, L_prev, V_prev = np.zeros(N, dtype=bool), np.zeros((N, 3)), np.zeros((N, 3))      # mutation 7 reads these
    n_rays, n_shadow, n_shadow_sq = np.zeros(N), np.zeros(N), np.zeros(N)
    terminated, dropped = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
    alive = np.arange(N)

    def nearest(p, d, skip=None):
        b, oc2, disc = df.sphere_roots(p, d, centre, r2)
        s = np.sqrt(np.maximum(disc, 0.0))
        t = np.where(b - s >= 0.0, b - s, b + s)
        t = np.where((disc >= 0.0) & (t >= 0.0), t, np.inf)
        if skip is not None:
            t[np.arange(len(p))[skip >= 0], skip[skip >= 0]] = np.inf
        k = np.argmin(t, axis=1)
        return t[np.arange(len(p)), k], k

    def sky_colour(d):
        col, rw, _, _ = df.equirect_texel(d, map_w, map_h)                           # rule: the sky's colour is ambient x the texel the miss shader would read
        return ambient[None, :] * hdri[np.clip(rw, 0, map_h - 1), np.clip(col, 0, map_w - 1), :3]

    def light_sample(P, R, Vl, prim, mat, is_ggx, alpha, thr_a):
        """One full light sample: the pick (the sky among them), the direction, the MIS-weighted radiance -> contrib (k, 3), w (k, 3), reach, skip."""
        k = len(P)
        pick = rng.integers(0, n_l if (mutate == 9 and n_l) else n_pick, k)
        u0, u1 = rng.random(k), rng.random(k)
        is_sky = pick == n_l
        lp = lights[np.minimum(pick, max(n_l - 1, 0))] if n_l else np.zeros(k, dtype=np.int64)
        w, reach, p_src, Le, ok = np.zeros((k, 3)), np.full(k, np.inf), np.ones(k), np.zeros((k, 3)), np.zeros(k, dtype=bool)
        s = np.flatnonzero(~is_sky)
        if len(s):
            wc = centre[lp[s]] - P[s]
            d2 = (wc * wc).sum(axis=1)
            ok[s] = (lp[s] != prim[s]) & (d2 > r2[lp[s]])
            d = np.sqrt(d2)
            wc = wc / d[:, None]
            pdf_c, omc = df.cone_pdf(np.minimum(r2[lp[s]] / d2, 1.0))                 # D4
            cos_t = 1.0 - u0[s] * omc
            sin_t = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
            phi = 2.0 * np.pi * u1[s]
            t_, b_ = df.basis_about(wc)
            w[s] = sin_t[:, None] * (np.cos(phi)[:, None] * t_ + np.sin(phi)[:, None] * b_) + cos_t[:, None] * wc
            reach[s] = d * cos_t - np.sqrt(np.maximum(0.0, r2[lp[s]] - (d * sin_t) ** 2))
            p_src[s], Le[s] = pdf_c, emission[material[lp[s]]]
        s = np.flatnonzero(is_sky)
        if len(s):
            dirs, rw, col, _, _ = sd.sample(sky, u0[s], u1[s])
            w[s], p_src[s], ok[s] = dirs, sky["dens"][rw, col], True
            Le[s] = sky_colour(dirs)
        Ll = _local(R, w)
        with np.errstate(invalid="ignore", divide="ignore"):
            f_ggx = np.nan_to_num(df.ggx_eval_cos(F0[mat], alpha, Ll, Vl)[0])
            p_ggx = np.nan_to_num(df.ggx_vndf_pdf_of_direction(alpha, Ll, Vl)) if (ggx_pdf and mutate != 8) else np.zeros(k)      # rule: the GGX closure pdf is 0 without the switch
        p_lam = sd.lambert_pdf(Ll[:, 2])                                             # rule: the light sample weighs against the closure's LOCAL pdf
        f = np.where(is_ggx[:, None], f_ggx, albedo[mat] * p_lam[:, None])
        p_b = np.where(is_ggx, p_ggx, p_lam)
        p_l = sel * p_src
        weight = p_l / np.maximum(1e-6, p_l * p_l + p_b * p_b)                       # D6: power_heuristic(p_l, p_b) / p_l
        carried = np.where(is_sky[:, None], (thr_a[:, 0] * f[:, 0])[:, None], thr_a * f)                                           # Q10 carried into the sky's light sample
        contrib = Le * carried * weight[:, None]
        contrib = np.where((ok & (Ll[:, 2] >= 0.0))[:, None], contrib, 0.0)
        return contrib, w, reach, np.where(is_sky, -1, lp)

    for bounce in range(max_bounces + 1):
        if len(alive) == 0:
            break
        a = alive
        n_rays[a] += 1.0
        if bounce == 0:
            t_hit, k = first["t"][row[a]], first["prim"][row[a]]
        else:
            t_hit, k = nearest(O[a], D[a])
        found = np.isfinite(t_hit)
        miss = a[~found]
        if has_sky and len(miss):
            rad[miss] += (thr[miss, 0] * miss_w[miss])[:, None] * sky_colour(D[miss])  # Q10; rule: a miss keeps miss_weight of throughput x sky
        terminated[miss] = True
        a, t_hit, k = a[found], t_hit[found], k[found]
        if bounce >= max_bounces - 1:                                                # Q5: a path that still hits on the last bounce is dropped whole
            rad[a] = 0.0
            dropped[a] = True
            break
        if len(a) == 0:
            break
        Da = D[a]
        hit = O[a] + Da * t_hit[:, None]
        nrm = (hit - centre[k]) / np.sqrt(r2[k])[:, None]
        inside = (nrm * Da).sum(axis=1) >= 0.0
        nrm = np.where(inside[:, None], -nrm, nrm)
        R = df.frame_about(nrm)
        Vl = _local(R, -Da)
        P = hit + OFFSET * nrm
        mat = material[k]
        is_ggx = closures[mat] == 1                                                  # rule: the closure is the hit material's
        a2r = rough[mat] ** 2
        alpha = a2r + (1.0 - a2r) * (decay[bounce] if bounce < len(decay) else 0.0)
        tmax = trans[mat].max(axis=1)
        iface = np.zeros(len(a), dtype=bool)
        if transmission:
            iface = (tmax > 0.0) & (inside | (rng.random(len(a)) < tmax))            # rule (G3): always from inside, with probability tmax from outside

        # ---- the light sample
        if n_pick:
            s = np.arange(len(a)) if mutate == 3 else np.flatnonzero(~iface)         # rule: no light sample at an interface hit
            if len(s):
                args = (P[s], R[s], Vl[s], k[s], mat[s], is_ggx[s], alpha[s], thr[a[s]])
                if light_ris:
                    w_sum, v_s = np.zeros(len(s)), np.zeros(len(s))
                    c_s, w_s, reach_s, skip_s = np.zeros((len(s), 3)), np.zeros((len(s), 3)), np.zeros(len(s)), np.full(len(s), -1)
                    for _ in range(M):                                               # rule: every candidate is a full light sample
                        contrib, w, reach, skip = light_sample(*args)
                        v = contrib.max(axis=1)                                      # ris_definitions: the largest channel; an early leaver weighs 0 and still counts
                        w_sum += v
                        take = (v > 0.0) & (rng.random(len(s)) * w_sum < v)
                        c_s[take], v_s[take], w_s[take], reach_s[take], skip_s[take] = contrib[take], v[take], w[take], reach[take], skip[take]
                    cast = v_s > 0.0
                    factor = w_sum / ((1.0 if mutate == 10 else float(M)) * np.where(cast, v_s, 1.0))
                    contrib, w, reach, skip = c_s * factor[:, None], w_s, reach_s, skip_s
                else:
                    contrib, w, reach, skip = light_sample(*args)
                    cast = contrib.max(axis=1) > 0.0
                c = np.flatnonzero(cast)                                             # rule: one shadow ray, to the kept candidate
                seen = ~(nearest(P[s][c], w[c], skip=skip[c])[0] < reach[c])
                rad[a[s][c]] += np.where(seen[:, None], contrib[c], 0.0)
                n_shadow[a[s][c]] += 1.0

        # ---- an emitter hit
        em = emission[mat].max(axis=1) > 0.0
        if em.any():
            e = np.flatnonzero(em)
            if bounce > 0 and n_l:
                oc = centre[k[e]] - O[a[e]]
                g = sel_hit * df.cone_pdf(np.minimum(r2[k[e]] / (oc * oc).sum(axis=1), 1.0))[0]
                p_in = pdf_in[a[e]]
                if mutate == 7:
                    with np.errstate(invalid="ignore", divide="ignore"):
                        p_in = np.where(lam_sampled[a[e]], np.nan_to_num(df.ggx_vndf_pdf_of_direction(alpha[e], L_prev[a[e]], V_prev[a[e]])), p_in)
                weight = df.power_heuristic(p_in, g)
                if mutate != 4:
                    weight = np.where(after_iface[a[e]], 1.0, weight)                # rule: the emitter hit that follows an interface weighs 1
                rad[a[e]] += thr[a[e]] * weight[:, None] * emission[mat[e]]
            else:
                rad[a[e]] += emission[mat[e]]                                        # Q9

        # ---- the closure sample
        b0, b1, s1 = rng.random(len(a)), rng.random(len(a)), rng.random(len(a))
        g_rows, l_rows, i_rows = np.flatnonzero(is_ggx & ~iface), np.flatnonzero(~is_ggx & ~iface), np.flatnonzero(iface)
        Ll, pdf_new, mw, t_new = np.zeros((len(a), 3)), np.zeros(len(a)), np.ones(len(a)), thr[a].copy()
        if len(g_rows):
            H = df.ggx_visible_normal(alpha[g_rows], Vl[g_rows], b0[g_rows], b1[g_rows])[0]
            L = 2.0 * (H * Vl[g_rows]).sum(axis=1)[:, None] * H - Vl[g_rows]
            L = L / np.linalg.norm(L, axis=1, keepdims=True)
            with np.errstate(invalid="ignore", divide="ignore"):
                est = np.where((L[:, 2] > 0.0)[:, None], np.nan_to_num(df.ggx_vndf_weight(F0[mat[g_rows]], alpha[g_rows], L, Vl[g_rows])[0]), 0.0)
                if ggx_pdf:
                    pdf_new[g_rows] = np.nan_to_num(df.ggx_vndf_pdf_of_direction(alpha[g_rows], L, Vl[g_rows]))                    # rule: from the SAMPLING hit's alpha and local view
            Ll[g_rows], t_new[g_rows] = L, t_new[g_rows] * est
        if len(l_rows):
            r_, phi = np.sqrt(b0[l_rows]), 2.0 * np.pi * b1[l_rows]                  # Malley: a uniform disk, lifted
            Ll[l_rows] = np.stack([r_ * np.cos(phi), r_ * np.sin(phi), np.sqrt(np.maximum(0.0, 1.0 - r_ * r_))], axis=1)
            t_new[l_rows] = t_new[l_rows] * albedo[mat[l_rows]]                      # rule: the opaque lobe of a transmissive material is not reweighted
            if mutate == 12 and transmission:
                glassy = tmax[l_rows] > 0.0
                t_new[l_rows] = np.where(glassy[:, None], t_new[l_rows] / np.where(glassy, 1.0 - tmax[l_rows], 1.0)[:, None], t_new[l_rows])
        refracted = np.zeros(len(a), dtype=bool)
        if len(i_rows):
            Li, _, reflected, _ = gd.interface(Vl[i_rows], ior[mat[i_rows]], ~inside[i_rows], s1[i_rows])
            Ll[i_rows] = Li
            refracted[i_rows] = ~reflected
            enter = i_rows[~reflected & ~inside[i_rows]]
            if mutate != 11:
                t_new[enter] = t_new[enter] * (trans[mat[enter]] / tmax[enter][:, None])                                        # rule (G2): entering multiplies by transmission / tmax; no other weight
        wdir = _world(R, Ll)
        if len(l_rows):
            pdf_new[l_rows] = sd.lambert_pdf(wdir[l_rows, 2])                        # Q8 / D5: the WORLD-z pdf travels with a Lambertian-sampled ray
        if mutate == 6 and not ggx_pdf and len(g_rows):
            pdf_new[g_rows] = sd.lambert_pdf(wdir[g_rows, 2])
        if sky is not None:
            p_sky = sd.pdf(sky, wdir, map_w, map_h)
            mw = np.where(is_ggx, sd.miss_weight(sel, p_sky, pdf_new) if ggx_pdf else (1.0 if mutate == 2 else 0.0),                # rule: 0 for a GGX sample without the pdf, the vndf heuristic with it
                          sd.miss_weight(sel, p_sky, sd.lambert_pdf(Ll[:, 2])))                                                   # rule: the Lambert LOCAL pdf for a Lambertian sample
            mw = np.where(iface, sd.miss_weight(sel, p_sky, sd.lambert_pdf(wdir[:, 2])) if mutate == 5 else 1.0, mw)                # rule: the sky miss that follows an interface weighs 1
        p = t_new.max(axis=1)
        live = rng.random(len(a)) < p                                                # Q6: from bounce 0, max(throughput), unclamped
        terminated[a[~live]] = True
        al = a[live]
        thr[al] = t_new[live] / p[live][:, None]
        O[al] = np.where(refracted[live][:, None], hit[live] - OFFSET * nrm[live], P[live])
        D[al] = wdir[live]
        pdf_in[al], miss_w[al], after_iface[al] = pdf_new[live], mw[live], iface[live]
        lam_sampled[al], L_prev[al], V_prev[al] = (~is_ggx & ~iface)[live], Ll[live], Vl[live]
        alive = al

    out = {}
    for name, v in (("sum", rad), ("sum_sq", rad * rad)):
        out[name] = np.zeros((m, 3)); np.add.at(out[name], row, v)
    for name, v in (("rays", n_rays), ("rays_sq", n_rays * n_rays), ("shadow", n_shadow), ("shadow_sq", n_shadow * n_shadow),
                    ("terminated", terminated.astype(f64)), ("dropped", dropped.astype(f64))):
        out[name] = np.zeros(m); np.add.at(out[name], row, v)
    assert (terminated ^ dropped).all()
    return out


# ---- the scene -----------------------------------------------------------------------------------------------------------------------
W = H = 32                                 # four tiles: every tile-indexed path is exercised and a workgroup is one tile
MAX_BOUNCES = 8
DECAY = (0.0, 0.1, 0.3, 0.6, 1.0)
LENS_APERTURE = 0.05
SUN_POWER = 400.0
GGX_ROUGHNESS = 0.7
LAMP_A_EMISSION, LAMP_B_EMISSION = (20.0, 10.0, 4.0), (4.0, 10.0, 18.0)
GLASS_TRANSMISSION = (0.36, 0.48, 0.6)    # tmax < 1: at the issue's (0.9, 0.95, 1.0) the opaque lobe of the glass is never chosen and mutation 12 divides by 0; the stronger tint is mutation 11's
# name, centre, radius, material
# in the order the tree builders leave them in, so that authoring order = tree order and Q11 (the light's authoring index compared with the hit's tree
# index in the self-hit skip) cannot bite: test_scene_guard and test_rays_are_the_fixtures assert it.
# lamp_a is large and stands on the camera's side (+z) of the GGX ball and of the ground between them: a closure-sampled ray that finds it carries a
# world-z pdf (Q8) of the size of the light's own pdf there, which is where the emitter-hit heuristic (mutations 1 and 6) has something to weigh
SPHERES = (("ground", (0.0, -100.0, 0.0), 100.0, 0), ("lamp_b", (-0.45, 1.45, 0.2), 0.45, 4), ("ggx_ball", (0.0, 0.5, 0.0), 0.5, 1),
           ("glass_ball", (-0.7, 0.45, 1.2), 0.45, 2), ("lamp_a", (1.1, 0.7, 1.0), 0.7, 3))
SKY_LABEL = len(SPHERES)                   # the region of the camera rays that meet no sphere
REGION_NAMES = tuple(s[0] for s in SPHERES) + ("sky",)


def composed_scene(mirt):
    """test_sky_sampling_gpu.sun_scene grown to five spheres: a Lambertian ground ball, a GGX ball (roughness GGX_ROUGHNESS, coloured F0), a glass ball
    (transmission GLASS_TRANSMISSION, IOR 1.5, a non-black albedo: its opaque lobe shows), two emitters of different size and colour, under
    sky_definitions.sun_map with ambient 1.  Every material carries both an albedo and {F0, roughness}: the closure table decides which is read."""
    S = mirt.scene
    cam = S.Camera(eye=(0.0, 1.2, 4.0), direction=(0.0, -0.2, -1.0), focal_length=35.0, exposure=1.0)
    mat = [S._material(albedo=(0.7, 0.7, 0.7), F0=(0.04, 0.04, 0.04), roughness=0.6),
           S._material(albedo=(0.8, 0.3, 0.2), F0=(0.9, 0.6, 0.3), roughness=GGX_ROUGHNESS),
           S._material(albedo=(0.3, 0.25, 0.2), F0=(0.3, 0.25, 0.2), roughness=0.5, transmission=GLASS_TRANSMISSION, IOR_minus_one=0.5),
           S._material(emission=LAMP_A_EMISSION, roughness=0.5),
           S._material(emission=LAMP_B_EMISSION, roughness=0.5)]
    geo = [S._sphere(c, r * r, m) for _, c, r, m in SPHERES]
    sc = S.Scene(np.array(geo, dtype=S.SPHERE), np.array(mat, dtype=S.MATERIAL), cam, np.ones(3, dtype=f32), name="composed")
    sc.hdri = sd.sun_map(sun=(6, 40), power=SUN_POWER)                              # elevation ~ 51 degrees, in front of the camera to its right
    return sc


def focus_depth(sc):
    """The lens is focused on the GGX ball's centre."""
    return float(np.linalg.norm(np.asarray(dict((s[0], s[1]) for s in SPHERES)["ggx_ball"]) - np.asarray(sc.camera.eye, dtype=f64)))


def sampler_scene(sc):
    """A project Scene as composed_sampler's dict (the binary32 members, widened)."""
    g, m = sc.geometry, sc.material
    out = dict(centre=g["position"].astype(f64), radius_sq=g["radius_sq"].astype(f64), material=g["material_ID"].astype(np.int64),
               albedo=m["albedo"].astype(f64), emission=m["emission"].astype(f64), F0=m["F0"].astype(f64), roughness=m["roughness"].astype(f64),
               transmission=m["transmission"].astype(f64), ior=1.0 + m["IOR_minus_one"].astype(f64))
    if np.any(sc.ambient):
        out["hdri"], out["ambient"] = np.asarray(sc.hdri, dtype=f32), np.asarray(sc.ambient, dtype=f32).astype(f64)
    return out


CLOSURES = {"lambert": [0, 0, 0, 0, 0], "ggx": [1, 1, 1, 1, 1], "mixed": [0, 1, 0, 1, 0]}


def composed_forms():
    """The 80 forms: closures x light_ris x transmission x sky sampling x ggx_pdf (ggx and mixed only) x lens -> list of dicts."""
    out = []
    for closures, ris, glass, sky, pdf, lens in itertools.product(CLOSURES, (0, 4), (False, True), (False, True), (False, True), (False, True)):
        if pdf and closures == "lambert":
            continue
        out.append(dict(closures=closures, ris=ris, glass=glass, sky=sky, pdf=pdf, lens=lens))
    return out


def form_name(f):
    return f"{f['closures']}-ris{f['ris']}-glass{int(f['glass'])}-sky{int(f['sky'])}-pdf{int(f['pdf'])}-lens{int(f['lens'])}"


def form_seed(f):
    return 7000 + composed_forms().index(f)


def regions_of(sc, rays_per_acc):
    """Labels per slot from the float64 first hits of every accumulation's rays: the sphere every ray of the slot meets (SKY_LABEL: none of them
    meets one), -1 where the rays of a slot see more than one primitive or a hit is undecided in binary32 -> labels (slots,)."""
    scn = sampler_scene(sc)
    label = None
    for p, d in rays_per_acc:
        hit = df.closest_hit(np.asarray(p, dtype=f64), np.asarray(d, dtype=f64), scn["centre"], scn["radius_sq"])
        prim = np.where(hit["unsure"], -2, np.where(hit["prim"] < 0, SKY_LABEL, hit["prim"]))
        label = prim if label is None else np.where(label == prim, label, -2)
    return np.where(label < 0, -1, label)


def twin_run(sc, rays_per_acc, form, n_paths=1, mutate=None, seed=None):
    """composed_sampler for one form over the rays of every accumulation ((p, d) each (slots, 3)) -> per-slot statistics: E, var (slots, 3) of one
    path's contribution, the per-path means and variances of the counters over the whole frame, and the number of paths per slot."""
    scn = sampler_scene(sc)
    n_acc, slots = len(rays_per_acc), len(rays_per_acc[0][0])
    P = np.concatenate([np.asarray(p, dtype=f64) for p, _ in rays_per_acc])
    D = np.concatenate([np.asarray(d, dtype=f64) for _, d in rays_per_acc])
    sky = sd.table(scn["hdri"], scn["ambient"].astype(f32)) if form["sky"] else None
    out = composed_sampler(scn, (P, D), n_paths, MAX_BOUNCES, np.random.default_rng(form_seed(form) if seed is None else seed), closures=CLOSURES[form["closures"]],
                           light_ris=form["ris"], transmission=form["glass"], sky=sky, ggx_pdf=form["pdf"], decay=DECAY, mutate=mutate)
    per = n_acc * n_paths
    s1, s2 = out["sum"].reshape(n_acc, slots, 3).sum(axis=0), out["sum_sq"].reshape(n_acc, slots, 3).sum(axis=0)
    E = s1 / per
    res = dict(E=E, var=np.maximum(s2 / per - E * E, 0.0) * per / max(per - 1, 1), paths=per)
    n = per * slots
    for name in ("rays", "shadow", "terminated", "dropped"):
        mean = out[name].sum() / n
        sq = out[name + "_sq"].sum() / n if name + "_sq" in out else mean
        res[name], res[name + "_var"] = float(mean), float(max(sq - mean * mean, 0.0))
    return res


def region_figures(twin, labels):
    """What the fixture holds of one form: per region (REGION_NAMES order) the mean expectation (3,) and the summed per-pixel variance (3,), the pixel
    count, and the counters."""
    E, V, K = np.zeros((len(REGION_NAMES), 3)), np.zeros((len(REGION_NAMES), 3)), np.zeros(len(REGION_NAMES))
    for r in range(len(REGION_NAMES)):
        k = labels == r
        K[r] = k.sum()
        if k.any():
            E[r], V[r] = twin["E"][k].mean(axis=0), twin["var"][k].sum(axis=0)
    counters = np.array([twin[n] for n in ("rays", "shadow", "terminated", "dropped")] + [twin[n + "_var"] for n in ("rays", "shadow", "terminated", "dropped")])
    return E, V, K, counters


def region_z(got_mean, E, V, K, n_acc, twin_paths):
    """z of a backend's regional means (regions, 3) against the twin's: the standard error is built as test_definitions_cpu.region_stats builds it,
    from the twin's per-path variance at n_acc, plus the twin's own standard error of the mean - never from the backend's buckets.  A region
    whose expectation and variance are both 0 must be 0 exactly (z = 0 then, inf otherwise)."""
    se = np.sqrt(V * (1.0 / n_acc + 1.0 / twin_paths)) / np.maximum(K, 1)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(se > 0, (got_mean - E) / se, np.where(got_mean == E, 0.0, np.inf))
    return z, se


def slot_means(acc, n_acc):
    """The accumulator [tile][bucket][rgb][256] as per-slot means (tiles * 256, 3): slots are raygen's ray order."""
    a = np.asarray(acc, dtype=f64).sum(axis=1)                                      # [tile][rgb][256]
    return np.moveaxis(a, 1, 2).reshape(-1, 3) / n_acc


def regional_means(acc, n_acc, labels):
    img = slot_means(acc, n_acc)
    return np.array([img[labels == r].mean(axis=0) if (labels == r).any() else np.zeros(3) for r in range(len(REGION_NAMES))])
