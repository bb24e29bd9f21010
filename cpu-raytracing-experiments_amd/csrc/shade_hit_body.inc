// The per-hit shading, Renderer.hpp:169-404: closest-hit shader, next event estimation, emissive MIS, the closure sample and the Russian
// roulette for one ray that hit `hrec.prim` at `hrec.tfar`.  ONE text, included as statements (not a function: see DESIGN.md,
// "One per-hit shading text") by its two users in kernels.hpp:
//   * k_shade, phase 2 (shade_kernel_body.inc, the body of both of its overloads) — held to the oracle bit for bit by tests/test_gpu_parity.py, test_ggx_gpu.py, test_lens_gpu.py,
//     test_radiance_in_contrib.py and test_definitions_gpu.py;
//   * stream_shade_hit (k_tile_stream, exact stream order) — held by tests/test_exact_stream_order.py.
// The names are k_shade's.  The including scope provides
//   constants           GGX; MIXED (true: the closure is the hit material's — ggx_hit below is bit `mat` of closure_mask, a uint64_t the scope provides
//                       too, and the GGX rows {F0, roughness} are read from s_ggx (LDS) beside s_albedo, mirt_set_material_closures; false: ggx_hit is
//                       the constant GGX and none of that is named by an instruction); RIS (true: the NEE light is picked among ris_m candidates, a uint32_t the scope provides too); GLASS (true: a
//                       transmissive material can take the dielectric interface below, mirt_set_transmission; false: none of that text is compiled in);
//                       SKY (true: the environment map is light number n_lights of next event estimation, mirt_set_sky_sampling — the scope then
//                       provides sky (SkyTable) and a light_selection_pdf of 1 / (n_lights + 1), and gets miss_w (float) written with survive: the
//                       MIS weight the miss shader gives thr.r x sky should ndir miss; false: none of that text is compiled in);
//                       PDF (true: mirt_set_ggx_pdf — a GGX hit's closure pdf is ggx_pdf(alpha, L, Vl) where it is 0 otherwise: in next event estimation's
//                       two heuristics and in miss_w; the scope gets pdf_out (float) written with survive, the pdf_in of the bounce that will shade
//                       ndir, and itself passes as pdf_in what the sampling bounce left there; false: none of that text is compiled in)
//   read                sc, fp, s_albedo, s_emission (the material tables in LDS), bounce, gloss_decay, light_selection_pdf,
//                       pdf_in (out->pdf of the bounce that sampled D, Q8), hrec (HitRec), prim (= hrec.prim), D (f3);
//                       GLASS only: s_glass (LDS, {transmission.rgb, 1 + IOR_minus_one} per material) and after_interface (bool: D was sampled
//                       by a dielectric interface, so no light sample could have produced it)
//   read and written    thr (f3: the closure's estimator, then the roulette's 1 / (1 - q), in place)
//   written             P, L, srad, E, ndir (f3), light_distance (float), has_shadow, has_E, terminated, survive (bool; has_E is always
//                       assigned, the other three flags are only ever set: the scope starts them at false — k_shade's locals do;
//                       stream_shade_hit binds survive and has_shadow to its StreamHit, which k_tile_stream zeroes before the call); L, light_distance and srad
//                       are assigned with has_shadow, E with has_E, ndir with survive; GLASS only: via_interface (bool, only ever set: ndir was
//                       sampled by the interface — the scope hands it to the next bounce as after_interface); MIXED only: sampled_ggx (bool, assigned
//                       with survive: ndir was sampled by Closure<GGX> — the scope hands it to the next bounce, whose pdf_in is then 0)
//   three expressions   SHADE_HIT_ORIGIN (f3), SHADE_HIT_ACC and SHADE_HIT_SEED (uint32_t): the ray's origin, its accumulation number and
//                       its seed[ID] (Renderer.hpp:74,107), evaluated where they stand below — k_shade loads and derives them from its
//                       stream at these points, and its registers depend on that order.  #undef'd at the end of this file.
#if !defined(SHADE_HIT_ORIGIN) || !defined(SHADE_HIT_ACC) || !defined(SHADE_HIT_SEED)
#error "shade_hit_body.inc: define SHADE_HIT_ORIGIN, SHADE_HIT_ACC and SHADE_HIT_SEED before including it (see the list above)"
#endif
// CLOSEST HIT SHADER, Renderer.hpp:169-214
const float depth = hrec.tfar;
const float4 hs = sc.spheres[prim];
const int32_t mat = sc.prim_mat[prim];
const f3 O = SHADE_HIT_ORIGIN;
const f3 hit{ O.x + D.x * depth, O.y + D.y * depth, O.z + D.z * depth };
f3 N = normalize3(f3{ hit.x - hs.x, hit.y - hs.y, hit.z - hs.z });
const bool from_inside = dot3(N, D) >= 0.0f;
if (from_inside) N = f3{ -N.x, -N.y, -N.z };
const quat T = tangent_space(N);
const f3 Vl = to_local(T, f3{ -D.x, -D.y, -D.z });
P = { hit.x + N.x * 1e-4f, hit.y + N.y * 1e-4f, hit.z + N.z * 1e-4f };
const float4 em = s_emission[mat];
const bool ggx_hit = MIXED ? ((closure_mask >> mat) & 1ull) != 0ull : GGX;      // the closure that shades this hit: the material's (MIXED) or the frame's
const float4 alb = (MIXED && ggx_hit) ? s_ggx[mat] : s_albedo[mat];
const bool is_emissive = max_sel(em.x, max_sel(em.y, em.z)) > MIRT_FLT_EPSILON;
f3 F0{0.0f, 0.0f, 0.0f};
float alpha = 0.0f;
if (ggx_hit) {                                                     // closure set-up, Renderer.hpp:210-212
	F0 = { alb.x, alb.y, alb.z };
	float a = alb.w; a *= a;
	alpha = a + (1.0f - a) * gloss_decay;
}
const uint32_t acc = SHADE_HIT_ACC;
const uint32_t seed = SHADE_HIT_SEED;
// (The closure stream is hashed here and again in BRDF SAMPLING below, on purpose: the lobe must be known before next event estimation, and the text
// below stays the one the instantiations without GLASS compile, draw for draw.)
// DIELECTRIC INTERFACE, lobe choice (no reference text: Renderer.hpp reads neither transmission nor IOR_minus_one).  A material is transmissive
// when tmax = max(transmission.rgb) > 0.  A hit reached from inside its sphere always takes the interface, one from outside with probability tmax:
// s0 < tmax, s0 and s1 the 4th and 5th draws of this bounce's closure stream (the first three stay b0, b1 and the roulette's).  Selection
// probability and lobe weight cancel, so the throughput of neither lobe is reweighted.  Any other hit draws what it draws without GLASS.
bool interface = false;
float4 glass = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
float glass_tmax = 0.0f, glass_s1 = 0.0f;
if (GLASS) {
	glass = s_glass[mat];
	glass_tmax = max_sel(glass.x, max_sel(glass.y, glass.z));
	if (glass_tmax > 0.0f) {
		uint32_t rng = hash_2d(acc, seed + bounce * 2u + 1u);
		(void)pcg_generate(rng); (void)pcg_generate(rng); (void)pcg_generate(rng);
		const float s0 = rand_unit_float(rng);
		glass_s1 = rand_unit_float(rng);
		interface = from_inside || s0 < glass_tmax;
	}
}

// NEXT EVENT ESTIMATION, Renderer.hpp:247-298
if (fp.mis && !(GLASS && interface)) {                             // the interface is a delta closure: no light sample can meet it
	uint32_t rng = hash_2d(acc, seed + bounce * 2u);
	if (RIS) {
		// RIS<count>, Sampling.hpp:25-54: ris_m candidates from the plain draw's own stream, one kept by a weighted reservoir.  A candidate's weight is
		// the largest channel of its radiance (integrand x MIS weight / source pdf); one that leaves the text early weighs 0 and still counts.
		// ris_m is a kernel argument: the counter stays scalar and only the body diverges.
		float weight_sum = 0.0f, w_sel = 0.0f;
		for (uint32_t cand = 0u; cand < ris_m; cand++) {
			const float u0 = rand_unit_float(rng);
			const float u1 = rand_unit_float(rng);
			const int32_t selected = static_cast<int32_t>(rand_bounded_int(rng, SKY ? fp.n_lights + 1u : fp.n_lights));
			const float r = rand_unit_float(rng);                      // Reservoir::Update's draw, taken for every candidate
#define NEE_ACCEPT(Ld, ldist, rad) { const float w = max_sel(max_sel(rad.x, rad.y), rad.z); weight_sum += w; \
			if (weight_sum == w || r < w / weight_sum) { w_sel = w; L = Ld; light_distance = ldist; srad = rad; } }   /* w > 0 here: the text left on w <= 0; the first positive candidate is taken whatever r (rand_unit_float reaches 1.0f) */
#include "nee_sample_body.inc"
#undef NEE_ACCEPT
		}
		if (w_sel > 0.0f) {
			has_shadow = true;
			const float k = weight_sum / (static_cast<float>(ris_m) * w_sel);      // one candidate: w / (1 * w) = 1, the plain draw word for word
			srad = { srad.x * k, srad.y * k, srad.z * k };
		}
	} else {
		const float u0 = rand_unit_float(rng);
		const float u1 = rand_unit_float(rng);
		const int32_t selected = static_cast<int32_t>(rand_bounded_int(rng, SKY ? fp.n_lights + 1u : fp.n_lights));
#define NEE_ACCEPT(Ld, ldist, rad) has_shadow = true; L = Ld; light_distance = ldist; srad = rad;
#include "nee_sample_body.inc"
#undef NEE_ACCEPT
	}
}
// EMISSIVE PRIMITIVE HIT, Renderer.hpp:319-353
has_E = is_emissive;
if (is_emissive) {
	if (fp.mis && bounce > 0) {
		const float radius2 = hs.w;
		const float center_dist2 = depth * (depth + Vl.z * (2.0f * __builtin_sqrtf(radius2))) + radius2;
		float weight = powerHeuristic(pdf_in, light_selection_pdf * spherePdf(radius2, center_dist2));
		if (GLASS && after_interface) weight = 1.0f;                // the ray left a dielectric interface: the extension ray is the only sampler of this path
		E = { (thr.x * weight) * em.x, (thr.y * weight) * em.y, (thr.z * weight) * em.z };
	} else {
		E = { em.x, em.y, em.z };                                   // Q9: no throughput
	}
}
// BRDF SAMPLING - BOUNCE, Renderer.hpp:357-404
{
	uint32_t rng = hash_2d(acc, seed + bounce * 2u + 1u);
	const float b0 = rand_unit_float(rng);
	const float b1 = rand_unit_float(rng);
	f3 sd;
	if (GLASS && interface) {
		// entering: the tint transmission / tmax, once per pass through the ball; leaving, reflected or totally reflected: weight 1.
		// In WORLD space (sd is the next direction itself): the tangent frame is ill-conditioned near N.z = -1 (device_math.hpp)
		float F; bool reflected, tir;
		dielectric_interface(D, N, glass.w, !from_inside, glass_s1, sd, F, reflected, tir);
		if (!reflected) {
			if (!from_inside) thr = { thr.x * (glass.x / glass_tmax), thr.y * (glass.y / glass_tmax), thr.z * (glass.z / glass_tmax) };
			P = { hit.x - N.x * 1e-4f, hit.y - N.y * 1e-4f, hit.z - N.z * 1e-4f };
		}
	} else if (ggx_hit) {                                                  // Closure<GGX>::sample, DataStreams.hpp:200-218
		f3 est;
		ggx_sample(F0, alpha, Vl, b0, b1, sd, est);
		thr = { thr.x * est.x, thr.y * est.y, thr.z * est.z };
	} else {
		sd = hemisphere(b0, b1);                                    // Closure::sample, DataStreams.hpp:177-181
		thr = { thr.x * alb.x, thr.y * alb.y, thr.z * alb.z };
	}
	const float q = 1.0f - max_sel(thr.x, max_sel(thr.y, thr.z));
	if (rand_unit_float(rng) < q) {
		terminated = true;                                          // Russian roulette, Renderer.hpp:377-383
	} else {
		const float inv = 1.0f / max_sel(MIRT_FLT_EPSILON, 1.0f - q);
		thr = { thr.x * inv, thr.y * inv, thr.z * inv };
		ndir = to_world(T, sd);
		if (GLASS && interface) { ndir = sd; via_interface = true; }
		if (MIXED) sampled_ggx = ggx_hit;                           // Q8: pdf_in of an emitter this ray hits belongs to the closure that sampled it
		if (PDF) {
			// mirt_set_ggx_pdf: the pdf_in of the next bounce travels with the ray.  A GGX hit: p~ of sd, from THIS hit's alpha and Vl — nothing of it
			// can be recomputed from ndir.  A Lambertian hit: Q8's word, (1 / pi) max(0, world z) of ndir as stored, the bits the next bounce would
			// recompute.  An interface: never read (after_interface makes the weight 1).
			if (GLASS && interface) pdf_out = 0.0f;
			else if (ggx_hit) pdf_out = ggx_pdf(alpha, sd, Vl);
			else pdf_out = MIRT_INV_PI * max_sel(0.0f, ndir.z);
		}
		if (SKY) {
			// What the miss shader may keep of thr.r x sky: the power heuristic of the closure's pdf of sd — the LOCAL one: next event estimation
			// weighs against that, and Q8's world-z pdf_in would break the partition of unity — against sel x the sky's density of ndir.
			// An interface is a delta closure (no light sample meets it): 1.  Closure<GGX>::pdf is 0: 0, as for the emitters such a ray hits —
			// unless PDF (mirt_set_ggx_pdf): then the heuristic of p~, as for those emitters too.
			if (GLASS && interface) miss_w = 1.0f;
			else if (ggx_hit) { uint32_t prow, pcol; miss_w = PDF ? powerHeuristic(pdf_out, light_selection_pdf * sky_pdf(sc, sky, ndir.x, ndir.y, ndir.z, prow, pcol)) : 0.0f; }   // PDF: next event estimation weighs against the same p~
			else { uint32_t prow, pcol; miss_w = powerHeuristic(MIRT_INV_PI * max_sel(0.0f, sd.z), light_selection_pdf * sky_pdf(sc, sky, ndir.x, ndir.y, ndir.z, prow, pcol)); }
		}
		survive = true;
	}
}
#undef SHADE_HIT_ORIGIN
#undef SHADE_HIT_ACC
#undef SHADE_HIT_SEED
