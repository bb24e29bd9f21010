// One light sample of next event estimation, Renderer.hpp:261-296: from the gather of light `selected` to the MIS-weighted radiance a shadow ray
// towards it would carry.  Included as statements by shade_hit_body.inc, once for the plain draw and once inside the RIS candidate loop, so both
// run ONE text.  Reads selected, u0, u1 and everything shade_hit_body.inc has in scope at that point; a sample that survives every early-out
// ends in NEE_ACCEPT(direction, distance, radiance), which the including scope defines; one that does not leaves nothing behind.
// SKY (mirt_set_sky_sampling): light number n_lights is the environment map.  Ld is drawn from the table with density q; p~ = sky_pdf(Ld) is the
// density both MIS weights are formed from (sky_eval's own cell arithmetic: in its edge bands it may name the neighbour of the cell that was
// drawn).  Estimator: f L w(p~) / (sel q), with w the power heuristic of sel p~ against the closure's pdf — powerHeuristic_over_f gives w / (sel p~),
// times p~ / q (1.0f exactly wherever the two cells agree).  L x f is sky_eval(Ld).rgb x (thr.r x f.r): Q10 carried over, the miss shader's
// red-channel throughput on all three channels, so that the expectation is the plain path's.  One shadow ray, tfar = FLT_MAX.
// PDF (mirt_set_ggx_pdf): a GGX hit's closure pdf in both power heuristics is ggx_pdf(alpha, Ll, Vl) instead of 0; light RIS reads nothing new (its weights come from rad).
if (SKY && selected == static_cast<int32_t>(fp.n_lights)) {
	do {
		float sky_q; uint32_t srow, scol;
		const f3 Ld = sky_sample(sky, u0, u1, sky_q, srow, scol);
		const f3 Ll = to_local(T, Ld);
		if (Ll.z < 0.0f) break;
		float fx;
		if (ggx_hit) fx = ggx_eval(F0, alpha, Ll, Vl).x;
		else fx = alb.x * (MIRT_INV_PI * max_sel(0.0f, Ll.z));
		const f3 Le = sky_eval(sc, Ld.x, Ld.y, Ld.z);
		const float k = thr.x * fx;
		f3 rad{ Le.x * k, Le.y * k, Le.z * k };
		const float sky_p = sky_pdf(sc, sky, Ld.x, Ld.y, Ld.z, srow, scol);
		const float brdf_pdf = ggx_hit ? (PDF ? ggx_pdf(alpha, Ll, Vl) : 0.0f) : MIRT_INV_PI * max_sel(0.0f, Ll.z);   // PDF: mirt_set_ggx_pdf
		const float w = powerHeuristic_over_f(light_selection_pdf * sky_p, brdf_pdf) * (sky_p / sky_q);
		rad.x *= w; rad.y *= w; rad.z *= w;
		if (max_sel(max_sel(rad.x, rad.y), rad.z) <= 0.0f) break;
		NEE_ACCEPT(Ld, MIRT_FLT_MAX, rad)
	} while (false);
} else {
const float4 lp = sc.light_sphere[selected];                    // scene.geometry[lighting_acceleration.prims[selected]]
const float4 lem = sc.light_emit[selected];                     // its material's emission, and the prim id
const int32_t light_primID = static_cast<int32_t>(__float_as_uint(lem.w));
do {
	if (light_primID == prim) break;                             // Q11: geometry-order id vs BVH-order id
	f3 Wc{ lp.x - P.x, lp.y - P.y, lp.z - P.z };
	const float center_dist2 = dot3(Wc, Wc);
	if (center_dist2 <= lp.w) break;
	const float center_dist = __builtin_sqrtf(center_dist2);
	{ const float inv = 1.0f / center_dist; Wc.x *= inv; Wc.y *= inv; Wc.z *= inv; }
	const float sinThetaMax2 = lp.w / center_dist2;
	{
		const float NdotW = (2.0f * T.w) * (Wc.z * T.w + Wc.x * T.y - T.x * Wc.y) - Wc.z;
		if (NdotW < 0.0f && sinThetaMax2 < NdotW * NdotW) break;
	}
	float ldist, lpdf;
	const f3 Ld = sample_direction_to_sphere(Wc, sinThetaMax2, center_dist, lp.w, u0, u1, ldist, lpdf);
	const f3 Ll = to_local(T, Ld);
	if (Ll.z < 0.0f) break;
	f3 rad{ lem.x * thr.x, lem.y * thr.y, lem.z * thr.z };
	if (ggx_hit) {  // Closure<GGX>::eval, DataStreams.hpp:189-195
		const f3 f = ggx_eval(F0, alpha, Ll, Vl);
		rad.x *= f.x; rad.y *= f.y; rad.z *= f.z;
	} else {    // Closure<LambertianDiffuse>::eval, DataStreams.hpp:169-172
		const float f = MIRT_INV_PI * max_sel(0.0f, Ll.z);
		rad.x *= alb.x * f; rad.y *= alb.y * f; rad.z *= alb.z * f;
	}
	lpdf *= light_selection_pdf;
	const float brdf_pdf = ggx_hit ? (PDF ? ggx_pdf(alpha, Ll, Vl) : 0.0f) : MIRT_INV_PI * max_sel(0.0f, Ll.z);  // DataStreams.hpp:173-176 / :196-198 (0, "TODO"); PDF: mirt_set_ggx_pdf
	const float w = powerHeuristic_over_f(lpdf, brdf_pdf);
	rad.x *= w; rad.y *= w; rad.z *= w;
	if (max_sel(max_sel(rad.x, rad.y), rad.z) <= 0.0f) break;
	NEE_ACCEPT(Ld, ldist, rad)
} while (false);
}
