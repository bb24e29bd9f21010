// tests/native/ggx_twin.cpp — TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
// The oracle (oracle/oracle.cpp, included whole: every helper, trace mode and the tile-list machinery is shared) with the
// reference's closure switch made a runtime argument: brdf = 0 is Closure<LambertianDiffuse> (the oracle's own path), brdf = 1
// is Closure<GGX> (`#define BRDF 1`, Renderer.hpp:70, DataStreams.hpp:184-219) with the gloss decay table the reference names
// but never declares (Renderer.hpp:212) supplied by the caller.  Everything else restates the oracle's accumulate_tile
// (Renderer.hpp:83-432) line for line.  The tests compile this file with oracle/Makefile's CXXFLAGS into a temporary directory;
// it is never linked into the product.
#include "../../oracle/oracle.cpp"

namespace {

struct GgxParams {
	int brdf = 0;
	std::vector<float> decay;                 // gloss_decay_table by bounce; entries beyond its length are 0
	float at(size_t bounce) const { return bounce < decay.size() ? decay[bounce] : 0.0f; }
};

struct ClosureData {                          // shaderdata_stream.closure[ID] of either type (DataStreams.hpp:164-219)
	float albedo[N][3];
	float F0[N][3];
	float alpha[N];
};

// Renderer.hpp:83-432 — one tile, one Accumulate() call, with the closure of `g.brdf`
static void accumulate_tile_brdf(const Oracle& o, const GgxParams& g, uint32_t LaunchIndex, size_t slab, uint32_t accumulations, float* accumulator, LocalCounters& lc) {
	const uint32_t light_count = static_cast<uint32_t>(o.lights.size());
	const float light_selection_pdf = 1.0f / static_cast<float>(o.lights.size());
	const bool has_ambient = std_max(o.sky.ambient[0], std_max(o.sky.ambient[1], o.sky.ambient[2])) > 0.0f;
	const uint32_t bucket_index = accumulations % o.buckets;
	const bool MIS = o.mis && light_count > 0;                                  // Q12 guard
	const bool GGX = g.brdf == 1;

	float* out_r = accumulator + (slab * o.buckets + bucket_index) * 3 * TileSize;
	float* out_g = out_r + TileSize;
	float* out_b = out_g + TileSize;
	const int32_t tile_x = static_cast<int32_t>(TileRoot * (LaunchIndex % o.h_tiles));
	const int32_t tile_y = static_cast<int32_t>(TileRoot * (LaunchIndex / o.h_tiles));

	static thread_local RayStream ray_stream;
	static thread_local ShaderData sd;
	static thread_local ClosureData cl;
	uint16_t sort_buffer[MaxMaterialID + 2];
	Buffer* in = &ray_stream.buffers[0];
	Buffer* outb = &ray_stream.buffers[1];

	for (size_t i = 0; i < N; i++) {                                            // :97-109
		in->radiance.r[i] = in->radiance.g[i] = in->radiance.b[i] = 0.0f;
		in->throughput.r[i] = in->throughput.g[i] = in->throughput.b[i] = 1.0f;
		in->pixelID[i] = static_cast<uint32_t>(i);
		ray_stream.seed[i] = static_cast<uint32_t>(static_cast<int32_t>((LaunchIndex * TileSize + i) * (o.max_bounces * 2 + 1)));
	}
	for (size_t ID = 0; ID < TileSize; ID++) {                                  // :113-127
		int32_t x = tile_x + static_cast<int32_t>(ID) % static_cast<int32_t>(TileRoot);
		int32_t y = tile_y + static_cast<int32_t>(ID) / static_cast<int32_t>(TileRoot);
		uint32_t rng_state = hash_2d(accumulations, ray_stream.seed[ID]);
		float cs[2]; cs[0] = rand_unit_float(&rng_state); cs[1] = rand_unit_float(&rng_state);
		v3 dir = generate_ray_dir(o.camera, x, y, cs);
		in->dir.x[ID] = dir.x; in->dir.y[ID] = dir.y; in->dir.z[ID] = dir.z;
		in->p.x[ID] = o.camera.pos.x; in->p.y[ID] = o.camera.pos.y; in->p.z[ID] = o.camera.pos.z;
	}
	size_t active_rays = N;
	for (size_t bounce = 0; bounce < o.max_bounces && active_rays > 0; bounce++, std::swap(in, outb)) {   // :131
		ray_stream.termination.zero(); ray_stream.has_shadowray.zero();
		ray_stream.shadow_rays.occluded.zero(); sd.is_emissive.zero();
		memset(sort_buffer, 0, sizeof sort_buffer);
		for (size_t i = 0; i < ((active_rays + 7) / 8) * 8; i++) {
			ray_stream.hit.tfar[i] = FLT_MAX; ray_stream.hit.matID[i] = -1; ray_stream.hit.primID[i] = -1;
		}
		traverse(o, *in, ray_stream.hit, active_rays, lc);                      // :165
		const float decay = g.at(bounce);

		for (size_t ID = 0; ID < active_rays; ID++) {                           // :169-214 closest-hit shader
			const int32_t mat_ID = ray_stream.hit.matID[ID];
			if (mat_ID == -1) continue;
			const int32_t prim_ID = ray_stream.hit.primID[ID];
			const float depth = ray_stream.hit.tfar[ID];
			const v3 D{ in->dir.x[ID], in->dir.y[ID], in->dir.z[ID] };
			v3 hit_point{ in->p.x[ID] + D.x * depth, in->p.y[ID] + D.y * depth, in->p.z[ID] + D.z * depth };
			const Sphere& hp = o.bvh.prims[prim_ID];
			v3 Nn{ hit_point.x - hp.px, hit_point.y - hp.py, hit_point.z - hp.pz };
			Nn = normalize3(Nn);
			if (dot3(Nn, D) >= 0.0f) Nn = v3{ -Nn.x, -Nn.y, -Nn.z };
			q4 T = tangent_space(Nn);
			v3 Vlocal = to_local(T, v3{ -D.x, -D.y, -D.z });
			sd.P.x[ID] = hit_point.x + Nn.x * 1e-4f;
			sd.P.y[ID] = hit_point.y + Nn.y * 1e-4f;
			sd.P.z[ID] = hit_point.z + Nn.z * 1e-4f;
			sd.V.x[ID] = Vlocal.x; sd.V.y[ID] = Vlocal.y; sd.V.z[ID] = Vlocal.z;
			sd.T.x[ID] = T.x; sd.T.y[ID] = T.y; sd.T.z[ID] = T.z; sd.T.w[ID] = T.w;
			const Material& m = o.material[mat_ID];
			if (std_max(m.emission[0], std_max(m.emission[1], m.emission[2])) > FLT_EPSILON) sd.is_emissive.set(ID);
			if (GGX) {                                                           // :209-212
				cl.F0[ID][0] = m.F0[0]; cl.F0[ID][1] = m.F0[1]; cl.F0[ID][2] = m.F0[2];
				float alpha = m.roughness; alpha *= alpha;
				cl.alpha[ID] = alpha + (1.0f - alpha) * decay;
			} else {                                                             // :207-208
				cl.albedo[ID][0] = m.albedo[0]; cl.albedo[ID][1] = m.albedo[1]; cl.albedo[ID][2] = m.albedo[2];
			}
		}
		const size_t miss_count = sort_rayID(static_cast<uint32_t>(o.material.size()), static_cast<uint32_t>(active_rays),
		                                     ray_stream.RayID, ray_stream.hit.matID, sort_buffer);   // :235-241
		const size_t hit_count = active_rays - miss_count;

		const bool skip_dropped_nee = o.trav_mode == 2 && !(bounce < o.max_bounces - 1);   // as the oracle: the product emits no NEE rays for dropped hits
		if (MIS && !skip_dropped_nee) {                                          // :247-315
			size_t shadow_index = 0;
			ShadowStream& sh = ray_stream.shadow_rays;
			for (size_t i = 0; i < hit_count; i++) {
				const int32_t ID = static_cast<int32_t>(ray_stream.RayID[miss_count + i]);
				uint32_t rng_state = hash_2d(accumulations, ray_stream.seed[in->pixelID[ID]] + static_cast<uint32_t>(bounce) * 2);
				float ls[2]; ls[0] = rand_unit_float(&rng_state); ls[1] = rand_unit_float(&rng_state);
				int32_t selected_light = static_cast<int32_t>(rand_bounded_int(&rng_state, light_count));
				int32_t light_primID = o.lights[selected_light];
				const Sphere& light_prim = o.geometry[light_primID];
				if (light_primID == ray_stream.hit.primID[ID]) continue;          // Q11
				v3 Wc{ light_prim.px - sd.P.x[ID], light_prim.py - sd.P.y[ID], light_prim.pz - sd.P.z[ID] };
				float center_dist2 = dot3(Wc, Wc);
				if (center_dist2 <= light_prim.radius_sq) continue;
				float center_dist = sqrtf(center_dist2);
				{ float inv = 1.0f / center_dist; Wc.x *= inv; Wc.y *= inv; Wc.z *= inv; }
				float sinThetaMax2 = light_prim.radius_sq / center_dist2;
				{
					float NdotW = (2.0f * sd.T.w[ID]) * (Wc.z * sd.T.w[ID] + Wc.x * sd.T.y[ID] - sd.T.x[ID] * Wc.y) - Wc.z;
					if (NdotW < 0.0f && sinThetaMax2 < NdotW * NdotW) continue;
				}
				float light_distance, light_pdf;
				v3 L = sample_direction_to_sphere(Wc, sinThetaMax2, center_dist, light_prim.radius_sq, ls[0], ls[1], &light_distance, &light_pdf);
				q4 T{ sd.T.x[ID], sd.T.y[ID], sd.T.z[ID], sd.T.w[ID] };
				v3 Llocal = to_local(T, L);
				if (Llocal.z < 0.0f) continue;
				const Material& lm = o.material[light_prim.material_ID];
				v3 radiance{ lm.emission[0] * in->throughput.r[ID], lm.emission[1] * in->throughput.g[ID], lm.emission[2] * in->throughput.b[ID] };
				float brdf_pdf;
				if (GGX) {                                                       // Closure<GGX>::eval / pdf, DataStreams.hpp:189-198
					const v3 f = ggx_eval(v3{ cl.F0[ID][0], cl.F0[ID][1], cl.F0[ID][2] }, cl.alpha[ID], Llocal, v3{ sd.V.x[ID], sd.V.y[ID], sd.V.z[ID] });
					radiance.x *= f.x; radiance.y *= f.y; radiance.z *= f.z;
					brdf_pdf = 0.0f;
				} else {                                                         // Closure<Lambertian>::eval / pdf, DataStreams.hpp:169-176
					float NdotL = std_max(0.0f, Llocal.z);
					float f = kOneOverPi * NdotL;
					radiance.x *= cl.albedo[ID][0] * f; radiance.y *= cl.albedo[ID][1] * f; radiance.z *= cl.albedo[ID][2] * f;
					brdf_pdf = kOneOverPi * std_max(0.0f, Llocal.z);
				}
				light_pdf *= light_selection_pdf;
				float w = powerHeuristic_over_f(light_pdf, brdf_pdf);
				radiance.x *= w; radiance.y *= w; radiance.z *= w;
				if (std_max(std_max(radiance.x, radiance.y), radiance.z) <= 0.0f) continue;
				sh.dir.x[shadow_index] = L.x; sh.dir.y[shadow_index] = L.y; sh.dir.z[shadow_index] = L.z;
				sh.p.x[shadow_index] = sd.P.x[ID]; sh.p.y[shadow_index] = sd.P.y[ID]; sh.p.z[shadow_index] = sd.P.z[ID];
				sh.tfar[shadow_index] = light_distance;
				sh.radiance.r[shadow_index] = radiance.x; sh.radiance.g[shadow_index] = radiance.y; sh.radiance.b[shadow_index] = radiance.z;
				ray_stream.has_shadowray.set(ID);
				++shadow_index;
			}
			traverse_shadow(o, sh, shadow_index, lc);                            // :302
			for (size_t i = miss_count, shadow_ID = 0; i < active_rays; i++) {   // :304-314
				const int32_t ID = static_cast<int32_t>(ray_stream.RayID[i]);
				if (ray_stream.has_shadowray.test(ID)) {
					if (!sh.occluded.test(shadow_ID)) {
						in->radiance.r[ID] += sh.radiance.r[shadow_ID];
						in->radiance.g[ID] += sh.radiance.g[shadow_ID];
						in->radiance.b[ID] += sh.radiance.b[shadow_ID];
					}
					++shadow_ID;
				}
			}
		}
		if (MIS && bounce > 0) {                                                 // :319-343 (in->pdf: the previous bounce's closure pdf)
			for (size_t ID = 0; ID < active_rays; ID++) {
				if (!sd.is_emissive.test(ID)) continue;
				v3 throughput{ in->throughput.r[ID], in->throughput.g[ID], in->throughput.b[ID] };
				const Sphere& light_prim = o.bvh.prims[ray_stream.hit.primID[ID]];
				const float radius2 = light_prim.radius_sq;
				const float depth = ray_stream.hit.tfar[ID];
				const float NdotV = sd.V.z[ID];
				float center_dist2 = depth * (depth + NdotV * (2.0f * sqrtf(radius2))) + radius2;
				float weight = powerHeuristic(in->pdf[ID], light_selection_pdf * spherePdf(radius2, center_dist2));
				throughput.x *= weight; throughput.y *= weight; throughput.z *= weight;
				const float* em = o.material[ray_stream.hit.matID[ID]].emission;
				in->radiance.r[ID] += throughput.x * em[0];
				in->radiance.g[ID] += throughput.y * em[1];
				in->radiance.b[ID] += throughput.z * em[2];
			}
		} else {                                                                 // :344-353 (Q9: no throughput)
			for (size_t ID = 0; ID < active_rays; ID++) {
				if (!sd.is_emissive.test(ID)) continue;
				const float* em = o.material[ray_stream.hit.matID[ID]].emission;
				in->radiance.r[ID] += em[0]; in->radiance.g[ID] += em[1]; in->radiance.b[ID] += em[2];
			}
		}
		size_t output_index = 0;                                                 // :357-404
		if (bounce < o.max_bounces - 1) {
			for (size_t i = 0; i < hit_count; i++) {
				const int32_t ID = static_cast<int32_t>(ray_stream.RayID[miss_count + i]);
				uint32_t rng_state = hash_2d(accumulations, ray_stream.seed[in->pixelID[ID]] + static_cast<uint32_t>(bounce) * 2 + 1);
				float bs[2]; bs[0] = rand_unit_float(&rng_state); bs[1] = rand_unit_float(&rng_state);
				v3 sdir, estimator;
				if (GGX) {                                                       // Closure<GGX>::sample, DataStreams.hpp:200-218
					ggx_sample(v3{ cl.F0[ID][0], cl.F0[ID][1], cl.F0[ID][2] }, cl.alpha[ID], v3{ sd.V.x[ID], sd.V.y[ID], sd.V.z[ID] }, bs[0], bs[1], &sdir, &estimator);
				} else {                                                         // DataStreams.hpp:177-181
					sdir = hemisphere(bs[0], bs[1]);
					estimator = v3{ cl.albedo[ID][0], cl.albedo[ID][1], cl.albedo[ID][2] };
				}
				v3 throughput{ in->throughput.r[ID] * estimator.x, in->throughput.g[ID] * estimator.y, in->throughput.b[ID] * estimator.z };
				{
					float q = 1.0f - std_max(throughput.x, std_max(throughput.y, throughput.z));
					if (rand_unit_float(&rng_state) < q) { ray_stream.termination.set(ID); continue; }
					float inv = 1.0f / std_max(FLT_EPSILON, 1.0f - q);
					throughput.x *= inv; throughput.y *= inv; throughput.z *= inv;
				}
				q4 T{ sd.T.x[ID], sd.T.y[ID], sd.T.z[ID], sd.T.w[ID] };
				sdir = to_world(T, sdir);
				outb->p.x[output_index] = sd.P.x[ID]; outb->p.y[output_index] = sd.P.y[ID]; outb->p.z[output_index] = sd.P.z[ID];
				outb->dir.x[output_index] = sdir.x; outb->dir.y[output_index] = sdir.y; outb->dir.z[output_index] = sdir.z;
				outb->throughput.r[output_index] = throughput.x; outb->throughput.g[output_index] = throughput.y; outb->throughput.b[output_index] = throughput.z;
				outb->radiance.r[output_index] = in->radiance.r[ID]; outb->radiance.g[output_index] = in->radiance.g[ID]; outb->radiance.b[output_index] = in->radiance.b[ID];
				outb->pixelID[output_index] = in->pixelID[ID];
				// :401 — Closure<GGX>::pdf = 0 ("TODO", DataStreams.hpp:196-198); Lambertian: Q8, pdf of the WORLD-space dir
				outb->pdf[output_index] = GGX ? 0.0f : kOneOverPi * std_max(0.0f, sdir.z);
				output_index++;
			}
		}
		for (size_t i = 0; i < miss_count; i++) ray_stream.termination.set(ray_stream.RayID[i]);   // :408-410
		if (has_ambient) {                                                       // :411-420 (Q10)
			for (size_t i = 0; i < miss_count; i++) {
				const int32_t ID = static_cast<int32_t>(ray_stream.RayID[i]);
				v3 sky_value = sky_eval(o.sky, in->dir.x[ID], in->dir.y[ID], in->dir.z[ID]);
				in->radiance.r[ID] += in->throughput.r[ID] * sky_value.x;
				in->radiance.g[ID] += in->throughput.r[ID] * sky_value.y;
				in->radiance.b[ID] += in->throughput.r[ID] * sky_value.z;
			}
		}
		for (size_t ID = 0; ID < active_rays; ID++) {                            // :424-430
			if (!ray_stream.termination.test(ID)) continue;
			const uint32_t px = in->pixelID[ID];
			out_r[px] += in->radiance.r[ID];
			out_g[px] += in->radiance.g[ID];
			out_b[px] += in->radiance.b[ID];
			lc.terminated++;
		}
		active_rays = output_index;                                              // :431
	}
}

static void accumulate_brdf(Oracle& o, const GgxParams& g) {                      // the oracle's accumulate(), Renderer.hpp:73-75,433
	++o.accumulations;
	const uint32_t tiles = o.tile_list.empty() ? o.h_tiles * o.v_tiles : static_cast<uint32_t>(o.tile_list.size());
	int nthreads = o.threads > 0 ? o.threads : static_cast<int>(std::thread::hardware_concurrency());
	if (nthreads < 1) nthreads = 1;
	if (static_cast<uint32_t>(nthreads) > tiles) nthreads = static_cast<int>(tiles ? tiles : 1);
	std::atomic<uint32_t> next{0};
	auto worker = [&]() {
		LocalCounters lc;
		for (;;) {
			uint32_t t = next.fetch_add(1);
			if (t >= tiles) break;
			accumulate_tile_brdf(o, g, o.tile_list.empty() ? t : o.tile_list[t], t, o.accumulations, o.accumulator.data(), lc);
		}
		flush(o.counters, lc);
	};
	if (nthreads == 1) { worker(); return; }
	std::vector<std::thread> pool;
	for (int i = 0; i < nthreads; i++) pool.emplace_back(worker);
	for (auto& t : pool) t.join();
}

} // namespace

extern "C" {
// n_calls x Accumulate() with the closure `brdf` (0 Lambertian, 1 GGX) and gloss decay table decay[0..n_decay)
int ggx_twin_accumulate(void* h, uint32_t n_calls, int brdf, const float* decay, uint32_t n_decay) {
	if (brdf != 0 && brdf != 1) return -1;
	GgxParams g;
	g.brdf = brdf;
	if (decay && n_decay) g.decay.assign(decay, decay + n_decay);
	Oracle& o = *static_cast<Oracle*>(h);
	for (uint32_t i = 0; i < n_calls; i++) accumulate_brdf(o, g);
	return 0;
}
} // extern "C"
