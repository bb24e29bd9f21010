// The body of k_shade's two overloads (kernels.hpp, "Block-iterations"): phase 1 over the rays of a block-iteration, the regrouping of the hits, phase 2
// (shade_hit_body.inc) and the compaction into the next stream and the shadow queue.  Included as statements by both kernels; names the template
// arguments FIRST .. PDF and the kernel arguments of MIRT_SHADE_PARAMS.
	const QueueView qin = FIRST ? queue_identity(fp.n_pix * fp.batch_n) : queue_view(in_queue);
	const uint32_t n = qin.pre[kSegs];
	const uint32_t n_chunks = (fp.n_pix + kShadeBlock - 1u) / kShadeBlock;      // FIRST
	const bool last_bounce = !(bounce < fp.max_bounces - 1u);                 // Renderer.hpp:358
	const float light_selection_pdf = 1.0f / static_cast<float>(SKY ? fp.n_lights + 1u : fp.n_lights);  // Renderer.hpp:78 (SKY: the sky is one more light)
	__shared__ uint32_t append_scratch[72];
	__shared__ uint32_t compact_scratch[17];
	__shared__ uint32_t hit_list[kShadeBlock];
	__shared__ float4 s_albedo[MIRT_MAX_MATERIALS + 1], s_emission[MIRT_MAX_MATERIALS + 1];      // scene.material: 2 KB, read by every hit (GGX: s_albedo = {F0, roughness})
	__shared__ float4 s_glass[GLASS ? MIRT_MAX_MATERIALS + 1 : 1];                             // GLASS only (no instruction of the others names it: they get no LDS for it)
	__shared__ float4 s_ggx[MIXED ? MIRT_MAX_MATERIALS + 1 : 1];                               // MIXED only, likewise: {F0, roughness} beside s_albedo = {albedo}
	uint32_t c_term = 0, c_drop = 0, parity = 0;
	const uint32_t n_units = n_chunks * fp.first_groups;                       // FIRST: pieces of work = (chunk, group of accumulations)
	if (FIRST ? blockIdx.x >= n_units : blockIdx.x * kShadeBlock >= n) return;
	for (uint32_t m = threadIdx.x; m < sc.n_mat; m += kShadeBlock) { s_albedo[m] = GGX ? mat_ggx[m] : sc.mat_albedo[m]; s_emission[m] = sc.mat_emission[m]; if (GLASS) s_glass[m] = sc.mat_glass[m]; if (MIXED) s_ggx[m] = mat_ggx[m]; }
	__syncthreads();            // the table is read by every wave in phase 2; k_shade<FIRST> reaches no other barrier before that (the early return above is block-uniform)

	// !FIRST: this lane's ray of the stream for the block-iteration at hand, and its hit record: requested one iteration ahead, so that the
	// first of the iteration's three dependent memory round trips is already under way
	uint32_t next_slot = 0u; int32_t next_prim = -1;
	if (!FIRST) {
		next_slot = (blockIdx.x * kShadeBlock + threadIdx.x < n) ? queue_slot(qin, blockIdx.x * kShadeBlock, blockIdx.x * kShadeBlock + threadIdx.x) : 0u;
		next_prim = hit_in[next_slot].prim;
	}
	// FIRST: the pixel of this lane in the chunk at hand, and what depends on it alone
	uint32_t unit = blockIdx.x, chunk = 0u, slot_it = 0u, slot_end = 0u, pix = 0u, pix_seed = 0u;
	int32_t pix_x = 0, pix_y = 0;
	bool pix_frozen = false;                                                  // SPARSE
	for (uint32_t base = blockIdx.x * kShadeBlock; FIRST ? unit < n_units : base < n; parity ^= 1u) {
		const bool new_unit = FIRST && slot_it == slot_end;                    // wave-uniform
		if (new_unit) {
			chunk = unit / fp.first_groups;
			const uint32_t g = unit - chunk * fp.first_groups;
			slot_it = g * fp.batch_n / fp.first_groups; slot_end = (g + 1u) * fp.batch_n / fp.first_groups;
		}
		const uint32_t iteration = FIRST ? chunk * fp.batch_n + slot_it : base / kShadeBlock;     // FIRST: every (chunk, slot) exactly once
		// ---- phase 1, one lane per ray of the stream: misses end here; hits are only listed ----
		bool is_hit = false;
		uint32_t my_slot = next_slot;
		int32_t my_prim = next_prim;
		float my_tfar = 0.0f;
		f3 my_D{0, 0, 0};
		f3 my_O{0, 0, 0};                                                       // LENS: the sample's point on the lens
		uint32_t my_path = 0u;
		bool lane_on;
		f3 W0{0.0f, 0.0f, 0.0f};                                               // FIRST: the word this path starts with
		if (FIRST) {
			if (new_unit) {                                                      // a new chunk of pixels
				pix = chunk * kShadeBlock + threadIdx.x;
				if (pix < fp.n_pix) {
					uint32_t tile;
					pixel_xy(fp, pix, tile, pix_x, pix_y);
					pix_seed = tile_seed(fp, tile, pix & 255u);
					if (SPARSE) pix_frozen = tile_frozen[pix >> 8] != 0u;
				}
			}
			lane_on = pix < fp.n_pix;
			if (SPARSE) lane_on = lane_on && !pix_frozen;
			my_slot = slot_it * fp.n_pix + pix;                                 // the ray's index in the batch = where k_trace stored a hit record for it
			if (lane_on) {
				// RAY GENERATION, Renderer.hpp:113-127 (primary_ray with the pixel's part taken from the chunk set-up); the two lines mirror camera_ray<LENS>
				my_D = camera_sample(fp.cam, pix_x, pix_y, fp.acc_base + slot_it + 1u, pix_seed);
				if (LENS) lens_ray(fp.cam, lens, my_D, fp.acc_base + slot_it + 1u, pix_seed, fp.max_bounces, my_O, my_D);
				my_path = (slot_it << fp.pix_bits) | pix;
				{ const HitRec h = hit_in[my_slot]; my_prim = h.prim; my_tfar = h.tfar; }      // the hit record of k_primary_hits / k_trace
			}
			if (++slot_it == slot_end) unit += gridDim.x;
		} else {
			lane_on = base + threadIdx.x < n;
			const uint32_t nb = base + gridDim.x * kShadeBlock;
			next_slot = (nb + threadIdx.x < n) ? queue_slot(qin, nb, nb + threadIdx.x) : 0u;
			next_prim = hit_in[next_slot].prim;
			base = nb;
		}
		{
			if (lane_on) {
				const uint32_t i = my_slot;
				const int32_t prim = my_prim;
				if (prim < 0) {
					// MISS SHADER, Renderer.hpp:408-420 (Q10: throughput.r scales all three channels).  Without ambient light the path just
					// ends: its word holds its result already (ACCUMULATION, Renderer.hpp:424-430, is k_merge_contrib's)
					if (sc.has_ambient) {
						if (FIRST) {
							const f3 env = sky_eval(sc, my_D.x, my_D.y, my_D.z);
							W0 = { 0.0f + 1.0f * env.x, 0.0f + 1.0f * env.y, 0.0f + 1.0f * env.z };
						} else {
							const float4 b = in.b[i];                                      // {dir, throughput.r}
							const float thr_x = SKY ? b.w * in.w[i] : b.w;                 // SKY: the MIS weight of this direction against the sky's own sampling
							const f3 env = sky_eval(sc, b.x, b.y, b.z);
							float* w = contrib + contrib_index(fp.batch_n, fp.pix_bits, __float_as_uint(in.a[i].w) & ((GLASS || MIXED) ? kDestPath : ~0u));
							w[0] += thr_x * env.x; w[1] += thr_x * env.y; w[2] += thr_x * env.z;
						}
					}
					c_term++;
				} else if (last_bounce) {
					c_drop++;                                                         // Q5: still alive after the last bounce -> never accumulated: the word goes back to +0
					if (!FIRST) {                                                     // (FIRST: W0 is +0)
						float* w = contrib + contrib_index(fp.batch_n, fp.pix_bits, __float_as_uint(in.a[i].w) & ((GLASS || MIXED) ? kDestPath : ~0u));
						w[0] = 0.0f; w[1] = 0.0f; w[2] = 0.0f;
					}
				} else is_hit = true;
			}
		}
		// ---- regroup: the closest-hit shader is ~800 VALU instructions per ray and only 40-60 % of a secondary stream hits;
		// packing the hits of the block into its first waves runs that code on full waves (lane utilisation 0.42 -> ~0.9) ----
		// (Not for primary rays: ~95 % of them hit, the stream is already dense, and the two barriers cost more than they save.)
		const uint32_t n_hits = FIRST ? 0u : block_compact(is_hit, my_slot, compact_scratch, hit_list);

		// ---- phase 2, one lane per hit ----
		bool survive = false, has_shadow = false, terminated = false, has_E = false;
		bool via_interface = false;                                            // GLASS
		bool sampled_ggx = false;                                              // MIXED
		float miss_w = 1.0f;                                                   // SKY
		float pdf_out = 0.0f;                                                  // PDF
		uint32_t path = 0;
		f3 P{0, 0, 0}, ndir{0, 0, 0}, L{0, 0, 0}, srad{0, 0, 0}, E{0, 0, 0};
		f3 thr{1.0f, 1.0f, 1.0f};
		float light_distance = 0.0f;
		if (FIRST ? is_hit : threadIdx.x < n_hits) {
			const uint32_t i = FIRST ? my_slot : hit_list[threadIdx.x];
			f3 D = my_D;                                                       // bounce 0 has no stream: the ray is a function of its index (phase 1)
			path = my_path;
			f3 O_in{0, 0, 0};
			float pdf_in = 0.0f;
			bool after_interface = false;                                      // GLASS
			bool after_ggx = GGX;                                              // MIXED: D was sampled by Closure<GGX> (kSampledGGX); otherwise every D was, or none
			if (!FIRST) {                                                      // the ray's three records
				const float4 a = in.a[i], b = in.b[i];
				const float2 c = in.c[i];
				O_in = { a.x, a.y, a.z }; path = __float_as_uint(a.w);
				if (MIXED) after_ggx = (path & kSampledGGX) != 0u;
				if (GLASS) after_interface = (path & kViaInterface) != 0u;
				if (GLASS || MIXED) path &= kDestPath;
				D = { b.x, b.y, b.z };
				thr = { b.w, c.x, c.y };
				pdf_in = after_ggx ? 0.0f : MIRT_INV_PI * max_sel(0.0f, D.z);     // out->pdf of the bounce that sampled D (Q8), bit for bit; Closure<GGX>::pdf = 0
				if (PDF) pdf_in = pdf_plane_in[i];                                       // ... unless the sampling bounce stored it (mirt_set_ggx_pdf)
			}
			const HitRec hrec = FIRST ? HitRec{ my_tfar, my_prim } : hit_in[i];
			const int32_t prim = hrec.prim;
			{
#define SHADE_HIT_ORIGIN (FIRST ? (LENS ? my_O : f3{ fp.cam.pos[0], fp.cam.pos[1], fp.cam.pos[2] }) : O_in)
#define SHADE_HIT_ACC (fp.acc_base + (path >> fp.pix_bits) + 1u)
#define SHADE_HIT_SEED (FIRST ? pix_seed : path_seed(fp, path & fp.pix_mask))
#include "shade_hit_body.inc"
			}
		}
		// ---- stream compaction: wave64 ballot + mbcnt prefix inside each wave, one atomic per workgroup and stream ----
		uint32_t slot, sslot;
		block_append2(survive, has_shadow, next_queue, shadow_queue, iteration % kSegs, append_scratch, parity, slot, sslot);
		// (R + unoccluded NEE) + E is finished by k_trace's shadow_finish once the occlusion is known: an emissive hit with a light
		// record pending sends E along (kDestFull); one without adds E to the path's word here.
		const bool full = has_shadow & has_E;
		if (survive) {
			out.a[slot] = make_float4(P.x, P.y, P.z, __uint_as_float((GLASS && via_interface ? path | kViaInterface : path) | (MIXED && sampled_ggx ? kSampledGGX : 0u)));
			out.b[slot] = make_float4(ndir.x, ndir.y, ndir.z, thr.x);
			out.c[slot] = make_float2(thr.y, thr.z);
			if (SKY) out.w[slot] = miss_w;
			if (PDF) pdf_plane_out[slot] = pdf_out;
		}
		if (has_shadow) {
			// the record holds its own ray and its path id (kernels.hpp ShadowBuf): k_trace reads nothing of the surviving ray
			sh.a[sslot] = make_float4(P.x, P.y, P.z, light_distance);
			sh.b[sslot] = make_float4(L.x, L.y, L.z, __uint_as_float(path | (survive ? 0u : kDestAccum) | (full ? kDestFull : 0u)));
			sh.c[sslot] = make_float4(srad.x, srad.y, srad.z, 0.0f);
			if (full) sh.d[sslot] = make_float4(E.x, E.y, E.z, 0.0f);
		}
		if (has_E & !has_shadow) {
			if (FIRST) W0 = { 0.0f + E.x, 0.0f + E.y, 0.0f + E.z };
			else {
				float* w = contrib + contrib_index(fp.batch_n, fp.pix_bits, path);
				w[0] += E.x; w[1] += E.y; w[2] += E.z;
			}
		}
		// FIRST is pixel-major — this iteration's lanes are 512 consecutive pixels of one slot, i.e. two contiguous 3-KB runs of the buffer
		if (FIRST && lane_on) {
			float* w = contrib + contrib_index(fp.batch_n, fp.pix_bits, my_path);
			w[0] = W0.x; w[1] = W0.y; w[2] = W0.z;
		}
		c_term += (terminated && !has_shadow) ? 1u : 0u;
	}
	wave_sum(c_term, &ctr->terminated);
	wave_sum(c_drop, &ctr->dropped);
