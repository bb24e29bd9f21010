// primary_hits_wave_body.inc — the body of k_primary_hits_wave and of its sparse twin (kernels.hpp), included by both with SPARSE a constant: one text, and the kernel
// without frozen tiles compiles to the instructions it has always had.  SPARSE reads tile_frozen[local tile] (mirt_freeze_tiles).
// Names it expects in scope: COUNT, SPARSE (constants); sc, fp, cand, hit_out, ctr; tile_frozen and active_pix (read when SPARSE).
	__shared__ HitRec stage[kWaveHitsWaves][kWaveHitsStage];
	const uint32_t lane = lane_id();
	const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
	const uint32_t n_runs = fp.n_pix / kWaveHitsRun, n_groups = hits_wave_groups(fp.batch_n);
	const uint32_t out_p = hits_wave_out_pixel(lane);                              // write-out: this lane's pixel of the run
	uint32_t c_spheres = 0;
	const float ox = fp.cam.pos[0], oy = fp.cam.pos[1], oz = fp.cam.pos[2];
	for (uint32_t run = blockIdx.x * kWaveHitsWaves + wave; run < n_runs; run += gridDim.x * kWaveHitsWaves) {
		const uint32_t base = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(run * kWaveHitsRun)));     // first local pixel of the run: wave-uniform
		if (SPARSE && tile_frozen[base >> 8] != 0u) continue;
		const uint32_t cnt_v = cand[base + out_p];                                   // lane p (and p + 16, ...): the count of pixel p of the run
		const uint32_t skip = static_cast<uint32_t>(__ballot(cnt_v == kCandOverflow)) & 0xffffu;      // pixels without a list: k_trace<kPrimaryList> writes their records
		if (skip == 0xffffu) continue;
		uint32_t tile; int32_t x0, y;
		pixel_xy(fp, base, tile, x0, y);                                             // the run's pixels: (x0 + p, y), ID = (base & 255) + p
		const uint32_t seed0 = tile * kTileSize + (base & 255u), seed_mul = fp.max_bounces * 2u + 1u;
		auto count_of = [&](uint32_t p) { return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(cnt_v), static_cast<int>(p))) + 1u; };   // entries + 1; 0 without a list
		// Lane k's entry of pixel p's list, and that sphere.  Every lane loads, whatever the list's length — the lanes beyond it read the last entry
		// again (the count word of an empty list) and sphere 0, and nobody reads what they hold: with loads that some lanes or some passes skip, the
		// in-order load counter would have to be waited down to zero before the tests, with the next pixel's loads just issued.
		auto load_ids = [&](uint32_t p) { const uint32_t c1 = count_of(p); return cand[static_cast<size_t>(min(lane + 1u, c1 ? c1 - 1u : 0u)) * fp.n_pix + base + p]; };
		auto load_sphere = [&](uint32_t p, uint32_t j) { return sc.spheres[lane + 1u < count_of(p) ? j : 0u]; };
		for (uint32_t g = 0; g < n_groups; g++) {
			const uint32_t slot = g * 64u + lane;                                     // lanes beyond batch_n compute a ray nobody stores
			uint32_t id_cur = load_ids(0), id_next = load_ids(1);
			float4 s_cur = load_sphere(0, id_cur);
			for (uint32_t p = 0; p < kWaveHitsRun; p++) {
				// the sphere of pixel p + 1 and the list entry of pixel p + 2 (the run's last pixel again beyond it): in flight during the tests of pixel p
				const float4 s_next = load_sphere(min(p + 1u, kWaveHitsRun - 1u), id_next);
				const uint32_t id_next2 = load_ids(min(p + 2u, kWaveHitsRun - 1u));
				const uint32_t cnt1 = count_of(p);
				if (cnt1 != 0u) {
					const uint32_t cnt = cnt1 - 1u;
					uint32_t rng = hash_2d(fp.acc_base + slot + 1u, (seed0 + p) * seed_mul);      // mirrors camera_sample(.., tile_seed(fp, tile, (base & 255) + p)), Renderer.hpp:74,107,117
					const float s0 = rand_unit_float(rng);
					const float s1 = rand_unit_float(rng);
					const f3 d = camera_ray_dir(fp.cam, x0 + static_cast<int32_t>(p), y, s0, s1);
					float tfar = MIRT_FLT_MAX; int32_t prim = -1;                          // hit reset, Renderer.hpp:150-158
					for (uint32_t k = 0; k < cnt; k++) {
						const int32_t j = __builtin_amdgcn_readlane(static_cast<int>(id_cur), static_cast<int>(k));
						const float4 s{ __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s_cur.x), static_cast<int>(k))), __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s_cur.y), static_cast<int>(k))),
						                __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s_cur.z), static_cast<int>(k))), __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s_cur.w), static_cast<int>(k))) };
						sphere_closest_tie(s, j, ox, oy, oz, d.x, d.y, d.z, tfar, prim);
					}
					if (COUNT && slot < fp.batch_n) c_spheres += cnt;
					stage[wave][hits_wave_stage_index(p, lane)] = HitRec{ tfar, prim };
				}
				id_cur = id_next; id_next = id_next2; s_cur = s_next;
			}
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
			const uint32_t n_slots = hits_wave_group_slots(fp.batch_n, g);
			if (!((skip >> out_p) & 1u)) {
				for (uint32_t pass = 0; pass < kWaveHitsPasses; pass++) {
					const uint32_t s = hits_wave_out_slot(lane, pass);
					if (s >= n_slots) break;
					hit_out[static_cast<size_t>(g * 64u + s) * fp.n_pix + base + out_p] = stage[wave][hits_wave_stage_index(out_p, s)];
				}
			}
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
		}
	}
	if (COUNT) wave_sum(c_spheres, &ctr->spheres);
	if (blockIdx.x == 0 && threadIdx.x == 0 && fp.n_pix) atomicAdd(&ctr->rays, static_cast<unsigned long long>(SPARSE ? active_pix : fp.n_pix) * fp.batch_n);     // Renderer.hpp:165: every camera ray of the batch
