// primary_hits_body.inc — the body of k_primary_hits and of its sparse twin (kernels.hpp), included by both with SPARSE a constant: one text, and the kernel
// without frozen tiles compiles to the instructions it has always had.  SPARSE reads tile_frozen[local tile] (mirt_freeze_tiles).
// Names it expects in scope: COUNT, SPARSE (constants); sc, fp, cand, hit_out, ctr; tile_frozen and active_pix (read when SPARSE).
	if (blockIdx.x == 0 && threadIdx.x == 0 && fp.n_pix) atomicAdd(&ctr->rays, static_cast<unsigned long long>(SPARSE ? active_pix : fp.n_pix) * fp.batch_n);     // Renderer.hpp:165: every camera ray of the batch
	uint32_t c_spheres = 0;
	const float ox = fp.cam.pos[0], oy = fp.cam.pos[1], oz = fp.cam.pos[2];
	for (uint32_t pix = blockIdx.x * kBlock + threadIdx.x; pix < fp.n_pix; pix += gridDim.x * kBlock) {
		if (SPARSE && tile_frozen[pix >> 8] != 0u) continue;
		const uint32_t cnt = cand[pix];
		if (cnt == kCandOverflow) continue;
		uint32_t tile; int32_t x, y;
		pixel_xy(fp, pix, tile, x, y);
		const uint32_t seed = tile_seed(fp, tile, pix & 255u);
		float4 s[kCandRegs]; int32_t id[kCandRegs];
		for (uint32_t k = 0; k < kCandRegs; k++) {
			id[k] = k < cnt ? static_cast<int32_t>(cand[static_cast<size_t>(k + 1u) * fp.n_pix + pix]) : -1;
			s[k] = sc.spheres[id[k] < 0 ? 0 : id[k]];
		}
		for (uint32_t slot = 0; slot < fp.batch_n; slot++) {
			const f3 d = camera_sample(fp.cam, x, y, fp.acc_base + slot + 1u, seed);
			float tfar = MIRT_FLT_MAX; int32_t prim = -1;                          // hit reset, Renderer.hpp:150-158
			for (uint32_t k = 0; k < kCandRegs; k++) if (id[k] >= 0) sphere_closest_tie(s[k], id[k], ox, oy, oz, d.x, d.y, d.z, tfar, prim);
			for (uint32_t k = kCandRegs; k < kCandMax; k++) {                      // the rest of a long list, from L1
				if (__ballot(k < cnt) == 0ull) break;
				if (k < cnt) {
					const uint32_t j = cand[static_cast<size_t>(k + 1u) * fp.n_pix + pix];
					sphere_closest_tie(sc.spheres[j], static_cast<int32_t>(j), ox, oy, oz, d.x, d.y, d.z, tfar, prim);
				}
			}
			if (COUNT) c_spheres += cnt;
			const size_t i = static_cast<size_t>(slot) * fp.n_pix + pix;
			hit_out[i] = HitRec{ tfar, prim };
		}
	}
	if (COUNT) wave_sum(c_spheres, &ctr->spheres);
