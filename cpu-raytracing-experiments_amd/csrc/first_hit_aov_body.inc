// first_hit_aov_body.inc — the body of k_first_hit_aov and of its sparse twin (kernels.hpp), included by both with SPARSE a constant: one text, and the kernel
// without frozen tiles compiles to the instructions it has always had.  SPARSE reads tile_frozen[local tile] (mirt_freeze_tiles).
// Names it expects in scope: LENS, SPARSE (constants); sc, fp, hit_in, mat_colour, aov, lens; tile_frozen (read when SPARSE).
	f3 O{ fp.cam.pos[0], fp.cam.pos[1], fp.cam.pos[2] };
	for (uint32_t pix = blockIdx.x * kBlock + threadIdx.x; pix < fp.n_pix; pix += gridDim.x * kBlock) {
		if (SPARSE && tile_frozen[pix >> 8] != 0u) continue;
		uint32_t tile; int32_t x, y;
		pixel_xy(fp, pix, tile, x, y);
		const uint32_t seed = tile_seed(fp, tile, pix & 255u);
		float* w = aov + static_cast<size_t>(pix >> 8) * (kAovPlanes * kTileSize) + (pix & 255u);
		float sum[kAovPlanes];
		for (uint32_t k = 0; k < kAovPlanes; k++) sum[k] = w[k * kTileSize];
		int32_t cached = -1;
		float4 hs = make_float4(0.0f, 0.0f, 0.0f, 0.0f), colour = hs;
		for (uint32_t slot = 0; slot < fp.batch_n; slot++) {
			f3 D;
			camera_ray<LENS>(fp, lens, x, y, fp.acc_base + slot + 1u, seed, O, D);
			const HitRec h = hit_in[static_cast<size_t>(slot) * fp.n_pix + pix];
			if (h.prim < 0) { sum[0] += kAovMissDepth; continue; }
			if (h.prim != cached) { hs = sc.spheres[h.prim]; colour = mat_colour[sc.prim_mat[h.prim]]; cached = h.prim; }
			const float depth = h.tfar;
			const f3 hit{ O.x + D.x * depth, O.y + D.y * depth, O.z + D.z * depth };      // mirrors shade_hit_body.inc's hit and N, Renderer.hpp:169-214
			f3 N = normalize3(f3{ hit.x - hs.x, hit.y - hs.y, hit.z - hs.z });
			if (dot3(N, D) >= 0.0f) N = f3{ -N.x, -N.y, -N.z };
			sum[0] += depth;
			sum[1] += N.x; sum[2] += N.y; sum[3] += N.z;
			sum[4] += colour.x; sum[5] += colour.y; sum[6] += colour.z;
		}
		for (uint32_t k = 0; k < kAovPlanes; k++) w[k * kTileSize] = sum[k];
	}
