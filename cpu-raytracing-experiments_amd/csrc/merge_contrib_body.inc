// merge_contrib_body.inc — the body of k_merge_contrib and of its sparse twin (kernels.hpp), included by both with SPARSE a constant: one text, and the kernel
// without frozen tiles compiles to the instructions it has always had.  SPARSE reads tile_frozen[local tile] (mirt_freeze_tiles).
// Names it expects in scope: SPARSE (constant); accum, contrib, n_tiles, buckets, batch_n, acc_base; tile_frozen (read when SPARSE).
	constexpr uint32_t kQuads = kTileSize / 4u;                                 // 4-pixel groups per tile
	const size_t n_items = static_cast<size_t>(n_tiles) * kQuads;
	const uint32_t first = min(buckets, batch_n);
	for (size_t item = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; item < n_items; item += static_cast<size_t>(gridDim.x) * kBlock) {
		const size_t tile = item / kQuads; const uint32_t q = static_cast<uint32_t>(item % kQuads);
		if (SPARSE && tile_frozen[tile] != 0u) continue;
		for (uint32_t k0 = 0; k0 < first; k0++) {
			const uint32_t bucket = (acc_base + k0 + 1u) % buckets;
			float4* dst = accum + (tile * buckets + bucket) * 3u * kQuads + q;  // channel c of the 4 pixels: dst[c * kQuads]
			float4 r = dst[0], g = dst[kQuads], b = dst[2u * kQuads];
			for (uint32_t k = k0; k < batch_n; k += buckets) {
				const float4* src = contrib + ((tile * batch_n + k) * kQuads + q) * 3u;
				const float4 c0 = src[0], c1 = src[1], c2 = src[2];                // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
				r.x += c0.x; g.x += c0.y; b.x += c0.z;
				r.y += c0.w; g.y += c1.x; b.y += c1.y;
				r.z += c1.z; g.z += c1.w; b.z += c2.x;
				r.w += c2.y; g.w += c2.z; b.w += c2.w;
			}
			dst[0] = r; dst[kQuads] = g; dst[2u * kQuads] = b;
		}
	}
