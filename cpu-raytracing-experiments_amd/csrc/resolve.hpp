// resolve.hpp — the kernels that read a finished accumulator or AOV slab and never run inside a batch: k_resolve_aov (mirt_render_aov), k_resolve
// (mirt_render) and k_noise (mirt_noise, mirt_tile_above), with the helpers only they and the denoised resolve (denoise.hpp) use.
// Owned by mirt_resolve.hip: a header that defines a non-template __global__ function is included by exactly one .hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_math.hpp"
#include "tile_map.hpp"
#include "kernel_types.hpp"

namespace mirt {

// mirt_render_aov: one of the three outputs of the slab above, row-major over the image (row 0 = y 0), 1 (depth) or 3 floats per pixel.
// Depth and colour: sum / accumulations; normal: normalize3(sum), (0,0,0) where the sum has no length.  IEEE division and sqrt.
constexpr int kAovDepth = 0, kAovNormal = 1, kAovAlbedo = 2;
__global__ __launch_bounds__(kBlock) void k_resolve_aov(const float* __restrict__ aov, float* __restrict__ out, uint32_t n_pix, TileMap tiles, int which, float accumulations_all,
                                                           const uint32_t* __restrict__ tile_counts) {
	for (uint32_t pix = blockIdx.x * kBlock + threadIdx.x; pix < n_pix; pix += gridDim.x * kBlock) {
		const float accumulations = tile_counts ? static_cast<float>(tile_counts[pix >> 8]) : accumulations_all;     // a context with frozen tiles: each tile at its own count
		const float* src = aov + static_cast<size_t>(pix >> 8) * (kAovPlanes * kTileSize) + (pix & 255u);
		const size_t at = tiles.pixel_offset(pix >> 8, pix & 255u, 1u);
		if (which == kAovDepth) { out[at] = src[0] / accumulations; continue; }
		const uint32_t first = which == kAovNormal ? 1u : 4u;
		f3 v{ src[first * kTileSize], src[(first + 1u) * kTileSize], src[(first + 2u) * kTileSize] };
		if (which == kAovNormal) v = dot3(v, v) == 0.0f ? f3{ 0.0f, 0.0f, 0.0f } : normalize3(v);
		else v = { v.x / accumulations, v.y / accumulations, v.z / accumulations };
		out[at * 3u] = v.x; out[at * 3u + 1u] = v.y; out[at * 3u + 2u] = v.z;
	}
}

// ------------------------------------------------------------------------------------------------
// MEDIAN OF MEANS & TONEMAPPING — Renderer::Render, Renderer.hpp:436-478
// ------------------------------------------------------------------------------------------------
MIRT_DI float median_k(float* v, uint32_t k) {
	if (k == 5) return median5(v[0], v[1], v[2], v[3], v[4]);               // the reference network, Sampling.hpp:13-21
	for (uint32_t a = 1; a < k; a++) {                                      // generalisation (Q19): insertion sort
		float key = v[a]; int b = static_cast<int>(a) - 1;
		while (b >= 0 && key < v[b]) { v[b + 1] = v[b]; b--; }
		v[b + 1] = key;
	}
	return (k & 1u) ? v[k / 2] : (v[k / 2 - 1] + v[k / 2]) * 0.5f;
}
// tile_counts (NULL for a context without a frozen tile): every tile at its own sample count — scale = exposure / (float)(count / buckets), the
// binary32 operations the host forms scale_all with.  The same in k_noise and k_resolve_aov.
__global__ __launch_bounds__(kBlock) void k_resolve(const float* __restrict__ accum, float4* __restrict__ fb, uint32_t n_pix, TileMap tiles, uint32_t buckets, float scale_all,
                                                    const uint32_t* __restrict__ tile_counts, float exposure) {
	for (uint32_t pix = blockIdx.x * kBlock + threadIdx.x; pix < n_pix; pix += gridDim.x * kBlock) {
		const float scale = tile_counts ? exposure / static_cast<float>(tile_counts[pix >> 8] / buckets) : scale_all;
		const float* src = accum + static_cast<size_t>(pix >> 8) * buckets * 3u * kTileSize + (pix & 255u);
		float ch[3];
		for (uint32_t c = 0; c < 3; c++) {
			float v[16];
			for (uint32_t b = 0; b < 16; b++) if (b < buckets) v[b] = src[(static_cast<size_t>(b) * 3u + c) * kTileSize];
			ch[c] = scale * median_k(v, buckets);                               // Renderer.hpp:453-455
		}
		tonemapping(ch[0], ch[1], ch[2]);                                       // Renderer.hpp:461
		fb[tiles.pixel_offset(pix >> 8, pix & 255u, 1u)] = make_float4(ch[0], ch[1], ch[2], 1.0f);   // Renderer.hpp:447,465
	}
}

// ------------------------------------------------------------------------------------------------
// NOISE ESTIMATE — mirt_noise (mirt.h, "per-pixel noise estimate"): the relative standard error of the mean of the bucket means
// ------------------------------------------------------------------------------------------------
// One 256-thread workgroup per owned tile, lane ID = pixel ID: the coalesced plane reads of k_resolve.  Per pixel the quantity of mirt.h, one
// rounding per operation in the stated order (-ffp-contract=off; IEEE division and square root).  A pixel is usable when the word of e is
// below 0x7f800000 (finite, sign bit clear); only usable pixels enter what follows:
//   tile maximum   on the words (for non-negative floats the order of the words is the order of the values): a wave64 xor-butterfly, then
//                  the four wave partials through LDS — exact, whatever the order;
//   tile sum       FIXED ORDER: inside a wave the xor-butterfly with strides 32, 16, 8, 4, 2, 1 — at each step a lane adds its partner's
//                  partial to its own (a + b = b + a, so both lanes of a pair hold the same word), i.e. a balanced binary tree over the 64
//                  lanes with the pairs (l, l ^ 32) at its leaves; then ((w0 + w1) + w2) + w3 over the four waves; unusable pixels add +0;
//   tile record    {max, sum / count (0 when count = 0), count, 256 - count} as four floats;
//   histogram      bin = word >> 20 (< 2040 for a usable pixel): LDS uint32 atomics, then the non-zero bins are added to the 2048-word
//                  device histogram with integer atomics — integer adds, so the result does not depend on scheduling.
constexpr uint32_t kNoiseBins = 2048u;
constexpr uint32_t kNoiseUsableBelow = 0x7f800000u;
constexpr uint32_t kNoiseMaxBuckets = 16u;     // one y_j per register; mirt_noise asserts that MIRT_MAX_BUCKETS fits
__global__ __launch_bounds__(kTileSize) void k_noise(const float* __restrict__ accum, float* __restrict__ map, float4* __restrict__ tile_rec, uint32_t* __restrict__ hist,
                                                     TileMap tiles, uint32_t buckets, float scale_all, float floor_,
                                                     const uint32_t* __restrict__ tile_counts, float exposure, uint32_t* __restrict__ above, float target) {
	__shared__ uint32_t bins[kNoiseBins];
	__shared__ uint32_t w_max[kTileSize / 64u], w_cnt[kTileSize / 64u], w_above[kTileSize / 64u];
	__shared__ float w_sum[kTileSize / 64u];
	const uint32_t local = blockIdx.x, ID = threadIdx.x;
	const float scale = tile_counts ? exposure / static_cast<float>(tile_counts[local] / buckets) : scale_all;
	for (uint32_t b = ID; b < kNoiseBins; b += kTileSize) bins[b] = 0u;
	const float* src = accum + static_cast<size_t>(local) * buckets * 3u * kTileSize + ID;
	float y[kNoiseMaxBuckets];
	float sum = 0.0f;
	for (uint32_t j = 0; j < kNoiseMaxBuckets; j++) if (j < buckets) {
		const float r = src[(static_cast<size_t>(j) * 3u) * kTileSize], g = src[(static_cast<size_t>(j) * 3u + 1u) * kTileSize], b = src[(static_cast<size_t>(j) * 3u + 2u) * kTileSize];
		y[j] = scale * ((0.2126f * r + 0.7152f * g) + 0.0722f * b);
		sum = j ? sum + y[j] : y[j];
	}
	const float mean = sum / static_cast<float>(buckets);
	float ss = 0.0f;
	for (uint32_t j = 0; j < kNoiseMaxBuckets; j++) if (j < buckets) {
		const float d = y[j] - mean;
		ss = j ? ss + d * d : d * d;
	}
	const float var = ss / static_cast<float>(buckets - 1u);
	const float se = __builtin_sqrtf(var / static_cast<float>(buckets));
	const float denom = mean + floor_;
	const float e = denom == 0.0f ? 0.0f : se / denom;
	if (map) map[tiles.pixel_offset(local, ID, 1u)] = e;
	const uint32_t word = __float_as_uint(e);
	const bool usable = word < kNoiseUsableBelow;
	uint32_t m = usable ? word : 0u;
	float s = usable ? e : 0.0f;
	for (int off = 32; off > 0; off >>= 1) {
		m = max(m, static_cast<uint32_t>(__shfl_xor(static_cast<int>(m), off, 64)));
		s = s + __shfl_xor(s, off, 64);
	}
	const unsigned long long usable_m = __ballot(usable);
	const unsigned long long above_m = __ballot(usable && e > target);         // above[tile] (mirt_tile_above): usable pixels with e > target
	const uint32_t wave = ID >> 6;
	if ((ID & 63u) == 0u) { w_max[wave] = m; w_sum[wave] = s; w_cnt[wave] = static_cast<uint32_t>(__popcll(usable_m)); w_above[wave] = static_cast<uint32_t>(__popcll(above_m)); }
	__syncthreads();                                                          // bins are zero, wave partials are written
	if (usable) atomicAdd(&bins[word >> 20], 1u);
	if (ID == 0u) {
		const uint32_t t_max = max(max(w_max[0], w_max[1]), max(w_max[2], w_max[3]));
		const float t_sum = ((w_sum[0] + w_sum[1]) + w_sum[2]) + w_sum[3];
		const uint32_t n = (w_cnt[0] + w_cnt[1]) + (w_cnt[2] + w_cnt[3]);
		tile_rec[local] = make_float4(__uint_as_float(t_max), n ? t_sum / static_cast<float>(n) : 0.0f, static_cast<float>(n), static_cast<float>(kTileSize - n));
		if (above) above[local] = (w_above[0] + w_above[1]) + (w_above[2] + w_above[3]);
	}
	__syncthreads();
	for (uint32_t b = ID; b < kNoiseBins; b += kTileSize) { const uint32_t v = bins[b]; if (v) atomicAdd(&hist[b], v); }
}

} // namespace mirt
