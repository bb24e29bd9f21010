// VARIANCE-GUIDED A-TROUS RESOLVE — mirt_render_atrous (mirt.h, "variance-guided à-trous denoised resolve": the definition, step by step).
// Three kernels, all binary32 with one rounding per operation in the order mirt.h states (-ffp-contract=off; IEEE division and square root):
//   k_denoise_prepare   steps 1-5: one 256-thread workgroup per tile, lane = pixel ID — the coalesced plane reads of k_resolve and k_noise —
//                       writing three row-major full-image float4 buffers through TileMap::pixel_offset:
//                       cv = (x_r, x_g, x_b, v), gd = (N.x, N.y, N.z, z), mu = (m_r, m_g, m_b, usable).
//   k_atrous<STAGED>    step 6, one pass: one 16 x 16 pixel block per workgroup, reads cv (A) and gd, writes cv (B).
//   k_denoise_finish    step 7: x * m, tonemapping, A = 1 into the float4 frame.
// HOW USABILITY TRAVELS: it is decided once, in step 5, and never changes.  An unusable pixel is stored with z = NaN in gd (z is finite for
// every usable pixel, and nobody reads the z of an unusable one), cv = (s_r, s_g, s_b, -1) and mu = (1, 1, 1, 0): a tap is usable when its
// gd.w equals itself, every pass copies an unusable centre unchanged, and the finish forms s * 1 = s, the word mirt_render tonemaps.  The
// same test skips a tap outside the image in the staged variant, whose halo is filled with z = NaN there.
// STAGED (steps 1 and 2): neighbouring lanes share most taps, so the block and its halo of 2 * step pixels are staged in LDS — 32 B per
// pixel, (16 + 8)^2 x 32 B = 18 KB at step 2.  From step 4 on the 25 taps of a block are 25 disjoint 16 x 16 blocks, each tap one coalesced
// row-segment load per wave: read straight from global memory.  Both variants evaluate the same text, fetch() aside, so they give the same words
// (which of them runs is a launch choice: profiles/denoise.txt).
#pragma once
#include "resolve.hpp"

#include <float.h>

namespace mirt {

struct DenoiseDev { float sigma_lum, sigma_depth, lum_floor; uint32_t normal_squarings; };

// kAtrousBlock (pixels a side: a tile of the image) and kAtrousStagedMaxStep: kernel_types.hpp, where the context reads its default from
constexpr uint32_t kAtrousStagedSide = kAtrousBlock + 4u * kAtrousStagedMaxStep;    // block + 2 * step of halo on either side

MIRT_DI bool dn_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }
MIRT_DI bool dn_usable(const float4& g) { return g.w == g.w; }
MIRT_DI float dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

__global__ __launch_bounds__(kTileSize) void k_denoise_prepare(const float* __restrict__ accum, const float* __restrict__ aov, float4* __restrict__ cv, float4* __restrict__ gd,
                                                               float4* __restrict__ mu, TileMap tiles, uint32_t buckets, float scale_all, float count_all,
                                                               const uint32_t* __restrict__ tile_counts, float exposure, uint32_t demodulate, float albedo_floor) {
	const uint32_t local = blockIdx.x, ID = threadIdx.x;
	const float scale = tile_counts ? exposure / static_cast<float>(tile_counts[local] / buckets) : scale_all;     // k_resolve's
	const float count = tile_counts ? static_cast<float>(tile_counts[local]) : count_all;                         // k_resolve_aov's
	const float* src = accum + static_cast<size_t>(local) * buckets * 3u * kTileSize + ID;
	float ch[3][kNoiseMaxBuckets];
	float sum = 0.0f;
	float y[kNoiseMaxBuckets];
	for (uint32_t j = 0; j < kNoiseMaxBuckets; j++) if (j < buckets) {
		for (uint32_t c = 0; c < 3; c++) ch[c][j] = src[(static_cast<size_t>(j) * 3u + c) * kTileSize];
		y[j] = scale * dn_lum(ch[0][j], ch[1][j], ch[2][j]);                   // 2. variance: y_j, mean, var of mirt_noise
		sum = j ? sum + y[j] : y[j];
	}
	const float mean = sum / static_cast<float>(buckets);
	float ss = 0.0f;
	for (uint32_t j = 0; j < kNoiseMaxBuckets; j++) if (j < buckets) {
		const float d = y[j] - mean;
		ss = j ? ss + d * d : d * d;
	}
	const float var = ss / static_cast<float>(buckets - 1u);
	float v = var / static_cast<float>(buckets);
	float s[3];
	for (uint32_t c = 0; c < 3; c++) s[c] = scale * median_k(ch[c], buckets);     // 1. signal: k_resolve's operations before tonemapping
	const float* a = aov + static_cast<size_t>(local) * (kAovPlanes * kTileSize) + ID;   // 3. guides: mirt_render_aov's three outputs
	const float z = a[0] / count;
	f3 N{ a[kTileSize], a[2u * kTileSize], a[3u * kTileSize] };
	N = dot3(N, N) == 0.0f ? f3{ 0.0f, 0.0f, 0.0f } : normalize3(N);
	float m[3], x[3];
	for (uint32_t c = 0; c < 3; c++) {                                              // 4. modulator
		const float alb = a[(4u + c) * kTileSize] / count;
		m[c] = (demodulate && alb >= albedo_floor) ? alb : 1.0f;
		x[c] = s[c] / m[c];
	}
	const float lm = dn_lum(m[0], m[1], m[2]);
	v = v / (lm * lm);
	const bool usable = dn_finite(x[0]) && dn_finite(x[1]) && dn_finite(x[2]) && dn_finite(v) && dn_finite(z) && dn_finite(N.x) && dn_finite(N.y) && dn_finite(N.z)
	                    && v >= 0.0f;                                               // 5. usability
	const size_t at = tiles.pixel_offset(local, ID, 1u);
	if (usable) {
		cv[at] = make_float4(x[0], x[1], x[2], v);
		gd[at] = make_float4(N.x, N.y, N.z, z);
		mu[at] = make_float4(m[0], m[1], m[2], 1.0f);
	} else {
		cv[at] = make_float4(s[0], s[1], s[2], -1.0f);
		gd[at] = make_float4(N.x, N.y, N.z, __uint_as_float(0x7fc00000u));
		mu[at] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
	}
}

// One pass at `step`.  The image is w_img x h_img pixels (whole tiles) in rows of `width` float4; the grid is its 16 x 16 blocks.
template <bool STAGED>
__global__ __launch_bounds__(kAtrousBlock * kAtrousBlock) void k_atrous(const float4* __restrict__ cv_in, const float4* __restrict__ gd, float4* __restrict__ cv_out,
                                                                        uint32_t width, uint32_t w_img, uint32_t h_img, uint32_t step, DenoiseDev p) {
	__shared__ float4 s_cv[STAGED ? kAtrousStagedSide * kAtrousStagedSide : 1u], s_gd[STAGED ? kAtrousStagedSide * kAtrousStagedSide : 1u];
	if (STAGED && step > kAtrousStagedMaxStep) return;                              // (uniform) the halo would not fit
	const uint32_t lx = threadIdx.x & 15u, ly = threadIdx.x >> 4;
	const int32_t x = static_cast<int32_t>(blockIdx.x * kAtrousBlock + lx), y = static_cast<int32_t>(blockIdx.y * kAtrousBlock + ly);
	const uint32_t halo = 2u * step, side = kAtrousBlock + 2u * halo;
	if (STAGED) {
		const int32_t x0 = static_cast<int32_t>(blockIdx.x * kAtrousBlock) - static_cast<int32_t>(halo), y0 = static_cast<int32_t>(blockIdx.y * kAtrousBlock) - static_cast<int32_t>(halo);
		for (uint32_t i = threadIdx.x; i < side * side; i += kAtrousBlock * kAtrousBlock) {
			const int32_t qx = x0 + static_cast<int32_t>(i % side), qy = y0 + static_cast<int32_t>(i / side);
			const bool inside = qx >= 0 && qy >= 0 && qx < static_cast<int32_t>(w_img) && qy < static_cast<int32_t>(h_img);
			const size_t q = static_cast<size_t>(inside ? qy : 0) * width + static_cast<size_t>(inside ? qx : 0);
			s_gd[i] = inside ? gd[q] : make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0x7fc00000u));
			s_cv[i] = inside ? cv_in[q] : make_float4(0.0f, 0.0f, 0.0f, -1.0f);
		}
		__syncthreads();
	}
	// The tap at (dx, dy) PIXELS from the centre: false when it lies outside the image or is unusable.
	auto fetch = [&](int32_t dx, int32_t dy, float4& c, float4& g) -> bool {
		if (STAGED) {
			const uint32_t i = static_cast<uint32_t>(static_cast<int32_t>(ly + halo) + dy) * side + static_cast<uint32_t>(static_cast<int32_t>(lx + halo) + dx);
			g = s_gd[i];
			if (!dn_usable(g)) return false;
			c = s_cv[i];
			return true;
		}
		const int32_t qx = x + dx, qy = y + dy;
		if (qx < 0 || qy < 0 || qx >= static_cast<int32_t>(w_img) || qy >= static_cast<int32_t>(h_img)) return false;
		const size_t q = static_cast<size_t>(qy) * width + static_cast<size_t>(qx);
		g = gd[q];
		if (!dn_usable(g)) return false;
		c = cv_in[q];
		return true;
	};
	const size_t at = static_cast<size_t>(y) * width + static_cast<size_t>(x);
	float4 cp, gp;
	if (!fetch(0, 0, cp, gp)) { cv_out[at] = cv_in[at]; return; }                  // an unusable centre passes through
	// smoothed variance: 3 x 3 at distance 1, whatever the step, over the neighbours whose normal does not turn away (variance does not cross a crease)
	const bool p_zero = gp.x == 0.0f && gp.y == 0.0f && gp.z == 0.0f;
	float G = 0.0f, K = 0.0f;
	bool first = true;
	for (int32_t dy = -1; dy <= 1; dy++)
		for (int32_t dx = -1; dx <= 1; dx++) {
			float4 c, g;
			if (!fetch(dx, dy, c, g)) continue;
			if (dx != 0 || dy != 0) {
				const bool both_zero = p_zero && g.x == 0.0f && g.y == 0.0f && g.z == 0.0f;
				if (!both_zero && !((gp.x * g.x + gp.y * g.y) + gp.z * g.z > 0.0f)) continue;
			}
			const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);      // 1/16 1/8 1/16; 1/8 1/4 1/8; 1/16 1/8 1/16
			const float kv = k * c.w;
			G = first ? kv : G + kv;
			K = first ? k : K + k;
			first = false;
		}
	const float gv = G / K;
	const float sd = p.sigma_lum * __builtin_sqrtf(gv) + p.lum_floor;
	const float l_p = dn_lum(cp.x, cp.y, cp.z);
	float W = 0.0f, X[3] = { 0.0f, 0.0f, 0.0f }, V = 0.0f;
	first = true;
#pragma unroll
	for (int32_t dy = -2; dy <= 2; dy++) {
#pragma unroll
		for (int32_t dx = -2; dx <= 2; dx++) {
			float4 c, g;
			float w;
			if (dx == 0 && dy == 0) { c = cp; w = 0.140625f; }                          // 9/64
			else {
				if (!fetch(dx * static_cast<int32_t>(step), dy * static_cast<int32_t>(step), c, g)) continue;
				const float hy = dy == 0 ? 0.375f : ((dy == 1 || dy == -1) ? 0.25f : 0.0625f), hx = dx == 0 ? 0.375f : ((dx == 1 || dx == -1) ? 0.25f : 0.0625f);
				float wn = 1.0f;
				if (!(p_zero && g.x == 0.0f && g.y == 0.0f && g.z == 0.0f)) {
					const float nn = (gp.x * g.x + gp.y * g.y) + gp.z * g.z;
					wn = nn > 0.0f ? nn : 0.0f;
					for (uint32_t q = 0; q < p.normal_squarings; q++) wn = wn * wn;
				}
				const int32_t ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
				const float dist = static_cast<float>(step * static_cast<uint32_t>(ax > ay ? ax : ay));
				const float tz = __builtin_fabsf(gp.w - g.w) / (p.sigma_depth * ((gp.w < g.w ? g.w : gp.w) * dist) + FLT_MIN);
				const float tl = __builtin_fabsf(l_p - dn_lum(c.x, c.y, c.z)) / sd;
				w = (((hy * hx) * wn) * (1.0f / (1.0f + tz * tz))) * (1.0f / (1.0f + tl * tl));
			}
			const float ww = w * w;
			W = first ? w : W + w;
			X[0] = first ? w * c.x : X[0] + w * c.x;
			X[1] = first ? w * c.y : X[1] + w * c.y;
			X[2] = first ? w * c.z : X[2] + w * c.z;
			V = first ? ww * c.w : V + ww * c.w;
			first = false;
		}
	}
	cv_out[at] = make_float4(X[0] / W, X[1] / W, X[2] / W, V / (W * W));
}

__global__ __launch_bounds__(kBlock) void k_denoise_finish(const float4* __restrict__ cv, const float4* __restrict__ mu, float4* __restrict__ fb, uint32_t n_pix, TileMap tiles) {
	for (uint32_t pix = blockIdx.x * kBlock + threadIdx.x; pix < n_pix; pix += gridDim.x * kBlock) {
		const size_t at = tiles.pixel_offset(pix >> 8, pix & 255u, 1u);
		const float4 c = cv[at], m = mu[at];
		float r = c.x * m.x, g = c.y * m.y, b = c.z * m.z;
		tonemapping(r, g, b);
		fb[at] = make_float4(r, g, b, 1.0f);
	}
}

}  // namespace mirt
