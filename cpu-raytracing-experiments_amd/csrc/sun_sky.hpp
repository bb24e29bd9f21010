// sun_sky.hpp — k_sun_sky: the Preetham sky and the sun disc of mirt_set_sun_sky, baked straight into the context's environment map.
// The definition is in include/mirt.h ("analytic sun and sky"), step by step in binary32; float64 statement: tests/sun_sky_definitions.py; numpy
// twin in this operation order: sun_sky_definitions.twin.  Built unfused like every kernel here (-ffp-contract=off), IEEE division and square
// root; sinf, cosf, expf and atan2f are the device library's full-precision functions.
#pragma once
#include "device_math.hpp"
#include "sun_sky_host.hpp"

namespace mirt {

constexpr uint32_t kSunSkyBlock = 256;

// 2 sin^2(pi k / (2 rows)): 1 - sin el(k) measured from the pole, el(k) = pi (1/2 - k / rows).  Never a difference of nearly equal numbers.
MIRT_DI float sun_sky_edge(uint32_t k, float rows) {
	const float h = sinf(MIRT_HALF_PI * (static_cast<float>(k) / rows));
	return 2.0f * (h * h);
}

// One sub-sample: the sky seen along e (the direction itself above the horizon, its foot on the horizon below), the disc along d.
MIRT_DI f3 sun_sky_sample(const mirt_sun_sky::Args& a, f3 e, f3 d, bool below) {
	const f3 s{ a.sun[0], a.sun[1], a.sun[2] };
	const float ct = max_sel(e.y, 0x1p-6f);
	const f3 m{ e.x - s.x, e.y - s.y, e.z - s.z }, p{ e.x + s.x, e.y + s.y, e.z + s.z };
	const float g = 2.0f * atan2f(__builtin_sqrtf(dot3(m, m)), __builtin_sqrtf(dot3(p, p)));      // the angle between e and the sun, well conditioned from 0 to pi
	const float cg = dot3(e, s);
	const float cg2 = cg * cg;
	float v[3];
	for (int k = 0; k < 3; k++) {
		const float* c = a.perez[k];
		const float F = (1.0f + c[0] * expf(c[1] / ct)) * ((1.0f + c[2] * expf(c[3] * g)) + c[4] * cg2);
		v[k] = (a.zenith[k] * F) * a.inv_f0[k];
	}
	const float Y = v[0];
	const float X = (v[1] / v[2]) * Y;
	const float Z = (((1.0f - v[1]) - v[2]) / v[2]) * Y;
	f3 rgb{ (3.2404542f * X + -1.5371385f * Y) + -0.4985314f * Z, (-0.9692660f * X + 1.8760108f * Y) + 0.0415560f * Z, (0.0556434f * X + -0.2040259f * Y) + 1.0572252f * Z };
	rgb = { max_sel(0.0f, rgb.x) * a.sky_scale, max_sel(0.0f, rgb.y) * a.sky_scale, max_sel(0.0f, rgb.z) * a.sky_scale };
	if (below) rgb = { rgb.x * a.ground[0], rgb.y * a.ground[1], rgb.z * a.ground[2] };
	const f3 u{ d.x - s.x, d.y - s.y, d.z - s.z };
	const float limb = ((a.ramp_edge - 0.5f * dot3(u, u)) * a.ramp_inv);                              // (cos gamma - cos alpha) / (cos 0.9 alpha - cos alpha), 1 - cos gamma = |d - sun|^2 / 2
	const float wgt = min_sel(max_sel(0.0f, limb), 1.0f);
	return { rgb.x + wgt * a.sun_rgb[0], rgb.y + wgt * a.sun_rgb[1], rgb.z + wgt * a.sun_rgb[2] };
}

// One thread per texel of the w x h map, the duplicate last column (= column 0) and last row (= row h - 2) included; one 16-byte store each.
__global__ __launch_bounds__(kSunSkyBlock) void k_sun_sky(const mirt_sun_sky::Args a, float4* __restrict__ hdri) {
	const uint32_t idx = blockIdx.x * kSunSkyBlock + threadIdx.x;
	if (idx >= a.w * a.h) return;
	const uint32_t cols = a.w - 1u, rows = a.h - 1u;
	const uint32_t tr = idx / a.w, tc = idx - tr * a.w;
	const uint32_t r = tr < rows ? tr : rows - 1u, c = tc < cols ? tc : 0u;
	const bool north = 2u * r + 1u <= rows;                                      // the cell's edges are measured from the nearer pole
	const float frows = static_cast<float>(rows);
	const float ta = sun_sky_edge(north ? r : rows - r, frows), tb = sun_sky_edge(north ? r + 1u : rows - (r + 1u), frows);
	const float fden = static_cast<float>(4u * cols);
	const int32_t n0 = static_cast<int32_t>(8u * c + 1u) - static_cast<int32_t>(4u * cols);
	float sn[4], cs[4];
	for (int j = 0; j < 4; j++) {
		const float phi = MIRT_PI * (static_cast<float>(n0 + 2 * j) / fden);
		sn[j] = sinf(phi); cs[j] = cosf(phi);
	}
	f3 sum{ 0.0f, 0.0f, 0.0f };
	for (int i = 0; i < 4; i++) {
		const float t = ta + (0.125f * static_cast<float>(2 * i + 1)) * (tb - ta);
		const float y = north ? 1.0f - t : t - 1.0f;
		const float ce = __builtin_sqrtf(t * (2.0f - t));
		const bool below = y < 0.0f;
		for (int j = 0; j < 4; j++) {
			const f3 d{ ce * cs[j], y, ce * sn[j] };
			const f3 e = below ? f3{ cs[j], 0.0f, sn[j] } : d;
			const f3 v = sun_sky_sample(a, e, d, below);
			sum = (i | j) ? f3{ sum.x + v.x, sum.y + v.y, sum.z + v.z } : v;
		}
	}
	hdri[idx] = make_float4(sum.x * 0.0625f, sum.y * 0.0625f, sum.z * 0.0625f, 1.0f);
}

} // namespace mirt
