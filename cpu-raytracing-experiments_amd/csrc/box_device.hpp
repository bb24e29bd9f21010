// box_device.hpp — the device functions every maker of traversal records shares: the documented leaf box of a sphere (bvh_layout.hpp
// build_records: r = sqrt(radius_sq), pad = 2^-18 (max|c| + r), one binary32 step outward of (c - r) - pad and (c + r) + pad), the union of
// two boxes, and the outward-rounding binary16 encoders.  Used by the GPU builder (lbvh_build.hip) and by the refit (refit.hpp), so that a
// refitted tree holds, word for word, the boxes a fresh build over the same topology writes.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

namespace mirt_box {

constexpr float kPadRel = 0x1p-18f;                     // bvh_layout.hpp kPadRel

__device__ __forceinline__ float next_up(float x) {                       // finite x
	if (x == 0.0f) return __uint_as_float(1u);
	uint32_t b = __float_as_uint(x);
	return __uint_as_float(x > 0.0f ? b + 1u : b - 1u);
}
__device__ __forceinline__ float next_down(float x) { return -next_up(-x); }

struct Box { float lo[3], hi[3]; };

// The leaf box of sphere s = {centre, radius_sq}, as mirt_host::build_records computes it.
__device__ __forceinline__ Box sphere_leaf_box(const float4 s, float* radius_out = nullptr) {
	const float c[3] = { s.x, s.y, s.z };
	const float r = __builtin_sqrtf(s.w);
	float amax = fabsf(c[0]);
	if (amax < fabsf(c[1])) amax = fabsf(c[1]);
	if (amax < fabsf(c[2])) amax = fabsf(c[2]);
	const float pad = kPadRel * (amax + r);
	Box b;
	for (int a = 0; a < 3; a++) {
		b.lo[a] = next_down((c[a] - r) - pad);
		b.hi[a] = next_up((c[a] + r) + pad);
	}
	if (radius_out) *radius_out = r;
	return b;
}

__device__ __forceinline__ Box box_union(const Box& x, const Box& y) {
	Box b;
	for (int a = 0; a < 3; a++) { b.lo[a] = (y.lo[a] < x.lo[a]) ? y.lo[a] : x.lo[a]; b.hi[a] = (x.hi[a] < y.hi[a]) ? y.hi[a] : x.hi[a]; }
	return b;
}

__device__ __forceinline__ uint32_t half_down(float f) {                  // largest binary16 <= f
	return static_cast<uint32_t>(__half_as_ushort(__float2half_rd(f)));
}
__device__ __forceinline__ uint32_t half_up(float f) {
	return static_cast<uint32_t>(__half_as_ushort(__float2half_ru(f)));
}

} // namespace mirt_box
