// TEMPORAL HISTORY FOR THE DENOISED RESOLVE — mirt_render_temporal (mirt.h, "temporal history for the denoised resolve": the definition, step by step).
// One kernel, k_reproject, between k_denoise_prepare and the first k_atrous pass of denoise.hpp: steps 2 (reproject), 3 (blend) and the (x, v) and
// length planes of step 4 (history write).  Binary32, one rounding per operation in the order mirt.h states (-ffp-contract=off; IEEE division and
// square root).  One 16 x 16 pixel block per workgroup over the row-major images of denoise.hpp: cv = (x_r, x_g, x_b, v), gd = (N.x, N.y, N.z, z)
// with z = NaN marking an unusable pixel, and one float per pixel for the history length.
// THE HISTORY WRITE IS THE BLEND: the kernel writes the blended (x, v) and the length ONCE, into buffers the history does not occupy (a tap reads
// any pixel of the old history while other workgroups write, so it cannot be updated in place); with update = 1 the host then renames them — they
// become the history, the old history's become scratch (mirt_resolve.hip, mirt_render_temporal).  The guides of a call are the history's guides
// unchanged, so that plane is renamed too and nothing is copied.  The a-trous passes read the blend and never write it: spatial blur does not
// compound over frames.
// NO LDS STAGING, and why: per pixel the kernel gathers 2 x 2 taps of two float4 images and one float image (eight float4 gathers, four scalars).
// Where the 16 x 16 block's taps land in the history is known only after every lane has run the reprojection, and is a window of unbounded size
// under a dolly or a rotation about the view axis, so a staged variant needs a block-wide bounding-box reduction, a barrier and the direct path as
// its fallback — for a reuse of 4 (k_atrous at step 1 stages for a reuse of 25).  Under the small moves the feature serves, a wave's 4 x 16 pixels
// gather four 16-pixel row segments per tap and image, 256 contiguous bytes each: the coalesced shape already, with the 2 x 2 overlap served by
// L1 / L2.  The kernel is one pass over five images and is priced beside k_atrous in profiles/temporal.txt.
// STATISTICS: every lane ends in exactly one of five classes; each wave ballots each class and lane 0 adds the population count with one 64-bit
// atomic per wave and class that has a member.  Every wave of the image adding to the same five words serialises the adds (one address: the slow
// shape of a global atomic), so the counts are kept in kTemporalStatSlots copies, each on a 128-byte line of its own, a workgroup adding to copy
// (block index mod slots); the host sums the copies (one copy against 256: profiles/temporal.txt).
#pragma once
#include "denoise.hpp"

namespace mirt {

struct TemporalDev {
	CameraParams cam, prev;        // this call's camera; the one the history was taken under
	float max_ratio, depth_tol, normal_min;
	uint32_t take;                 // 1: the call takes the history (mirt.h step 2's conditions on the call); 0: every usable pixel is `no_history`
	uint32_t identity;             // 1: cam equals prev word for word: the map is the identity by definition
};

constexpr uint32_t kTemporalStatSlots = 256u, kTemporalStatPitch = 16u;      // copies of the five counts; 64-bit words between two copies (128 B)
enum : uint32_t { kTemporalReprojected = 0u, kTemporalNoHistory = 1u, kTemporalOutside = 2u, kTemporalRejected = 3u, kTemporalUnusable = 4u, kTemporalClasses = 5u };

// OBJECT MOTION (mirt_set_sphere_motion, mirt.h "keeping the history across sphere moves"): what k_reproject<true> reads besides — this call's id map
// (id_map.hpp: the BVH-order sphere of every pixel centre, -1 for none), the id plane of the call that wrote the history, the sphere table now
// and the snapshot of it the history was taken under.  A pixel whose sphere's four words differ between the two tables is carried back to where
// that point of the sphere was (translation and uniform scale: normals keep), and a tap is taken only where the history shows the same sphere.
// The plain instantiation is handed an empty struct as its last argument and names none of this: its device code is what it was before the template.
template <bool MOTION> struct MotionDev {};
template <> struct MotionDev<true> {
	const int32_t* __restrict__ ids;       // this call's id map
	const int32_t* __restrict__ hist_ids;  // the history's
	const float4* __restrict__ now;        // {pos, radius_sq} by BVH-order id, now ...
	const float4* __restrict__ then;       // ... and when the history was written
};

// The image is w_img x h_img pixels (whole tiles) in rows of `width` pixels; the grid is its 16 x 16 blocks, block (bx, by) = tile by * gridDim.x + bx.
template <bool MOTION>
__global__ __launch_bounds__(kAtrousBlock * kAtrousBlock) void k_reproject(const float4* __restrict__ cv_in, const float4* __restrict__ gd, const float4* __restrict__ hx,
                                                                            const float4* __restrict__ hg, const float* __restrict__ hn, float4* __restrict__ cv_out,
                                                                            float* __restrict__ len_out, unsigned long long* __restrict__ stats, uint32_t width, uint32_t w_img,
                                                                            uint32_t h_img, const uint32_t* __restrict__ tile_counts, uint32_t count_all, TemporalDev p, MotionDev<MOTION> mo) {
	const uint32_t lx = threadIdx.x & 15u, ly = threadIdx.x >> 4;
	const int32_t px = static_cast<int32_t>(blockIdx.x * kAtrousBlock + lx), py = static_cast<int32_t>(blockIdx.y * kAtrousBlock + ly);
	const size_t at = static_cast<size_t>(py) * width + static_cast<size_t>(px);
	const float nf = static_cast<float>(tile_counts ? tile_counts[blockIdx.y * gridDim.x + blockIdx.x] : count_all);
	const float4 c = cv_in[at], g = gd[at];
	float4 out = c;
	float len = nf;
	uint32_t cls = kTemporalNoHistory;
	if (!dn_usable(g)) { cls = kTemporalUnusable; len = 0.0f; }
	else if (p.take && !(g.x == 0.0f && g.y == 0.0f && g.z == 0.0f)) {
		float fx = static_cast<float>(px), fy = static_cast<float>(py), zr = g.w;            // the identity map
		bool behind = false;
		// MOTION: the pixel's sphere and whether it moved (any of its four words differs between the two tables); a moved sphere has no identity map
		int32_t id = -1;
		bool moved = false, scaled = false;
		float4 now{}, then{};
		if constexpr (MOTION) {
			id = mo.ids[at];
			if (id >= 0) {
				now = mo.now[id]; then = mo.then[id];
				scaled = __float_as_uint(now.w) != __float_as_uint(then.w);
				moved = scaled || __float_as_uint(now.x) != __float_as_uint(then.x) || __float_as_uint(now.y) != __float_as_uint(then.y) || __float_as_uint(now.z) != __float_as_uint(then.z);
			}
		}
		if (!p.identity || (MOTION && moved)) {
			const f3 d = camera_ray_dir(p.cam, px, py, 0.5f, 0.5f);
			f3 P{ p.cam.pos[0] + d.x * g.w, p.cam.pos[1] + d.y * g.w, p.cam.pos[2] + d.z * g.w };
			if constexpr (MOTION) {
				if (moved) {                                                                      // P' = c0 + (P - c) * s: the same point of the sphere, where it was
					f3 o{ P.x - now.x, P.y - now.y, P.z - now.z };
					if (scaled && now.w > 0.0f) { const float s = __builtin_sqrtf(then.w / now.w); o.x = o.x * s; o.y = o.y * s; o.z = o.z * s; }
					P.x = then.x + o.x; P.y = then.y + o.y; P.z = then.z + o.z;
				}
			}
			const f3 r{ P.x - p.prev.pos[0], P.y - p.prev.pos[1], P.z - p.prev.pos[2] };
			zr = __builtin_sqrtf(dot3(r, r));
			const float conj[4] = { -p.prev.orient[0], -p.prev.orient[1], -p.prev.orient[2], p.prev.orient[3] };
			const f3 q = camera_axis(conj, r);
			if (q.z / p.prev.z <= 0.0f) behind = true;                                          // behind the history's camera
			else {
				const float t = p.prev.z / q.z;
				fx = (q.x * t + p.prev.half_width) - 0.5f;
				fy = (q.y * t + p.prev.half_height) - 0.5f;
			}
		}
		const float ixf = __builtin_floorf(fx), iyf = __builtin_floorf(fy);
		// some tap of the 2 x 2 lies in the image exactly when ix is in [-1, w - 1] and iy in [-1, h - 1] (a NaN or an infinity fails every comparison)
		if (behind || !(ixf >= -1.0f && ixf <= static_cast<float>(w_img - 1u) && iyf >= -1.0f && iyf <= static_cast<float>(h_img - 1u))) cls = kTemporalOutside;
		else {
			const float wx = fx - ixf, wy = fy - iyf, ux = 1.0f - wx, uy = 1.0f - wy;
			const int32_t ix = static_cast<int32_t>(ixf), iy = static_cast<int32_t>(iyf);
			float B = 0.0f, X[3] = { 0.0f, 0.0f, 0.0f }, V = 0.0f, L = 0.0f;
			bool first = true;
#pragma unroll
			for (int32_t j = 0; j < 2; j++) {
#pragma unroll
				for (int32_t i = 0; i < 2; i++) {                                                 // taps (0,0), (1,0), (0,1), (1,1)
					const int32_t tx = ix + i, ty = iy + j;
					if (tx < 0 || ty < 0 || tx >= static_cast<int32_t>(w_img) || ty >= static_cast<int32_t>(h_img)) continue;
					const size_t q = static_cast<size_t>(ty) * width + static_cast<size_t>(tx);
					const float4 tg = hg[q];
					const float tn = hn[q];
					if (!dn_usable(tg) || !(tn > 0.0f)) continue;
					if (!(__builtin_fabsf(tg.w - zr) <= p.depth_tol * zr)) continue;
					if (!((g.x * tg.x + g.y * tg.y) + g.z * tg.z >= p.normal_min)) continue;
					if constexpr (MOTION) { if (mo.hist_ids[q] != id) continue; }                 // another surface stood there: what a moving ball uncovers is `rejected`
					const float4 tc = hx[q];
					const float b = (i ? wx : ux) * (j ? wy : uy);
					B = first ? b : B + b;
					X[0] = first ? b * tc.x : X[0] + b * tc.x;
					X[1] = first ? b * tc.y : X[1] + b * tc.y;
					X[2] = first ? b * tc.z : X[2] + b * tc.z;
					V = first ? b * tc.w : V + b * tc.w;
					L = first ? b * tn : L + b * tn;
					first = false;
				}
			}
			if (first || B == 0.0f) cls = kTemporalRejected;
			else {
				cls = kTemporalReprojected;
				const float xh[3] = { X[0] / B, X[1] / B, X[2] / B }, vh = V / B;
				float nh = L / B;
				const float cap = p.max_ratio * nf;
				nh = cap < nh ? cap : nh;
				const float a = nf / (nf + nh), oma = 1.0f - a;
				out.x = xh[0] + a * (c.x - xh[0]);
				out.y = xh[1] + a * (c.y - xh[1]);
				out.z = xh[2] + a * (c.z - xh[2]);
				out.w = (a * a) * c.w + (oma * oma) * vh;
				len = nf + nh;
			}
		}
	}
	cv_out[at] = out;
	len_out[at] = len;
	const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
	for (uint32_t k = 0; k < kTemporalClasses; k++) {
		const unsigned long long m = __ballot(cls == k);
		if (lane == 0u && m != 0ull) atomicAdd(&stats[((blockIdx.y * gridDim.x + blockIdx.x) % kTemporalStatSlots) * kTemporalStatPitch + k], static_cast<unsigned long long>(__popcll(m)));
	}
}

}  // namespace mirt
