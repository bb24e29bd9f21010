// FIRST-HIT ID MAP — mirt_id_map (mirt.h, "first-hit id map"): per pixel of the whole image the sphere the un-jittered pinhole ray through the pixel
// centre meets first, and how far away: what mirt_pick_focus finds for one pixel, for all of them in ONE launch.
// No ray stream is written or read: ray i is pixel (i % width, i / width), generated from its index by camera_ray_dir(cam, x, y, 0.5f, 0.5f) — the
// statement mirt_pick_focus evaluates on the host — and walked through the context's own closest-hit traversal (trace_queue: every record layout,
// the tree in LDS or not; the brute-force loop without a tree), the persistent waves reserving chunks of pixels from one work counter.  The
// result is stored by the lane that finished the ray, one int32 and one float per pixel, row-major in rows of `width`: the layout of the
// resolve's full-image planes (denoise.hpp), so mirt_render_temporal hands the prim plane to k_reproject<MOTION> as it is.
// A pixel-centre direction is normalised (|D|^2 - 1 is a few ulp), so no ray of this kernel is "fat" (kernels.hpp trav_begin); the list it is
// handed has no room, which makes a ray that were walk the tree like any other.
// SceneDev and the trace kernels are untouched: this is one more caller of trace_queue, as k_primary_cand is.
#pragma once
#include "kernels.hpp"

namespace mirt {

struct IdMapDev {
	CameraParams cam;
	uint32_t width, n_pix;      // pixels per row; width * height (below 2^31)
	float inv_width;            // 1 / width, for udiv_f
};

MIRT_DI void id_map_ray(const IdMapDev& p, uint32_t i, float& px, float& py, float& pz, float& dx, float& dy, float& dz) {
	uint32_t x;
	const uint32_t y = udiv_f(i, p.width, p.inv_width, x);
	const f3 d = camera_ray_dir(p.cam, static_cast<int32_t>(x), static_cast<int32_t>(y), 0.5f, 0.5f);
	px = p.cam.pos[0]; py = p.cam.pos[1]; pz = p.cam.pos[2]; dx = d.x; dy = d.y; dz = d.z;
}
// prim: the BVH-order id hit.primID refers to, -1 on a miss; dist: tfar, INFINITY on a miss.  Either plane may be NULL.
MIRT_DI void id_map_store(int32_t* __restrict__ prim_out, float* __restrict__ dist_out, uint32_t i, float tfar, int32_t prim) {
	if (prim_out) prim_out[i] = prim;
	if (dist_out) dist_out[i] = prim >= 0 ? tfar : __builtin_inff();
}

// words[0]: the launch's work counter, words[1]: the count of the fat-ray list without room; both zeroed before the launch.
__global__ __launch_bounds__(kTraceBlock, 8) void k_id_map(SceneDev sc, IdMapDev p, int32_t* __restrict__ prim_out, float* __restrict__ dist_out, uint32_t* words) {
	extern __shared__ float4 lds[];
	const uint32_t n = p.n_pix;
	if (n == 0u) return;
	uint32_t c_nodes = 0, c_spheres = 0;
	if (sc.use_bvh && sc.n_recs != 0) {
		if (static_cast<uint64_t>(blockIdx.x) * 64u >= static_cast<uint64_t>(n)) return;       // more workgroups than minimum-size chunks: skip the staging too
		const TraceLds tl = stage_bvh(sc, lds);
		auto load_ray = [&](uint32_t i, float& px, float& py, float& pz, float& dx, float& dy, float& dz, float& tf) {
			id_map_ray(p, i, px, py, pz, dx, dy, dz);
			tf = MIRT_FLT_MAX;                                                                 // hit reset, Renderer.hpp:150-158
		};
		auto store_result = [&](uint32_t i, const Trav& t, bool) { id_map_store(prim_out, dist_out, i, t.tfar, t.prim); };
		trace_queue<kClosest, false>(sc, tl, Queue{ nullptr, 0u }, n, words, FatList{ words + 1, nullptr, 0u }, c_nodes, c_spheres, load_ray, store_result);
	} else {
		// brute force over all prims (policy.use_bvh = 0); also the no-spheres case
		for (uint32_t base = blockIdx.x * kTraceBlock; base < n; base += gridDim.x * kTraceBlock) {
			const bool active = base + threadIdx.x < n;
			const uint32_t i = active ? base + threadIdx.x : 0u;
			float px = 0, py = 0, pz = 0, dx = 1, dy = 1, dz = 1;
			if (active) id_map_ray(p, i, px, py, pz, dx, dy, dz);
			float tfar = MIRT_FLT_MAX;
			int32_t prim = -1;
			if (sc.use_bvh == 0) traverse_brute<false, false>(sc, lds, active, px, py, pz, dx, dy, dz, tfar, prim, c_spheres);
			if (active) id_map_store(prim_out, dist_out, i, tfar, prim);
		}
	}
}

}  // namespace mirt
