// light_list.hpp — the kernels of mirt_update_materials (include/mirt.h, "updating materials in place"): material ids scattered into both
// orders, and the next-event-estimation light tables regenerated on the device.  The light list is the reference's LightingAcceleration
// constructor (Scene.hpp:12-16): the geometry-order ids of the spheres whose material emits, ascending — an ordered stream compaction over the
// geometry-order table (GeometryTable below), which mirt_set_scene uploads and k_update_spheres / k_assign_materials keep current.
//
//   k_assign_materials   scatters the edited material ids into prim_mat (BVH order) and into the geometry-order table.
//   k_light_count        one thread per sphere: a wave's flags by __ballot, its count by __popcll; the workgroup's total of its waves' counts.
//   k_light_scan         one workgroup: the exclusive running sum of the workgroups' totals, kLightScanPass at a time; the last sum is n_lights.
//   k_light_scatter      the flags again; light l = workgroup offset + counts of the waves before + flagged lanes before; the two rows of light l.
// Whether a material emits is decided on the host (bvh_build.hpp emits(), the expression of mirt_light_list) and arrives as one bit per
// material: the kernels test a bit.  No atomics, every position a function of the flags alone: the same words on every run and every device.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mirt {

constexpr uint32_t kLightBlock = 256;            // spheres per workgroup of the compaction (one per thread): mirt_debug_lights info[1]
constexpr uint32_t kLightScanPass = 256;         // workgroup totals one pass of k_light_scan covers (one per thread): mirt_debug_lights info[2]
constexpr uint32_t kLightWaves = kLightBlock / 64u;

// The authoring-order geometry as the compaction reads it: what NEE's table is made from (Renderer.hpp:261-263 reads scene.geometry[light]).
struct GeometryTable {
	float4* sphere;          // [n_spheres] {centre, radius_sq}
	int32_t* material;       // [n_spheres] material_ID
};

__global__ __launch_bounds__(kLightBlock) void k_assign_materials(uint32_t n, const uint32_t* __restrict__ bvh_index, const uint32_t* __restrict__ geometry_index,
                                                                  const int32_t* __restrict__ material_id, int32_t* __restrict__ prim_mat, GeometryTable geo, uint32_t n_spheres) {
	const uint32_t i = blockIdx.x * kLightBlock + threadIdx.x;
	if (i >= n) return;
	const uint32_t b = bvh_index[i], g = geometry_index[i];
	const int32_t m = material_id[i];
	if (b < n_spheres) prim_mat[b] = m;                                        // (validated on the host; distinct indices: no two threads share a word)
	if (g < n_spheres) geo.material[g] = m;
}

// Sphere i is a light: its material's bit in `emit_mask`.  Material ids are below MIRT_MAX_MATERIALS (63) by validation; the mask keeps the shift defined anyway.
__device__ __forceinline__ bool light_flag(const int32_t* __restrict__ material, uint32_t i, uint32_t n, uint64_t emit_mask) {
	return i < n && ((emit_mask >> (static_cast<uint32_t>(material[i]) & 63u)) & 1ull) != 0ull;
}

// The flagged spheres of this wave before this lane, and of the workgroup's waves before this wave (wave_count: LDS, one word per wave).
// Every thread of the workgroup calls it (a barrier inside).  Returns this thread's rank within the workgroup; *total = the workgroup's count.
__device__ __forceinline__ uint32_t light_rank_in_block(bool flag, uint32_t* wave_count, uint32_t* total) {
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const unsigned long long ballot = __ballot(flag);
	if (lane == 0) wave_count[wave] = static_cast<uint32_t>(__popcll(ballot));
	__syncthreads();
	uint32_t before = 0, all = 0;
#pragma unroll
	for (uint32_t w = 0; w < kLightWaves; w++) { const uint32_t c = wave_count[w]; all += c; if (w < wave) before += c; }
	*total = all;
	return before + static_cast<uint32_t>(__popcll(ballot & ((1ull << lane) - 1ull)));
}

__global__ __launch_bounds__(kLightBlock) void k_light_count(const int32_t* __restrict__ material, uint32_t n, uint64_t emit_mask, uint32_t* __restrict__ block_total) {
	__shared__ uint32_t wave_count[kLightWaves];
	const uint32_t i = blockIdx.x * kLightBlock + threadIdx.x;
	uint32_t total;
	(void)light_rank_in_block(light_flag(material, i, n, emit_mask), wave_count, &total);
	if (threadIdx.x == 0) block_total[blockIdx.x] = total;
}

// One workgroup.  block_total[b] becomes the number of lights in the workgroups before b; *n_lights the number of all.  A pass: every thread
// one total, an inclusive scan within the wave by shuffles, the waves' sums through LDS, the carry of the passes before in a register.
__global__ __launch_bounds__(kLightScanPass) void k_light_scan(uint32_t* __restrict__ block_total, uint32_t n_blocks, uint32_t* __restrict__ n_lights) {
	__shared__ uint32_t wave_sum[kLightScanPass / 64u];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t carry = 0;
	for (uint32_t base = 0; base < n_blocks; base += kLightScanPass) {
		const uint32_t b = base + threadIdx.x;
		const uint32_t own = b < n_blocks ? block_total[b] : 0u;
		uint32_t incl = own;
#pragma unroll
		for (uint32_t d = 1; d < 64u; d <<= 1) { const uint32_t up = __shfl_up(incl, d, 64); if (lane >= d) incl += up; }
		if (lane == 63u) wave_sum[wave] = incl;
		__syncthreads();
		uint32_t before = 0, all = 0;
#pragma unroll
		for (uint32_t w = 0; w < kLightScanPass / 64u; w++) { const uint32_t c = wave_sum[w]; all += c; if (w < wave) before += c; }
		if (b < n_blocks) block_total[b] = carry + before + incl - own;
		carry += all;
		__syncthreads();                                                          // wave_sum is written again by the next pass
	}
	if (threadIdx.x == 0) *n_lights = carry;
}

// light_sphere[l] = the geometry row of light l; light_emit[l] = {emission.rgb of its material, the bits of its geometry id}: the words
// mirt_set_scene's flatten_tables writes.  capacity: rows of both tables (the count read back after k_light_scan; a rank beyond it is not stored).
__global__ __launch_bounds__(kLightBlock) void k_light_scatter(GeometryTable geo, uint32_t n, uint64_t emit_mask, const uint32_t* __restrict__ block_offset,
                                                               const float4* __restrict__ mat_emission, float4* __restrict__ light_sphere, float4* __restrict__ light_emit, uint32_t capacity) {
	__shared__ uint32_t wave_count[kLightWaves];
	const uint32_t i = blockIdx.x * kLightBlock + threadIdx.x;
	const bool flag = light_flag(geo.material, i, n, emit_mask);
	uint32_t total;
	const uint32_t rank = light_rank_in_block(flag, wave_count, &total);
	if (!flag) return;
	const uint32_t l = block_offset[blockIdx.x] + rank;
	if (l >= capacity) return;
	const float4 e = mat_emission[static_cast<uint32_t>(geo.material[i]) & 63u];
	light_sphere[l] = geo.sphere[i];
	light_emit[l] = make_float4(e.x, e.y, e.z, __int_as_float(static_cast<int32_t>(i)));
}

} // namespace mirt
