// refit.hpp — the kernels of mirt_update_spheres (include/mirt.h, "moving spheres in place"): new boxes for the records the trace kernels
// already walk.  The topology stays — every reference, every unused slot — and every box becomes what a fresh build over that topology
// writes: a leaf slot the documented box of its sphere (box_device.hpp sphere_leaf_box = bvh_layout.hpp build_records), an inner slot the
// binary32 union of the used slots of the record it points at, binary16 planes those binary32 boxes rounded outward (directed rounding is
// monotone, so rounding the union equals the union of the rounded).  The three layouts of bvh_layout.hpp are one form here: a record of 2 or
// 4 slots, each unused, a leaf (kLeafBit | prim) or a record index; whichever builder made them (host SAH, the caller's tree, the GPU LBVH).
//
//   k_update_spheres   scatters the edited {centre, radius_sq} packets into the sphere table and into the geometry-order table.
//   k_refit_links      once per tree: every record's parent and number of used slots, every prim's leaf record, read from the records.
//   k_refit            one thread per prim climbs from its leaf record; the last of a record's used slots to arrive owns the record
//                      (lbvh_build.hip k_inner_boxes' arrival counters), rewrites it whole and leaves its binary32 union for the parent.
// Integer atomics on the counters only, whole-word stores only, no float atomics: the same records on every run.
#pragma once
#include "box_device.hpp"

namespace mirt {

constexpr uint32_t kRefitBlock = 256;
constexpr uint32_t kRefitNoParent = 0xffffffffu;
constexpr uint32_t kRefitLeafBit = 0x80000000u;          // bvh_layout.hpp kLeafBit
constexpr int kRefitF32 = 0, kRefitHalf = 1, kRefitWide = 2;   // mirt_debug_tree's layout numbers

// What a refit reads besides the records: one allocation, laid out by the host (mirt_launch.hip refit_links).
struct RefitLinks {
	uint32_t* parent;        // [n_recs] the record whose slot points at this one; kRefitNoParent for record 0
	uint32_t* used;          // [n_recs] used slots
	uint32_t* leaf_rec;      // [n_prims] the record that holds the prim's leaf
	uint32_t* arrivals;      // [n_recs] zeroed before every k_refit
	mirt_box::Box* box;      // [n_recs] the binary32 union of the record's used slots, written by its owner
};

// ---- one record in registers: W words, S slots --------------------------------------------------------------------------------------
template <int L> struct RefitRecord {
	static constexpr int W = L == kRefitHalf ? 8 : 16, S = L == kRefitWide ? 4 : 2;
	uint32_t w[W];
	__device__ __forceinline__ void load(const uint4* recs, uint32_t r) {
		const uint4* q = recs + static_cast<size_t>(r) * (W / 4);
		for (int i = 0; i < W / 4; i++) { const uint4 v = q[i]; w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w; }
	}
	__device__ __forceinline__ void store(uint4* recs, uint32_t r) const {
		uint4* q = recs + static_cast<size_t>(r) * (W / 4);
		for (int i = 0; i < W / 4; i++) q[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
	}
	__device__ __forceinline__ uint32_t ref(int k) const { return w[(L == kRefitHalf ? 6 : 12) + k]; }
	// the word and the bit offset of slot k's plane on axis a (hi: the upper plane)
	static __device__ __forceinline__ int word(int a, int hi, int k) { return L == kRefitF32 ? a * 4 + hi * 2 + k : L == kRefitHalf ? a * 2 + hi : a * 4 + hi * 2 + (k >> 1); }
	static __device__ __forceinline__ int shift(int k) { return L == kRefitF32 ? 0 : 16 * (k & 1); }
	// unused: the x planes carry the layout's empty marker (FLT_MAX twice in the f32 single-leaf record, +inf binary16 otherwise); no box of
	// finite spheres has a lower plane of +inf or both planes at FLT_MAX
	__device__ __forceinline__ bool unused(int k) const {
		if (L == kRefitF32) return w[word(0, 0, k)] == 0x7f7fffffu && w[word(0, 1, k)] == 0x7f7fffffu;
		return ((w[word(0, 0, k)] >> shift(k)) & 0xffffu) == 0x7c00u;
	}
	__device__ __forceinline__ void set_box(int k, const mirt_box::Box& b) {
		for (int a = 0; a < 3; a++) {
			if (L == kRefitF32) { w[word(a, 0, k)] = __float_as_uint(b.lo[a]); w[word(a, 1, k)] = __float_as_uint(b.hi[a]); }
			else {
				const uint32_t keep = ~(0xffffu << shift(k));
				w[word(a, 0, k)] = (w[word(a, 0, k)] & keep) | (mirt_box::half_down(b.lo[a]) << shift(k));
				w[word(a, 1, k)] = (w[word(a, 1, k)] & keep) | (mirt_box::half_up(b.hi[a]) << shift(k));
			}
		}
	}
};

__global__ __launch_bounds__(kRefitBlock) void k_update_spheres(uint32_t n, const uint32_t* __restrict__ index, const uint32_t* __restrict__ geometry_index, const float4* __restrict__ packet,
                                                                float4* __restrict__ spheres, float4* __restrict__ geometry_spheres, uint32_t n_spheres) {
	const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
	if (i >= n) return;
	const uint32_t j = index[i], g = geometry_index[i];
	const float4 p = packet[i];
	if (j < n_spheres) spheres[j] = p;                                       // (validated on the host; distinct indices: no two threads share a row)
	if (g < n_spheres) geometry_spheres[g] = p;                              // the same sphere in authoring order (light_list.hpp GeometryTable)
}

// One thread per record.  A validated tree points at every record but the first exactly once and holds every prim in exactly one leaf, so
// no two threads write the same word.
template <int L> __global__ __launch_bounds__(kRefitBlock) void k_refit_links(const uint4* __restrict__ recs, uint32_t n_recs, uint32_t n_prims, RefitLinks links) {
	const uint32_t r = blockIdx.x * kRefitBlock + threadIdx.x;
	if (r >= n_recs) return;
	RefitRecord<L> rec;
	rec.load(recs, r);
	uint32_t used = 0;
#pragma unroll
	for (int k = 0; k < RefitRecord<L>::S; k++) {
		if (rec.unused(k)) continue;
		used++;
		const uint32_t ref = rec.ref(k);
		if (ref & kRefitLeafBit) { const uint32_t prim = ref & ~kRefitLeafBit; if (prim < n_prims) links.leaf_rec[prim] = r; }
		else if (ref < n_recs) links.parent[ref] = r;
	}
	links.used[r] = used;
	if (r == 0) links.parent[0] = kRefitNoParent;
}

template <int L> __global__ __launch_bounds__(kRefitBlock) void k_refit(uint4* recs, uint32_t n_recs, const float4* __restrict__ spheres, uint32_t n_prims, RefitLinks links) {
	const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
	if (i >= n_prims) return;
	uint32_t node = links.leaf_rec[i];
	while (node < n_recs) {                                                  // kRefitNoParent ends the climb
		__threadfence();
		if (atomicAdd(&links.arrivals[node], 1u) + 1u != links.used[node]) return;   // a sibling subtree is not finished yet
		__threadfence();
		RefitRecord<L> rec;
		rec.load(recs, node);
		const volatile mirt_box::Box* done = links.box;
		mirt_box::Box all{};
		bool first = true;
#pragma unroll
		for (int k = 0; k < RefitRecord<L>::S; k++) {
			if (rec.unused(k)) continue;                                         // kept as it is
			const uint32_t ref = rec.ref(k);
			mirt_box::Box b;
			if (ref & kRefitLeafBit) b = mirt_box::sphere_leaf_box(spheres[ref & ~kRefitLeafBit]);
			else for (int a = 0; a < 3; a++) { b.lo[a] = done[ref].lo[a]; b.hi[a] = done[ref].hi[a]; }
			rec.set_box(k, b);
			all = first ? b : mirt_box::box_union(all, b);
			first = false;
		}
		rec.store(recs, node);
		links.box[node] = all;
		node = links.parent[node];
	}
}

} // namespace mirt
