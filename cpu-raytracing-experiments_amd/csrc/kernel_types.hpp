// kernel_types.hpp — what the host layers and the kernels share: the POD argument types and the constants a launch is sized with.
// No kernel and no device function is defined here (the accessors of SkyTable aside), so every layer may include it: ctx.hpp does, for the
// API layer (mirt_capi.hip) and the resolve layer (mirt_resolve.hip); kernels.hpp does, for the kernels.  What a type means is described beside
// the kernels that read it (kernels.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "device_math.hpp"
#include "tile_map.hpp"

namespace mirt {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kShadeBlock = 512;           // shade: 73-80 VGPRs = 24 waves per CU = three 8-wave workgroups; k_shade<ShadeWaves8, ...> (shade_waves): 64 VGPRs = a fourth (forced to 64 with packed FP32 selected: 15-28 spills, 92 -> 109 ms per cfg4 step; 1024-thread workgroups: one per CU, every barrier stalls the CU)
constexpr uint32_t kTraceBlock = 1024;          // trace kernels: one workgroup per CU stages the BVH into LDS once per launch
constexpr uint32_t kLdsStack = 16;              // traversal-stack entries per lane kept in LDS (deeper ones spill to scratch)
constexpr uint32_t kLdsStackWide = 12;          // ... with binary16 records but u32 entries (> 32768 records or spheres): 48 KB, so that two workgroups still share a CU
constexpr uint32_t kLeafBit = 0x80000000u;      // child reference flag (bvh_layout.hpp)
constexpr uint32_t kStack = 64;                 // Stack<StackFrame,64>, BVH.hpp:321
constexpr uint32_t kDestAccum = 0x80000000u;    // shadow-entry destination flag: the path ended at this hit (counted as terminated once its shadow ray is done)

struct SceneDev {
	const float4* recs;         // GPU-internal child-pair records, 4 float4 each, breadth-first (bvh_layout.hpp)
	const float4* spheres;      // acceleration_structure.prims (BVH order): {pos.xyz, radius_sq}
	const int32_t* prim_mat;    //   "  material_ID
	const float4* light_sphere; // per light (lighting_acceleration.prims order): scene.geometry[light] = {pos.xyz, radius_sq} (Renderer.hpp:261-262)
	const float4* light_emit;   //   "   {emission of its material .xyz, bits of the geometry-order prim id} (Renderer.hpp:263,283)
	const float4* mat_albedo;   // scene.material[].albedo
	const float4* mat_emission; // scene.material[].emission
	const float4* hdri;         // sky.hdri_data RGBA
	const float4* mat_glass;    // scene.material[]: {transmission.rgb, 1 + IOR_minus_one} — read by the GLASS instantiations of k_shade only (mirt_set_transmission)
	uint32_t n_spheres, n_recs, n_mat, n_lights;
	uint32_t lds_recs;          // records [0, lds_recs) are staged in LDS by the trace kernels (top of the tree)
	uint32_t lds_spheres;       // spheres [0, lds_spheres) likewise (all of them, or none)
	uint32_t half_boxes;        // 1: recs are the 32-B binary16 records (2 float4 each)
	uint32_t wide;              // 1 (with half_boxes): recs are 64-B binary16 records of up to FOUR children (bvh_layout.hpp build_wide_half_records)
	uint32_t chunk_max;         // rays per reservation from a launch's work counter, upper limit (pick_chunk)
	uint32_t leaf_batch;        // lanes of a wave that must stand at a leaf before it runs a leaf pass (trace_persistent)
	uint32_t refill_idle;       // idle lanes of a wave that trigger a refill (trace_persistent)
	uint32_t stack16;           // 1: record and prim indices fit 15 bits and the LDS stack holds u16 entries (binary16 records, <= 32768 records and spheres)
	float ambient[3];
	int32_t hdri_w, hdri_h;
	float hdri_fw, hdri_fh;
	uint32_t has_ambient;       // Renderer.hpp:79
	uint32_t use_bvh;
};

// RayStream<>::Buffer, DataStreams.hpp:75-88 — 16-byte records, `capacity` rays per plane: a lane moves a ray with two dwordx4 (and one dwordx2)
// instead of one dword per member.  40 B per ray.
struct StreamBuf {
	float4* a;                  // {p.xyz, bits of path}: path = (batch slot << FrameParams::pix_bits) | local pixel index (tile_local*256 + ID); stands in for pixelID + seed[]
	                            // (k_shade<GLASS> also sets kViaInterface in this word, k_shade<MIXED> kSampledGGX; no other kernel reads it: k_trace takes p only, and a shadow record gets the bare id)
	float4* b;                  // {dir.xyz, throughput.r}
	float2* c;                  // {throughput.g, throughput.b} — read by the hits only (the miss shader scales by throughput.r, Q10)
	                            // (radiance has no plane: a path's running sum is its word of the contribution buffer, contrib_index)
	                            // (`pdf` has no plane: Closure::pdf of the sampled direction is (1/pi) max(0, dir.z) of the WORLD-space dir
	                            //  (Q8, Renderer.hpp:386,401), a function of the stored direction, recomputed by the bounce that needs it)
	float* w;                   // mirt_set_sky_sampling only (nullptr otherwise, and no other kernel than k_shade<SKY> names it): the MIS weight the miss shader gives
	                            // thr.r x sky should this ray miss — the power heuristic of the closure's LOCAL pdf of the direction against the sky's (k_shade, SKY)
	                            // (mirt_set_ggx_pdf adds one more 4-byte plane per stream, out->pdf of the closure sample that made the ray.  It is NOT a member: this
	                            //  struct is an argument of every trace kernel too, and growing it moves their and the SKY kernels' scalar registers.  k_shade takes
	                            //  the two planes as its last arguments, pdf_plane_in / pdf_plane_out, which only its PDF instantiations name.)
};
// RayStream<>::ShadowStream, DataStreams.hpp:113-126, plus the deferred-add operands.  A record holds its own ray — k_trace's refill is two
// independent dwordx4 — and is 48 B for the common case (64 B with the emissive add); the path radiance waits in the path's contribution word.
struct ShadowBuf {
	float4* a;                  // {origin.xyz, tfar}
	float4* b;                  // {dir.xyz, bits of dest}: dest = path id | kDestAccum (the path ended at this hit) | kDestFull
	float4* c;                  // {NEE radiance carried by the shadow ray, unused}
	float4* d;                  // kDestFull records only: {emissive add of this bounce, unused}
};
struct FrameParams {
	CameraParams cam;
	uint32_t h_tiles;           // Renderer.hpp:59
	uint32_t first_tile;        // first global LaunchIndex owned by this context
	uint32_t run_tiles;         // the context owns runs of run_tiles consecutive LaunchIndices, stride_tiles apart (interleaved tile rows,
	uint32_t stride_tiles;      // mirt_set_tile_rows); stride_tiles = 0: one contiguous range (mirt_set_tile_range)
	uint32_t n_pix;             // local pixels = local tiles * 256
	uint32_t pix_bits;          // a path id is (batch slot << pix_bits) | local pixel, below 2^30: the fewer pixels a context owns, the more
	uint32_t pix_mask;          // accumulations fit a batch ((1 << pix_bits) - 1)
	uint32_t acc_base;          // `accumulations` before this batch
	uint32_t batch_n;           // accumulations in flight in this batch = slots of its contribution buffer [tile][slot][256][rgb]
	uint32_t max_bounces;
	uint32_t buckets;
	uint32_t mis;               // MIS && light_count > 0 (Q12 guard)
	uint32_t n_lights;
	uint32_t first_groups;      // k_shade<FIRST>: a chunk of 512 pixels x the batch's accumulations is handed out in this many pieces (small images: enough pieces for an even load)
	float inv_n_pix, inv_h_tiles, inv_run_tiles;   // 1/n_pix, 1/h_tiles, 1/run_tiles for udiv_f (no integer division in the kernels)
};
// RayStream<>::Hit, DataStreams.hpp:90-111 (tfar, primID; matID is looked up by the shader): ONE 8-B record per ray, written by the lane that finished
// the ray and read back by k_shade with one instruction each (two dword planes until round 3: two scattered 4-B stores and loads per ray).
struct alignas(8) HitRec { float tfar; int32_t prim; };
struct DevCounters {
	unsigned long long rays, shadow_rays, nodes, spheres, shadow_nodes, shadow_spheres, terminated, dropped;
};

// A ray queue's counters (kernels.hpp "ray queues"): kSegs dense segments, one counter per 128-B line.
constexpr uint32_t kSegs = 8;
constexpr uint32_t kSegPitch = 32;              // u32 words between two segment counters (128 B)
struct Queue { uint32_t* n; uint32_t seg_cap; };  // n[k * kSegPitch] = rays in segment k
// Launch-shape defaults of the persistent trace kernels (kernels.hpp "persistent waves with in-kernel lane refill") and the fat-ray list.
constexpr uint32_t kChunkMax = 512;    // default of SceneDev::chunk_max.  Measured (k_trace ms per step, 256 / 512 / 4096): cfg2 14.9 / 13.6 / 14.1, cfg4 - / 381.5 / 402.3 (larger chunks: uneven tails)
constexpr uint32_t kLeafBatch = 16;    // default of SceneDev::leaf_batch.  Measured (k_trace ms per cfg4 step; 8 / 16 / 24 / 32 / 40): 252.9 / 247.7 / 253.1 / 274.2 / 314.8; before the split 284.9
constexpr uint32_t kRefillIdle = 32;   // measured on cfg2: 8 -> 15.3 ms of trace per step, 16 -> 13.9, 24..40 -> 13.5 (a refill runs the ~200-instruction ray set-up on the whole wave)
struct FatList { uint32_t* count; uint32_t* rays; uint32_t capacity; };
constexpr uint32_t kBruteChunk = 1024;   // 16 KiB of float4
// The first-hit AOV slab (kernels.hpp "FIRST BOUNCE OUTPUTS").
constexpr uint32_t kAovPlanes = 7;
constexpr float kAovMissDepth = 1e4f;             // Renderer.hpp:228
// The sampling table of the environment map (kernels.hpp "The environment map as a light": the layout is described there).
struct SkyTable {
	const float* t;             // nullptr: no table (the switch is off)
	uint32_t rows, cols;
	MIRT_DI const float* marg() const { return t; }
	MIRT_DI const float* rowsum() const { return t + rows; }
	MIRT_DI const float* tn() const { return t + 2u * rows; }
	MIRT_DI const float* ts() const { return t + 3u * rows + 1u; }
	MIRT_DI const float* cond() const { return t + 4u * rows + 2u; }
	MIRT_DI const float* dens() const { return t + 4u * rows + 2u + static_cast<size_t>(rows) * cols; }
};
inline size_t sky_table_floats(uint32_t rows, uint32_t cols) { return 4u * static_cast<size_t>(rows) + 2u + 2u * static_cast<size_t>(rows) * cols; }

// mirt_render_atrous (denoise.hpp): the pixel block of a pass, and the largest step whose pass stages its block in LDS (the default of MIRT_TUNE_DENOISE_STAGED).
constexpr uint32_t kAtrousBlock = 16u;                     // pixels a side: a tile of the image
constexpr uint32_t kAtrousStagedMaxStep = 2u;

} // namespace mirt
