// ctx.hpp — the context behind the C-ABI (include/mirt.h), shared by its three layers:
//   mirt_capi.hip     the API layer: entry points that validate, edit context state and call the launch layer.  It includes no kernel.
//   mirt_launch.hip   the launch layer: the batch pipeline, the kernel tables and every launch of kernels.hpp, id_map.hpp, refit.hpp,
//                     light_list.hpp and sun_sky.hpp.  Its functions are declared at the end of this file.
//   mirt_resolve.hip  the resolve layer: everything that reads a finished accumulator (resolve.hpp, denoise.hpp, temporal.hpp).
// Only the kernel-side TYPES are included here (kernel_types.hpp), never a kernel.
//
// Ownership: every device allocation, stream and event is a member with a destructor (DeviceBuffer, Stream, Event), grouped by lifetime into
// the member structs of mirt_ctx.  A new buffer is a member of the group whose lifetime it shares; nothing is released by name anywhere.
#pragma once
#include "../../include/mirt.h"
#include "kernel_types.hpp"
#include "sun_sky_host.hpp"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#pragma GCC visibility push(hidden)      // shared between the layers, not exported: libmirt.so's symbols are those of mirt.h

struct DeviceBuffer {
	void* ptr = nullptr;
	size_t bytes = 0;
	DeviceBuffer() = default;
	DeviceBuffer(DeviceBuffer&& o) noexcept : ptr(std::exchange(o.ptr, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
	DeviceBuffer& operator=(DeviceBuffer&& o) noexcept { if (this != &o) { release(); ptr = std::exchange(o.ptr, nullptr); bytes = std::exchange(o.bytes, 0); } return *this; }
	~DeviceBuffer() { release(); }
	hipError_t ensure(size_t want) {
		if (want <= bytes && ptr) return hipSuccess;
		release();
		if (want == 0) return hipSuccess;
		hipError_t e = hipMalloc(&ptr, want);
		if (e == hipSuccess) bytes = want;
		return e;
	}
	void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; bytes = 0; }
	template <class T> T* as() const { return static_cast<T*>(ptr); }
};
// Function-local buffers of the debug entry points: freed on every return path, as any DeviceBuffer is.
using ScopedBuffer = DeviceBuffer;

// A HIP stream / event that goes with its owner.  Created through `s` / `e`; read as the handle itself.
struct Stream {
	hipStream_t s = nullptr;
	Stream() = default;
	Stream(Stream&& o) noexcept : s(std::exchange(o.s, nullptr)) {}
	~Stream() { if (s) (void)hipStreamDestroy(s); }
	operator hipStream_t() const { return s; }
};
struct Event {
	hipEvent_t e = nullptr;
	Event() = default;
	Event(Event&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
	~Event() { if (e) (void)hipEventDestroy(e); }
	operator hipEvent_t() const { return e; }
};

struct TimedLaunch { int klass; hipEvent_t start, stop; };

// One batch in flight: its own HIP stream, ray streams and contribution buffer.  Move-only, built in place (ensure_streams).  Destroyed — events,
// buffers, then the stream: members in reverse order — only after the caller has synchronised every stream.
struct PipeSlot {
	Stream stream;
	DeviceBuffer arena;              // ray streams
	DeviceBuffer counts;             // ray queue counters, work counters and fat-ray counts of one batch: addressed through BatchCounters only
	DeviceBuffer contrib;            // this batch's path radiances, [tile][slot][256][rgb] (kernels.hpp contrib_index)
	DeviceBuffer fat;                // fat-ray index lists: [closest kFatCapacity][shadow kFatCapacity]
	DeviceBuffer sky_w;              // mirt_set_sky_sampling(1) only: StreamBuf::w of the two ray streams, one 4-byte plane each
	DeviceBuffer pdf_p;              // mirt_set_ggx_pdf(1) only: one more 4-byte plane for each of the two ray streams (k_shade's pdf_plane_in / pdf_plane_out)
	float* pdf_plane[2]{};           // ... the plane of stream_buf[b]; nullptr while the switch is off
	Event batch_done;                // recorded on `stream` after the batch's last kernel
	Event merged;                    // recorded on the main stream after the batch was merged (slot reusable)
	Event aov_done;                  // mirt_set_aov(1) only: recorded on `stream` after the batch's k_first_hit_aov (created by the first such batch)
	bool in_use = false;
	uint64_t cand_gen = 0;           // the build of the context's candidate lists this slot's stream has waited for (CandidateLists::cand_gen)
	uint64_t listed_gen = 0;         // likewise for CandidateLists::listed_active
	mirt::StreamBuf stream_buf[2]{};
	mirt::ShadowBuf shadow_buf{};
	mirt::HitRec* hit = nullptr;     // RayStream<>::Hit: one 8-B {tfar, primID} record per ray (two planes' worth of the arena)
	PipeSlot() = default;
	PipeSlot(PipeSlot&&) = default;
};

// ---- the member structs of mirt_ctx: one per lifetime, each with at most one drop() -------------------------------------------------------
// The scene on the device, from mirt_set_scene until the next one (the two in-place updates edit it).
struct SceneTablesDev {
	DeviceBuffer recs, recs_wide, spheres, prim_mat, light_sphere, light_emit, mat_albedo, mat_emission, mat_ggx, mat_glass, hdri;
	// mirt_update_spheres: what the refit reads besides the records (refit.hpp RefitLinks; one allocation, built from the records by the first refit of a
	// tree, invalidated by mirt_set_scene), the uploaded edit list, and the host side of the light table (ids and rows as mirt_set_scene flattened them)
	DeviceBuffer refit_links, refit_edits;
	bool refit_links_valid = false;
	std::vector<int32_t> light_ids;
	std::vector<float4> light_sphere_host;
	// mirt_update_materials: the authoring-order geometry on the device (light_list.hpp GeometryTable: what the light tables are regenerated from; uploaded
	// by mirt_set_scene, kept current by both updates), the workgroup totals of the compaction with the count behind them, and the emission rows as uploaded
	DeviceBuffer geo_sphere, geo_mat, light_scan;
	std::vector<float4> emi_host;
	std::vector<float4> glass_host;  // the scene's {transmission.rgb, 1 + IOR_minus_one} per material, as uploaded: what the switch validates and looks for glass in
	std::vector<float4> alb_host, ggx_host;   // the scene's {albedo} and {F0, roughness} rows as uploaded: what the merged colour table below is made from
	DeviceBuffer mat_merged;         // MIXED only: per material the colour of its closure, for k_first_hit_aov; uploaded by the first launch that reads it after a change
	bool mat_merged_valid = false;
	DeviceBuffer gloss_decay_dev;    // the gloss decay table as k_tile_stream reads it (its bounce loop runs inside the kernel); uploaded by the first launch after a change
	bool gloss_decay_dev_valid = false;
};
// Candidate lists of the camera rays (k_primary_cand, kernels.hpp kCollect).  They are a function of the scene and its tree, the camera, the image
// size and the tiles this context owns — not of the accumulation index, the batch size or any random draw — so the first batch that wants them
// builds them on the main stream and every later batch on every slot reads them, until a call that changes one of those clears cand_valid.
struct CandidateLists {
	DeviceBuffer cand;               // per local pixel: candidate spheres of its bundle of camera rays, kCandStride words
	DeviceBuffer cand_listed;        // the local pixels without a list (more than kCandMax candidates), in any order: k_trace<kPrimaryList> traces all their samples
	DeviceBuffer cand_words;         // the build's own counter words: addressed through CandWords only
	Event cand_built;                // recorded on the main stream after the latest build; batches on other streams wait for it
	uint64_t cand_gen = 0;           // number of builds so far
	bool cand_valid = false;
	DeviceBuffer listed_active;      // word 0: count, words 1..: cand_listed ∩ active tiles (k_listed_active), what k_trace<., kPrimaryList> traces once a tile is frozen
	Event listed_built;              // recorded on the main stream after the latest k_listed_active; batches on other streams wait for it
	uint64_t listed_for_cand = 0, listed_for_freeze = 0, listed_gen = 0;   // the lists' build and the mask listed_active was made from; its own build number
};
// Per-tile adaptive sampling (mirt_freeze_tiles): a frozen tile takes no more samples until the accumulator is zeroed or overwritten.  Frozen
// sets only grow, so every active tile's count is `accumulations`; a frozen tile's is the value `accumulations` had when it froze.
struct Freezes {
	std::vector<uint8_t> frozen;     // per local tile; empty = none
	std::vector<uint32_t> frozen_at; // count of a frozen tile
	uint32_t n_frozen = 0;           // 0: every launch is the one of a context without the feature
	DeviceBuffer tile_frozen;        // the mask as the sparse kernels read it, one word per local tile
	DeviceBuffer active_list;        // word 0: local pixels of the active tiles, words 1..: those pixels (mirt_freeze_tiles; what k_trace<., kPrimaryActive> traces, list and count as kPrimaryList's)
	DeviceBuffer tile_counts;        // per-tile counts for the resolves (uploaded by the call that resolves)
	uint64_t freeze_gen = 0;         // number of mask changes so far
	// No tile is frozen (host state only: the device copies are read while n_frozen != 0 and rewritten by the call that raises it).
	void drop() { frozen.clear(); frozen_at.clear(); n_frozen = 0; }
};
// mirt_set_sky_sampling: the sampling table of the environment map, held only while the switch is on and a scene is set.
struct SkySampling {
	DeviceBuffer table;              // kernel_types.hpp SkyTable, built by build_sky_table beside the scene's `hdri`
	mirt::SkyTable dev{};            // ... as the kernels see it (t = nullptr: none)
	float total = 0.0f;              // the table's last marginal running sum; 0 (a black map, no ambient light): the switch changes no launch
	void drop() { table.release(); dev = mirt::SkyTable{}; total = 0.0f; }
};
// mirt_render_atrous (denoise.hpp): full-image float4 buffers, cv ping-pong; allocated by the first call, dropped by mirt_resize.
struct DenoiseScratch {
	DeviceBuffer cv[2], gd, mu;
	void drop() { for (DeviceBuffer* b : { &cv[0], &cv[1], &gd, &mu }) b->release(); }
};
// mirt_render_temporal (temporal.hpp): the history — (x, v), the guides and the length in samples of the last call with update = 1, the camera
// and the demodulation settings it was taken under — plus one float image of scratch for the lengths a call writes and the five class counts.
// mirt_set_sphere_motion(1): the history also carries the id map of the call that wrote it (id; id_cur: this call's, renamed with update = 1 as
// the guides are) and the sphere table it was taken under (snap, copied when a call with update = 1 finds the table changed since the last copy:
// spheres_gen of the geometry context counts its mirt_update_spheres calls).  id_out / id_words: mirt_id_map's two planes and k_id_map's counter words.
struct History {
	DeviceBuffer x, g, n, len, stats;
	bool valid = false;
	mirt::CameraParams cam{};
	uint32_t demodulate = 0, width = 0, height = 0;
	float albedo_floor = 0.0f;
	DeviceBuffer id, id_cur, snap, id_out, id_words;
	bool snap_valid = false;
	uint64_t snap_gen = 0;
	// The history goes (mirt.h "history lifetime"); the scratch (len, stats, id_out, id_words) stays.  The caller has made the context's device the current one.
	void drop() {
		for (DeviceBuffer* b : { &x, &g, &n, &len, &id, &id_cur, &snap }) b->release();
		valid = false; snap_valid = false;
	}
};
// mirt_noise / mirt_tile_above: one float4 record and one count per local tile, MIRT_NOISE_BINS histogram words (allocated by the first call).
struct NoiseScratch { DeviceBuffer above, rec, hist; };
// Launch-shape knobs for measurements (profiles/gpu_cycle.sh A/B runs), read from the environment at mirt_create: MIRT_TUNE_TRACE_WGS /
// MIRT_TUNE_SHADE_WGS = workgroups per CU, MIRT_TUNE_CHUNK = rays per work reservation, MIRT_TUNE_LEAF_BATCH = lanes at a leaf that
// trigger a leaf pass, MIRT_TUNE_REFILL_IDLE = idle lanes that trigger a refill.  They never change results.
struct TuneKnobs {
	uint32_t trace_wgs = 2, shade_wgs = 0, chunk = mirt::kChunkMax, leaf_batch = mirt::kLeafBatch, refill_idle = mirt::kRefillIdle, wide = 1;
	uint32_t denoise_staged = mirt::kAtrousStagedMaxStep;   // MIRT_TUNE_DENOISE_STAGED: largest a-trous step whose pass stages its block in LDS (0: none do; profiles/denoise.txt)
};
// policy.profile: the bracketing events of the launches not harvested yet, and the pool they return to.
struct Profiling {
	std::vector<TimedLaunch> pending;
	std::vector<hipEvent_t> free_events;
	mirt_kernel_times times{};
	Profiling() = default;
	Profiling(const Profiling&) = delete;
	Profiling& operator=(const Profiling&) = delete;
	~Profiling() {
		for (const TimedLaunch& t : pending) { (void)hipEventDestroy(t.start); (void)hipEventDestroy(t.stop); }
		for (hipEvent_t e : free_events) (void)hipEventDestroy(e);
	}
};
// The pinned staging copy of the framebuffer for mirt_render (pageable memory halves the copy rate).
struct PinnedFrame {
	float* ptr = nullptr;
	size_t bytes = 0;
	PinnedFrame() = default;
	PinnedFrame(const PinnedFrame&) = delete;
	PinnedFrame& operator=(const PinnedFrame&) = delete;
	~PinnedFrame() { release(); }
	void release() { if (ptr) (void)hipHostFree(ptr); ptr = nullptr; bytes = 0; }
};

// Members are destroyed in reverse order: the main stream is declared first, so every buffer, event and slot goes before it.
struct mirt_ctx {
	int device = 0;
	int n_cu = 256;
	Stream stream;
	std::string error;

	mirt_policy policy{ 16, 5, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0 };         // RendererPolicy defaults, Renderer.hpp:19-26,41,71; USEBVH false BVH.hpp:307; BRDF 0 :70
	uint32_t width = 0, height = 0, h_tiles = 0, v_tiles = 0;
	uint32_t first_tile = 0, n_tiles = 0;
	uint32_t run_tiles = 1, stride_tiles = 0;   // interleaved tile rows (mirt_set_tile_rows); stride 0 = one contiguous range: see tile_map()
	uint32_t accumulations = 0;
	bool have_scene = false, have_camera = false;

	// scene
	SceneTablesDev tables;
	mirt::SceneDev scene{};
	bool env_baked = false;          // the environment map in `tables.hdri` was written by k_sun_sky (mirt_set_sun_sky), not handed over by the caller
	uint32_t transmission = 0;       // mirt_set_transmission: 1 = a transmissive material takes the dielectric interface (the GLASS instantiations of k_shade)
	bool scene_has_glass = false;    // some material of the scene has max(transmission) > 0: only then does the switch change the kernels launched
	uint32_t sky_sampling = 0;       // mirt_set_sky_sampling: 1 = the environment map is one more NEE light (the SKY instantiations of k_shade, while sky_active())
	SkySampling sky;
	uint32_t ggx_pdf = 0;            // mirt_set_ggx_pdf: 1 = Closure<GGX>::pdf is ggx_pdf in the MIS weights (the PDF instantiations of k_shade, while a material of the scene ends up GGX)
	// mirt_set_material_closures: closure (0 Lambertian, 1 GGX) of material m; a material at or beyond its end takes policy.brdf.  Empty (the default):
	// every launch is the one of a context without the call.  What a launch does with it is closure_plan()'s to say, and nobody else's.
	std::vector<uint8_t> closures;
	std::vector<float> gloss_decay;  // gloss_decay_table (Renderer.hpp:212) by bounce, read at launch (mirt_set_gloss_decay); missing entries are 0
	uint32_t light_ris = 0;          // mirt_set_light_ris: candidates per NEE light pick; 0 = the uniform draw, the kernels without the candidate loop
	uint32_t stream_order = 0;       // mirt_set_stream_order: 1 = a batch is one k_tile_stream launch (the reference's stream slots and scalar tail, brute force)
	mirt::CameraParams camera{};
	mirt::LensParams lens{};         // mirt_set_lens: aperture > 0 = every camera ray is a thin-lens ray (the LENS kernels); the axes follow the camera (update_lens_axes)
	uint32_t bvh_depth = 0;
	CandidateLists lists;
	bool allow_half = true;           // binary16 records when adequate (mirt_debug_set(ctx, "half_boxes", 0) forces f32)

	// frame state
	DeviceBuffer accumulator;        // [local tile][bucket][3][256] f32
	uint32_t aov_on = 0;             // mirt_set_aov: every batch also sums its camera rays' depth, normal and closure colour
	DeviceBuffer aov;                // [local tile][plane 0..6][256] f32 (kernels.hpp k_first_hit_aov); allocated while aov_on
	hipEvent_t aov_prev = nullptr;   // aov_done of the latest pipelined batch: the next batch's k_first_hit_aov waits for it (borrowed from its slot)
	DeviceBuffer framebuffer;        // width*height float4
	PinnedFrame frame_host;
	DeviceBuffer counters;           // DevCounters
	NoiseScratch noise;
	DenoiseScratch dn;
	History hist;
	uint32_t history_motion = 0;     // mirt_set_sphere_motion
	uint64_t spheres_gen = 0;        // mirt_update_spheres calls so far (what a history's snapshot is compared with)
	mirt_ctx* motion_geometry = nullptr;   // mirt_set_motion_geometry: the context whose scene the id map and the sphere tables are read from (NULL: this one)
	std::vector<PipeSlot> slots;     // batches in flight (policy.streams)
	uint64_t planned_for = 0;        // local pixel count batch_mem_cap was planned for (0 = plan again)
	uint32_t batch_mem_cap = 256;     // accumulations per batch the device memory allows (lowered by ensure_streams when the plan does not fit)
	uint32_t capacity = 0;           // rays per stream plane (= kSegs * seg_cap)
	uint32_t seg_cap = 0;            // slots per queue segment
	uint32_t arena_bounces = 0;
	uint64_t batch_seq = 0;
	Freezes freeze;

	uint32_t deferred = 0;            // Accumulate() calls accepted by mirt_accumulate_async but not launched yet (fewer than a batch)
	TuneKnobs tune;
	bool debug_poison_contrib = false;   // MIRT_DEBUG_POISON_CONTRIB=1: fill every contribution buffer with a NaN pattern before each batch (tests: every word is written)
	Profiling prof;
};

// ---- what every layer uses of the context -----------------------------------------------------------------------------------------
inline thread_local std::string g_create_error;
inline int fail(mirt_ctx* ctx, int code, const char* fmt, ...) {
	char buf[512];
	va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
	if (ctx) ctx->error = buf; else g_create_error = buf;
	return code;
}
#define HIP_TRY(ctx, expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return fail(ctx, MIRT_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); } while (0)

inline hipError_t sync_all(mirt_ctx* c) {
	for (PipeSlot& sl : c->slots) if (sl.stream) { hipError_t e = hipStreamSynchronize(sl.stream); if (e != hipSuccess) return e; }
	return hipStreamSynchronize(c->stream);
}
inline uint32_t grid_for(const mirt_ctx* c, uint64_t work_items) {
	uint64_t blocks = (work_items + mirt::kBlock - 1) / mirt::kBlock;
	const uint64_t cap = static_cast<uint64_t>(c->n_cu) * 8u;      // grid-stride beyond 8 workgroups per CU
	if (blocks > cap) blocks = cap;
	if (blocks < 1) blocks = 1;
	return static_cast<uint32_t>(blocks);
}

// ---- launch bracketing (policy.profile) ---------------------------------------------------------
inline hipEvent_t take_event(mirt_ctx* c) {
	if (!c->prof.free_events.empty()) { hipEvent_t e = c->prof.free_events.back(); c->prof.free_events.pop_back(); return e; }
	hipEvent_t e = nullptr;
	(void)hipEventCreate(&e);
	return e;
}
inline void harvest(mirt_ctx* c) {
	if (c->prof.pending.empty()) return;
	(void)sync_all(c);
	for (TimedLaunch& t : c->prof.pending) {
		float ms = 0.0f;
		if (hipEventElapsedTime(&ms, t.start, t.stop) == hipSuccess) { c->prof.times.ms[t.klass] += ms; c->prof.times.launches[t.klass]++; }
		c->prof.free_events.push_back(t.start); c->prof.free_events.push_back(t.stop);
	}
	c->prof.pending.clear();
}
struct Bracket {
	mirt_ctx* c; int klass; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
	Bracket(mirt_ctx* ctx, int k, hipStream_t stream = nullptr) : c(ctx), klass(k), st(stream ? stream : static_cast<hipStream_t>(ctx->stream)) {
		if (c->policy.profile) { a = take_event(c); b = take_event(c); (void)hipEventRecord(a, st); }
	}
	~Bracket() {
		if (c->policy.profile) { (void)hipEventRecord(b, st); c->prof.pending.push_back(TimedLaunch{ klass, a, b }); }
	}
};

inline bool lens_on(const mirt_ctx* c) { return c->lens.aperture > 0.0f; }
// The context's n_tiles local tiles in the image (tile_map.hpp).
inline mirt::TileMap tile_map(const mirt_ctx* c) { return mirt::TileMap{ c->first_tile, c->run_tiles, c->stride_tiles, c->h_tiles, c->width }; }
inline uint32_t tile_count(const mirt_ctx* c, uint32_t local) { return (c->freeze.n_frozen && c->freeze.frozen[local]) ? c->freeze.frozen_at[local] : c->accumulations; }

inline int check_ready(mirt_ctx* c) {
	if (!c) return MIRT_ERR_ARG;
	if (!c->have_scene) return fail(c, MIRT_ERR_STATE, "mirt_set_scene has not been called");
	if (!c->have_camera) return fail(c, MIRT_ERR_STATE, "mirt_set_camera has not been called");
	if (c->width == 0 && c->height == 0) return fail(c, MIRT_ERR_STATE, "mirt_resize has not been called");
	return MIRT_OK;
}

template <class T>
int upload(mirt_ctx* c, DeviceBuffer& buf, const std::vector<T>& host) {
	HIP_TRY(c, buf.ensure(std::max<size_t>(host.size(), 1) * sizeof(T)));
	if (!host.empty()) HIP_TRY(c, hipMemcpyAsync(buf.ptr, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
	return MIRT_OK;
}

// ---- what exact stream order excludes: the rows are named here because two layers refuse by them (the table itself: mirt_capi.hip) -------
enum ExactRow { X_LENS, X_FROZEN, X_LIGHT_RIS, X_TRANSMISSION, X_SKY_SAMPLING, X_GGX_PDF, X_CLOSURES, X_AOV, X_ROWS };
int refuse_under_exact_order(mirt_ctx* c, ExactRow row);                     // mirt_capi.hip

// ---- the launch layer (mirt_launch.hip) ---------------------------------------------------------------------------------------------
// mirt_set_scene's arguments, and the records the kernels walk for them (host copies: they outlive the stream synchronisation that ends their uploads).
struct SceneArgs {
	const mirt_sphere *geometry, *bvh_prims; uint32_t n_spheres;
	const mirt_bvh_node* nodes; uint32_t n_nodes;
	const mirt_material* materials; uint32_t n_materials;
	const int32_t* lights; uint32_t n_lights;
	const float *ambient_color, *hdri_rgba; uint32_t hdri_w, hdri_h;
};
struct SceneRecords {
	std::vector<float> f32;                 // host copies, as in SceneTables
	std::vector<uint32_t> half, wide;
	uint32_t n_recs = 0, depth = 0;
	bool is_half = false, is_wide = false;
	bool in_recs_wide = false;              // the records lie in tables.recs_wide instead of tables.recs (the GPU builder writes both layouts)
};
// The launch rule of mirt_set_material_closures (closure_plan, mirt_launch.hip).
struct ClosurePlan { bool mixed, ggx; unsigned long long mask; };

uint32_t batch_limit(const mirt_ctx* c);
uint32_t wanted_slots(const mirt_ctx* c);
void plan_batches(mirt_ctx* c);
int ensure_streams(mirt_ctx* c);
int launch_batch(mirt_ctx* c, uint32_t batch_n);
// The preambles of an entry point (their order of steps is stated beside their definitions and nowhere else).
int flush_deferred(mirt_ctx* c);
int flush_and_wait(mirt_ctx* c);
int drop_and_wait(mirt_ctx* c);
ClosurePlan closure_plan(const mirt_ctx* c);
int build_scene_records(mirt_ctx* c, const SceneArgs& a, const std::vector<float4>& sph, SceneRecords& t);
int plan_trace_lds(mirt_ctx* c);
int build_sky_table(mirt_ctx* c);
hipError_t bake_sun_sky(mirt_ctx* c, const mirt_sun_sky::Args& a, size_t n_texels, float4* dst);     // k_sun_sky on the main stream; not synchronised
int debug_trace(mirt_ctx* c, const char* who, size_t n, const float* p_xyz, const float* dir_xyz, const float* tfar, void* result);
int launch_id_map(mirt_ctx* c, const mirt_ctx* gs, int32_t* prim_dev, float* dist_dev);
// The device halves of mirt_update_spheres and mirt_update_materials: the caller has validated the edit and waited for every batch.
int launch_update_spheres(mirt_ctx* c, uint32_t n, const uint32_t* bvh_index, const uint32_t* geometry_index, const float* xyz_rsq);
int launch_update_materials(mirt_ctx* c, uint32_t n_assign, const uint32_t* bvh_index, const uint32_t* geometry_index, const int32_t* material_ID);

#pragma GCC visibility pop
