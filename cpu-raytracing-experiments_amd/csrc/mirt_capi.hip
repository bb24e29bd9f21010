// mirt_capi.hip — C-ABI (include/mirt.h) over the HIP kernels in kernels.hpp.
//
// Host-side stand-in for the state Renderer<Policy> keeps (Renderer.hpp:38-49): scene reference,
// accumulator, width/height, accumulations, h_tiles/v_tiles — with the scene copied to HBM, the
// accumulator resident in HBM in the reference's AccumulationTile layout, and the per-tile ray
// streams replaced by one set of frame-wide SoA streams (see kernels.hpp).
//
// There is no CPU fallback: every entry point that computes needs a gfx950 device and fails with
// MIRT_ERR_NO_DEVICE / MIRT_ERR_HIP otherwise.
#include "../../include/mirt.h"
#include "kernels.hpp"
#include "denoise.hpp"
#include "temporal.hpp"
#include "id_map.hpp"
#include "sun_sky.hpp"
#include "refit.hpp"
#include "light_list.hpp"
#include "scene_update_host.hpp"
#include "bvh_layout.hpp"
#include "bvh_build.hpp"
#include "lbvh_build.hpp"
#include "noise_host.hpp"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

using namespace mirt;

namespace {

thread_local std::string g_create_error;

struct DeviceBuffer {
	void* ptr = nullptr;
	size_t bytes = 0;
	hipError_t ensure(size_t want) {
		if (want <= bytes && ptr) return hipSuccess;
		if (ptr) { (void)hipFree(ptr); ptr = nullptr; bytes = 0; }
		if (want == 0) return hipSuccess;
		hipError_t e = hipMalloc(&ptr, want);
		if (e == hipSuccess) bytes = want;
		return e;
	}
	void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; bytes = 0; }
	template <class T> T* as() const { return static_cast<T*>(ptr); }
};

// Function-local buffers of the debug entry points: freed on every return path.
struct ScopedBuffer : DeviceBuffer {
	ScopedBuffer() = default;
	ScopedBuffer(const ScopedBuffer&) = delete;
	ScopedBuffer& operator=(const ScopedBuffer&) = delete;
	~ScopedBuffer() { release(); }
};

struct TimedLaunch { int klass; hipEvent_t start, stop; };

// One batch in flight: its own HIP stream, ray streams and contribution buffer.
struct PipeSlot {
	hipStream_t stream = nullptr;
	DeviceBuffer arena;              // ray streams
	DeviceBuffer counts;             // ray queue counters, work counters and fat-ray counts of one batch: addressed through BatchCounters only
	DeviceBuffer contrib;            // this batch's path radiances, [tile][slot][256][rgb] (kernels.hpp contrib_index)
	DeviceBuffer fat;                // fat-ray index lists: [closest kFatCapacity][shadow kFatCapacity]
	DeviceBuffer sky_w;              // mirt_set_sky_sampling(1) only: StreamBuf::w of the two ray streams, one 4-byte plane each
	DeviceBuffer pdf_p;              // mirt_set_ggx_pdf(1) only: one more 4-byte plane for each of the two ray streams (k_shade's pdf_plane_in / pdf_plane_out)
	float* pdf_plane[2]{};           // ... the plane of stream_buf[b]; nullptr while the switch is off
	hipEvent_t batch_done = nullptr; // recorded on `stream` after the batch's last kernel
	hipEvent_t merged = nullptr;     // recorded on the main stream after the batch was merged (slot reusable)
	hipEvent_t aov_done = nullptr;   // mirt_set_aov(1) only: recorded on `stream` after the batch's k_first_hit_aov (created by the first such batch)
	bool in_use = false;
	uint64_t cand_gen = 0;           // the build of the context's candidate lists this slot's stream has waited for (mirt_ctx::cand_gen)
	uint64_t listed_gen = 0;         // likewise for mirt_ctx::listed_active
	StreamBuf stream_buf[2]{};
	ShadowBuf shadow_buf{};
	HitRec* hit = nullptr;           // RayStream<>::Hit: one 8-B {tfar, primID} record per ray (two planes' worth of the arena)
	// Buffers, events and stream.  The caller has synchronised every stream.
	void release() {
		arena.release(); counts.release(); contrib.release(); fat.release(); sky_w.release(); pdf_p.release();
		for (hipEvent_t* e : { &batch_done, &merged, &aov_done }) { if (*e) (void)hipEventDestroy(*e); *e = nullptr; }
		if (stream) (void)hipStreamDestroy(stream);
		stream = nullptr;
	}
};

} // namespace

struct mirt_ctx {
	int device = 0;
	int n_cu = 256;
	hipStream_t stream = nullptr;
	std::string error;

	mirt_policy policy{ 16, 5, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0 };         // RendererPolicy defaults, Renderer.hpp:19-26,41,71; USEBVH false BVH.hpp:307; BRDF 0 :70
	uint32_t width = 0, height = 0, h_tiles = 0, v_tiles = 0;
	uint32_t first_tile = 0, n_tiles = 0;
	uint32_t run_tiles = 1, stride_tiles = 0;   // interleaved tile rows (mirt_set_tile_rows); stride 0 = one contiguous range: see tile_map()
	uint32_t accumulations = 0;
	bool have_scene = false, have_camera = false;

	// scene
	DeviceBuffer recs, recs_wide, spheres, prim_mat, light_sphere, light_emit, mat_albedo, mat_emission, mat_ggx, mat_glass, hdri;
	SceneDev scene{};
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
	bool env_baked = false;          // the environment map in `hdri` was written by k_sun_sky (mirt_set_sun_sky), not handed over by the caller
	uint32_t transmission = 0;       // mirt_set_transmission: 1 = a transmissive material takes the dielectric interface (the GLASS instantiations of k_shade)
	std::vector<float4> glass_host;  // the scene's {transmission.rgb, 1 + IOR_minus_one} per material, as uploaded: what the switch validates and looks for glass in
	bool scene_has_glass = false;    // some material of the scene has max(transmission) > 0: only then does the switch change the kernels launched
	uint32_t sky_sampling = 0;       // mirt_set_sky_sampling: 1 = the environment map is one more NEE light (the SKY instantiations of k_shade, while sky_active())
	DeviceBuffer sky_table;          // its sampling table (kernels.hpp SkyTable), built by build_sky_table beside `hdri`; held only while the switch is on and a scene is set
	SkyTable sky{};                  // ... as the kernels see it (t = nullptr: none)
	uint32_t ggx_pdf = 0;            // mirt_set_ggx_pdf: 1 = Closure<GGX>::pdf is ggx_pdf in the MIS weights (the PDF instantiations of k_shade, while a material of the scene ends up GGX)
	float sky_total = 0.0f;          // the table's last marginal running sum; 0 (a black map, no ambient light): the switch changes no launch
	// mirt_set_material_closures: closure (0 Lambertian, 1 GGX) of material m; a material at or beyond its end takes policy.brdf.  Empty (the default):
	// every launch is the one of a context without the call.  What a launch does with it is closure_plan()'s to say, and nobody else's.
	std::vector<uint8_t> closures;
	std::vector<float4> alb_host, ggx_host;   // the scene's {albedo} and {F0, roughness} rows as uploaded: what the merged colour table below is made from
	DeviceBuffer mat_merged;         // MIXED only: per material the colour of its closure, for k_first_hit_aov; uploaded by the first launch that reads it after a change
	bool mat_merged_valid = false;
	std::vector<float> gloss_decay;  // gloss_decay_table (Renderer.hpp:212) by bounce, read at launch (mirt_set_gloss_decay); missing entries are 0
	uint32_t light_ris = 0;          // mirt_set_light_ris: candidates per NEE light pick; 0 = the uniform draw, the kernels without the candidate loop
	uint32_t stream_order = 0;       // mirt_set_stream_order: 1 = a batch is one k_tile_stream launch (the reference's stream slots and scalar tail, brute force)
	DeviceBuffer gloss_decay_dev;    // the table as k_tile_stream reads it (its bounce loop runs inside the kernel); uploaded by the first launch after a change
	bool gloss_decay_dev_valid = false;
	CameraParams camera{};
	LensParams lens{};               // mirt_set_lens: aperture > 0 = every camera ray is a thin-lens ray (the LENS kernels); the axes follow the camera (update_lens_axes)
	uint32_t bvh_depth = 0;
	// Candidate lists of the camera rays (k_primary_cand, kernels.hpp kCollect).  They are a function of the scene and its tree, the camera, the image
	// size and the tiles this context owns — not of the accumulation index, the batch size or any random draw — so the first batch that wants them
	// builds them on the main stream and every later batch on every slot reads them, until a call that changes one of those clears cand_valid.
	DeviceBuffer cand;               // per local pixel: candidate spheres of its bundle of camera rays, kCandStride words
	DeviceBuffer cand_listed;        // the local pixels without a list (more than kCandMax candidates), in any order: k_trace<kPrimaryList> traces all their samples
	DeviceBuffer cand_words;         // the build's own counter words: addressed through CandWords only
	hipEvent_t cand_built = nullptr; // recorded on the main stream after the latest build; batches on other streams wait for it
	uint64_t cand_gen = 0;           // number of builds so far
	bool cand_valid = false;
	bool allow_half = true;           // binary16 records when adequate (mirt_debug_set(ctx, "half_boxes", 0) forces f32)

	// frame state
	DeviceBuffer accumulator;        // [local tile][bucket][3][256] f32
	uint32_t aov_on = 0;             // mirt_set_aov: every batch also sums its camera rays' depth, normal and closure colour
	DeviceBuffer aov;                // [local tile][plane 0..6][256] f32 (kernels.hpp k_first_hit_aov); allocated while aov_on
	hipEvent_t aov_prev = nullptr;   // aov_done of the latest pipelined batch: the next batch's k_first_hit_aov waits for it (borrowed from its slot)
	DeviceBuffer framebuffer;        // width*height float4
	float* frame_host = nullptr;     // pinned staging copy of the framebuffer for mirt_render (pageable memory halves the copy rate)
	size_t frame_host_bytes = 0;
	DeviceBuffer counters;           // DevCounters
	DeviceBuffer noise_above;        // mirt_tile_above: one count per local tile
	DeviceBuffer noise_rec, noise_hist;   // mirt_noise: one float4 record per local tile, MIRT_NOISE_BINS histogram words (allocated by the first call)
	DeviceBuffer dn_cv[2], dn_gd, dn_mu;  // mirt_render_atrous (denoise.hpp): full-image float4 buffers, cv ping-pong; allocated by the first call, released by mirt_resize
	// mirt_render_temporal (temporal.hpp): the history — (x, v), the guides and the length in samples of the last call with update = 1, the camera
	// and the demodulation settings it was taken under — plus one float image of scratch for the lengths a call writes and the five class counts.
	DeviceBuffer th_x, th_g, th_n, th_len, th_stats;
	bool th_valid = false;
	CameraParams th_cam{};
	uint32_t th_demodulate = 0, th_width = 0, th_height = 0;
	float th_albedo_floor = 0.0f;
	// mirt_set_sphere_motion(1): the history also carries the id map of the call that wrote it (th_id; th_id_cur: this call's, renamed with update = 1 as
	// the guides are) and the sphere table it was taken under (th_snap, copied when a call with update = 1 finds the table changed since the last copy:
	// spheres_gen of the geometry context counts its mirt_update_spheres calls).  id_out / id_words: mirt_id_map's two planes and k_id_map's counter words.
	uint32_t history_motion = 0;
	DeviceBuffer th_id, th_id_cur, th_snap, id_out, id_words;
	bool th_snap_valid = false;
	uint64_t th_snap_gen = 0, spheres_gen = 0;
	mirt_ctx* motion_geometry = nullptr;   // mirt_set_motion_geometry: the context whose scene the id map and the sphere tables are read from (NULL: this one)
	std::vector<PipeSlot> slots;     // batches in flight (policy.streams)
	uint64_t planned_for = 0;        // local pixel count batch_mem_cap was planned for (0 = plan again)
	uint32_t batch_mem_cap = 256;     // accumulations per batch the device memory allows (lowered by ensure_streams when the plan does not fit)
	uint32_t capacity = 0;           // rays per stream plane (= kSegs * seg_cap)
	uint32_t seg_cap = 0;            // slots per queue segment
	uint32_t arena_bounces = 0;
	uint64_t batch_seq = 0;

	// Per-tile adaptive sampling (mirt_freeze_tiles): a frozen tile takes no more samples until the accumulator is zeroed or overwritten.  Frozen
	// sets only grow, so every active tile's count is `accumulations`; a frozen tile's is the value `accumulations` had when it froze.
	std::vector<uint8_t> frozen;     // per local tile; empty = none
	std::vector<uint32_t> frozen_at; // count of a frozen tile
	uint32_t n_frozen = 0;           // 0: every launch is the one of a context without the feature
	DeviceBuffer tile_frozen;        // the mask as the sparse kernels read it, one word per local tile
	DeviceBuffer active_list;        // word 0: local pixels of the active tiles, words 1..: those pixels (mirt_freeze_tiles; what k_trace<., kPrimaryActive> traces, list and count as kPrimaryList's)
	DeviceBuffer tile_counts;        // per-tile counts for the resolves (uploaded by the call that resolves)
	DeviceBuffer listed_active;      // word 0: count, words 1..: cand_listed ∩ active tiles (k_listed_active), what k_trace<., kPrimaryList> traces once a tile is frozen
	hipEvent_t listed_built = nullptr; // recorded on the main stream after the latest k_listed_active; batches on other streams wait for it
	uint64_t freeze_gen = 0;         // number of mask changes so far
	uint64_t listed_for_cand = 0, listed_for_freeze = 0, listed_gen = 0;   // the lists' build and the mask listed_active was made from; its own build number

	uint32_t deferred = 0;            // Accumulate() calls accepted by mirt_accumulate_async but not launched yet (fewer than a batch)
	// launch-shape knobs for measurements (profiles/gpu_cycle.sh A/B runs), read from the environment at mirt_create: MIRT_TUNE_TRACE_WGS /
	// MIRT_TUNE_SHADE_WGS = workgroups per CU, MIRT_TUNE_CHUNK = rays per work reservation, MIRT_TUNE_LEAF_BATCH = lanes at a leaf that
	// trigger a leaf pass, MIRT_TUNE_REFILL_IDLE = idle lanes that trigger a refill.  They never change results.
	uint32_t tune_trace_wgs = 2, tune_shade_wgs = 0, tune_chunk = kChunkMax, tune_leaf_batch = kLeafBatch, tune_refill_idle = kRefillIdle, tune_wide = 1;
	uint32_t tune_denoise_staged = kAtrousStagedMaxStep;   // MIRT_TUNE_DENOISE_STAGED: largest a-trous step whose pass stages its block in LDS (0: none do; profiles/denoise.txt)
	bool debug_poison_contrib = false;   // MIRT_DEBUG_POISON_CONTRIB=1: fill every contribution buffer with a NaN pattern before each batch (tests: every word is written)
	// profiling
	std::vector<TimedLaunch> pending;
	std::vector<hipEvent_t> free_events;
	mirt_kernel_times times{};
};

namespace {

int fail(mirt_ctx* ctx, int code, const char* fmt, ...) {
	char buf[512];
	va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
	if (ctx) ctx->error = buf; else g_create_error = buf;
	return code;
}
#define HIP_TRY(ctx, expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return fail(ctx, MIRT_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); } while (0)

// Accumulations traced together as one batch (path id = (slot << pix_bits) | pixel below 2^30: bits 30 and 31 stay free for flags).
// Every launch of a batch ends in a tail while its longest rays finish and starts with the staging of the tree top, so
// launches want to be LARGE — and 288 GB of HBM is there to be used for ray streams (144 B per ray and batch in flight, + 12 B of contribution buffer).
// Measured on one MI355X (Mray/s; accumulations per batch x batches in flight on separate HIP streams):
//   cfg4 4096^2 S(100000):  5 x 3: 4919   8 x 1: 5435   16 x 1: 5726   32 x 1: 5838   16 x 2: 5013
//   one eighth of cfg4:     16 x 3: 4367  32 x 3: 4981  64 x 3: 5103   64 x 1: 5498
//   cfg3 1920x1088 S(10000): 16 x 3: 5378  32 x 3: 5753  64 x 3: 5700  64 x 1: 6354
//   cfg2 1024^2 S(1000):    32 x 3: 7510  64 x 3: 8011  64 x 1: 7654
// Hence: aim at 1 G primary rays per batch (round 2: 512 M; see kBatchRays) (at most max_slots() accumulations, at most what the free device memory holds), and keep
// ONE batch in flight once a batch carries 96 M primary rays or more — launches that fill the chip for milliseconds gain
// nothing from sharing it with another stream's kernels and lose to the interleaving — three below that (other batches fill the tails).
constexpr uint32_t kMaxBatch = 256;         // upper limit of accumulations per batch; a context's own limit is what its path ids hold (max_slots)
constexpr uint64_t kBatchRays = 1024ull << 20;   // round 3, cfg4 on the whole image (Mray/s, one batch in flight): 32 accumulations per batch 7970, 48: 8154, 63: 8218; 2 x 32: 7232, 2 x 24: 7192
constexpr uint64_t kSerialRays = 96ull << 20;
constexpr size_t kStreamPlanes = 2 * 10 + 2 + 16;      // two ray streams (40 B), hit (tfar, prim), shadow stream (four 16-B records): in 4-byte planes per ray of capacity
// Path id = (batch slot << pix_bits) | local pixel, below 2^30 (bits 30 and 31 of the words that carry it are flags): a context that owns
// all 2^24 pixels of a 4096^2 image has room for 64 slots, one that owns an eighth of it (a rank of an 8-GPU run) for 512.
uint32_t pix_bits_of(const mirt_ctx* c) { uint32_t b = 8; while ((1ull << b) < static_cast<uint64_t>(c->n_tiles) * kTileSize) b++; return b; }
// ... and a stream slot must stay below 2^30 as well (two flag bits in the words that carry it): pixels x slots + the padding of the kSegs queue segments
uint32_t max_slots(const mirt_ctx* c) {
	const uint64_t n_pix = std::max<uint64_t>(static_cast<uint64_t>(c->n_tiles) * kTileSize, 1);
	const uint64_t by_slots = ((1ull << 30) - 3ull * kSegs * kShadeBlock) / n_pix;
	return static_cast<uint32_t>(std::max<uint64_t>(std::min<uint64_t>(std::min<uint64_t>(kMaxBatch, 1u << (30u - std::min<uint32_t>(pix_bits_of(c), 24u))), by_slots), 1));
}
uint32_t batch_floor(const mirt_ctx* c) { return std::max<uint32_t>(std::min<uint32_t>(c->policy.buckets, 5u), 1u); }   // the reference's natural group: five calls, five buckets
uint32_t batch_limit(const mirt_ctx* c) {
	if (c->policy.max_batch) return std::min(c->policy.max_batch, max_slots(c));
	const uint64_t n_pix = static_cast<uint64_t>(c->n_tiles) * kTileSize;
	if (n_pix == 0) return 1;
	const uint64_t b = std::max<uint64_t>((kBatchRays + n_pix / 2) / n_pix, batch_floor(c));
	return static_cast<uint32_t>(std::min<uint64_t>(std::min<uint64_t>(b, max_slots(c)), std::max<uint32_t>(c->batch_mem_cap, 1u)));
}

uint32_t grid_for(const mirt_ctx* c, uint64_t work_items) {
	uint64_t blocks = (work_items + kBlock - 1) / kBlock;
	const uint64_t cap = static_cast<uint64_t>(c->n_cu) * 8u;      // grid-stride beyond 8 workgroups per CU
	if (blocks > cap) blocks = cap;
	if (blocks < 1) blocks = 1;
	return static_cast<uint32_t>(blocks);
}

// Trace kernels are launched as a resident grid (as many 512-thread workgroups as their LDS footprint lets a
// CU hold) and grid-stride over the stream, so each workgroup stages the BVH into LDS once per launch.
constexpr uint32_t kLdsPerCu = 160u * 1024u;
// LDS plan of a trace workgroup (1024 lanes): staged BVH bytes + a per-lane traversal stack.
//   binary16 records, <= 32768 records and spheres: 16 u16 entries (32 KB) + up to 48 KB staged  -> TWO workgroups (32 waves) per CU
//   binary16 records, more of them:     12 u32 entries (48 KB) + up to 32 KB staged  -> two workgroups per CU
//   f32 records:                        16 u32 entries (64 KB) + up to 96 KB staged  -> one workgroup per CU
// Staged: the whole tree and every sphere packet when they fit the budget (1k spheres: 64 + 16 KB), otherwise the top of the
// tree only (records are breadth-first) and spheres from L2.  Brute force (policy.use_bvh = 0) stages one chunk of spheres.
struct LdsPlan {
	uint32_t stack16;                  // a stack entry = 15-bit record or prim index + the leaf flag
	uint32_t rec_bytes, lds_recs, lds_spheres, staged_bytes, stack_bytes;     // one record as fetched; records / sphere packets staged
	uint32_t launch_bytes;             // dynamic LDS of a trace launch under the current policy
	uint32_t wgs_per_cu;               // workgroups a CU holds at that footprint, at most tune_trace_wgs (2 x 1024 threads = 32 waves, the CU's limit)
};
LdsPlan lds_plan(const mirt_ctx* c) {
	const SceneDev& s = c->scene;
	const bool half = s.half_boxes != 0;
	LdsPlan p{};
	p.stack16 = (half && s.n_recs <= 32768 && s.n_spheres <= 32768) ? 1u : 0u;
	p.rec_bytes = (half && !s.wide) ? 32u : 64u;
	p.stack_bytes = half ? (p.stack16 ? kLdsStack * kTraceBlock * 2u : kLdsStackWide * kTraceBlock * 4u) : kLdsStack * kTraceBlock * 4u;
	const uint32_t budget = half ? (p.stack16 ? 48u * 1024u : 32u * 1024u) : 96u * 1024u;
	if (static_cast<uint64_t>(s.n_recs) * p.rec_bytes + static_cast<uint64_t>(s.n_spheres) * 16u <= budget) { p.lds_recs = s.n_recs; p.lds_spheres = s.n_spheres; }
	else { p.lds_recs = std::min<uint32_t>(s.n_recs, budget / p.rec_bytes); p.lds_spheres = 0; }
	p.staged_bytes = p.lds_recs * p.rec_bytes + p.lds_spheres * 16u;
	p.launch_bytes = c->policy.use_bvh ? p.staged_bytes + p.stack_bytes : kBruteChunk * 16u;
	p.wgs_per_cu = std::min(std::max(kLdsPerCu / p.launch_bytes, 1u), c->tune_trace_wgs);
	return p;
}
uint32_t trace_lds(const mirt_ctx* c) { return lds_plan(c).launch_bytes; }
uint32_t trace_grid(const mirt_ctx* c, uint64_t work_items) {
	uint64_t blocks = (work_items + kTraceBlock - 1) / kTraceBlock;
	const uint64_t cap = static_cast<uint64_t>(c->n_cu) * lds_plan(c).wgs_per_cu;
	if (blocks > cap) blocks = cap;
	if (blocks < 1) blocks = 1;
	return static_cast<uint32_t>(blocks);
}

hipError_t sync_all(mirt_ctx* c) {
	for (PipeSlot& sl : c->slots) if (sl.stream) { hipError_t e = hipStreamSynchronize(sl.stream); if (e != hipSuccess) return e; }
	return hipStreamSynchronize(c->stream);
}
constexpr uint32_t kQueueWords = kSegs * kSegPitch;     // one ray queue's counters: one per 128-B line (kernels.hpp "ray queues"; k_shade's appends are sensitive to it)
constexpr uint32_t kFatCapacity = 1u << 16;   // rays per list and launch that may take the brute-force detour (a few per million qualify)
// The counter words of one batch of nb bounces (PipeSlot::counts; the debug trace entry points keep a private one with nb = 1), zeroed before
// the batch's first launch: 2 nb + 2 queues of kQueueWords, then 4 nb single words (+ 8 spare).  Every offset is stated here and nowhere else.
struct BatchCounters {
	uint32_t* w; uint32_t nb, seg_cap;
	static size_t words(uint32_t nb) { return static_cast<size_t>(2 * nb + 2) * kQueueWords + static_cast<size_t>(nb) * 4 + 8; }
	Queue queue(uint32_t k) const { return Queue{ w + static_cast<size_t>(k) * kQueueWords, seg_cap }; }
	uint32_t* word(uint32_t k) const { return w + static_cast<size_t>(2 * nb + 2) * kQueueWords + k; }
	Queue stream_queue(uint32_t b) const { return queue(b); }                // b = 0 .. nb: rays entering bounce b (b >= 1)
	Queue shadow_queue(uint32_t b) const { return queue(nb + 1 + b); }       // b = 0 .. nb - 1: NEE rays emitted at bounce b
	Queue empty_queue() const { return queue(2 * nb + 1); }                  // "no shadow rays pending"
	uint32_t* closest_work(uint32_t b) const { return word(b); }             // per-launch work counters of the persistent trace kernels
	uint32_t* shadow_work(uint32_t b) const { return word(nb + b); }
	// per-launch fat-ray counts; `lists`: the slot's index lists, [closest kFatCapacity][shadow kFatCapacity]
	FatList fat_closest(uint32_t b, uint32_t* lists) const { return FatList{ word(2 * nb + b), lists, kFatCapacity }; }
	FatList fat_shadow(uint32_t b, uint32_t* lists) const { return FatList{ word(3 * nb + b), lists + kFatCapacity, kFatCapacity }; }
};
// The counter words of one build of the candidate lists (mirt_ctx::cand_words), zeroed before it; listed_pixels is read by every batch that uses the lists.
struct CandWords {
	uint32_t* w;
	static constexpr size_t kWords = 4;
	uint32_t* work() const { return w; }                                     // work counter of k_primary_cand
	uint32_t* unused_fat_count() const { return w + 1; }                     // count of the zero-capacity list k_primary_cand is handed
	uint32_t* listed_pixels() const { return w + 2; }                        // pixels without a candidate list (their list: mirt_ctx::cand_listed)
};
BatchCounters batch_counters(const mirt_ctx* c, const PipeSlot& sl) { return BatchCounters{ sl.counts.as<uint32_t>(), c->policy.max_bounces, c->seg_cap }; }
uint32_t wanted_slots(const mirt_ctx* c) {
	if (c->policy.streams) return std::min<uint32_t>(c->policy.streams, 8u);
	return static_cast<uint64_t>(c->n_tiles) * kTileSize * batch_limit(c) >= kSerialRays ? 1u : 3u;
}
// Device bytes of the batches in flight for the current plan (ray streams + contribution buffers).
uint64_t streams_bytes(const mirt_ctx* c) {
	const uint64_t rays = static_cast<uint64_t>(c->n_tiles) * kTileSize * batch_limit(c);
	return wanted_slots(c) * (rays * 4u * (kStreamPlanes + (c->ggx_pdf ? 2u : 0u)) + rays * 12u);      // mirt_set_ggx_pdf: the closure-pdf plane of both streams, 4 B per ray each
}

// Automatic batch size: as large as kBatchRays asks, but within 80 % of the device memory that is free plus what this context's own ray
// streams hold already (other contexts and processes may share the device).  Allocates nothing: mirt_get_policy reports the plan before
// the first launch; ensure_streams re-carves the arena when the plan changed.  Planned once per pixel count (mirt_set_policy resets it
// when a field the plan depends on changes).
void plan_batches(mirt_ctx* c) {
	const uint64_t n_pix = static_cast<uint64_t>(c->n_tiles) * kTileSize;
	if (c->policy.max_batch || n_pix == 0 || c->planned_for == n_pix) return;
	c->batch_mem_cap = kMaxBatch;
	size_t free_b = 0, total_b = 0, own = 0;
	for (const PipeSlot& sl : c->slots) own += sl.arena.bytes + sl.contrib.bytes;
	if (hipSetDevice(c->device) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess)
		while (batch_limit(c) > batch_floor(c) && streams_bytes(c) > (free_b + own) / 5 * 4) c->batch_mem_cap = std::max(batch_limit(c) / 2, batch_floor(c));
	c->planned_for = n_pix;
}

// Carve each slot's frame-wide ray streams out of one allocation.
int ensure_streams(mirt_ctx* c) {
	const uint64_t n_pix = static_cast<uint64_t>(c->n_tiles) * kTileSize;
	if (n_pix * batch_limit(c) == 0) return MIRT_OK;
	plan_batches(c);
	const uint64_t cap64 = n_pix * batch_limit(c);
	if (n_pix > (1u << 24)) return fail(c, MIRT_ERR_ARG, "more than 2^24 pixels per context (%llu); shard the tile range", (unsigned long long)n_pix);
	if (cap64 + 3ull * kSegs * kShadeBlock > (1ull << 30)) return fail(c, MIRT_ERR_ARG, "stream capacity %llu too large", (unsigned long long)cap64);   // path ids and stream slots stay below 2^30 (a shadow record's dest word carries two flag bits: kDestAccum, kDestFull)
	// a ray queue is kSegs segments of seg_cap slots (kernels.hpp "ray queues"): a plane holds kSegs * seg_cap entries
	// (+ 2 blocks: k_shade<FIRST> iterates pixel-major, and when the pixel count is an odd multiple of 256 its half-filled last chunk adds iterations)
	const uint32_t seg_cap = static_cast<uint32_t>((((cap64 + kShadeBlock - 1) / kShadeBlock + kSegs - 1) / kSegs + 2) * kShadeBlock);
	const uint32_t cap = seg_cap * kSegs;
	const uint32_t nb = c->policy.max_bounces;
	const uint32_t want = wanted_slots(c);
	const size_t acc_bytes = static_cast<size_t>(c->n_tiles) * batch_limit(c) * 3 * kTileSize * sizeof(float);     // contribution buffer: [tile][slot][256][rgb]
	if (cap == c->capacity && nb == c->arena_bounces && c->slots.size() == want && c->slots[0].contrib.bytes >= acc_bytes &&
	    (c->slots[0].sky_w.ptr != nullptr) == (c->sky_sampling != 0) && (c->slots[0].pdf_p.ptr != nullptr) == (c->ggx_pdf != 0)) return MIRT_OK;
	HIP_TRY(c, sync_all(c));
	c->aov_prev = nullptr;                                                   // (every batch has finished; the event's slot may go away below)
	while (c->slots.size() > want) { c->slots.back().release(); c->slots.pop_back(); }
	while (c->slots.size() < want) {
		PipeSlot sl;
		HIP_TRY(c, hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
		HIP_TRY(c, hipEventCreateWithFlags(&sl.batch_done, hipEventDisableTiming));
		HIP_TRY(c, hipEventCreateWithFlags(&sl.merged, hipEventDisableTiming));
		c->slots.push_back(sl);
	}
	const size_t planes = kStreamPlanes;
	const size_t plane_bytes = (static_cast<size_t>(cap) * 4 + 255) & ~static_cast<size_t>(255);
	for (PipeSlot& sl : c->slots) {
		sl.in_use = false;                                                   // (the caller has synchronised every stream)
		hipError_t e = sl.arena.ensure(planes * plane_bytes);
		const char* what = "ray streams";
		if (e == hipSuccess) { e = sl.counts.ensure(BatchCounters::words(nb) * sizeof(uint32_t)); what = "queue counters"; }
		if (e == hipSuccess) { e = sl.fat.ensure(2u * kFatCapacity * sizeof(uint32_t)); what = "fat-ray lists"; }
		if (e == hipSuccess) { e = sl.contrib.ensure(acc_bytes); what = "contribution buffer"; }
		if (e == hipSuccess && c->sky_sampling) { e = sl.sky_w.ensure(2 * plane_bytes); what = "miss-weight planes"; }
		if (!c->sky_sampling) sl.sky_w.release();
		if (e == hipSuccess && c->ggx_pdf) { e = sl.pdf_p.ensure(2 * plane_bytes); what = "closure-pdf planes"; }
		if (!c->ggx_pdf) sl.pdf_p.release();
		if (e != hipSuccess) {
			// not enough device memory after all (someone else took it meanwhile — another context or process planning against the same
			// free memory): halve the automatic batch and plan again
			(void)hipGetLastError();
			if (e == hipErrorOutOfMemory && !c->policy.max_batch && batch_limit(c) > batch_floor(c)) {
				for (PipeSlot& other : c->slots) { other.arena.release(); other.contrib.release(); other.sky_w.release(); other.pdf_p.release(); }
				c->capacity = 0;
				c->batch_mem_cap = std::max(batch_limit(c) / 2, batch_floor(c));
				return ensure_streams(c);
			}
			return fail(c, MIRT_ERR_HIP, "%s (%zu bytes of ray streams per batch in flight): %s", what, planes * plane_bytes, hipGetErrorString(e));
		}
		char* p = sl.arena.as<char>();
		auto take = [&](size_t n_planes) { void* r = p; p += n_planes * plane_bytes; return r; };     // plane_bytes is a multiple of 256: every record plane is 16-B-aligned
		for (int b = 0; b < 2; b++) {
			StreamBuf& s = sl.stream_buf[b];
			s.a = (float4*)take(4); s.b = (float4*)take(4); s.c = (float2*)take(2);
			s.w = sl.sky_w.ptr ? reinterpret_cast<float*>(sl.sky_w.as<char>() + b * plane_bytes) : nullptr;
			sl.pdf_plane[b] = sl.pdf_p.ptr ? reinterpret_cast<float*>(sl.pdf_p.as<char>() + b * plane_bytes) : nullptr;
		}
		sl.hit = (HitRec*)take(2);                                         // 8 B per ray
		ShadowBuf& h = sl.shadow_buf;
		h.a = (float4*)take(4); h.b = (float4*)take(4); h.c = (float4*)take(4); h.d = (float4*)take(4);
	}
	c->capacity = cap;
	c->seg_cap = seg_cap;
	c->arena_bounces = nb;
	return MIRT_OK;
}

size_t aov_floats(const mirt_ctx* c) { return c->aov_on ? static_cast<size_t>(c->n_tiles) * kAovPlanes * kTileSize : 0; }
// The AOV slab of the current tile set, zeroed (nothing while AOVs are off).  The caller has synchronised every stream.
int alloc_aov(mirt_ctx* c) {
	const size_t floats = aov_floats(c);
	HIP_TRY(c, c->aov.ensure(floats * sizeof(float)));
	if (floats) HIP_TRY(c, hipMemsetAsync(c->aov.ptr, 0, floats * sizeof(float), c->stream));
	return MIRT_OK;
}

// No tile is frozen (host state only: the device copies are read while n_frozen != 0 and rewritten by the call that raises it).
void clear_freezes(mirt_ctx* c) { c->frozen.clear(); c->frozen_at.clear(); c->n_frozen = 0; }
uint32_t tile_count(const mirt_ctx* c, uint32_t local) { return (c->n_frozen && c->frozen[local]) ? c->frozen_at[local] : c->accumulations; }
// The mask and the list of active pixels as the sparse kernels read them.  The caller has synchronised every stream.
int upload_freezes(mirt_ctx* c) {
	if (c->n_frozen == 0) return MIRT_OK;
	std::vector<uint32_t> mask(c->n_tiles), list(1);
	list.reserve(static_cast<size_t>(c->n_tiles - c->n_frozen) * kTileSize + 1);
	for (uint32_t t = 0; t < c->n_tiles; t++) {
		mask[t] = c->frozen[t] ? 1u : 0u;
		if (!c->frozen[t]) for (uint32_t id = 0; id < kTileSize; id++) list.push_back(t * kTileSize + id);
	}
	list[0] = static_cast<uint32_t>(list.size() - 1);
	HIP_TRY(c, c->tile_frozen.ensure(mask.size() * sizeof(uint32_t)));
	HIP_TRY(c, c->active_list.ensure((static_cast<size_t>(c->n_tiles) * kTileSize + 1) * sizeof(uint32_t)));
	HIP_TRY(c, hipMemcpy(c->tile_frozen.ptr, mask.data(), mask.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
	HIP_TRY(c, hipMemcpy(c->active_list.ptr, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
	c->freeze_gen++;
	return MIRT_OK;
}
// The per-tile counts for a resolve kernel: NULL while no tile is frozen (the kernels then do what they have always done).  The caller has
// synchronised every stream, and the kernel it launches is on the main stream, behind this copy.
int upload_tile_counts(mirt_ctx* c, const uint32_t** dev) {
	*dev = nullptr;
	if (c->n_frozen == 0) return MIRT_OK;
	std::vector<uint32_t> counts(c->n_tiles);
	for (uint32_t t = 0; t < c->n_tiles; t++) counts[t] = tile_count(c, t);
	HIP_TRY(c, c->tile_counts.ensure(counts.size() * sizeof(uint32_t)));
	HIP_TRY(c, hipMemcpy(c->tile_counts.ptr, counts.data(), counts.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
	*dev = c->tile_counts.as<uint32_t>();
	return MIRT_OK;
}

int alloc_accumulator(mirt_ctx* c) {
	const size_t floats = static_cast<size_t>(c->n_tiles) * c->policy.buckets * 3 * kTileSize;
	HIP_TRY(c, sync_all(c));
	HIP_TRY(c, c->accumulator.ensure(floats * sizeof(float)));
	if (floats) HIP_TRY(c, hipMemsetAsync(c->accumulator.ptr, 0, floats * sizeof(float), c->stream));
	if (c->aov_on) { const int r = alloc_aov(c); if (r) return r; }
	HIP_TRY(c, hipMemsetAsync(c->counters.ptr, 0, sizeof(DevCounters), c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	for (PipeSlot& sl : c->slots) sl.in_use = false;
	c->accumulations = 0;
	clear_freezes(c);
	return MIRT_OK;
}

// ---- launch bracketing (policy.profile) ---------------------------------------------------------
hipEvent_t take_event(mirt_ctx* c) {
	if (!c->free_events.empty()) { hipEvent_t e = c->free_events.back(); c->free_events.pop_back(); return e; }
	hipEvent_t e = nullptr;
	(void)hipEventCreate(&e);
	return e;
}
void harvest(mirt_ctx* c) {
	if (c->pending.empty()) return;
	(void)sync_all(c);
	for (TimedLaunch& t : c->pending) {
		float ms = 0.0f;
		if (hipEventElapsedTime(&ms, t.start, t.stop) == hipSuccess) { c->times.ms[t.klass] += ms; c->times.launches[t.klass]++; }
		c->free_events.push_back(t.start); c->free_events.push_back(t.stop);
	}
	c->pending.clear();
}
struct Bracket {
	mirt_ctx* c; int klass; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
	Bracket(mirt_ctx* ctx, int k, hipStream_t stream = nullptr) : c(ctx), klass(k), st(stream ? stream : ctx->stream) {
		if (c->policy.profile) { a = take_event(c); b = take_event(c); (void)hipEventRecord(a, st); }
	}
	~Bracket() {
		if (c->policy.profile) { (void)hipEventRecord(b, st); c->pending.push_back(TimedLaunch{ klass, a, b }); }
	}
};

// half-angle of a pixel's bundle of camera rays: half a pixel diagonal (0.7072) at distance >= |z|; + 1e-4: a sample's own cone half-width
// (1.38e-3 .. 1.47e-3, from |D|^2 - 1 of its normalised direction) may exceed the axis ray's by 8.5e-5
float bundle_half_angle(const mirt_ctx* c) { return (0.7072f / std::fabs(c->camera.z)) * 1.01f + 1e-4f; }

// The camera's +x, +y and -z in world space, for lens_ray: binary32, the quat * vec3 formula of camera_ray_dir (device_math.hpp camera_axis).
void update_lens_axes(mirt_ctx* c) {
	const f3 r = camera_axis(c->camera.orient, f3{ 1.0f, 0.0f, 0.0f }), u = camera_axis(c->camera.orient, f3{ 0.0f, 1.0f, 0.0f }), f = camera_axis(c->camera.orient, f3{ 0.0f, 0.0f, -1.0f });
	c->lens.right[0] = r.x; c->lens.right[1] = r.y; c->lens.right[2] = r.z;
	c->lens.up[0] = u.x; c->lens.up[1] = u.y; c->lens.up[2] = u.z;
	c->lens.fwd[0] = f.x; c->lens.fwd[1] = f.y; c->lens.fwd[2] = f.z;
}
bool lens_on(const mirt_ctx* c) { return c->lens.aperture > 0.0f; }

// The context's n_tiles local tiles in the image (tile_map.hpp).
TileMap tile_map(const mirt_ctx* c) { return TileMap{ c->first_tile, c->run_tiles, c->stride_tiles, c->h_tiles, c->width }; }
// The history of mirt_render_temporal goes (mirt.h "history lifetime").  The caller has made the context's device the current one.
void drop_history(mirt_ctx* c) {
	for (DeviceBuffer* b : { &c->th_x, &c->th_g, &c->th_n, &c->th_len, &c->th_id, &c->th_id_cur, &c->th_snap }) b->release();
	c->th_valid = false; c->th_snap_valid = false;
}
void set_tile_map(mirt_ctx* c, const TileMap& m, uint32_t n_tiles) { c->first_tile = m.first_tile; c->run_tiles = m.run_tiles; c->stride_tiles = m.stride_tiles; c->n_tiles = n_tiles; }

// mirt_set_sky_sampling changes the kernels launched only where its light can be drawn and can carry something.
bool sky_active(const mirt_ctx* c) { return c->sky_sampling && c->sky.t && c->sky_total > 0.0f && c->policy.mis && c->scene.has_ambient && !c->stream_order; }

// The launch rule of mirt_set_material_closures.  The effective closure of material m is closures[m], or policy.brdf at and beyond the table's end.
// If materials 0 .. n_mat - 1 of the scene all take closure k, the kernels of policy.brdf = k are launched (mixed = false, ggx = k): the same device
// code, hence that policy's words.  Otherwise the MIXED instantiations run with `mask` (bit m = material m is GGX).  The material LIST decides, not
// which materials the spheres use.  Exact stream order excludes a table (both setters), so k_tile_stream only ever sees policy.brdf.
struct ClosurePlan { bool mixed, ggx; unsigned long long mask; };
ClosurePlan closure_plan(const mirt_ctx* c) {
	const bool policy_ggx = c->policy.brdf != 0;
	if (c->closures.empty() || !c->have_scene) return ClosurePlan{ false, policy_ggx, 0ull };
	unsigned long long mask = 0ull;
	const uint32_t n_mat = c->scene.n_mat;                                    // 1 .. MIRT_MAX_MATERIALS (63): every bit index is below 64
	for (uint32_t m = 0; m < n_mat; m++)
		if (m < c->closures.size() ? c->closures[m] != 0 : policy_ggx) mask |= 1ull << m;
	const unsigned long long all = (1ull << n_mat) - 1ull;
	if (mask == 0ull) return ClosurePlan{ false, false, 0ull };
	if (mask == all) return ClosurePlan{ false, true, 0ull };
	return ClosurePlan{ true, false, mask };
}

FrameParams frame_params(const mirt_ctx* c, uint32_t acc_base, uint32_t batch_n) {
	FrameParams fp{};
	const TileMap m = tile_map(c);
	fp.cam = c->camera;
	fp.h_tiles = m.h_tiles;
	fp.first_tile = m.first_tile;
	fp.run_tiles = m.run_tiles;
	fp.stride_tiles = m.stride_tiles;
	fp.n_pix = c->n_tiles * kTileSize;
	fp.pix_bits = pix_bits_of(c); fp.pix_mask = (1u << fp.pix_bits) - 1u;
	fp.acc_base = acc_base;
	fp.batch_n = batch_n;
	fp.max_bounces = c->policy.max_bounces;
	fp.buckets = c->policy.buckets;
	fp.n_lights = c->scene.n_lights;
	fp.mis = (c->policy.mis && (c->scene.n_lights > 0 || sky_active(c))) ? 1u : 0u;       // Q12 guard (mirt_set_sky_sampling: the sky counts as a light)
	fp.first_groups = 1;
	fp.inv_n_pix = fp.n_pix ? 1.0f / static_cast<float>(fp.n_pix) : 0.0f;
	fp.inv_h_tiles = fp.h_tiles ? 1.0f / static_cast<float>(fp.h_tiles) : 0.0f;
	fp.inv_run_tiles = 1.0f / static_cast<float>(fp.run_tiles);
	return fp;
}

// The scene as the trace kernels of a launch see it: what mirt_set_scene left, the policy's use_bvh and the launch-shape knobs.
SceneDev trace_scene(const mirt_ctx* c) {
	SceneDev sc = c->scene;
	sc.use_bvh = c->policy.use_bvh;
	sc.chunk_max = c->tune_chunk; sc.leaf_batch = c->tune_leaf_batch; sc.refill_idle = c->tune_refill_idle;
	return sc;
}

// Every instantiation a launch of the trace stage may pick, by template argument; a combination that does not exist is nullptr (launch_trace
// refuses it).  k_trace and k_primary_cand use dynamic LDS: plan_trace_lds raises their limit by walking trace_kernel() and kPrimaryCand, so a
// k_trace that can be launched cannot be missed there.
// The counting kernels come FIRST ([!count]): the order in which k_trace<true, .> and k_trace<false, .> are first named decides hipcc's register
// assignment in k_trace<., kPrimaryNone> (same resources, another instruction stream: profiles/trace_launch_refactor.txt), and with this order
// the device code of every older instantiation is what it has been since the kernels were tuned and measured (profiles/one_trace_kernel.txt).
constexpr int kPrimaryForms = 4;
static_assert(kPrimaryNone == 0 && kPrimaryAll == 1 && kPrimaryList == 2 && kPrimaryActive == 3, "the trace tables are indexed by PRIMARY");
auto trace_kernel(bool count, int primary, bool lens) {
	static const decltype(&k_trace<true, kPrimaryNone>) table[2][2][kPrimaryForms] = {      // [lens][!count][primary]; kernels.hpp: the lens concerns bounce 0, and no lists are read under it
		{ { k_trace<true, kPrimaryNone>, k_trace<true, kPrimaryAll>, k_trace<true, kPrimaryList>, k_trace<true, kPrimaryActive> },
		  { k_trace<false, kPrimaryNone>, k_trace<false, kPrimaryAll>, k_trace<false, kPrimaryList>, k_trace<false, kPrimaryActive> } },
		{ { nullptr, k_trace<true, kPrimaryAll, true>, nullptr, k_trace<true, kPrimaryActive, true> }, { nullptr, k_trace<false, kPrimaryAll, true>, nullptr, k_trace<false, kPrimaryActive, true> } } };
	return primary < 0 || primary >= kPrimaryForms ? nullptr : table[lens][!count][primary];
}
// kPrimaryActive has no k_trace_fat of its own: its fat rays are kPrimaryList's, over the same list (launch_trace).
auto trace_fat_kernel(bool count, int primary, bool lens) {
	using K = decltype(&k_trace_fat<true, kPrimaryNone>);
	static const K table[2][2][3] = {                                      // [lens][!count][primary]
		{ { k_trace_fat<true, kPrimaryNone>, k_trace_fat<true, kPrimaryAll>, k_trace_fat<true, kPrimaryList> },
		  { k_trace_fat<false, kPrimaryNone>, k_trace_fat<false, kPrimaryAll>, k_trace_fat<false, kPrimaryList> } },
		{ { nullptr, k_trace_fat<true, kPrimaryAll, true>, k_trace_fat<true, kPrimaryList, true> },
		  { nullptr, k_trace_fat<false, kPrimaryAll, true>, k_trace_fat<false, kPrimaryList, true> } } };
	if (primary == kPrimaryActive) primary = kPrimaryList;
	return primary < 0 || primary > kPrimaryList ? K(nullptr) : table[lens][!count][primary];
}
const decltype(&k_primary_cand<true>) kPrimaryCand[2] = { k_primary_cand<true>, k_primary_cand<false> };                                    // [!count]
const decltype(&k_tile_stream<false>) kTileStream[2] = { k_tile_stream<false>, k_tile_stream<true> };                                         // [ggx]

// One selector per stage that has SPARSE / LENS / RIS instantiations (kernels.hpp), named after the tables above; within each, the
// instantiations of the default path first.  sparse = a tile is frozen (mirt_freeze_tiles), ris = mirt_set_light_ris above 0 where NEE runs.
auto primary_hits_kernel(bool count, bool wave, bool sparse) {      // wave: one wave per pixel, for the batches that fill a wave (kernels.hpp kWaveHitsMinBatch)
	static const decltype(&k_primary_hits<true>) table[2][2][2] = {      // [sparse][wave][!count]
		{ { k_primary_hits<true>, k_primary_hits<false> }, { k_primary_hits_wave<true>, k_primary_hits_wave<false> } },
		{ { k_primary_hits<true, true>, k_primary_hits<false, true> }, { k_primary_hits_wave<true, true>, k_primary_hits_wave<false, true> } } };
	return table[sparse][wave][!count];
}
// k_shade: every instantiation there is, generated from ShadeForm::valid() (kernels.hpp) and indexed by ShadeForm::bits(); a form that does not
// exist is never instantiated and is nullptr (launch_batch refuses it).  The pack names the instantiations in the order of their bits, FIRST the
// least significant: with this order the device code of all 251 kernels of this file is what it was under the hand-written tables
// (profiles/shade_form_table.txt; compare again with profiles/compare_kernels.py when a bit is added, the order of first naming has moved hipcc's
// register assignment before — see the trace tables above).
using ShadeKernel = decltype(&k_shade<false, false>);
template <uint32_t BITS>
constexpr ShadeKernel shade_entry() {
	constexpr ShadeForm f = ShadeForm::from_bits(BITS);
	if constexpr (!f.valid()) return nullptr;
	else if constexpr (shade_waves(f) == 8u) return &k_shade<ShadeWaves8, f.first, f.ggx, f.lens, f.sparse, f.ris, f.glass, f.sky, f.mixed, f.pdf>;
	else return &k_shade<f.first, f.ggx, f.lens, f.sparse, f.ris, f.glass, f.sky, f.mixed, f.pdf>;
}
template <uint32_t... BITS>
ShadeKernel shade_kernel(ShadeForm f, std::integer_sequence<uint32_t, BITS...>) {
	static const ShadeKernel table[] = { shade_entry<BITS>()... };
	return table[f.bits()];
}
ShadeKernel shade_kernel(ShadeForm f) { return shade_kernel(f, std::make_integer_sequence<uint32_t, 1u << ShadeForm::kBits>{}); }
// The k_shade of one bounce of a batch: the one place where a switch of the context turns into a template argument.  What the launch passes for
// a flag's arguments (ris_m, the sky table, the pdf planes) it reads from this value too.
ShadeForm shade_form(const mirt_ctx* c, const FrameParams& fp, const ClosurePlan& plan, uint32_t bounce, bool lens, bool sparse) {
	ShadeForm f{};
	f.first = bounce == 0;
	// lens and sparse (a tile is frozen, mirt_freeze_tiles) concern bounce 0 only
	f.lens = f.first && lens;
	f.sparse = f.first && sparse;
	// mirt_set_light_ris: the candidate loop is worth running only where NEE runs
	f.ris = fp.mis && c->light_ris;
	// mirt_set_transmission: only while the scene has a transmissive material
	f.glass = c->transmission && c->scene_has_glass;
	// mirt_set_sky_sampling: only where the sky's light can be drawn and can carry something
	f.sky = sky_active(c);
	// mirt_set_material_closures: the kernels of the one closure every material takes, or the MIXED ones
	f.mixed = plan.mixed; f.ggx = plan.ggx;
	// mirt_set_ggx_pdf: only where Closure<GGX> shades a hit; an all-Lambertian plan launches what it launched without the switch
	f.pdf = c->ggx_pdf && (plan.mixed || plan.ggx);
	return f;
}
auto first_hit_aov_kernel(bool lens, bool sparse) {
	static const decltype(&k_first_hit_aov<false>) table[2][2] = { { k_first_hit_aov<false>, k_first_hit_aov<true> }, { k_first_hit_aov<false, true>, k_first_hit_aov<true, true> } };   // [sparse][lens]
	return table[sparse][lens];
}
auto merge_kernel(bool sparse) { return sparse ? k_merge_contrib<true> : k_merge_contrib<false>; }

// What varies between the launches of the trace stage: a bounce of a batch, or the rays of a debug entry point.
struct TraceLaunch {
	StreamBuf in; HitRec* hit;                       // closest-hit rays (no stream with PRIMARY) and their hit records
	Queue closest_queue; uint32_t* closest_work;
	ShadowBuf sh; ShadowSink sink;                   // shadow rays and where their outcome goes
	Queue shadow_queue; uint32_t* shadow_work;
	FatList fat_closest, fat_shadow;
	const uint32_t* listed_pixels;                   // kPrimaryList: count of the pixels listed at in.a (NULL otherwise)
	DevCounters* ctr;
};
// k_trace<count, primary, lens> over n_rays, then (with a tree) the few rays too "fat" for it: brute force, one workgroup each.
// kPrimaryList / kPrimaryActive: t.in.a is the pixel list and t.listed_pixels its count (kernels.hpp stream_pixel_list); lens: at bounce 0 only.
int launch_trace(mirt_ctx* c, hipStream_t st, const SceneDev& sc, const FrameParams& fp, uint64_t n_rays, bool count, int primary, const TraceLaunch& t, bool lens = false) {
	const auto trace = trace_kernel(count, primary, lens);
	const auto fat = trace_fat_kernel(count, primary, lens);
	if (!trace || !fat) return fail(c, MIRT_ERR_ARG, "no trace kernel for primary = %d%s", primary, lens ? " under a lens" : "");
	hipLaunchKernelGGL(trace, dim3(trace_grid(c, n_rays)), dim3(kTraceBlock), trace_lds(c), st, sc, fp, t.in, t.hit, t.closest_queue, t.closest_work,
	                   t.sh, t.sink, t.shadow_queue, t.shadow_work, t.fat_closest, t.fat_shadow, t.ctr, c->lens);
	// a large scene (100 k spheres: ~100 us per ray) wants as many fat rays in flight as there are (a few hundred per launch); k_trace_fat grid-strides
	const uint32_t fat_grid = sc.n_spheres > 4096 ? static_cast<uint32_t>(c->n_cu) * 2u : 64u;
	if (sc.use_bvh) hipLaunchKernelGGL(fat, dim3(fat_grid), dim3(1024), 0, st, sc, fp, t.in, t.hit, t.fat_closest, t.sh, t.sink, t.fat_shadow, t.ctr, t.listed_pixels, c->lens);
	return MIRT_OK;
}

// mirt_set_stream_order(1): a batch is ONE launch — the whole bounce loop of a (tile, accumulation) stream runs in one workgroup, in the reference's
// slot order (kernels.hpp "EXACT STREAM ORDER"); brute force whatever policy.use_bvh says.  Same contribution buffer and merge as the default path.
int launch_tile_stream(mirt_ctx* c, hipStream_t st, const SceneDev& sc, const FrameParams& fp, uint32_t batch_n, float* contrib, DevCounters* ctr, bool count) {
	if (!c->gloss_decay_dev_valid) {                                                  // (batches in flight on other streams may still read the old table)
		HIP_TRY(c, sync_all(c));
		HIP_TRY(c, c->gloss_decay_dev.ensure(std::max<size_t>(c->gloss_decay.size(), 1) * sizeof(float)));
		if (!c->gloss_decay.empty()) HIP_TRY(c, hipMemcpy(c->gloss_decay_dev.ptr, c->gloss_decay.data(), c->gloss_decay.size() * sizeof(float), hipMemcpyHostToDevice));
		c->gloss_decay_dev_valid = true;
	}
	Bracket t(c, MIRT_K_TRACE, st);
	hipLaunchKernelGGL(kTileStream[c->policy.brdf != 0], dim3(c->n_tiles * batch_n), dim3(kTileSize), 0, st, sc, fp, contrib, ctr, c->mat_ggx.as<float4>(),
	                   c->gloss_decay_dev.as<float>(), static_cast<uint32_t>(c->gloss_decay.size()), count ? 1u : 0u);
	return MIRT_OK;
}

// Builds the context's candidate lists (mirt_ctx::cand ...) for the current scene, camera and tile set: one cone traversal per local pixel
// (kernels.hpp kCollect).  The build runs on the main stream.  Every batch launched so far is ahead of it there — the main stream waits for a
// batch's batch_done before it merges the batch — so a rebuild cannot overtake a batch that still reads the previous lists; batches on
// other streams wait for cand_built (launch_batch).
int build_primary_lists(mirt_ctx* c, const SceneDev& sc, const FrameParams& fp, bool count) {
	HIP_TRY(c, c->cand.ensure(static_cast<size_t>(fp.n_pix) * kCandStride * sizeof(uint32_t)));
	HIP_TRY(c, c->cand_listed.ensure(static_cast<size_t>(fp.n_pix) * sizeof(uint32_t)));        // at most every pixel is without a list
	HIP_TRY(c, c->cand_words.ensure(CandWords::kWords * sizeof(uint32_t)));
	if (!c->cand_built) HIP_TRY(c, hipEventCreateWithFlags(&c->cand_built, hipEventDisableTiming));
	const CandWords cw{ c->cand_words.as<uint32_t>() };
	HIP_TRY(c, hipMemsetAsync(cw.w, 0, CandWords::kWords * sizeof(uint32_t), c->stream));
	{ Bracket t(c, MIRT_K_TRACE);
	  const FatList none{ cw.unused_fat_count(), nullptr, 0u };
	  hipLaunchKernelGGL(kPrimaryCand[!count], dim3(trace_grid(c, fp.n_pix)), dim3(kTraceBlock), trace_lds(c), c->stream, sc, fp, c->cand.as<uint32_t>(), bundle_half_angle(c),
	                     cw.work(), none, c->counters.as<DevCounters>(), c->cand_listed.as<uint32_t>(), cw.listed_pixels()); }
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipEventRecord(c->cand_built, c->stream));
	c->cand_gen++;
	c->cand_valid = true;
	return MIRT_OK;
}

// mirt_set_aov(1): the camera rays' hit records of the batch lie in sl.hit (slot * n_pix + pixel) from the bounce-0 trace launches until the
// bounce-1 trace overwrites them; k_first_hit_aov runs in between, on the batch's own stream.  The slab holds running sums and float
// addition does not associate, so batches in flight on different streams must reach it in batch order: each waits for the event recorded
// after the previous batch's kernel.  (One batch at a time: everything is on the main stream already.)
int launch_first_hit_aov(mirt_ctx* c, PipeSlot& sl, hipStream_t st, const SceneDev& sc, const FrameParams& fp) {
	const bool pipelined = c->slots.size() > 1;
	if (pipelined) {
		if (!sl.aov_done) HIP_TRY(c, hipEventCreateWithFlags(&sl.aov_done, hipEventDisableTiming));
		if (c->aov_prev && c->aov_prev != sl.aov_done) HIP_TRY(c, hipStreamWaitEvent(st, c->aov_prev, 0));   // (the slot's own previous batch is ahead on this very stream)
	}
	{ Bracket t(c, MIRT_K_RESOLVE, st);
	  const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((static_cast<uint64_t>(fp.n_pix) + kBlock - 1) / kBlock, static_cast<uint64_t>(c->n_cu) * 64u));
	  // the closure colour of the first hit: albedo under Lambertian, F0 under GGX; MIXED: one merged table, per material the row of its closure
	  const ClosurePlan plan = closure_plan(c);
	  if (plan.mixed && !c->mat_merged_valid) {
	    std::vector<float4> merged(c->scene.n_mat);
	    for (uint32_t m = 0; m < c->scene.n_mat; m++) merged[m] = ((plan.mask >> m) & 1ull) ? c->ggx_host[m] : c->alb_host[m];
	    HIP_TRY(c, sync_all(c));                                                  // (batches in flight on other streams may still read the old table)
	    HIP_TRY(c, c->mat_merged.ensure(merged.size() * sizeof(float4)));
	    HIP_TRY(c, hipMemcpy(c->mat_merged.ptr, merged.data(), merged.size() * sizeof(float4), hipMemcpyHostToDevice));
	    c->mat_merged_valid = true;
	  }
	  const float4* colour = plan.mixed ? c->mat_merged.as<float4>() : plan.ggx ? c->mat_ggx.as<float4>() : c->scene.mat_albedo;
	  hipLaunchKernelGGL(first_hit_aov_kernel(lens_on(c), c->n_frozen != 0), dim3(grid), dim3(kBlock), 0, st, sc, fp, sl.hit, colour, c->aov.as<float>(), c->lens, c->tile_frozen.as<uint32_t>()); }
	if (pipelined) { HIP_TRY(c, hipEventRecord(sl.aov_done, st)); c->aov_prev = sl.aov_done; }
	return MIRT_OK;
}

// One batch = up to batch_limit() consecutive Accumulate() calls traced together (path id = (slot << pix_bits) | pixel).
// Consecutive accumulation indices land in buckets (acc % buckets, Renderer.hpp:82), and the ORDER of the adds into a
// bucket word is part of the result.  Each path of a batch keeps its radiance in its own word of the batch's contribution buffer
// [tile][slot][256][rgb] — stored at bounce 0 for every path, so the buffer is never cleared, and added to where the reference
// adds to the path's radiance (kernels.hpp contrib_index) — and k_merge_contrib, enqueued on the main stream in batch order,
// applies the slots to their buckets in ascending order — so batches of any size (launches several times longer than their
// tails) and up to policy.streams batches in flight on their own HIP streams (other batches fill those tails) leave every
// bucket's add order, hence the result, exactly as in the reference.  (A running sum cannot live in an accumulator word, which
// holds earlier samples: A + R is not ((A + S0) + E0) + ...; hence a buffer for every batch, however small.)
int launch_batch(mirt_ctx* c, uint32_t batch_n) {
	FrameParams fp = frame_params(c, c->accumulations, batch_n);
	const uint32_t nb = c->policy.max_bounces;
	const uint64_t total = static_cast<uint64_t>(fp.n_pix) * batch_n;
	// Once a tile is frozen (mirt_freeze_tiles) bounce 0 and the merge run their SPARSE instantiations; while none is, every launch below picks the dense ones.
	const bool sparse = c->n_frozen != 0;
	const uint32_t* tile_frozen = c->tile_frozen.as<uint32_t>();
	const uint32_t active_pix = (c->n_tiles - c->n_frozen) * kTileSize;
	if (total == 0 || active_pix == 0) { c->accumulations += batch_n; return MIRT_OK; }   // every tile frozen: the call is only counted; or no tile owned (an image below 16 px, a group member beyond the last tile row): ++accumulations over an empty parallel_for, Renderer.hpp:74-75
	const bool pipelined = c->slots.size() > 1;
	PipeSlot& sl = c->slots[c->batch_seq % c->slots.size()];
	hipStream_t st = pipelined ? sl.stream : c->stream;
	const BatchCounters bc = batch_counters(c, sl);
	// Camera rays of a batch go through per-pixel candidate lists when a pixel is sampled often enough to pay for its cone traversal
	// (policy.trace_primary_rays = 1 switches that off: every primary ray then walks the tree; results are identical either way).
	// (The half-angle bound assumes view.orient rotates: a non-unit quaternion, which the reference's View never holds (Camera.hpp:48-50),
	// would shear the image plane — such a camera gets no lists.)
	const float qn = c->camera.orient[0] * c->camera.orient[0] + c->camera.orient[1] * c->camera.orient[1] + c->camera.orient[2] * c->camera.orient[2] + c->camera.orient[3] * c->camera.orient[3];
	// Under a lens every camera ray walks the tree (the trace_primary_rays = 1 route, whatever that field says): a pixel's rays no longer share an
	// origin, so its lists — cones from cam.pos — do not bound them; they are neither built nor read, and cand_valid stays what it was (the lists
	// depend on scene, camera, size and tiles, not on the lens: valid ones serve the next pinhole batch).
	const bool lens = lens_on(c);
	const bool bundle = c->policy.use_bvh && c->scene.n_recs != 0 && !c->policy.trace_primary_rays && batch_n >= 3 && c->camera.z != 0.0f && std::fabs(qn - 1.0f) < 1e-4f && !c->stream_order && !lens;
	DevCounters* ctr = c->counters.as<DevCounters>();
	const float4* mat_ggx = c->mat_ggx.as<float4>();
	float* contrib = sl.contrib.as<float>();                                      // slot k of the buffer = accumulation acc_base + k + 1
	uint32_t* fat_lists = sl.fat.as<uint32_t>();
	const SceneDev sc = trace_scene(c);
	const bool count = c->policy.count_traffic != 0;
	// k_shade's grid: as many 512-thread workgroups as are resident per CU at the launched form's waves per SIMD (shade_waves: three at 6, four at 8); more only adds passes
	// (tune_shade_wgs, MIRT_TUNE_SHADE_WGS: one figure for every form instead, for sweeps; 0 = follow the form)
	const ClosurePlan plan = closure_plan(c);
	const auto shade_grid = [&](const ShadeForm& f) {
		const uint32_t wgs = c->tune_shade_wgs ? c->tune_shade_wgs : shade_waves(f) * 4u / (kShadeBlock / 64u);
		return static_cast<uint32_t>(std::min<uint64_t>((total + kShadeBlock - 1) / kShadeBlock, static_cast<uint64_t>(c->n_cu) * wgs));
	};
	{	// k_shade<FIRST> hands out (512-pixel chunk, group of accumulations) pieces: at least ~8 per workgroup of bounce 0's grid, so that a small image loads the grid evenly
		const uint32_t sgrid = shade_grid(shade_form(c, fp, plan, 0, lens, sparse));
		const uint64_t n_chunks = (static_cast<uint64_t>(fp.n_pix) + kShadeBlock - 1) / kShadeBlock;
		const uint64_t want = (8ull * sgrid + n_chunks - 1) / n_chunks;
		fp.first_groups = static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>(want, 1), batch_n));
	}

	if (pipelined && sl.in_use) HIP_TRY(c, hipStreamWaitEvent(st, sl.merged, 0));   // the slot's previous batch has been merged: buffers are free
	// (The contribution buffer needs no clearing: bounce 0 stores the word of every path.)
	if (c->debug_poison_contrib)
		HIP_TRY(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(sl.contrib.ptr), 0x7fc0deadu, sl.contrib.bytes / sizeof(float), st));   // a quiet NaN
	HIP_TRY(c, hipMemsetAsync(bc.w, 0, BatchCounters::words(nb) * sizeof(uint32_t), st));
	if (bundle) {
		// the lists outlive the batch: built by the first batch that wants them, read by all after it.  (A counting pass builds them every time: its
		// box and sphere counts are those of a batch that does all of its work.)
		if (!c->cand_valid || count) { const int r = build_primary_lists(c, sc, fp, count); if (r) return r; }
		if (pipelined && sl.cand_gen != c->cand_gen) { HIP_TRY(c, hipStreamWaitEvent(st, c->cand_built, 0)); sl.cand_gen = c->cand_gen; }
		if (sparse) {
			// the listed pixels of the active tiles: made on the main stream behind the lists' build (and, like it, behind every earlier batch's merge
			// wait), again whenever the lists or the mask have changed
			if (c->listed_gen == 0 || c->listed_for_cand != c->cand_gen || c->listed_for_freeze != c->freeze_gen) {
				HIP_TRY(c, c->listed_active.ensure((static_cast<size_t>(fp.n_pix) + 1) * sizeof(uint32_t)));
				if (!c->listed_built) HIP_TRY(c, hipEventCreateWithFlags(&c->listed_built, hipEventDisableTiming));
				uint32_t* la = c->listed_active.as<uint32_t>();
				HIP_TRY(c, hipMemsetAsync(la, 0, sizeof(uint32_t), c->stream));
				const CandWords words{ c->cand_words.as<uint32_t>() };
				hipLaunchKernelGGL(k_listed_active, dim3(grid_for(c, fp.n_pix)), dim3(kBlock), 0, c->stream, c->cand_listed.as<uint32_t>(), words.listed_pixels(), tile_frozen, la + 1, la);
				HIP_TRY(c, hipGetLastError());
				HIP_TRY(c, hipEventRecord(c->listed_built, c->stream));
				c->listed_for_cand = c->cand_gen; c->listed_for_freeze = c->freeze_gen; c->listed_gen++;
			}
			if (pipelined && sl.listed_gen != c->listed_gen) { HIP_TRY(c, hipStreamWaitEvent(st, c->listed_built, 0)); sl.listed_gen = c->listed_gen; }
		}
	}
	const CandWords cw{ c->cand_words.as<uint32_t>() };
	if (c->stream_order) {
		const int r = launch_tile_stream(c, st, sc, fp, batch_n, contrib, ctr, count);
		if (r) return r;
	} else {
		// bounce 0 has no ray stream: k_trace<PRIMARY> and k_shade<FIRST> derive the camera ray from its index (RAY GENERATION, Renderer.hpp:113-127)
		for (uint32_t bounce = 0; bounce < nb; bounce++) {
			const StreamBuf& in = sl.stream_buf[bounce & 1u];
			const StreamBuf& out = sl.stream_buf[(bounce & 1u) ^ 1u];
			const bool shadow_pending = fp.mis && bounce > 0;           // NEE rays emitted by k_shade(bounce-1)
			const bool lists = bounce == 0 && bundle;
			{ Bracket t(c, MIRT_K_TRACE, st);
			  if (lists) {
			    // camera rays through the per-pixel candidate lists (kernels.hpp kCollect): k_primary_hits intersects every sample with its pixel's list.
			    // Pixels without a list are listed in cand_listed (count: listed_pixels) and all their samples traced like any other ray.
			    // A batch that fills a wave runs one wave per pixel, lanes = accumulations, over runs of 16 pixels (k_primary_hits_wave); a smaller one keeps one lane per pixel.
			    const bool wave = batch_n >= kWaveHitsMinBatch;
			    // wave: 8 KB of LDS per wave: five workgroups per CU are resident; four times that, grid-stride, so that a CU which gets fewer is not the tail
			    const uint64_t runs = static_cast<uint64_t>(fp.n_pix) / kWaveHitsRun;
			    const uint32_t wgrid = static_cast<uint32_t>(std::min<uint64_t>((runs + kWaveHitsWaves - 1) / kWaveHitsWaves, static_cast<uint64_t>(c->n_cu) * 20u));
			    const uint32_t hgrid = static_cast<uint32_t>(std::min<uint64_t>((static_cast<uint64_t>(fp.n_pix) + kBlock - 1) / kBlock, static_cast<uint64_t>(c->n_cu) * 64u));
			    hipLaunchKernelGGL(primary_hits_kernel(count, wave, sparse), dim3(wave ? wgrid : hgrid), dim3(kBlock), 0, st, sc, fp, c->cand.as<uint32_t>(), sl.hit, ctr, tile_frozen, active_pix);
			  }
			  // the adds of bounce-1 that waited for occlusion land in the paths' contribution words before k_shade adds this bounce's terms;
			  const ShadowSink sink{ contrib, batch_n, fp.pix_bits, nullptr };
			  StreamBuf rays = in;
			  // A listed launch reads nothing else of the stream: camera rays are functions of their index.  kPrimaryList: the pixels without a candidate
			  // list (once a tile is frozen: those of them in the active tiles); kPrimaryActive, a tile frozen and no lists: every pixel of the active tiles.
			  const int primary = bounce != 0 ? kPrimaryNone : lists ? kPrimaryList : sparse ? kPrimaryActive : kPrimaryAll;
			  uint32_t* listed_count = nullptr;
			  const uint32_t* list = nullptr;
			  if (primary == kPrimaryActive) { listed_count = c->active_list.as<uint32_t>(); list = listed_count + 1; }
			  else if (lists && sparse) { listed_count = c->listed_active.as<uint32_t>(); list = listed_count + 1; }
			  else if (lists) { listed_count = cw.listed_pixels(); list = c->cand_listed.as<uint32_t>(); }
			  if (list) rays.a = reinterpret_cast<float4*>(const_cast<uint32_t*>(list));      // kernels.hpp stream_pixel_list
			  const TraceLaunch tl{ rays, sl.hit, listed_count ? Queue{ listed_count, 0u } : bc.stream_queue(bounce), bc.closest_work(bounce),      // listed: n[0] = listed pixels
			                        sl.shadow_buf, sink, shadow_pending ? bc.shadow_queue(bounce - 1) : bc.empty_queue(), bc.shadow_work(shadow_pending ? bounce - 1 : 0),
			                        bc.fat_closest(bounce, fat_lists), bc.fat_shadow(bounce, fat_lists), listed_count, ctr };
			  // (the grid of a kPrimaryList launch is sized for the whole batch, as ever: its count is known on the device only)
			  const int r = launch_trace(c, st, sc, fp, primary == kPrimaryActive ? static_cast<uint64_t>(active_pix) * batch_n : total, count, primary, tl, bounce == 0 && lens);
			  if (r) return r; }
			if (bounce == 0 && c->aov_on) { const int r = launch_first_hit_aov(c, sl, st, sc, fp); if (r) return r; }
			{ Bracket t(c, MIRT_K_SHADE, st);
			  // policy.brdf = 1 (#define BRDF 1): Closure<GGX> with this bounce's gloss decay, passed by value
			  const float decay = bounce < c->gloss_decay.size() ? c->gloss_decay[bounce] : 0.0f;
			  const ShadeForm form = shade_form(c, fp, plan, bounce, lens, sparse);
			  const auto shade = shade_kernel(form);
			  if (!shade) return fail(c, MIRT_ERR_ARG, "no shade kernel for the form first %d ggx %d lens %d sparse %d ris %d glass %d sky %d mixed %d pdf %d",
			                          form.first, form.ggx, form.lens, form.sparse, form.ris, form.glass, form.sky, form.mixed, form.pdf);
			  hipLaunchKernelGGL(shade, dim3(shade_grid(form)), dim3(kShadeBlock), 0, st, sc, fp, in, sl.hit, out, sl.shadow_buf, bounce,
			                     bc.stream_queue(bounce), bc.stream_queue(bounce + 1), bc.shadow_queue(bounce), contrib, ctr, mat_ggx, decay, c->lens, form.ris ? c->light_ris : 0u, tile_frozen,
			                     form.sky ? c->sky : SkyTable{}, plan.mask, form.pdf ? sl.pdf_plane[bounce & 1u] : nullptr, form.pdf ? sl.pdf_plane[(bounce & 1u) ^ 1u] : nullptr); }
		}
	}
	HIP_TRY(c, hipGetLastError());
	// merges are enqueued on the main stream in batch order => every bucket receives its adds in accumulation order
	if (pipelined) {
		HIP_TRY(c, hipEventRecord(sl.batch_done, st));
		HIP_TRY(c, hipStreamWaitEvent(c->stream, sl.batch_done, 0));
	}
	{ Bracket t(c, MIRT_K_RESOLVE);
	  const dim3 mgrid(grid_for(c, static_cast<uint64_t>(c->n_tiles) * (kTileSize / 4u)));
	  hipLaunchKernelGGL(merge_kernel(sparse), mgrid, dim3(kBlock), 0, c->stream, c->accumulator.as<float4>(), sl.contrib.as<float4>(), c->n_tiles, c->policy.buckets, batch_n, fp.acc_base, tile_frozen); }
	HIP_TRY(c, hipGetLastError());
	if (pipelined) { HIP_TRY(c, hipEventRecord(sl.merged, c->stream)); sl.in_use = true; }
	c->batch_seq++;
	c->accumulations += batch_n;
	if (c->policy.profile && c->pending.size() > 512) harvest(c);
	return MIRT_OK;
}

template <class T>
int upload(mirt_ctx* c, DeviceBuffer& buf, const std::vector<T>& host) {
	HIP_TRY(c, buf.ensure(std::max<size_t>(host.size(), 1) * sizeof(T)));
	if (!host.empty()) HIP_TRY(c, hipMemcpyAsync(buf.ptr, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
	return MIRT_OK;
}

int check_ready(mirt_ctx* c) {
	if (!c) return MIRT_ERR_ARG;
	if (!c->have_scene) return fail(c, MIRT_ERR_STATE, "mirt_set_scene has not been called");
	if (!c->have_camera) return fail(c, MIRT_ERR_STATE, "mirt_set_camera has not been called");
	if (c->width == 0 && c->height == 0) return fail(c, MIRT_ERR_STATE, "mirt_resize has not been called");
	return MIRT_OK;
}

// Launches what mirt_accumulate_async has deferred.  Every entry point that observes results or changes what a launch
// reads (scene, camera, policy, size, tile range) calls this first, so deferral is invisible except in timing.
int flush_deferred(mirt_ctx* c) {
	if (!c->deferred) return MIRT_OK;
	const uint32_t n = c->deferred;
	c->deferred = 0;
	HIP_TRY(c, hipSetDevice(c->device));
	int r = ensure_streams(c); if (r) return r;
	return launch_batch(c, n);
}

// The two preambles of an entry point.  The order of their steps is what keeps deferral invisible, so it is stated here and nowhere else.
// An entry point that observes results, or changes what they are read with: what is deferred is launched, the context's device is the
// current one, and every stream has finished — the accumulator, the AOV slab and the counters hold every accumulation issued so far.
int flush_and_wait(mirt_ctx* c) {
	{ const int fr = flush_deferred(c); if (fr) return fr; }
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, sync_all(c));
	return MIRT_OK;
}
// An entry point that zeroes or overwrites the accumulator: what is deferred is dropped instead (it would be wiped anyway), then as above.
int drop_and_wait(mirt_ctx* c) {
	c->deferred = 0;
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, sync_all(c));
	return MIRT_OK;
}

// ---- mirt_set_scene, step by step --------------------------------------------------------------
struct SceneArgs {
	const mirt_sphere *geometry, *bvh_prims; uint32_t n_spheres;
	const mirt_bvh_node* nodes; uint32_t n_nodes;
	const mirt_material* materials; uint32_t n_materials;
	const int32_t* lights; uint32_t n_lights;
	const float *ambient_color, *hdri_rgba; uint32_t hdri_w, hdri_h;
};

// Validate everything the kernels index with: an out-of-range id would fault the GPU.
int check_scene_args(mirt_ctx* c, const SceneArgs& a) {
	if (a.n_spheres && (!a.geometry || !a.bvh_prims)) return fail(c, MIRT_ERR_ARG, "geometry / bvh_prims is NULL");
	if (a.n_spheres >= (1u << 26)) return fail(c, MIRT_ERR_ARG, "more than 2^26 spheres");      // 32-bit record offsets in the trace kernels (GPU-built trees do not pass build_records)
	if (a.n_nodes && !a.nodes) return fail(c, MIRT_ERR_ARG, "nodes is NULL");
	if (!a.materials || a.n_materials == 0 || a.n_materials > MIRT_MAX_MATERIALS) return fail(c, MIRT_ERR_ARG, "need 1..%u materials, got %u", MIRT_MAX_MATERIALS, a.n_materials);
	if (a.n_lights && !a.lights) return fail(c, MIRT_ERR_ARG, "lights is NULL");
	if (!a.ambient_color || !a.hdri_rgba || a.hdri_w == 0 || a.hdri_h == 0) return fail(c, MIRT_ERR_ARG, "sky needs ambient_color and an hdri of at least 1x1");
	for (uint32_t i = 0; i < a.n_spheres; i++) {
		if (a.geometry[i].material_ID < 0 || static_cast<uint32_t>(a.geometry[i].material_ID) >= a.n_materials ||
		    a.bvh_prims[i].material_ID < 0 || static_cast<uint32_t>(a.bvh_prims[i].material_ID) >= a.n_materials)
			return fail(c, MIRT_ERR_ARG, "sphere %u: material_ID out of range", i);
		// non-finite centres or radii would reach the tree builders' sorts and the box arithmetic as NaN (the reference has no check; UB there)
		for (const mirt_sphere* s : { &a.geometry[i], &a.bvh_prims[i] })
			if (!std::isfinite(s->position[0]) || !std::isfinite(s->position[1]) || !std::isfinite(s->position[2]) || !std::isfinite(s->radius_sq) || s->radius_sq < 0.0f)
				return fail(c, MIRT_ERR_ARG, "sphere %u: position / radius_sq must be finite, radius_sq >= 0", i);
	}
	for (uint32_t i = 0; i < a.n_lights; i++)
		if (a.lights[i] < 0 || static_cast<uint32_t>(a.lights[i]) >= a.n_spheres) return fail(c, MIRT_ERR_ARG, "light %u: index out of range", i);
	// children point forward and every node has at most one parent: the node array is a forest, so the breadth-first
	// re-layout (bvh_layout.hpp) visits at most n_nodes nodes (shared children would make it grow like Fibonacci numbers)
	std::vector<uint8_t> has_parent(a.n_nodes, 0);
	for (uint32_t i = 0; i < a.n_nodes; i++) {
		const mirt_bvh_node& nd = a.nodes[i];
		if (nd.prim_count == 0) {
			if (nd.first_id <= i || static_cast<uint64_t>(nd.first_id) + 1 >= a.n_nodes) return fail(c, MIRT_ERR_ARG, "node %u: child index %u invalid", i, nd.first_id);
			if (has_parent[nd.first_id] || has_parent[nd.first_id + 1]) return fail(c, MIRT_ERR_ARG, "node %u: child pair %u is referenced by more than one parent", i, nd.first_id);
			has_parent[nd.first_id] = has_parent[nd.first_id + 1] = 1;
		} else if (static_cast<uint64_t>(nd.first_id) + nd.prim_count > a.n_spheres) return fail(c, MIRT_ERR_ARG, "node %u: prim range out of bounds", i);
	}
	if (a.n_spheres && a.n_nodes == 0) return fail(c, MIRT_ERR_ARG, "spheres without BVH nodes");
	return MIRT_OK;
}

// The scene's tables as the kernels read them (host copies: they outlive the stream synchronisation that ends their uploads).
struct SceneTables {
	std::vector<float4> sph, lsp, lem, alb, emi, ggx, gls, sky, gsp;
	std::vector<int32_t> pm, gpm;
};
SceneTables flatten_tables(const SceneArgs& a) {
	SceneTables t;
	t.sph.resize(a.n_spheres); t.pm.resize(a.n_spheres); t.lsp.resize(a.n_lights); t.lem.resize(a.n_lights);
	t.gsp.resize(a.n_spheres); t.gpm.resize(a.n_spheres);
	t.alb.resize(a.n_materials); t.emi.resize(a.n_materials); t.ggx.resize(a.n_materials); t.gls.resize(a.n_materials); t.sky.resize(static_cast<size_t>(a.hdri_w) * a.hdri_h);
	for (uint32_t i = 0; i < a.n_spheres; i++) {
		t.sph[i] = make_float4(a.bvh_prims[i].position[0], a.bvh_prims[i].position[1], a.bvh_prims[i].position[2], a.bvh_prims[i].radius_sq);
		t.pm[i] = a.bvh_prims[i].material_ID;
		t.gsp[i] = make_float4(a.geometry[i].position[0], a.geometry[i].position[1], a.geometry[i].position[2], a.geometry[i].radius_sq);   // light_list.hpp GeometryTable
		t.gpm[i] = a.geometry[i].material_ID;
	}
	// NEE reads scene.geometry[light], then material[geometry[light].material_ID].emission (Renderer.hpp:261-263,283):
	// flattened to one table per light so the kernel makes two independent loads instead of four dependent ones
	for (uint32_t l = 0; l < a.n_lights; l++) {
		const mirt_sphere& g = a.geometry[a.lights[l]];
		const float* e = a.materials[g.material_ID].emission;
		t.lsp[l] = make_float4(g.position[0], g.position[1], g.position[2], g.radius_sq);
		float id_bits; const int32_t id = a.lights[l]; std::memcpy(&id_bits, &id, 4);
		t.lem[l] = make_float4(e[0], e[1], e[2], id_bits);
	}
	for (uint32_t i = 0; i < a.n_materials; i++) {
		const mirt_material& m = a.materials[i];
		t.alb[i] = make_float4(m.albedo[0], m.albedo[1], m.albedo[2], 0.0f);
		t.emi[i] = make_float4(m.emission[0], m.emission[1], m.emission[2], 0.0f);
		t.ggx[i] = make_float4(m.F0[0], m.F0[1], m.F0[2], m.roughness);   // Closure<GGX> (policy.brdf = 1)
		t.gls[i] = make_float4(m.transmission[0], m.transmission[1], m.transmission[2], 1.0f + m.IOR_minus_one);   // the dielectric interface (mirt_set_transmission)
	}
	std::memcpy(t.sky.data(), a.hdri_rgba, t.sky.size() * sizeof(float4));
	return t;
}

// mirt_set_transmission(1) asks this of the materials (rows {transmission.rgb, 1 + IOR_minus_one}); with the switch off no kernel reads them and
// nothing is asked, as ever.  A transmissive material (max(transmission) > 0) needs a finite index above 0.
// The rule itself is scene_update_host.hpp's check_glass_rows: mirt_update_materials asks it of the table an edit would leave.
int check_glass(mirt_ctx* c, const std::vector<float4>& gls) {
	char msg[256];
	if (const int r = mirt_scene_update::check_glass_rows(reinterpret_cast<const float*>(gls.data()), gls.size(), msg, sizeof msg)) return fail(c, r, "%s", msg);
	return MIRT_OK;
}
bool has_glass(const std::vector<float4>& gls) {
	for (const float4& g : gls) if (g.x > 0.0f || g.y > 0.0f || g.z > 0.0f) return true;
	return false;
}

// mirt_set_sky_sampling(1) asks this of the environment map (binary32, the kernels' own products): every texel that owns a cell has a finite
// importance max(t.rgb x ambient) >= 0, and the importances' sum stays inside binary32.  With the switch off nothing is asked, as ever.
int check_sky_texels(mirt_ctx* c, const float4* texels, uint32_t w, uint32_t h, const float amb[3]) {
	const uint32_t cols = std::max(w, 2u) - 1u, rows = std::max(h, 2u) - 1u;
	const double pi = 3.14159265358979323846;
	double sum = 0.0;
	for (uint32_t r = 0; r < rows; r++) {
		const double omega = (2.0 * pi / cols) * (std::cos(pi * r / rows) - std::cos(pi * (r + 1) / rows));
		for (uint32_t x = 0; x < cols; x++) {
			const float4 t = texels[static_cast<size_t>(r) * w + x];
			const float p[3] = { t.x * amb[0], t.y * amb[1], t.z * amb[2] };
			const float m = std::max(std::max(p[0], p[1]), p[2]);
			if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2])) || m < 0.0f)
				return fail(c, MIRT_ERR_ARG, "environment map texel (row %u, column %u): importance max(rgb x ambient_color) is negative or not finite (mirt_set_sky_sampling is on)", r, x);
			sum += static_cast<double>(m) * omega;
		}
	}
	if (!(sum < 0.5 * static_cast<double>(MIRT_FLT_MAX))) return fail(c, MIRT_ERR_ARG, "environment map: the importances sum to %g, beyond binary32 (mirt_set_sky_sampling is on)", sum);
	return MIRT_OK;
}
// The sampling table of the scene's environment map, built on the device from c->hdri (kernels.hpp k_sky_importance, k_sky_scan) on the main
// stream, which is synchronised before the total is read.  The caller has validated the texels and no batch is in flight.
int build_sky_table(mirt_ctx* c) {
	const SceneDev& s = c->scene;
	const uint32_t cols = static_cast<uint32_t>(std::max(s.hdri_w, 2) - 1), rows = static_cast<uint32_t>(std::max(s.hdri_h, 2) - 1);
	HIP_TRY(c, c->sky_table.ensure(sky_table_floats(rows, cols) * sizeof(float)));
	float* t = c->sky_table.as<float>();
	hipLaunchKernelGGL(k_sky_importance, dim3(rows), dim3(kSkyBlock), 0, c->stream, s.hdri, s.hdri_w, s.ambient[0], s.ambient[1], s.ambient[2], rows, cols, t);
	hipLaunchKernelGGL(k_sky_scan, dim3(rows), dim3(kSkyBlock), 0, c->stream, rows, cols, t);
	HIP_TRY(c, hipGetLastError());
	float total = 0.0f;
	HIP_TRY(c, hipMemcpyAsync(&total, t + rows - 1, sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	c->sky = SkyTable{ t, rows, cols };
	c->sky_total = total;
	return MIRT_OK;
}
void drop_sky_table(mirt_ctx* c) { c->sky_table.release(); c->sky = SkyTable{}; c->sky_total = 0.0f; }

// The records the kernels walk for this scene, uploaded (a host-built tree) or built in place (the GPU LBVH over c->spheres, uploaded by the caller).
struct SceneRecords {
	std::vector<float> f32;                 // host copies, as in SceneTables
	std::vector<uint32_t> half, wide;
	uint32_t n_recs = 0, depth = 0;
	bool is_half = false, is_wide = false;
	bool in_recs_wide = false;              // the records lie in c->recs_wide instead of c->recs (the GPU builder writes both layouts)
};
int build_scene_records(mirt_ctx* c, const SceneArgs& a, const std::vector<float4>& sph, SceneRecords& t) {
	const uint32_t n_spheres = a.n_spheres;
	if (c->policy.gpu_build && !c->policy.reference_tree && n_spheres >= 2) {
		// the tree the kernels walk, built where it is used (lbvh_build.hip); binary16 records under the same conditions as on the host
		t.n_recs = n_spheres - 1;
		t.is_half = c->allow_half;
		for (uint32_t i = 0; t.is_half && i < n_spheres; i++) {
			const float rad = std::sqrt(sph[i].w);
			const float amax = std::fmax(std::fmax(std::fabs(sph[i].x), std::fabs(sph[i].y)), std::fabs(sph[i].z)) + rad * 1.0001f;
			t.is_half = mirt_host::half_box_adequate(amax, 2.0f * rad, true);
		}
		HIP_TRY(c, c->recs.ensure(static_cast<size_t>(t.n_recs) * (t.is_half ? 32u : 64u)));
		const bool want_wide = t.is_half && c->tune_wide;                    // the 4-wide binary16 records as well (used when the tree is shallow enough)
		if (want_wide) HIP_TRY(c, c->recs_wide.ensure(static_cast<size_t>(t.n_recs) * 64u));
		std::string why;
		uint32_t n_wide = 0;
		if (!mirt_gpu::build_lbvh(c->stream, c->spheres.as<float4>(), n_spheres, t.is_half ? nullptr : c->recs.as<float>(), t.is_half ? c->recs.as<uint32_t>() : nullptr, &t.depth, &why,
		                          want_wide ? c->recs_wide.as<uint32_t>() : nullptr, &n_wide))
			return fail(c, MIRT_ERR_HIP, "GPU BVH build: %s", why.c_str());
		if (t.depth >= kStack) return fail(c, MIRT_ERR_ARG, "GPU-built BVH is %u levels deep (limit %u): set policy.gpu_build = 0 for this scene", t.depth, kStack);
		if (want_wide && n_wide && 3u * (t.depth / 2u) < kStack) { t.is_wide = t.in_recs_wide = true; t.n_recs = n_wide; }     // depth counts the leaf level: depth / 2 = wide levels, rounded up
		return MIRT_OK;
	}
	std::vector<mirt_bvh_node> own; std::vector<uint32_t> prim_of_slot;
	const bool caller_tree = c->policy.reference_tree || n_spheres == 0;
	if (caller_tree) {
		// traverse the caller's tree exactly as handed over (BVH.hpp:18-31 nodes over the BVH-order prims)
		own.assign(a.nodes, a.nodes + a.n_nodes);
		mirt_host::split_multi_prim_leaves(own);                         // the kernels know one-prim leaves only
	} else {
		// default: GPU-internal SAH tree over the same BVH-order prims (hit.primID keeps its meaning; results are identical)
		mirt_host::build_sah_tree(a.bvh_prims, n_spheres, own, prim_of_slot);
	}
	const std::vector<uint32_t>* slot_map = caller_tree ? nullptr : &prim_of_slot;
	const std::string why = mirt_host::build_records(own.data(), static_cast<uint32_t>(own.size()), a.bvh_prims, n_spheres, t.f32, &t.depth, slot_map);
	if (!why.empty()) return fail(c, MIRT_ERR_ARG, "%s BVH rejected: %s", caller_tree ? "caller's" : "internal", why.c_str());
	t.n_recs = static_cast<uint32_t>(t.f32.size() / 16);
	t.is_half = c->allow_half && mirt_host::build_half_records(t.f32, t.half);
	// 4-wide binary16 records when the tree allows (bvh_layout.hpp build_wide_half_records): half as many dependent fetches per ray
	uint32_t wide_levels = 0;
	t.is_wide = t.is_half && c->tune_wide && mirt_host::build_wide_half_records(t.f32, t.wide, &wide_levels);
	if (t.is_wide) t.n_recs = static_cast<uint32_t>(t.wide.size() / 16);
	return t.is_wide ? upload(c, c->recs, t.wide) : t.is_half ? upload(c, c->recs, t.half) : upload(c, c->recs, t.f32);
}

// The LDS staging plan of the scene just stored in c->scene, and room for it in every kernel that uses dynamic LDS.
int plan_trace_lds(mirt_ctx* c) {
	const LdsPlan p = lds_plan(c);
	c->scene.stack16 = p.stack16; c->scene.lds_recs = p.lds_recs; c->scene.lds_spheres = p.lds_spheres;
	const int lds_max = static_cast<int>(kLdsPerCu);
	for (int k = 0; k < 2 * kPrimaryForms * 2; k++)                               // every (count, primary, lens) that exists
		if (const auto f = trace_kernel(k & 1, (k >> 1) % kPrimaryForms, k >= 2 * kPrimaryForms)) HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(f), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
	for (const auto f : kPrimaryCand) HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(f), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
	HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_id_map), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
	return MIRT_OK;
}

void commit_scene(mirt_ctx* c, const SceneArgs& a, const SceneRecords& t) {
	SceneDev& s = c->scene;
	s.recs = t.in_recs_wide ? c->recs_wide.as<float4>() : c->recs.as<float4>(); s.spheres = c->spheres.as<float4>(); s.prim_mat = c->prim_mat.as<int32_t>();
	s.light_sphere = c->light_sphere.as<float4>(); s.light_emit = c->light_emit.as<float4>();
	s.mat_albedo = c->mat_albedo.as<float4>(); s.mat_emission = c->mat_emission.as<float4>();
	s.hdri = c->hdri.as<float4>(); s.mat_glass = c->mat_glass.as<float4>();
	s.n_spheres = a.n_spheres; s.n_recs = t.n_recs; s.n_mat = a.n_materials; s.n_lights = a.n_lights;
	s.half_boxes = t.is_half ? 1u : 0u;
	s.wide = t.is_wide ? 1u : 0u;
	c->bvh_depth = t.depth;
	for (int k = 0; k < 3; k++) s.ambient[k] = a.ambient_color[k];
	s.hdri_w = static_cast<int32_t>(a.hdri_w); s.hdri_h = static_cast<int32_t>(a.hdri_h);
	s.hdri_fw = static_cast<float>(static_cast<int32_t>(a.hdri_w) - 1);                 // Application.cpp:230-231
	s.hdri_fh = static_cast<float>(static_cast<int32_t>(a.hdri_h) - 1);
	{ const float x = a.ambient_color[0], y = a.ambient_color[1], z = a.ambient_color[2];
	  const float m1 = (y < z) ? z : y; const float m0 = (x < m1) ? m1 : x; s.has_ambient = (m0 > 0.0f) ? 1u : 0u; }   // Renderer.hpp:79
}

// Body of mirt_debug_trace_closest (tfar = NULL; result: n HitRec) and mirt_debug_trace_shadow (result: n occlusion words): n caller-supplied
// rays through the product's own k_trace and fat-ray pass, all of them in segment 0 of one queue (slot = ray number).
int debug_trace(mirt_ctx* c, const char* who, size_t n, const float* p_xyz, const float* dir_xyz, const float* tfar, void* result) {
	const bool shadow = tfar != nullptr;
	const size_t result_bytes = n * (shadow ? sizeof(uint32_t) : sizeof(HitRec));
	HIP_TRY(c, hipSetDevice(c->device));
	ScopedBuffer rays, res, cnt, ctr, fat;
	HIP_TRY(c, rays.ensure(n * 2 * sizeof(float4))); HIP_TRY(c, res.ensure(result_bytes)); HIP_TRY(c, cnt.ensure(BatchCounters::words(1) * 4));
	HIP_TRY(c, ctr.ensure(sizeof(DevCounters))); HIP_TRY(c, fat.ensure(2u * kFatCapacity * sizeof(uint32_t)));
	// the caller's planes as the records k_trace reads: plane a = {p, tfar} (closest-hit: {p, path}, unused), plane b = {dir, unused}
	float4* d = rays.as<float4>();
	{ std::vector<float4> rec(2 * n);
	  for (size_t i = 0; i < n; i++) {
	    rec[i] = make_float4(p_xyz[i], p_xyz[n + i], p_xyz[2 * n + i], shadow ? tfar[i] : 0.0f);
	    rec[n + i] = make_float4(dir_xyz[i], dir_xyz[n + i], dir_xyz[2 * n + i], 0.0f);
	  }
	  HIP_TRY(c, hipMemcpy(d, rec.data(), 2 * n * sizeof(float4), hipMemcpyHostToDevice)); }
	const BatchCounters bc{ cnt.as<uint32_t>(), 1u, 0u };
	const uint32_t n32 = static_cast<uint32_t>(n);
	HIP_TRY(c, hipMemset(cnt.ptr, 0, BatchCounters::words(1) * 4));
	HIP_TRY(c, hipMemcpy(shadow ? bc.shadow_queue(0).n : bc.stream_queue(0).n, &n32, 4, hipMemcpyHostToDevice));
	HIP_TRY(c, hipMemset(ctr.ptr, 0, sizeof(DevCounters)));
	TraceLaunch tl{};
	if (shadow) { tl.sh.a = d; tl.sh.b = d + n; tl.sink.occ = res.as<uint32_t>(); }   // the sink only records the occlusion flags
	else { tl.in.a = d; tl.in.b = d + n; tl.hit = res.as<HitRec>(); }
	tl.closest_queue = bc.stream_queue(0); tl.closest_work = bc.closest_work(0);
	tl.shadow_queue = bc.shadow_queue(0); tl.shadow_work = bc.shadow_work(0);
	tl.fat_closest = bc.fat_closest(0, fat.as<uint32_t>()); tl.fat_shadow = bc.fat_shadow(0, fat.as<uint32_t>());
	tl.ctr = ctr.as<DevCounters>();                                              // scratch: the context's counters stay as they are
	{ Bracket t(c, MIRT_K_TRACE);                                                // policy.profile: the launch is timed like those of a batch (mirt_get_kernel_times)
	  const int r = launch_trace(c, c->stream, trace_scene(c), FrameParams{}, n, false, kPrimaryNone, tl); if (r) return r; }
	hipError_t e = hipGetLastError();
	if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
	if (e == hipSuccess) e = hipMemcpy(result, res.ptr, result_bytes, hipMemcpyDeviceToHost);
	if (e != hipSuccess) return fail(c, MIRT_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
	return MIRT_OK;
}

// k_id_map (id_map.hpp) over the whole image of `c`, on c's stream, through the scene, the traversal settings and the camera of `gs` (c itself, or
// the geometry context of mirt_set_motion_geometry: same device).  Either plane may be NULL.  The caller has made the device current.
int launch_id_map(mirt_ctx* c, const mirt_ctx* gs, int32_t* prim_dev, float* dist_dev) {
	const uint64_t n = static_cast<uint64_t>(c->width) * c->height;
	if (n == 0) return MIRT_OK;
	if (n >= (1ull << 31)) return fail(c, MIRT_ERR_ARG, "id map: %u x %u pixels do not fit a 31-bit pixel index", c->width, c->height);
	HIP_TRY(c, c->id_words.ensure(2 * sizeof(uint32_t)));
	HIP_TRY(c, hipMemsetAsync(c->id_words.ptr, 0, 2 * sizeof(uint32_t), c->stream));
	const IdMapDev p{ gs->camera, c->width, static_cast<uint32_t>(n), 1.0f / static_cast<float>(c->width) };
	{ Bracket t(c, MIRT_K_RESOLVE);
	  hipLaunchKernelGGL(k_id_map, dim3(trace_grid(gs, n)), dim3(kTraceBlock), trace_lds(gs), c->stream, trace_scene(gs), p, prim_dev, dist_dev, c->id_words.as<uint32_t>()); }
	HIP_TRY(c, hipGetLastError());
	return MIRT_OK;
}

// ---- what exact stream order excludes (DESIGN.md "One switch table in the host layers") ------------------------------------------
// One row per feature that mirt_set_stream_order(ctx, 1) cannot run with.  The exclusion is a rule about pairs, and both directions of every
// pair read this table and nothing else: mirt_set_stream_order(ctx, 1) refuses with the first row that is on (refuse_exact_order), and a
// feature's entry point asked to turn the feature on under exact order refuses with its own row (refuse_under_exact_order).
struct ExactExcludes {
	uint32_t (*on)(const mirt_ctx*);   // 0 = off in this context; otherwise how much of it there is
	const char* why;                   // the message is "exact stream order <why>: <the call that lifts the refusal> first"
	const char* off;                   // what turns the feature off: a format that may print on()
};
enum ExactRow { X_LENS, X_FROZEN, X_LIGHT_RIS, X_TRANSMISSION, X_SKY_SAMPLING, X_GGX_PDF, X_CLOSURES, X_AOV, X_ROWS };
const ExactExcludes kExactExcludes[X_ROWS] = {
	/* X_LENS */         { [](const mirt_ctx* c) -> uint32_t { return lens_on(c); }, "replays the reference, which has no lens (Camera.hpp:80-88 ignores it)", "call mirt_set_lens(ctx, 0, 0)" },
	/* X_FROZEN */       { [](const mirt_ctx* c) { return c->n_frozen; }, "runs a tile's whole bounce loop in one launch and has no form that skips frozen tiles", "%u are frozen, mirt_reset" },
	/* X_LIGHT_RIS */    { [](const mirt_ctx* c) { return c->light_ris; }, "replays the reference, which draws its NEE light uniformly (Renderer.hpp:259)", "call mirt_set_light_ris(ctx, 0)" },
	/* X_TRANSMISSION */ { [](const mirt_ctx* c) { return c->transmission; }, "replays the reference, no closure of which reads transmission", "call mirt_set_transmission(ctx, 0)" },
	/* X_SKY_SAMPLING */ { [](const mirt_ctx* c) { return c->sky_sampling; }, "replays the reference, which draws its NEE light among the sphere lights only", "call mirt_set_sky_sampling(ctx, 0)" },
	/* X_GGX_PDF */      { [](const mirt_ctx* c) { return c->ggx_pdf; }, "replays the reference, whose Closure<GGX>::pdf is 0 (DataStreams.hpp:196-198)", "call mirt_set_ggx_pdf(ctx, 0)" },
	/* X_CLOSURES */     { [](const mirt_ctx* c) { return static_cast<uint32_t>(c->closures.size()); }, "replays the reference, every closure of which is policy.brdf's (Renderer.hpp:70)", "call mirt_set_material_closures(ctx, NULL, 0)" },
	/* X_AOV */          { [](const mirt_ctx* c) { return c->aov_on; }, "keeps no hit records (k_tile_stream runs a tile's whole bounce loop in one launch), so it cannot feed the first-hit AOVs", "call mirt_set_aov(ctx, 0)" },
};
int refuse_exact_order(mirt_ctx* c) {
	for (const ExactExcludes& x : kExactExcludes) if (const uint32_t n = x.on(c)) {
		char off[96];
		snprintf(off, sizeof off, x.off, n);
		return fail(c, MIRT_ERR_STATE, "exact stream order %s: %s first", x.why, off);
	}
	return MIRT_OK;
}
int refuse_under_exact_order(mirt_ctx* c, ExactRow row) {
	return c->stream_order ? fail(c, MIRT_ERR_STATE, "exact stream order %s: call mirt_set_stream_order(ctx, 0) first", kExactExcludes[row].why) : MIRT_OK;
}

// The preamble of a scalar switch's setter, in the order every one of them keeps: NULL, range (`range_fmt` prints value and max), refusal under exact
// stream order, a value the context already holds (kHeld: nothing is flushed and the setter returns MIRT_OK), the switch's own validation, and the
// flush: deferred accumulations render under the setting they were issued under.  What comes after BEGIN_SWITCH is the setter's own.
constexpr int kHeld = 1;
int begin_switch(mirt_ctx* c, uint32_t mirt_ctx::* field, uint32_t value, uint32_t max, const char* range_fmt, ExactRow row, int (*validate)(mirt_ctx*, uint32_t) = nullptr) {
	if (!c) return MIRT_ERR_ARG;
	if (value > max) return fail(c, MIRT_ERR_ARG, range_fmt, value, max);
	int r;
	if (value && (r = refuse_under_exact_order(c, row))) return r;
	if (value == c->*field) return kHeld;
	if (validate && (r = validate(c, value))) return r;
	return flush_deferred(c);
}
#define BEGIN_SWITCH(...) do { const int _r = begin_switch(__VA_ARGS__); if (_r) return _r == kHeld ? MIRT_OK : _r; } while (0)
// The getters of the uint32 switches; the exported symbols are exactly those of mirt.h.
#define SWITCH_GETTER(name, field) int mirt_get_##name(const mirt_ctx* c, uint32_t* value) { if (!c || !value) return MIRT_ERR_ARG; *value = c->field; return MIRT_OK; }

} // namespace

extern "C" {

const char* mirt_last_error(const mirt_ctx* ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

int mirt_create(int device, mirt_ctx** out) {
	if (!out) return fail(nullptr, MIRT_ERR_ARG, "out is NULL");
	*out = nullptr;
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n <= 0) return fail(nullptr, MIRT_ERR_NO_DEVICE, "no HIP device available (%s); mirt has no CPU path", hipGetErrorString(e));
	if (device < 0 || device >= n) return fail(nullptr, MIRT_ERR_ARG, "device %d out of range (have %d)", device, n);
	e = hipSetDevice(device);
	if (e != hipSuccess) return fail(nullptr, MIRT_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
	mirt_ctx* c = new mirt_ctx();
	c->device = device;
	if (const char* e = std::getenv("MIRT_TUNE_CHUNK")) c->tune_chunk = static_cast<uint32_t>(std::min(std::max(std::atoi(e), 64), 65536)) & ~63u;
	if (const char* e = std::getenv("MIRT_TUNE_REFILL_IDLE")) c->tune_refill_idle = static_cast<uint32_t>(std::min(std::max(std::atoi(e), 1), 64));
	if (const char* e = std::getenv("MIRT_TUNE_DENOISE_STAGED")) c->tune_denoise_staged = static_cast<uint32_t>(std::min(std::max(std::atoi(e), 0), static_cast<int>(kAtrousStagedMaxStep)));
	if (const char* e = std::getenv("MIRT_TUNE_WIDE")) c->tune_wide = std::atoi(e) != 0 ? 1u : 0u;
	if (const char* e = std::getenv("MIRT_TUNE_LEAF_BATCH")) c->tune_leaf_batch = static_cast<uint32_t>(std::min(std::max(std::atoi(e), 1), 64));
	if (const char* e = std::getenv("MIRT_TUNE_TRACE_WGS")) c->tune_trace_wgs = std::atoi(e) == 1 ? 1u : 2u;
	if (const char* e = std::getenv("MIRT_TUNE_SHADE_WGS")) c->tune_shade_wgs = static_cast<uint32_t>(std::min(std::max(std::atoi(e), 1), 16));
	if (const char* e = std::getenv("MIRT_DEBUG_POISON_CONTRIB")) c->debug_poison_contrib = std::atoi(e) != 0;
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
	if (e == hipSuccess) e = c->counters.ensure(sizeof(DevCounters));
	if (e == hipSuccess) e = hipMemsetAsync(c->counters.ptr, 0, sizeof(DevCounters), c->stream);
	if (e != hipSuccess) { int r = fail(nullptr, MIRT_ERR_HIP, "context setup: %s", hipGetErrorString(e)); delete c; return r; }
	*out = c;
	return MIRT_OK;
}

int mirt_destroy(mirt_ctx* c) {
	if (!c) return MIRT_ERR_ARG;
	(void)hipSetDevice(c->device);
	(void)sync_all(c);
	harvest(c);
	for (PipeSlot& sl : c->slots) sl.release();
	c->slots.clear();
	for (hipEvent_t e : c->free_events) (void)hipEventDestroy(e);
	DeviceBuffer* bufs[] = { &c->recs, &c->recs_wide, &c->spheres, &c->prim_mat, &c->light_sphere, &c->light_emit, &c->mat_albedo, &c->mat_emission,
	                         &c->mat_ggx, &c->mat_glass, &c->mat_merged, &c->hdri, &c->refit_links, &c->refit_edits, &c->geo_sphere, &c->geo_mat, &c->light_scan, &c->sky_table, &c->accumulator, &c->aov, &c->framebuffer, &c->counters, &c->gloss_decay_dev,
	                         &c->cand, &c->cand_listed, &c->cand_words, &c->noise_rec, &c->noise_hist, &c->noise_above,
	                         &c->dn_cv[0], &c->dn_cv[1], &c->dn_gd, &c->dn_mu, &c->tile_frozen, &c->active_list, &c->tile_counts,
	                         &c->th_x, &c->th_g, &c->th_n, &c->th_len, &c->th_stats, &c->th_id, &c->th_id_cur, &c->th_snap, &c->id_out, &c->id_words };
	for (DeviceBuffer* b : bufs) b->release();
	if (c->frame_host) (void)hipHostFree(c->frame_host);
	if (c->cand_built) (void)hipEventDestroy(c->cand_built);
	if (c->listed_built) (void)hipEventDestroy(c->listed_built);
	c->listed_active.release();
	if (c->stream) (void)hipStreamDestroy(c->stream);
	delete c;
	return MIRT_OK;
}

int mirt_set_scene(mirt_ctx* c, const mirt_sphere* geometry, const mirt_sphere* bvh_prims, uint32_t n_spheres,
                   const mirt_bvh_node* nodes, uint32_t n_nodes, const mirt_material* materials, uint32_t n_materials,
                   const int32_t* lights, uint32_t n_lights, const float ambient_color[3],
                   const float* hdri_rgba, uint32_t hdri_w, uint32_t hdri_h) {
	if (!c) return MIRT_ERR_ARG;
	{ const int fr = flush_deferred(c); if (fr) return fr; }
	const SceneArgs a{ geometry, bvh_prims, n_spheres, nodes, n_nodes, materials, n_materials, lights, n_lights, ambient_color, hdri_rgba, hdri_w, hdri_h };
	int r = check_scene_args(c, a); if (r) return r;
	HIP_TRY(c, hipSetDevice(c->device));
	const SceneTables t = flatten_tables(a);     // host copies of tables and records: alive until the stream has been synchronised
	if (c->transmission && (r = check_glass(c, t.gls))) return r;
	if (c->sky_sampling && (r = check_sky_texels(c, t.sky.data(), hdri_w, hdri_h, ambient_color))) return r;
	SceneRecords tree;
	if ((r = upload(c, c->spheres, t.sph)) || (r = build_scene_records(c, a, t.sph, tree)) || (r = upload(c, c->prim_mat, t.pm)) ||
	    (r = upload(c, c->light_sphere, t.lsp)) || (r = upload(c, c->light_emit, t.lem)) || (r = upload(c, c->mat_albedo, t.alb)) ||
	    (r = upload(c, c->mat_emission, t.emi)) || (r = upload(c, c->mat_ggx, t.ggx)) || (r = upload(c, c->mat_glass, t.gls)) || (r = upload(c, c->hdri, t.sky)) ||
	    (r = upload(c, c->geo_sphere, t.gsp)) || (r = upload(c, c->geo_mat, t.gpm))) return r;
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	c->cand_valid = false;                                                             // spheres or tree changed (a node-only update included)
	commit_scene(c, a, tree);
	drop_history(c);                                                                   // other surfaces: nothing of the old view may be reprojected onto them
	c->glass_host = t.gls; c->scene_has_glass = has_glass(t.gls);
	c->alb_host = t.alb; c->ggx_host = t.ggx; c->emi_host = t.emi; c->mat_merged_valid = false;
	if (c->sky_sampling) { HIP_TRY(c, sync_all(c)); if ((r = build_sky_table(c))) return r; }      // (a batch in flight on another stream may read the old table)
	if ((r = plan_trace_lds(c))) return r;
	c->have_scene = true;
	c->env_baked = false;
	c->refit_links_valid = false;                                                      // another tree
	c->light_ids.assign(lights, lights + n_lights); c->light_sphere_host = t.lsp;      // what mirt_update_spheres patches
	return MIRT_OK;
}

int mirt_set_camera(mirt_ctx* c, const float pos[3], const float orient_xyzw[4], float half_width, float half_height, float z, float exposure) {
	if (!c) return MIRT_ERR_ARG;
	if (!pos || !orient_xyzw) return fail(c, MIRT_ERR_ARG, "pos / orient is NULL");
	if (c->have_camera && std::memcmp(c->camera.pos, pos, 12) == 0 && std::memcmp(c->camera.orient, orient_xyzw, 16) == 0 &&
	    c->camera.half_width == half_width && c->camera.half_height == half_height && c->camera.z == z && c->camera.exposure == exposure)
		return MIRT_OK;                                                                // unchanged (a host that re-sends it every frame): nothing to flush
	{ const int fr = flush_deferred(c); if (fr) return fr; }                        // deferred accumulations belong to the camera they were issued under
	for (int k = 0; k < 3; k++) c->camera.pos[k] = pos[k];
	for (int k = 0; k < 4; k++) c->camera.orient[k] = orient_xyzw[k];
	c->camera.half_width = half_width; c->camera.half_height = half_height; c->camera.z = z; c->camera.exposure = exposure;
	c->have_camera = true;
	c->cand_valid = false;                                                             // every cone has moved
	update_lens_axes(c);
	return MIRT_OK;
}

// ---- thin lens ---------------------------------------------------------------------------------
int mirt_set_lens(mirt_ctx* c, float aperture_radius, float focus_depth) {
	if (!c) return MIRT_ERR_ARG;
	if (!std::isfinite(aperture_radius) || !std::isfinite(focus_depth)) return fail(c, MIRT_ERR_ARG, "lens: aperture_radius %g / focus_depth %g must be finite", static_cast<double>(aperture_radius), static_cast<double>(focus_depth));
	if (aperture_radius < 0.0f) return fail(c, MIRT_ERR_ARG, "lens: aperture_radius %g is negative", static_cast<double>(aperture_radius));
	if (aperture_radius > 0.0f && !(focus_depth > 0.0f)) return fail(c, MIRT_ERR_ARG, "lens: focus_depth %g must be above 0 with an open aperture", static_cast<double>(focus_depth));
	if (aperture_radius > 0.0f) { const int r = refuse_under_exact_order(c, X_LENS); if (r) return r; }
	if (aperture_radius == c->lens.aperture && focus_depth == c->lens.focus_depth) return MIRT_OK;
	{ const int fr = flush_deferred(c); if (fr) return fr; }                        // deferred accumulations render under the lens they were issued under
	c->lens.aperture = aperture_radius; c->lens.focus_depth = focus_depth;
	update_lens_axes(c);
	return MIRT_OK;
}
int mirt_get_lens(const mirt_ctx* c, float* aperture_radius, float* focus_depth) {
	if (!c || !aperture_radius || !focus_depth) return MIRT_ERR_ARG;
	*aperture_radius = c->lens.aperture; *focus_depth = c->lens.focus_depth;
	return MIRT_OK;
}
int mirt_pick_focus(mirt_ctx* c, uint32_t x, uint32_t y, float* distance, float* depth) {
	int r = check_ready(c); if (r) return r;
	if (!distance || !depth) return fail(c, MIRT_ERR_ARG, "distance / depth is NULL");
	if (x >= c->width || y >= c->height) return fail(c, MIRT_ERR_ARG, "pixel (%u, %u) outside the %u x %u image", x, y, c->width, c->height);
	// the un-jittered pinhole ray of the pixel (Application.cpp:288-295), evaluated here with the kernels' own function
	const f3 d = camera_ray_dir(c->camera, static_cast<int32_t>(x), static_cast<int32_t>(y), 0.5f, 0.5f);
	const float p[3] = { c->camera.pos[0], c->camera.pos[1], c->camera.pos[2] }, dir[3] = { d.x, d.y, d.z };
	HitRec hit{};
	if ((r = debug_trace(c, "pick_focus", 1, p, dir, nullptr, &hit))) return r;     // the context's own closest-hit traversal; touches none of its state
	const f3 fwd = camera_axis(c->camera.orient, f3{ 0.0f, 0.0f, -1.0f });
	const float cosine = dot3(d, fwd);
	*distance = hit.prim >= 0 ? hit.tfar : INFINITY;                                   // Application.cpp:298
	*depth = *distance * (cosine < 1.0f ? cosine : 1.0f);                              // (a cosine rounded above 1 would put the plane of focus behind the hit)
	return MIRT_OK;
}

int mirt_set_policy(mirt_ctx* c, const mirt_policy* p) {
	if (!c || !p) return MIRT_ERR_ARG;
	if (p->max_bounces < 1 || p->max_bounces > 1024) return fail(c, MIRT_ERR_ARG, "max_bounces %u out of range", p->max_bounces);
	if (p->buckets < 1 || p->buckets > MIRT_MAX_BUCKETS) return fail(c, MIRT_ERR_ARG, "buckets %u out of range 1..%u", p->buckets, MIRT_MAX_BUCKETS);
	if (p->brdf > 1) return fail(c, MIRT_ERR_ARG, "brdf %u is neither 0 (Lambertian) nor 1 (GGX)", p->brdf);
	{ const int fr = flush_and_wait(c); if (fr) return fr; }
	const bool realloc_acc = p->buckets != c->policy.buckets;
	// batch size / batches in flight are planned again only when something the plan depends on changes (a toggle like trace_primary_rays
	// leaves the ray-stream arena, tens of GB, where it is)
	const bool replan = p->max_batch != c->policy.max_batch || p->streams != c->policy.streams || p->buckets != c->policy.buckets || p->max_bounces != c->policy.max_bounces;
	// what decides the tree the lists were collected from, or whether lists are used at all
	if (p->use_bvh != c->policy.use_bvh || p->gpu_build != c->policy.gpu_build || p->reference_tree != c->policy.reference_tree || p->trace_primary_rays != c->policy.trace_primary_rays)
		c->cand_valid = false;
	if (p->brdf != c->policy.brdf) c->mat_merged_valid = false;                     // (the closure of the materials beyond the table's end)
	c->policy = *p;
	if (replan) c->planned_for = 0;
	if (realloc_acc) drop_history(c);                                               // its lengths count samples of another bucket layout
	if (realloc_acc && c->n_tiles) { int r = alloc_accumulator(c); if (r) return r; }
	return MIRT_OK;
}
int mirt_set_gloss_decay(mirt_ctx* c, const float* decay, uint32_t n) {
	if (!c) return MIRT_ERR_ARG;
	if (!decay) n = 0;
	if (n > 1024) return fail(c, MIRT_ERR_ARG, "gloss decay table of %u entries (at most 1024, the max_bounces limit)", n);
	for (uint32_t i = 0; i < n; i++)
		if (!(decay[i] >= 0.0f && decay[i] <= 1.0f)) return fail(c, MIRT_ERR_ARG, "gloss decay[%u] = %g is not in [0, 1]", i, static_cast<double>(decay[i]));
	{ const int fr = flush_deferred(c); if (fr) return fr; }                        // deferred accumulations render with the table they were issued under
	c->gloss_decay.assign(decay, decay + n);
	c->gloss_decay_dev_valid = false;
	return MIRT_OK;
}
int mirt_set_stream_order(mirt_ctx* c, uint32_t exact) {
	if (!c) return MIRT_ERR_ARG;
	if (exact > 1) return fail(c, MIRT_ERR_ARG, "stream order %u is neither 0 (any order, FMA form for every ray) nor 1 (the reference's slots and scalar tail)", exact);
	if (exact == c->stream_order) return MIRT_OK;
	if (exact) { const int r = refuse_exact_order(c); if (r) return r; }
	{ const int fr = flush_deferred(c); if (fr) return fr; }                        // deferred accumulations render in the mode they were issued under
	c->stream_order = exact;
	return MIRT_OK;
}
// ---- NEE light by resampled importance sampling -------------------------------------------------
int mirt_set_light_ris(mirt_ctx* c, uint32_t candidates) {
	BEGIN_SWITCH(c, &mirt_ctx::light_ris, candidates, MIRT_MAX_LIGHT_RIS, "light RIS: %u candidates (0 = off, at most %u)", X_LIGHT_RIS);
	c->light_ris = candidates;                                                      // the expectation is the same: no reset; the lists do not depend on it
	return MIRT_OK;
}
// ---- dielectric interface for transmissive materials ---------------------------------------------
int mirt_set_transmission(mirt_ctx* c, uint32_t on) {
	BEGIN_SWITCH(c, &mirt_ctx::transmission, on, 1u, "transmission %u is neither 0 (off: transmission and IOR_minus_one are read by no kernel) nor 1 (on)", X_TRANSMISSION,
	             [](mirt_ctx* c, uint32_t on) { return on && c->have_scene ? check_glass(c, c->glass_host) : MIRT_OK; });
	c->transmission = on;                                                           // another estimand: the caller resets; the camera-ray lists do not depend on it
	return MIRT_OK;
}
// ---- per-material closures ---------------------------------------------------------------------
int mirt_set_material_closures(mirt_ctx* c, const uint8_t* closure, uint32_t n) {
	if (!c) return MIRT_ERR_ARG;
	if (!closure) n = 0;
	if (n > MIRT_MAX_MATERIALS) return fail(c, MIRT_ERR_ARG, "material closures: %u entries (at most %u, MIRT_MAX_MATERIALS)", n, MIRT_MAX_MATERIALS);
	for (uint32_t m = 0; m < n; m++)
		if (closure[m] > 1) return fail(c, MIRT_ERR_ARG, "material closures: closure[%u] = %u is neither 0 (Lambertian) nor 1 (GGX)", m, closure[m]);
	if (n) { const int r = refuse_under_exact_order(c, X_CLOSURES); if (r) return r; }
	if (n == c->closures.size() && (n == 0 || std::memcmp(c->closures.data(), closure, n) == 0)) return MIRT_OK;
	{ const int fr = flush_deferred(c); if (fr) return fr; }                        // deferred accumulations render under the table they were issued under
	c->closures.assign(closure, closure + n);                                       // another estimand: the caller resets; the camera-ray lists do not depend on it
	c->mat_merged_valid = false;
	return MIRT_OK;
}
int mirt_get_material_closures(const mirt_ctx* c, uint8_t* closure_out, uint32_t capacity, uint32_t* n, uint32_t* mixed) {
	if (!c || !n || !mixed) return MIRT_ERR_ARG;
	const uint32_t have = static_cast<uint32_t>(c->closures.size());
	*n = have;
	*mixed = closure_plan(c).mixed ? 1u : 0u;
	if (have && (!closure_out || capacity < have)) return closure_out ? MIRT_ERR_ARG : MIRT_OK;    // closure_out = NULL: only the two counts are asked for
	if (have) std::memcpy(closure_out, c->closures.data(), have);
	return MIRT_OK;
}
// ---- the environment map as one more light of next event estimation ------------------------------
int mirt_set_sky_sampling(mirt_ctx* c, uint32_t on) {
	BEGIN_SWITCH(c, &mirt_ctx::sky_sampling, on, 1u, "sky sampling %u is neither 0 (off: the sky is met by extension rays only) nor 1 (on: it is one more light of next event estimation)", X_SKY_SAMPLING);
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, sync_all(c));                                                        // batches in flight read the table and the planes
	if (on && c->have_scene) {
		const SceneDev& s = c->scene;
		std::vector<float4> texels(static_cast<size_t>(s.hdri_w) * s.hdri_h);
		HIP_TRY(c, hipMemcpy(texels.data(), s.hdri, texels.size() * sizeof(float4), hipMemcpyDeviceToHost));
		int r = check_sky_texels(c, texels.data(), static_cast<uint32_t>(s.hdri_w), static_cast<uint32_t>(s.hdri_h), s.ambient);
		if (r || (r = build_sky_table(c))) { drop_sky_table(c); return r; }       // the switch stays off
	}
	if (!on) {
		drop_sky_table(c);
		for (PipeSlot& sl : c->slots) { sl.sky_w.release(); sl.stream_buf[0].w = sl.stream_buf[1].w = nullptr; }
	}
	c->sky_sampling = on;                                                           // the same expectation: no reset; the camera-ray lists do not depend on it
	return MIRT_OK;
}
// ---- the GGX closure's pdf in the MIS weights -----------------------------------------------------
int mirt_set_ggx_pdf(mirt_ctx* c, uint32_t on) {
	BEGIN_SWITCH(c, &mirt_ctx::ggx_pdf, on, 1u, "ggx pdf %u is neither 0 (off: Closure<GGX>::pdf is the reference's 0) nor 1 (on: the visible-normal density, in every MIS weight that reads it)", X_GGX_PDF);
	if (!on) {
		HIP_TRY(c, hipSetDevice(c->device));
		HIP_TRY(c, sync_all(c));                                                    // batches in flight write the planes
		for (PipeSlot& sl : c->slots) { sl.pdf_p.release(); sl.pdf_plane[0] = sl.pdf_plane[1] = nullptr; }
	}
	c->ggx_pdf = on;                                                                // formally another estimator: the caller resets; the camera-ray lists do not depend on it
	c->planned_for = 0;                                                             // the planes count in the automatic batch plan (streams_bytes)
	return MIRT_OK;
}
SWITCH_GETTER(ggx_pdf, ggx_pdf) SWITCH_GETTER(sky_sampling, sky_sampling) SWITCH_GETTER(transmission, transmission) SWITCH_GETTER(light_ris, light_ris)
SWITCH_GETTER(stream_order, stream_order)
int mirt_get_policy(const mirt_ctx* c, mirt_policy* p) {
	if (!c || !p) return MIRT_ERR_ARG;
	*p = c->policy;
	plan_batches(const_cast<mirt_ctx*>(c));        // the plan is a cache: made here if no launch has made it yet, so that the values below are the ones launches will use
	p->max_batch = batch_limit(c);                 // the values in effect where the caller left 0 = auto
	p->streams = wanted_slots(c);
	return MIRT_OK;
}

int mirt_resize(mirt_ctx* c, uint32_t width, uint32_t height) {
	if (!c) return MIRT_ERR_ARG;
	if (width > 65536 || height > 65536) return fail(c, MIRT_ERR_ARG, "size %ux%u too large", width, height);
	{ const int dr = drop_and_wait(c); if (dr) return dr; }                         // the accumulator is about to be zeroed (Renderer.hpp:61-62)
	c->width = width; c->height = height;
	c->cand_valid = false;                                                             // other pixels
	for (DeviceBuffer* b : { &c->dn_cv[0], &c->dn_cv[1], &c->dn_gd, &c->dn_mu }) b->release();   // mirt_render_atrous allocates them again at the new size
	drop_history(c);                                                                   // another image
	c->id_out.release();
	c->h_tiles = width / MIRT_TILE_ROOT; c->v_tiles = height / MIRT_TILE_ROOT;          // Renderer.hpp:59-60
	set_tile_map(c, TileMap::of_range(0u, c->h_tiles, width), c->h_tiles * c->v_tiles);
	HIP_TRY(c, c->framebuffer.ensure(std::max<size_t>(static_cast<size_t>(width) * height, 1) * sizeof(float4)));
	HIP_TRY(c, hipMemsetAsync(c->framebuffer.ptr, 0, c->framebuffer.bytes, c->stream));
	if (c->frame_host_bytes < c->framebuffer.bytes) {
		if (c->frame_host) (void)hipHostFree(c->frame_host);
		c->frame_host = nullptr; c->frame_host_bytes = 0;
		HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->frame_host), c->framebuffer.bytes, hipHostMallocDefault));
		c->frame_host_bytes = c->framebuffer.bytes;
	}
	return alloc_accumulator(c);                                                      // Renderer.hpp:61-62
}

int mirt_set_tile_range(mirt_ctx* c, uint32_t first_tile, uint32_t n_tiles) {
	if (!c) return MIRT_ERR_ARG;
	const uint64_t all = static_cast<uint64_t>(c->h_tiles) * c->v_tiles;
	if (static_cast<uint64_t>(first_tile) + n_tiles > all) return fail(c, MIRT_ERR_ARG, "tile range [%u,+%u) exceeds %llu tiles", first_tile, n_tiles, (unsigned long long)all);
	{ const int dr = drop_and_wait(c); if (dr) return dr; }                         // zeroes the accumulator
	set_tile_map(c, TileMap::of_range(first_tile, c->h_tiles, c->width), n_tiles);
	drop_history(c);
	c->cand_valid = false;                                                             // other local pixels
	return alloc_accumulator(c);
}

int mirt_set_tile_rows(mirt_ctx* c, uint32_t first_row, uint32_t row_stride) {
	if (!c) return MIRT_ERR_ARG;
	if (row_stride == 0) return fail(c, MIRT_ERR_ARG, "row_stride must be at least 1");
	{ const int dr = drop_and_wait(c); if (dr) return dr; }                         // zeroes the accumulator
	set_tile_map(c, TileMap::of_rows(first_row, row_stride, c->h_tiles, c->width), TileMap::tile_rows_owned(c->v_tiles, first_row, row_stride) * c->h_tiles);
	drop_history(c);
	c->cand_valid = false;                                                             // other local pixels
	return alloc_accumulator(c);
}

int mirt_reset(mirt_ctx* c) {
	if (!c) return MIRT_ERR_ARG;
	c->deferred = 0;                                                                   // what was not launched yet would be wiped anyway
	HIP_TRY(c, hipSetDevice(c->device));
	return alloc_accumulator(c);                                                      // Renderer.hpp:64-67
}

int mirt_accumulate_async(mirt_ctx* c, uint32_t n_calls) {
	int r = check_ready(c); if (r) return r;
	HIP_TRY(c, hipSetDevice(c->device));
	if ((r = ensure_streams(c))) return r;
	// Whole batches are launched now; a remainder waits for more calls (a frame loop that calls this once per frame still gets
	// full-size launches) and is launched by the next call that needs it: mirt_synchronize, a read, a state change.
	if (c->n_tiles == 0) { c->accumulations += n_calls; return MIRT_OK; }
	const uint32_t limit = batch_limit(c);
	uint64_t total = static_cast<uint64_t>(c->deferred) + n_calls;
	c->deferred = 0;
	while (total >= limit) {
		if ((r = launch_batch(c, limit))) return r;
		total -= limit;
	}
	c->deferred = static_cast<uint32_t>(total);
	return MIRT_OK;
}
int mirt_synchronize(mirt_ctx* c) {
	if (!c) return MIRT_ERR_ARG;
	return flush_and_wait(c);
}
int mirt_accumulate(mirt_ctx* c, uint32_t n_calls) {
	int r = mirt_accumulate_async(c, n_calls);
	if (r) return r;
	return mirt_synchronize(c);
}
int mirt_get_accumulations(const mirt_ctx* c, uint32_t* a) { if (!c || !a) return MIRT_ERR_ARG; *a = c->accumulations + c->deferred; return MIRT_OK; }

int mirt_accumulator_floats(const mirt_ctx* c, size_t* n) {
	if (!c || !n) return MIRT_ERR_ARG;
	*n = static_cast<size_t>(c->n_tiles) * c->policy.buckets * 3 * kTileSize;
	return MIRT_OK;
}
int mirt_read_accumulator(mirt_ctx* c, float* dst) {
	if (!c || !dst) return MIRT_ERR_ARG;
	size_t n = 0; mirt_accumulator_floats(c, &n);
	{ const int fr = flush_and_wait(c); if (fr) return fr; }
	if (n) HIP_TRY(c, hipMemcpy(dst, c->accumulator.ptr, n * sizeof(float), hipMemcpyDeviceToHost));
	return MIRT_OK;
}
int mirt_accumulator_device(mirt_ctx* c, void** ptr, size_t* bytes) {
	if (!c || !ptr || !bytes) return MIRT_ERR_ARG;
	size_t n = 0; mirt_accumulator_floats(c, &n);
	{ const int fr = flush_and_wait(c); if (fr) return fr; }                        // the caller reads the slab on a stream of its own (RCCL gather): everything enqueued here has landed
	*ptr = c->accumulator.ptr; *bytes = n * sizeof(float);
	return MIRT_OK;
}
int mirt_load_accumulator(mirt_ctx* c, const float* src, int src_is_device, uint32_t accumulations) {
	if (!c || !src) return MIRT_ERR_ARG;
	size_t n = 0; mirt_accumulator_floats(c, &n);
	{ const int dr = drop_and_wait(c); if (dr) return dr; }                         // overwritten below
	if (n && src != c->accumulator.ptr)                                                // src == the slab itself (filled in place by mirt_group_gather): only `accumulations` changes
		HIP_TRY(c, hipMemcpy(c->accumulator.ptr, src, n * sizeof(float), src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
	c->accumulations = accumulations;
	clear_freezes(c);                                                                  // every tile at `accumulations`; mirt_load_tile_counts applies per-tile counts
	return MIRT_OK;
}

// ---- first-hit AOVs ----------------------------------------------------------------------------
int mirt_set_aov(mirt_ctx* c, uint32_t on) {
	if (!c) return MIRT_ERR_ARG;
	if (on > 1) return fail(c, MIRT_ERR_ARG, "aov %u is neither 0 (off) nor 1 (sum depth, normal and albedo of every camera ray)", on);
	if (on == c->aov_on) return MIRT_OK;
	if (on) {
		{ const int r = refuse_under_exact_order(c, X_AOV); if (r) return r; }
		if (c->accumulations + c->deferred) return fail(c, MIRT_ERR_STATE, "AOVs can be turned on only before the first accumulation (%u issued): the sums would cover fewer samples than the frame; mirt_reset first", c->accumulations + c->deferred);
		HIP_TRY(c, hipSetDevice(c->device));
		HIP_TRY(c, sync_all(c));
		c->aov_on = 1;
		int r = alloc_aov(c);
		if (r == MIRT_OK && hipStreamSynchronize(c->stream) != hipSuccess) r = fail(c, MIRT_ERR_HIP, "zeroing the AOV slab failed");
		if (r) { c->aov_on = 0; c->aov.release(); }
		return r;
	}
	{ const int fr = flush_and_wait(c); if (fr) return fr; }                        // deferred accumulations were issued with AOVs on
	c->aov_on = 0;
	c->aov.release();
	return MIRT_OK;
}
SWITCH_GETTER(aov, aov_on)
int mirt_aov_floats(const mirt_ctx* c, size_t* n) { if (!c || !n) return MIRT_ERR_ARG; *n = aov_floats(c); return MIRT_OK; }
int mirt_read_aov(mirt_ctx* c, float* dst) {
	if (!c || !dst) return MIRT_ERR_ARG;
	if (!c->aov_on) return fail(c, MIRT_ERR_STATE, "AOVs are off (mirt_set_aov)");
	{ const int fr = flush_and_wait(c); if (fr) return fr; }
	if (aov_floats(c)) HIP_TRY(c, hipMemcpy(dst, c->aov.ptr, aov_floats(c) * sizeof(float), hipMemcpyDeviceToHost));
	return MIRT_OK;
}
int mirt_aov_device(mirt_ctx* c, void** ptr, size_t* bytes) {
	if (!c || !ptr || !bytes) return MIRT_ERR_ARG;
	if (!c->aov_on) return fail(c, MIRT_ERR_STATE, "AOVs are off (mirt_set_aov)");
	{ const int fr = flush_and_wait(c); if (fr) return fr; }
	*ptr = c->aov.ptr; *bytes = aov_floats(c) * sizeof(float);
	return MIRT_OK;
}
int mirt_load_aov(mirt_ctx* c, const float* src, int src_is_device) {
	if (!c || !src) return MIRT_ERR_ARG;
	if (!c->aov_on) return fail(c, MIRT_ERR_STATE, "AOVs are off (mirt_set_aov)");
	{ const int fr = flush_and_wait(c); if (fr) return fr; }                        // (their sums are overwritten below; their accumulator adds are not)
	if (aov_floats(c) && src != c->aov.ptr)                                         // src == the slab itself (filled in place by mirt_group_gather)
		HIP_TRY(c, hipMemcpy(c->aov.ptr, src, aov_floats(c) * sizeof(float), src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
	return MIRT_OK;
}
int mirt_render_aov(mirt_ctx* c, int which, float* out) {
	if (!c) return MIRT_ERR_ARG;
	int r = MIRT_OK;
	if (!c->aov_on) return fail(c, MIRT_ERR_STATE, "AOVs are off (mirt_set_aov)");
	if (which != MIRT_AOV_DEPTH && which != MIRT_AOV_NORMAL && which != MIRT_AOV_ALBEDO) return fail(c, MIRT_ERR_ARG, "no AOV %d (MIRT_AOV_DEPTH, _NORMAL, _ALBEDO)", which);
	if (!out) return fail(c, MIRT_ERR_ARG, "out is NULL");
	if (c->accumulations + c->deferred == 0) return MIRT_NOT_READY;
	{ const int fr = flush_and_wait(c); if (fr) return fr; }
	const uint32_t n_pix = c->n_tiles * kTileSize, ch = which == MIRT_AOV_DEPTH ? 1u : 3u;
	if (n_pix == 0) return MIRT_OK;
	const size_t image_floats = static_cast<size_t>(c->width) * c->height * ch;
	ScopedBuffer image;
	HIP_TRY(c, image.ensure(image_floats * sizeof(float)));
	const uint32_t* counts = nullptr;
	if ((r = upload_tile_counts(c, &counts))) return r;
	{ Bracket t(c, MIRT_K_RESOLVE);
	  hipLaunchKernelGGL(k_resolve_aov, dim3(grid_for(c, n_pix)), dim3(kBlock), 0, c->stream, c->aov.as<float>(), image.as<float>(), n_pix, tile_map(c), which,
	                     static_cast<float>(c->accumulations), counts); }
	HIP_TRY(c, hipGetLastError());
	std::vector<float> host(image_floats);                                           // pixels of other contexts' tiles are never written: copy ours only
	HIP_TRY(c, hipMemcpyAsync(host.data(), image.ptr, image_floats * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	copy_owned_tiles(tile_map(c), c->n_tiles, ch, host.data(), out);
	return MIRT_OK;
}

int mirt_render(mirt_ctx* c, float* rgba_host) {
	int r = check_ready(c); if (r) return r;
	if (!rgba_host) return fail(c, MIRT_ERR_ARG, "rgba_host is NULL");
	const uint32_t k = c->policy.buckets;
	const uint32_t issued = c->accumulations + c->deferred;
	if (issued == 0 || (issued % k) != 0) return MIRT_NOT_READY;                                    // Renderer.hpp:437 (nothing is launched for this)
	{ const int fr = flush_and_wait(c); if (fr) return fr; }
	const float scale = c->camera.exposure / static_cast<float>(c->accumulations / k);              // Renderer.hpp:439
	const uint32_t n_pix = c->n_tiles * kTileSize;
	const uint32_t* counts = nullptr;
	if ((r = upload_tile_counts(c, &counts))) return r;
	{ Bracket t(c, MIRT_K_RESOLVE);
	  hipLaunchKernelGGL(k_resolve, dim3(grid_for(c, n_pix)), dim3(kBlock), 0, c->stream, c->accumulator.as<float>(), c->framebuffer.as<float4>(),
	                     n_pix, tile_map(c), k, scale, counts, c->camera.exposure); }
	HIP_TRY(c, hipGetLastError());
	const size_t frame_floats = static_cast<size_t>(c->width) * c->height * 4;
	const bool whole = c->n_tiles == c->h_tiles * c->v_tiles && c->width == c->h_tiles * MIRT_TILE_ROOT && c->height == c->v_tiles * MIRT_TILE_ROOT;
	HIP_TRY(c, hipMemcpyAsync(c->frame_host, c->framebuffer.ptr, frame_floats * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	if (whole) std::memcpy(rgba_host, c->frame_host, frame_floats * sizeof(float));   // every pixel is this context's
	else copy_owned_tiles(tile_map(c), c->n_tiles, 4u, c->frame_host, rgba_host);                 // only this context's tiles
	return MIRT_OK;
}

// ---- variance-guided a-trous denoised resolve (denoise.hpp; the definition is in mirt.h) ------------------------------------------
int mirt_atrous_defaults(mirt_denoise_params* out) {
	if (!out) return MIRT_ERR_ARG;
	*out = mirt_denoise_params{ 5u, 5u, 1u, 4.0f, 0.05f, 1e-4f, 1.0f / 256.0f };
	return MIRT_OK;
}

} // extern "C"
namespace {
const mirt_ctx* motion_geometry_of(const mirt_ctx* c) { return c->motion_geometry ? c->motion_geometry : c; }
// The geometry context of a call that needs the id map: a scene, on this device, showing this camera (the group keeps all three in step).
int check_motion_geometry(mirt_ctx* c, const mirt_ctx* gs) {
	if (gs == c) return MIRT_OK;
	if (!gs->have_scene || !gs->have_camera) return fail(c, MIRT_ERR_STATE, "history motion: the geometry context has no scene or no camera");
	if (gs->device != c->device) return fail(c, MIRT_ERR_STATE, "history motion: the geometry context is on device %d, this one on device %d", gs->device, c->device);
	if (std::memcmp(&gs->camera, &c->camera, sizeof(CameraParams)) != 0) return fail(c, MIRT_ERR_STATE, "history motion: the geometry context shows another camera");
	return MIRT_OK;
}
bool unit_orient(const CameraParams& cam) {      // the condition the camera-ray candidate lists put on view.orient (launch_batch)
	const float qn = cam.orient[0] * cam.orient[0] + cam.orient[1] * cam.orient[1] + cam.orient[2] * cam.orient[2] + cam.orient[3] * cam.orient[3];
	return std::fabs(qn - 1.0f) < 1e-4f;
}
// mirt_render_atrous (tp == NULL: the launches and the words it has always had) and mirt_render_temporal (tp given: k_reproject between the
// prepare and the first pass, and the history).
int filtered_resolve(mirt_ctx* c, const mirt_denoise_params* p, const mirt_temporal_params* tp, float* rgba_host, float* history_len, mirt_temporal_stats* stats) {
	int r = check_ready(c); if (r) return r;
	if (!p) return fail(c, MIRT_ERR_ARG, "params is NULL");
	if (tp) {
		if (!mirt_noise_host::finite_nonneg(tp->max_ratio) || !mirt_noise_host::finite_nonneg(tp->depth_tol))
			return fail(c, MIRT_ERR_ARG, "temporal: max_ratio %g and depth_tol %g must be finite and >= 0", static_cast<double>(tp->max_ratio), static_cast<double>(tp->depth_tol));
		if (!(tp->normal_min >= -1.0f && tp->normal_min <= 1.0f)) return fail(c, MIRT_ERR_ARG, "temporal: normal_min %g must lie in [-1, 1]", static_cast<double>(tp->normal_min));
		if (tp->update > 1u) return fail(c, MIRT_ERR_ARG, "temporal: update %u is neither 0 nor 1", tp->update);
	}
	if (!rgba_host) return fail(c, MIRT_ERR_ARG, "rgba_host is NULL");
	if (p->iterations > 8u || p->normal_squarings > 8u || p->demodulate > 1u)
		return fail(c, MIRT_ERR_ARG, "denoise: iterations %u and normal_squarings %u must be 0..8, demodulate %u 0 or 1", p->iterations, p->normal_squarings, p->demodulate);
	if (!mirt_noise_host::finite_nonneg(p->sigma_lum) || !mirt_noise_host::finite_nonneg(p->sigma_depth))
		return fail(c, MIRT_ERR_ARG, "denoise: sigma_lum %g and sigma_depth %g must be finite and >= 0", static_cast<double>(p->sigma_lum), static_cast<double>(p->sigma_depth));
	if (!std::isfinite(p->lum_floor) || !(p->lum_floor > 0.0f)) return fail(c, MIRT_ERR_ARG, "denoise: lum_floor %g must be finite and > 0", static_cast<double>(p->lum_floor));
	if (!std::isfinite(p->albedo_floor)) return fail(c, MIRT_ERR_ARG, "denoise: albedo_floor is not finite");
	const uint32_t k = c->policy.buckets;
	if (!c->aov_on) return fail(c, MIRT_ERR_STATE, "denoise: AOVs are off (mirt_set_aov)");
	if (k < 2u) return fail(c, MIRT_ERR_STATE, "denoise: the variance guide needs buckets >= 2, the policy has %u", k);
	if (c->first_tile != 0u || c->stride_tiles != 0u || c->n_tiles != c->h_tiles * c->v_tiles)
		return fail(c, MIRT_ERR_STATE, "denoise: the context owns %u of the image's %u tiles; the stencil reads across tile borders, so it needs all of them", c->n_tiles, c->h_tiles * c->v_tiles);
	const uint32_t issued = c->accumulations + c->deferred;
	if (issued == 0 || (issued % k) != 0) return MIRT_NOT_READY;                                    // as mirt_render
	{ const int fr = flush_and_wait(c); if (fr) return fr; }
	if (c->n_tiles == 0) return MIRT_OK;
	// mirt_set_sphere_motion: where the id map and the sphere tables come from (this context, or the one mirt_set_motion_geometry named)
	const mirt_ctx* gs = motion_geometry_of(c);
	if (tp && c->history_motion && (r = check_motion_geometry(c, gs))) return r;
	const float scale = c->camera.exposure / static_cast<float>(c->accumulations / k);              // Renderer.hpp:439, as mirt_render
	const uint32_t n_pix = c->n_tiles * kTileSize;
	const size_t image_bytes = static_cast<size_t>(c->width) * c->height * sizeof(float4);
	for (DeviceBuffer* b : { &c->dn_cv[0], &c->dn_cv[1], &c->dn_gd, &c->dn_mu }) HIP_TRY(c, b->ensure(image_bytes));
	const uint32_t* counts = nullptr;
	if ((r = upload_tile_counts(c, &counts))) return r;
	const TileMap m = tile_map(c);
	{ Bracket t(c, MIRT_K_RESOLVE);
	  hipLaunchKernelGGL(k_denoise_prepare, dim3(c->n_tiles), dim3(kTileSize), 0, c->stream, c->accumulator.as<float>(), c->aov.as<float>(), c->dn_cv[0].as<float4>(),
	                     c->dn_gd.as<float4>(), c->dn_mu.as<float4>(), m, k, scale, static_cast<float>(c->accumulations), counts, c->camera.exposure, p->demodulate, p->albedo_floor); }
	HIP_TRY(c, hipGetLastError());
	// The passes go from `src` to `dst`; the two swap, and the buffer that becomes free after the first pass is `spare`.  Plain: cv[0] -> cv[1] -> cv[0].
	// Temporal: k_reproject writes the blend into cv[1], which the passes only read when it is to become the history (update = 1: the old history's
	// (x, v) image is the spare then, free as soon as k_reproject has read it).
	float4 *src = c->dn_cv[0].as<float4>(), *dst = c->dn_cv[1].as<float4>(), *spare = c->dn_cv[0].as<float4>();
	if (tp) {
		const size_t len_bytes = static_cast<size_t>(c->width) * c->height * sizeof(float);
		HIP_TRY(c, c->th_len.ensure(len_bytes));
		HIP_TRY(c, c->th_stats.ensure(kTemporalStatSlots * kTemporalStatPitch * sizeof(unsigned long long)));
		if (tp->update) { HIP_TRY(c, c->th_x.ensure(image_bytes)); HIP_TRY(c, c->th_g.ensure(image_bytes)); HIP_TRY(c, c->th_n.ensure(len_bytes)); }
		HIP_TRY(c, hipMemsetAsync(c->th_stats.ptr, 0, kTemporalStatSlots * kTemporalStatPitch * sizeof(unsigned long long), c->stream));
		TemporalDev td{};
		td.cam = c->camera; td.prev = c->th_cam;
		td.max_ratio = tp->max_ratio; td.depth_tol = tp->depth_tol; td.normal_min = tp->normal_min;
		// the call takes the history when there is one, of this image and these demodulation settings, and both cameras rotate
		// (x carries the exposure it was resolved under: a history of another exposure word is in other units)
		td.take = (c->th_valid && tp->max_ratio > 0.0f && c->th_width == c->width && c->th_height == c->height && c->th_demodulate == p->demodulate &&
		           std::memcmp(&c->th_albedo_floor, &p->albedo_floor, sizeof(float)) == 0 && std::memcmp(&c->th_cam.exposure, &c->camera.exposure, sizeof(float)) == 0 &&
		           unit_orient(c->camera) && unit_orient(c->th_cam)) ? 1u : 0u;
		td.identity = std::memcmp(&c->camera, &c->th_cam, sizeof(CameraParams)) == 0 ? 1u : 0u;
		if (!td.take) td.prev = c->camera;
		if (c->history_motion) {
			// the id map of this camera first, then the MOTION instantiation: the pixel's sphere, the table now and the table the history was taken under
			const size_t id_bytes = static_cast<size_t>(c->width) * c->height * sizeof(int32_t);
			HIP_TRY(c, c->th_id_cur.ensure(id_bytes));
			if (tp->update) { HIP_TRY(c, c->th_id.ensure(id_bytes)); HIP_TRY(c, c->th_snap.ensure(std::max<size_t>(gs->scene.n_spheres, 1) * sizeof(float4))); }
			if ((r = launch_id_map(c, gs, c->th_id_cur.as<int32_t>(), nullptr))) return r;
			const MotionDev<true> mo{ c->th_id_cur.as<int32_t>(), c->th_id.as<int32_t>(), gs->scene.spheres, c->th_snap.as<float4>() };
			Bracket t(c, MIRT_K_RESOLVE);
			hipLaunchKernelGGL(k_reproject<true>, dim3(c->h_tiles, c->v_tiles), dim3(kAtrousBlock * kAtrousBlock), 0, c->stream, c->dn_cv[0].as<float4>(), c->dn_gd.as<float4>(),
			                   c->th_x.as<float4>(), c->th_g.as<float4>(), c->th_n.as<float>(), c->dn_cv[1].as<float4>(), c->th_len.as<float>(), c->th_stats.as<unsigned long long>(),
			                   c->width, c->h_tiles * kAtrousBlock, c->v_tiles * kAtrousBlock, counts, c->accumulations, td, mo);
		} else {
			Bracket t(c, MIRT_K_RESOLVE);
			hipLaunchKernelGGL(k_reproject<false>, dim3(c->h_tiles, c->v_tiles), dim3(kAtrousBlock * kAtrousBlock), 0, c->stream, c->dn_cv[0].as<float4>(), c->dn_gd.as<float4>(),
			                   c->th_x.as<float4>(), c->th_g.as<float4>(), c->th_n.as<float>(), c->dn_cv[1].as<float4>(), c->th_len.as<float>(), c->th_stats.as<unsigned long long>(),
			                   c->width, c->h_tiles * kAtrousBlock, c->v_tiles * kAtrousBlock, counts, c->accumulations, td, MotionDev<false>{});
		}
		HIP_TRY(c, hipGetLastError());
		// the snapshot follows the table once the kernel has read the old one (stream order); skipped while no mirt_update_spheres came since the last copy
		if (c->history_motion && tp->update && gs->scene.n_spheres && (!c->th_snap_valid || c->th_snap_gen != gs->spheres_gen))
			HIP_TRY(c, hipMemcpyAsync(c->th_snap.ptr, gs->scene.spheres, static_cast<size_t>(gs->scene.n_spheres) * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
		src = c->dn_cv[1].as<float4>(); dst = c->dn_cv[0].as<float4>();
		spare = tp->update ? c->th_x.as<float4>() : c->dn_cv[1].as<float4>();
	}
	// From the second pass on, update = 1 writes into the old history's (x, v) image: a HIP error between here and the renaming below would
	// leave a history that claims to be valid over a scratch image, so such a return drops it (mirt.h, step 4).
	struct DropOnError { mirt_ctx* c; bool armed; ~DropOnError() { if (armed) c->th_valid = false; } } guard{ c, tp && tp->update && p->iterations >= 2u };
	const DenoiseDev dev{ p->sigma_lum, p->sigma_depth, p->lum_floor, p->normal_squarings };
	for (uint32_t i = 0; i < p->iterations; i++) {
		const uint32_t step = 1u << i;
		const bool staged = step <= c->tune_denoise_staged;
		Bracket t(c, MIRT_K_RESOLVE);
		hipLaunchKernelGGL(staged ? k_atrous<true> : k_atrous<false>, dim3(c->h_tiles, c->v_tiles), dim3(kAtrousBlock * kAtrousBlock), 0, c->stream,
		                   src, c->dn_gd.as<float4>(), dst, c->width, c->h_tiles * kAtrousBlock, c->v_tiles * kAtrousBlock, step, dev);
		float4* const next = i == 0u ? spare : src;
		src = dst; dst = next;
	}
	HIP_TRY(c, hipGetLastError());
	{ Bracket t(c, MIRT_K_RESOLVE);
	  hipLaunchKernelGGL(k_denoise_finish, dim3(grid_for(c, n_pix)), dim3(kBlock), 0, c->stream, src, c->dn_mu.as<float4>(), c->framebuffer.as<float4>(), n_pix, m); }
	HIP_TRY(c, hipGetLastError());
	// the frame leaves as mirt_render's does (the framebuffer is scratch: every resolve writes all of the context's tiles before it is read)
	const size_t frame_floats = static_cast<size_t>(c->width) * c->height * 4;
	const bool whole = c->width == c->h_tiles * MIRT_TILE_ROOT && c->height == c->v_tiles * MIRT_TILE_ROOT;
	HIP_TRY(c, hipMemcpyAsync(c->frame_host, c->framebuffer.ptr, frame_floats * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	std::vector<float> len_host;
	unsigned long long class_counts[kTemporalClasses] = {};
	std::vector<unsigned long long> count_slots(tp ? kTemporalStatSlots * kTemporalStatPitch : 0u);
	if (tp) {
		if (history_len) { len_host.resize(static_cast<size_t>(c->width) * c->height); HIP_TRY(c, hipMemcpyAsync(len_host.data(), c->th_len.ptr, len_host.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream)); }
		HIP_TRY(c, hipMemcpyAsync(count_slots.data(), c->th_stats.ptr, count_slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
	}
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	if (whole) std::memcpy(rgba_host, c->frame_host, frame_floats * sizeof(float));
	else copy_owned_tiles(m, c->n_tiles, 4u, c->frame_host, rgba_host);
	if (tp) {
		if (history_len) copy_owned_tiles(m, c->n_tiles, 1u, len_host.data(), history_len);
		for (uint32_t s = 0; s < kTemporalStatSlots; s++) for (uint32_t k = 0; k < kTemporalClasses; k++) class_counts[k] += count_slots[s * kTemporalStatPitch + k];
		if (stats) *stats = mirt_temporal_stats{ class_counts[kTemporalReprojected], class_counts[kTemporalNoHistory], class_counts[kTemporalOutside], class_counts[kTemporalRejected], class_counts[kTemporalUnusable] };
		if (tp->update) {                                                             // step 4: the blend, this call's guides and the lengths ARE the history now; the old ones are scratch
			std::swap(c->th_x, c->dn_cv[1]); std::swap(c->th_g, c->dn_gd); std::swap(c->th_n, c->th_len);
			c->th_cam = c->camera; c->th_demodulate = p->demodulate; c->th_albedo_floor = p->albedo_floor; c->th_width = c->width; c->th_height = c->height;
			if (c->history_motion) { std::swap(c->th_id, c->th_id_cur); c->th_snap_valid = true; c->th_snap_gen = gs->spheres_gen; }   // this call's id map IS the history's id plane now
			c->th_valid = true;
		}
	}
	guard.armed = false;
	return MIRT_OK;
}
} // namespace
extern "C" {

int mirt_render_atrous(mirt_ctx* c, const mirt_denoise_params* p, float* rgba_host) { return filtered_resolve(c, p, nullptr, rgba_host, nullptr, nullptr); }

// ---- temporal history for the denoised resolve (temporal.hpp; the definition is in mirt.h) -----------------------------------------
int mirt_temporal_defaults(mirt_temporal_params* out) {
	if (!out) return MIRT_ERR_ARG;
	*out = mirt_temporal_params{ 7.0f, 0.02f, 0.9f, 1u };
	return MIRT_OK;
}
int mirt_render_temporal(mirt_ctx* c, const mirt_denoise_params* p, const mirt_temporal_params* tp, float* rgba_host, float* history_len, mirt_temporal_stats* stats) {
	if (c && !tp) return fail(c, MIRT_ERR_ARG, "temporal params is NULL");
	return filtered_resolve(c, p, tp, rgba_host, history_len, stats);
}
int mirt_drop_history(mirt_ctx* c) {
	if (!c) return MIRT_ERR_ARG;
	HIP_TRY(c, hipSetDevice(c->device));
	drop_history(c);
	return MIRT_OK;
}
int mirt_history_info(const mirt_ctx* c, uint32_t* valid, uint64_t* bytes) {
	if (!c || !valid || !bytes) return MIRT_ERR_ARG;
	*valid = c->th_valid ? 1u : 0u;
	*bytes = static_cast<uint64_t>(c->th_x.bytes) + c->th_g.bytes + c->th_n.bytes + c->th_id.bytes + c->th_snap.bytes;   // the last two: mirt_set_sphere_motion(1) only
	return MIRT_OK;
}

// ---- first-hit id map, and the history kept across sphere moves (id_map.hpp, temporal.hpp; the definitions are in mirt.h) -------------
int mirt_id_map(mirt_ctx* c, int32_t* prim_out, float* distance_out) {
	int r = check_ready(c); if (r) return r;
	const mirt_ctx* gs = motion_geometry_of(c);
	if ((r = check_motion_geometry(c, gs))) return r;
	const size_t n = static_cast<size_t>(c->width) * c->height;
	if (n == 0 || (!prim_out && !distance_out)) return MIRT_OK;
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, c->id_out.ensure(n * (sizeof(int32_t) + sizeof(float))));
	int32_t* prim_dev = c->id_out.as<int32_t>();
	float* dist_dev = reinterpret_cast<float*>(prim_dev + n);
	if ((r = launch_id_map(c, gs, prim_out ? prim_dev : nullptr, distance_out ? dist_dev : nullptr))) return r;   // reads the scene and the camera, writes two planes of its own
	if (prim_out) HIP_TRY(c, hipMemcpyAsync(prim_out, prim_dev, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
	if (distance_out) HIP_TRY(c, hipMemcpyAsync(distance_out, dist_dev, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	return MIRT_OK;
}
int mirt_set_sphere_motion(mirt_ctx* c, uint32_t on) {
	if (!c) return MIRT_ERR_ARG;
	if (on > 1u) return fail(c, MIRT_ERR_ARG, "history motion %u is neither 0 nor 1", on);
	if (on == c->history_motion) return MIRT_OK;
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	drop_history(c);                                                                   // a history without an id plane cannot be taken with one, and the reverse
	c->history_motion = on;
	return MIRT_OK;
}
int mirt_get_sphere_motion(const mirt_ctx* c, uint32_t* on) { if (!c || !on) return MIRT_ERR_ARG; *on = c->history_motion; return MIRT_OK; }
int mirt_set_motion_geometry(mirt_ctx* c, mirt_ctx* geometry) {
	if (!c) return MIRT_ERR_ARG;
	geometry = geometry == c ? nullptr : geometry;
	if (geometry == c->motion_geometry) return MIRT_OK;
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	drop_history(c);                                                                   // ids of another scene
	c->motion_geometry = geometry;
	return MIRT_OK;
}

// ---- per-pixel noise estimate ------------------------------------------------------------------
} // extern "C"
namespace {
// mirt_noise, and mirt_tile_above when above_out is given: then `target` is what a usable pixel's e is compared with.
int noise_pass(mirt_ctx* c, float floor, float* map_out, float* tile_out, uint32_t* hist_out, mirt_noise_stats* stats, float target, uint32_t* above_out) {
	int r = check_ready(c); if (r) return r;
	const uint32_t k = c->policy.buckets;
	char why[256];
	if ((r = mirt_noise_host::check_noise_args(floor, k, why, sizeof why))) return fail(c, r, "%s", why);
	if (above_out && !mirt_noise_host::finite_nonneg(target)) return fail(c, MIRT_ERR_ARG, "target %g is not a finite value >= 0", static_cast<double>(target));
	const uint32_t issued = c->accumulations + c->deferred;
	if (issued == 0 || (issued % k) != 0) return MIRT_NOT_READY;                                    // as mirt_render
	{ const int fr = flush_and_wait(c); if (fr) return fr; }
	std::vector<float> rec(static_cast<size_t>(c->n_tiles) * 4);
	std::vector<uint32_t> hist(MIRT_NOISE_BINS, 0u);
	if (c->n_tiles) {
		static_assert(kNoiseBins == MIRT_NOISE_BINS, "k_noise bins by the rule of mirt.h");
		static_assert(MIRT_MAX_BUCKETS <= kNoiseMaxBuckets, "k_noise keeps one bucket luminance per register: every bucket mirt_set_policy accepts must fit");
		const float scale = c->camera.exposure / static_cast<float>(c->accumulations / k);          // Renderer.hpp:439, as mirt_render
		const TileMap m = tile_map(c);
		const size_t image_floats = static_cast<size_t>(c->width) * c->height;
		ScopedBuffer image;
		if (map_out) HIP_TRY(c, image.ensure(image_floats * sizeof(float)));
		HIP_TRY(c, c->noise_rec.ensure(rec.size() * sizeof(float)));
		HIP_TRY(c, c->noise_hist.ensure(MIRT_NOISE_BINS * sizeof(uint32_t)));
		if (above_out) HIP_TRY(c, c->noise_above.ensure(static_cast<size_t>(c->n_tiles) * sizeof(uint32_t)));
		const uint32_t* counts = nullptr;
		if ((r = upload_tile_counts(c, &counts))) return r;
		HIP_TRY(c, hipMemsetAsync(c->noise_hist.ptr, 0, MIRT_NOISE_BINS * sizeof(uint32_t), c->stream));
		{ Bracket t(c, MIRT_K_RESOLVE);
		  hipLaunchKernelGGL(k_noise, dim3(c->n_tiles), dim3(kTileSize), 0, c->stream, c->accumulator.as<float>(), map_out ? image.as<float>() : nullptr, c->noise_rec.as<float4>(),
		                     c->noise_hist.as<uint32_t>(), m, k, scale, floor, counts, c->camera.exposure, above_out ? c->noise_above.as<uint32_t>() : nullptr, target); }
		HIP_TRY(c, hipGetLastError());
		std::vector<float> host(map_out ? image_floats : 0);                             // pixels of other contexts' tiles are never written: copy ours only
		if (map_out) {                                                                   // only the 16-row bands that hold a tile of ours come back (one n-th of the image for a group member)
			uint32_t band = UINT32_MAX;
			for (uint32_t local = 0; local < c->n_tiles; local++) {                       // LaunchIndices ascend with the local index: each band is met once
				const uint32_t b = m.global_tile(local) / m.h_tiles;
				if (b == band) continue;
				band = b;
				const size_t off = static_cast<size_t>(b) * MIRT_TILE_ROOT * c->width;
				HIP_TRY(c, hipMemcpyAsync(host.data() + off, image.as<float>() + off, static_cast<size_t>(MIRT_TILE_ROOT) * c->width * sizeof(float), hipMemcpyDeviceToHost, c->stream));
			}
		}
		HIP_TRY(c, hipMemcpyAsync(rec.data(), c->noise_rec.ptr, rec.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(c, hipMemcpyAsync(hist.data(), c->noise_hist.ptr, MIRT_NOISE_BINS * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		if (above_out) HIP_TRY(c, hipMemcpyAsync(above_out, c->noise_above.ptr, static_cast<size_t>(c->n_tiles) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream));
		if (map_out) copy_owned_tiles(m, c->n_tiles, 1u, host.data(), map_out);
	}
	if (tile_out && !rec.empty()) std::memcpy(tile_out, rec.data(), rec.size() * sizeof(float));
	if (hist_out) std::memcpy(hist_out, hist.data(), MIRT_NOISE_BINS * sizeof(uint32_t));
	if (stats) mirt_noise_host::stats_from_tiles(rec.data(), c->n_tiles, stats);
	return MIRT_OK;
}
} // namespace
extern "C" {

int mirt_noise(mirt_ctx* c, float floor, float* map_out, float* tile_out, uint32_t* hist_out, mirt_noise_stats* stats) {
	return noise_pass(c, floor, map_out, tile_out, hist_out, stats, 0.0f, nullptr);
}

// ---- per-tile adaptive sampling ---------------------------------------------------------------------
int mirt_tile_above(mirt_ctx* c, float floor, float target, uint32_t* above_out, size_t capacity) {
	if (!c) return MIRT_ERR_ARG;
	if (!above_out) return fail(c, MIRT_ERR_ARG, "above_out is NULL");
	if (capacity < c->n_tiles) return fail(c, MIRT_ERR_ARG, "tile_above: room for %zu counts, %u local tiles", capacity, c->n_tiles);
	return noise_pass(c, floor, nullptr, nullptr, nullptr, nullptr, target, above_out);
}

int mirt_freeze_tiles(mirt_ctx* c, const uint8_t* freeze, size_t n_local_tiles) {
	int r = check_ready(c); if (r) return r;
	if (!freeze && n_local_tiles) return fail(c, MIRT_ERR_ARG, "freeze is NULL");
	if (n_local_tiles != c->n_tiles) return fail(c, MIRT_ERR_ARG, "freeze_tiles: a mask of %zu tiles, the context owns %u", n_local_tiles, c->n_tiles);
	if ((r = refuse_under_exact_order(c, X_FROZEN))) return r;
	const uint32_t issued = c->accumulations + c->deferred, k = c->policy.buckets;
	if (issued == 0) return fail(c, MIRT_ERR_STATE, "nothing accumulated yet: a frozen tile would hold no sample");
	if (issued % k != 0) return fail(c, MIRT_ERR_STATE, "%u accumulations so far: not a multiple of buckets (%u); a frozen tile must stay resolvable", issued, k);
	{ const int fr = flush_and_wait(c); if (fr) return fr; }                        // deferred accumulations were issued under the old mask
	bool changed = false;
	for (uint32_t t = 0; t < c->n_tiles; t++) {
		if (!freeze[t] || (c->n_frozen && c->frozen[t])) continue;
		if (c->frozen.empty()) { c->frozen.assign(c->n_tiles, 0); c->frozen_at.assign(c->n_tiles, 0u); }
		c->frozen[t] = 1; c->frozen_at[t] = c->accumulations; c->n_frozen++;
		changed = true;
	}
	return changed ? upload_freezes(c) : MIRT_OK;
}

int mirt_frozen_tiles(mirt_ctx* c, uint8_t* mask_out, size_t capacity) {
	if (!c) return MIRT_ERR_ARG;
	if (!mask_out && c->n_tiles) return fail(c, MIRT_ERR_ARG, "mask_out is NULL");
	if (capacity < c->n_tiles) return fail(c, MIRT_ERR_ARG, "frozen_tiles: room for %zu tiles, %u local tiles", capacity, c->n_tiles);
	for (uint32_t t = 0; t < c->n_tiles; t++) mask_out[t] = (c->n_frozen && c->frozen[t]) ? 1 : 0;
	return MIRT_OK;
}

int mirt_tile_counts(mirt_ctx* c, uint32_t* counts_out, size_t capacity) {
	if (!c) return MIRT_ERR_ARG;
	if (!counts_out) return fail(c, MIRT_ERR_ARG, "counts_out is NULL");
	if (capacity < c->n_tiles) return fail(c, MIRT_ERR_ARG, "tile_counts: room for %zu counts, %u local tiles", capacity, c->n_tiles);
	for (uint32_t t = 0; t < c->n_tiles; t++) counts_out[t] = (c->n_frozen && c->frozen[t]) ? c->frozen_at[t] : c->accumulations + c->deferred;
	return MIRT_OK;
}

int mirt_load_tile_counts(mirt_ctx* c, const uint32_t* counts, size_t n_local_tiles) {
	if (!c) return MIRT_ERR_ARG;
	if (!counts && n_local_tiles) return fail(c, MIRT_ERR_ARG, "counts is NULL");
	if (n_local_tiles != c->n_tiles) return fail(c, MIRT_ERR_ARG, "load_tile_counts: %zu counts, the context owns %u tiles", n_local_tiles, c->n_tiles);
	{ const int fr = flush_and_wait(c); if (fr) return fr; }
	const uint32_t k = c->policy.buckets;
	bool any = false;
	for (uint32_t t = 0; t < c->n_tiles; t++) {
		if (counts[t] == 0 || counts[t] % k != 0 || counts[t] > c->accumulations)
			return fail(c, MIRT_ERR_ARG, "load_tile_counts: tile %u has count %u; every count is a positive multiple of buckets (%u) and at most accumulations (%u)", t, counts[t], k, c->accumulations);
		any = any || counts[t] < c->accumulations;
	}
	if (any) { const int r = refuse_under_exact_order(c, X_FROZEN); if (r) return r; }
	clear_freezes(c);
	if (!any) return MIRT_OK;
	c->frozen.assign(c->n_tiles, 0); c->frozen_at.assign(c->n_tiles, 0u);
	for (uint32_t t = 0; t < c->n_tiles; t++) if (counts[t] < c->accumulations) { c->frozen[t] = 1; c->frozen_at[t] = counts[t]; c->n_frozen++; }
	return upload_freezes(c);
}

int mirt_accumulate_adaptive(mirt_ctx* c, const mirt_stop_rule* rule, uint32_t min_accumulations, mirt_adaptive_report* report) {
	int r = check_ready(c); if (r) return r;
	const uint32_t k = c->policy.buckets;
	char why[256];
	if ((r = mirt_noise_host::check_stop_rule(rule, k, c->accumulations + c->deferred, why, sizeof why))) return fail(c, r, "%s", why);
	if ((r = refuse_under_exact_order(c, X_FROZEN))) return r;
	return mirt_noise_host::accumulate_adaptive(rule, k, min_accumulations, c->n_tiles,
		[&](uint32_t* a) { return mirt_get_accumulations(c, a); },
		[&](uint32_t n) { return mirt_accumulate(c, n); },
		[&](float floor, float target, float* rec, uint32_t* above, mirt_noise_stats* st) { return noise_pass(c, floor, nullptr, rec, nullptr, st, target, above); },
		[&](uint8_t* mask) { return mirt_frozen_tiles(c, mask, c->n_tiles); },
		[&](const uint8_t* mask) { return mirt_freeze_tiles(c, mask, c->n_tiles); },
		[&](uint32_t* counts) { return mirt_tile_counts(c, counts, c->n_tiles); },
		[&](int code, const char* text) { return fail(c, code, "%s", text); },
		report);
}

int mirt_accumulate_until(mirt_ctx* c, const mirt_stop_rule* rule, mirt_noise_stats* last, uint32_t* issued) {
	int r = check_ready(c); if (r) return r;
	const uint32_t k = c->policy.buckets;
	char why[256];
	if ((r = mirt_noise_host::check_stop_rule(rule, k, c->accumulations + c->deferred, why, sizeof why))) return fail(c, r, "%s", why);
	std::vector<uint32_t> hist(MIRT_NOISE_BINS);
	return mirt_noise_host::accumulate_until(rule, k,
		[&](uint32_t* a) { return mirt_get_accumulations(c, a); },
		[&](uint32_t n) { return mirt_accumulate(c, n); },
		[&](float floor, uint32_t* h, mirt_noise_stats* st) { return mirt_noise(c, floor, nullptr, nullptr, h, st); },
		[&](int code, const char* text) { return fail(c, code, "%s", text); },
		last, issued, hist.data());
}

int mirt_get_counters(mirt_ctx* c, mirt_counters* out) {
	if (!c || !out) return MIRT_ERR_ARG;
	{ const int fr = flush_and_wait(c); if (fr) return fr; }
	DevCounters d;
	HIP_TRY(c, hipMemcpy(&d, c->counters.ptr, sizeof d, hipMemcpyDeviceToHost));
	out->rays = d.rays; out->shadow_rays = d.shadow_rays; out->nodes = d.nodes; out->spheres = d.spheres;
	out->shadow_nodes = d.shadow_nodes; out->shadow_spheres = d.shadow_spheres; out->terminated = d.terminated; out->dropped = d.dropped;
	return MIRT_OK;
}
int mirt_get_kernel_times(mirt_ctx* c, mirt_kernel_times* out, int reset) {
	if (!c || !out) return MIRT_ERR_ARG;
	HIP_TRY(c, hipSetDevice(c->device));
	harvest(c);
	*out = c->times;
	if (reset) c->times = mirt_kernel_times{};
	return MIRT_OK;
}
int mirt_get_stream(mirt_ctx* c, void** s) { if (!c || !s) return MIRT_ERR_ARG; *s = c->stream; return MIRT_OK; }

// ---- stage-level entry points -------------------------------------------------------------------
int mirt_debug_raygen(mirt_ctx* c, uint32_t accumulations, float* p_xyz, float* dir_xyz) {
	int r = check_ready(c); if (r) return r;
	if (!p_xyz || !dir_xyz || accumulations == 0) return fail(c, MIRT_ERR_ARG, "bad arguments");
	if (c->n_tiles == 0) return fail(c, MIRT_ERR_STATE, "no tiles owned");
	HIP_TRY(c, hipSetDevice(c->device));
	if ((r = ensure_streams(c))) return r;
	const FrameParams fp = frame_params(c, accumulations - 1, 1);
	const size_t n = fp.n_pix;
	HIP_TRY(c, sync_all(c));
	hipLaunchKernelGGL(lens_on(c) ? k_raygen<true> : k_raygen<false>, dim3(grid_for(c, n)), dim3(kBlock), 0, c->stream, fp, c->slots[0].stream_buf[0], batch_counters(c, c->slots[0]).stream_queue(0).n, c->lens);
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	const StreamBuf& s = c->slots[0].stream_buf[0];
	std::vector<float4> rec(2 * n);                                          // records {p, path}, {dir, throughput.r} -> the caller's planes
	HIP_TRY(c, hipMemcpy(rec.data(), s.a, n * sizeof(float4), hipMemcpyDeviceToHost));
	HIP_TRY(c, hipMemcpy(rec.data() + n, s.b, n * sizeof(float4), hipMemcpyDeviceToHost));
	for (size_t i = 0; i < n; i++) {
		p_xyz[i] = rec[i].x; p_xyz[n + i] = rec[i].y; p_xyz[2 * n + i] = rec[i].z;
		dir_xyz[i] = rec[n + i].x; dir_xyz[n + i] = rec[n + i].y; dir_xyz[2 * n + i] = rec[n + i].z;
	}
	return MIRT_OK;
}

int mirt_debug_trace_closest(mirt_ctx* c, size_t n, const float* p_xyz, const float* dir_xyz, float* tfar_out, int32_t* prim_out) {
	if (!c) return MIRT_ERR_ARG;
	if (!c->have_scene) return fail(c, MIRT_ERR_STATE, "mirt_set_scene has not been called");
	if (!p_xyz || !dir_xyz || !tfar_out || !prim_out || n == 0 || n >= (1ull << 31)) return fail(c, MIRT_ERR_ARG, "bad arguments");
	std::vector<HitRec> hits(n);
	const int r = debug_trace(c, "debug_trace_closest", n, p_xyz, dir_xyz, nullptr, hits.data());
	if (r == MIRT_OK) for (size_t i = 0; i < n; i++) { tfar_out[i] = hits[i].tfar; prim_out[i] = hits[i].prim; }
	return r;
}

int mirt_debug_trace_shadow(mirt_ctx* c, size_t n, const float* p_xyz, const float* dir_xyz, const float* tfar, uint8_t* occluded_out) {
	if (!c) return MIRT_ERR_ARG;
	if (!c->have_scene) return fail(c, MIRT_ERR_STATE, "mirt_set_scene has not been called");
	if (!p_xyz || !dir_xyz || !tfar || !occluded_out || n == 0 || n >= (1ull << 31)) return fail(c, MIRT_ERR_ARG, "bad arguments");
	std::vector<uint32_t> occ(n);
	const int r = debug_trace(c, "debug_trace_shadow", n, p_xyz, dir_xyz, tfar, occ.data());
	if (r == MIRT_OK) for (size_t i = 0; i < n; i++) occluded_out[i] = occ[i] ? 1 : 0;
	return r;
}

int mirt_debug_math(mirt_ctx* c, int fn, size_t n, const float* in, float* out) {
	if (!c) return MIRT_ERR_ARG;
	static const int n_in[15] = { 1, 2, 1, 2, 2, 6, 8, 3, 10, 9, 1, 6, 2, 3, 7 }, n_out[15] = { 2, 1, 1, 3, 3, 10, 5, 5, 3, 6, 1, 6, 6, 3, 1 };
	if (fn < 0 || fn > 14 || !in || !out || n == 0 || n >= (1u << 28)) return fail(c, MIRT_ERR_ARG, "bad arguments");
	HIP_TRY(c, hipSetDevice(c->device));
	ScopedBuffer din, dout;
	HIP_TRY(c, din.ensure(n * n_in[fn] * 4)); HIP_TRY(c, dout.ensure(n * n_out[fn] * 4));
	HIP_TRY(c, hipMemcpy(din.ptr, in, n * n_in[fn] * 4, hipMemcpyHostToDevice));
	const bool sky_fn = fn == 12 || fn == 13;
	if (sky_fn && !(c->sky.t && c->sky_total > 0.0f)) return fail(c, MIRT_ERR_STATE, "debug_math fn %d reads the sky sampling table: mirt_set_sky_sampling(ctx, 1) over a scene whose table has a total above 0 first", fn);
	if (fn == 14) hipLaunchKernelGGL(k_debug_ggx_pdf, dim3(grid_for(c, n)), dim3(kBlock), 0, c->stream, static_cast<uint32_t>(n), din.as<float>(), dout.as<float>());
	else if (sky_fn) hipLaunchKernelGGL(k_debug_sky, dim3(grid_for(c, n)), dim3(kBlock), 0, c->stream, fn, static_cast<uint32_t>(n), din.as<float>(), dout.as<float>(), c->scene, c->sky);
	else hipLaunchKernelGGL(k_debug_math, dim3(grid_for(c, n)), dim3(kBlock), 0, c->stream, fn, static_cast<uint32_t>(n), din.as<float>(), dout.as<float>());
	hipError_t e = hipGetLastError();
	if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
	if (e == hipSuccess) e = hipMemcpy(out, dout.ptr, n * n_out[fn] * 4, hipMemcpyDeviceToHost);
	if (e != hipSuccess) return fail(c, MIRT_ERR_HIP, "debug_math: %s", hipGetErrorString(e));
	return MIRT_OK;
}

int mirt_debug_primary_lists(mirt_ctx* c, uint32_t hist[10]) {
	int r = check_ready(c); if (r) return r;
	if (!hist) return fail(c, MIRT_ERR_ARG, "hist is NULL");
	if (!c->policy.use_bvh || c->scene.n_recs == 0 || c->n_tiles == 0) return fail(c, MIRT_ERR_STATE, "needs policy.use_bvh, a tree and at least one tile");
	{ const int fr = flush_deferred(c); if (fr) return fr; }
	HIP_TRY(c, hipSetDevice(c->device));
	if ((r = ensure_streams(c))) return r;
	HIP_TRY(c, sync_all(c));
	const FrameParams fp = frame_params(c, 0, 1);
	if (!c->cand_valid && (r = build_primary_lists(c, trace_scene(c), fp, false))) return r;   // (the lists of the current view: the ones the next batch reads)
	std::vector<uint32_t> host(static_cast<size_t>(fp.n_pix));                            // plane 0 of the lists: the counts
	HIP_TRY(c, hipMemcpyAsync(host.data(), c->cand.ptr, host.size() * 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	for (int k = 0; k < 10; k++) hist[k] = 0;
	for (size_t p = 0; p < fp.n_pix; p++) { const uint32_t n = host[p]; hist[n == kCandOverflow ? 9 : std::min<uint32_t>(n, 8u)]++; }     // hist[8]: 8 or more
	return MIRT_OK;
}

int mirt_debug_primary_counts(mirt_ctx* c, uint32_t* counts, size_t capacity) {
	int r = check_ready(c); if (r) return r;
	if (!counts) return fail(c, MIRT_ERR_ARG, "counts is NULL");
	if (!c->policy.use_bvh || c->scene.n_recs == 0 || c->n_tiles == 0) return fail(c, MIRT_ERR_STATE, "needs policy.use_bvh, a tree and at least one tile");
	{ const int fr = flush_deferred(c); if (fr) return fr; }
	HIP_TRY(c, hipSetDevice(c->device));
	if ((r = ensure_streams(c))) return r;
	HIP_TRY(c, sync_all(c));
	const FrameParams fp = frame_params(c, 0, 1);
	if (capacity < fp.n_pix) return fail(c, MIRT_ERR_ARG, "debug_primary_counts: room for %zu counts, %u local pixels", capacity, fp.n_pix);
	if (!c->cand_valid && (r = build_primary_lists(c, trace_scene(c), fp, false))) return r;   // (as mirt_debug_primary_lists)
	HIP_TRY(c, hipMemcpyAsync(counts, c->cand.ptr, static_cast<size_t>(fp.n_pix) * 4, hipMemcpyDeviceToHost, c->stream));     // plane 0 of the lists
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	return MIRT_OK;
}

int mirt_debug_info(mirt_ctx* c, uint32_t out[8]) {
	if (!c || !out) return MIRT_ERR_ARG;
	const SceneDev& s = c->scene;
	const LdsPlan p = lds_plan(c);
	out[0] = s.n_recs; out[1] = s.lds_recs; out[2] = s.lds_spheres; out[3] = c->bvh_depth; out[4] = s.half_boxes | (s.wide << 1);
	out[5] = p.launch_bytes; out[6] = p.wgs_per_cu; out[7] = static_cast<uint32_t>(c->n_cu);
	return MIRT_OK;
}
int mirt_debug_tree(mirt_ctx* c, void* dst, size_t capacity_bytes, uint32_t info[4]) {
	if (!c) return MIRT_ERR_ARG;
	if (!info) return fail(c, MIRT_ERR_ARG, "debug_tree: info is NULL");
	if (!c->have_scene) return fail(c, MIRT_ERR_STATE, "mirt_set_scene has not been called");
	const SceneDev& s = c->scene;
	const uint32_t rec_bytes = (s.half_boxes && !s.wide) ? 32u : 64u;
	info[0] = s.n_recs; info[1] = rec_bytes; info[2] = s.wide ? 2u : s.half_boxes ? 1u : 0u; info[3] = c->bvh_depth;
	if (!dst) return MIRT_OK;
	const size_t bytes = static_cast<size_t>(s.n_recs) * rec_bytes;
	if (capacity_bytes < bytes) return fail(c, MIRT_ERR_ARG, "debug_tree: %zu bytes of capacity, the records take %zu", capacity_bytes, bytes);
	if (bytes == 0) return MIRT_OK;
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	HIP_TRY(c, hipMemcpy(dst, s.recs, bytes, hipMemcpyDeviceToHost));             // the device copy the kernels walk, not SceneRecords' host vectors
	return MIRT_OK;
}
int mirt_debug_sky_table(mirt_ctx* c, float* dst, size_t capacity, uint32_t info[4]) {
	if (!c) return MIRT_ERR_ARG;
	if (!info) return fail(c, MIRT_ERR_ARG, "debug_sky_table: info is NULL");
	if (!c->sky.t) return fail(c, MIRT_ERR_STATE, "there is no sky sampling table: mirt_set_sky_sampling(ctx, 1) and mirt_set_scene first");
	const size_t floats = sky_table_floats(c->sky.rows, c->sky.cols);
	info[0] = c->sky.rows; info[1] = c->sky.cols; std::memcpy(&info[2], &c->sky_total, 4); info[3] = static_cast<uint32_t>(floats);
	if (!dst) return MIRT_OK;
	if (capacity < floats) return fail(c, MIRT_ERR_ARG, "debug_sky_table: room for %zu floats, the table takes %zu", capacity, floats);
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	HIP_TRY(c, hipMemcpy(dst, c->sky.t, floats * sizeof(float), hipMemcpyDeviceToHost));
	return MIRT_OK;
}
// ---- the Ambient update: the environment alone (mirt.h "replacing the environment map on its own") ----------------------------
// What mirt_set_environment and mirt_set_sun_sky share.  `texels` (w x h, validated by the caller's rules below) are uploaded, or, with bake != NULL,
// written by k_sun_sky on the main stream.  Nothing but the environment changes: the tree, the candidate lists, the LDS plan and the history stay.
static int replace_environment(mirt_ctx* c, const float amb[3], const float4* texels, uint32_t w, uint32_t h, const mirt_sun_sky::Args* bake) {
	const size_t n = static_cast<size_t>(w) * h;
	const bool new_map = texels || bake;
	{ const int fr = flush_and_wait(c); if (fr) return fr; }                      // batches in flight read the old map and the old table
	if (c->sky_sampling && !bake) {                                               // before anything is changed (a baked map is finite and non-negative by construction)
		std::vector<float4> old;
		if (!texels) {                                                            // the ambient-only form validates the map it keeps
			w = static_cast<uint32_t>(c->scene.hdri_w); h = static_cast<uint32_t>(c->scene.hdri_h);
			old.resize(static_cast<size_t>(w) * h);
			HIP_TRY(c, hipMemcpy(old.data(), c->scene.hdri, old.size() * sizeof(float4), hipMemcpyDeviceToHost));
		}
		const int r = check_sky_texels(c, texels ? texels : old.data(), w, h, amb);
		if (r) return r;
	}
	if (new_map) {
		DeviceBuffer fresh;                                                       // a larger map goes to a new allocation first: a failure leaves the old one in place
		DeviceBuffer& dst = n * sizeof(float4) > c->hdri.bytes ? fresh : c->hdri;
		HIP_TRY(c, dst.ensure(n * sizeof(float4)));
		hipError_t e = hipSuccess;
		if (bake) {
			hipLaunchKernelGGL(k_sun_sky, dim3(static_cast<uint32_t>((n + kSunSkyBlock - 1u) / kSunSkyBlock)), dim3(kSunSkyBlock), 0, c->stream, *bake, dst.as<float4>());
			e = hipGetLastError();
		} else e = hipMemcpyAsync(dst.ptr, texels, n * sizeof(float4), hipMemcpyHostToDevice, c->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(c->stream);                 // host buffers are copied, never retained
		if (e != hipSuccess) { fresh.release(); return fail(c, MIRT_ERR_HIP, "environment map: %s", hipGetErrorString(e)); }
		if (&dst == &fresh) { c->hdri.release(); c->hdri = fresh; }
		SceneDev& s = c->scene;
		s.hdri = c->hdri.as<float4>();
		s.hdri_w = static_cast<int32_t>(w); s.hdri_h = static_cast<int32_t>(h);
		s.hdri_fw = static_cast<float>(static_cast<int32_t>(w) - 1);              // as commit_scene
		s.hdri_fh = static_cast<float>(static_cast<int32_t>(h) - 1);
		c->env_baked = bake != nullptr;
	}
	{ SceneDev& s = c->scene;
	  for (int k = 0; k < 3; k++) s.ambient[k] = amb[k];
	  const float x = amb[0], y = amb[1], z = amb[2];
	  const float m1 = (y < z) ? z : y; const float m0 = (x < m1) ? m1 : x; s.has_ambient = (m0 > 0.0f) ? 1u : 0u; }   // Renderer.hpp:79, as commit_scene
	if (c->sky_sampling) { const int r = build_sky_table(c); if (r) return r; }
	return MIRT_OK;
}
int mirt_set_environment(mirt_ctx* c, const float ambient_color[3], const float* hdri_rgba, uint32_t w, uint32_t h) {
	if (!c) return MIRT_ERR_ARG;
	if (!ambient_color) return fail(c, MIRT_ERR_ARG, "ambient_color is NULL");
	const bool keep = !hdri_rgba && w == 0 && h == 0;
	if (!keep && (!hdri_rgba || w == 0 || h == 0)) return fail(c, MIRT_ERR_ARG, "the environment needs an hdri of at least 1x1, or NULL with 0 x 0 to keep the current one");
	if (!c->have_scene) return fail(c, MIRT_ERR_STATE, "mirt_set_environment replaces the environment of a scene: mirt_set_scene first");
	return replace_environment(c, ambient_color, reinterpret_cast<const float4*>(hdri_rgba), w, h, nullptr);
}
int mirt_read_environment(mirt_ctx* c, float* rgba_out, size_t capacity_floats, uint32_t info[4]) {
	if (!c) return MIRT_ERR_ARG;
	if (!info) return fail(c, MIRT_ERR_ARG, "read_environment: info is NULL");
	if (!c->have_scene) return fail(c, MIRT_ERR_STATE, "there is no environment: mirt_set_scene first");
	const SceneDev& s = c->scene;
	const size_t floats = static_cast<size_t>(s.hdri_w) * static_cast<size_t>(s.hdri_h) * 4u;
	info[0] = static_cast<uint32_t>(s.hdri_w); info[1] = static_cast<uint32_t>(s.hdri_h); info[2] = c->env_baked ? 1u : 0u; info[3] = 0u;
	if (!rgba_out) return MIRT_OK;
	if (capacity_floats < floats) return fail(c, MIRT_ERR_ARG, "read_environment: room for %zu floats, the map takes %zu", capacity_floats, floats);
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	HIP_TRY(c, hipMemcpy(rgba_out, s.hdri, floats * sizeof(float), hipMemcpyDeviceToHost));
	return MIRT_OK;
}
int mirt_sun_sky_defaults(mirt_sun_sky_params* out) { return mirt_sun_sky::defaults(out); }
int mirt_set_sun_sky(mirt_ctx* c, const mirt_sun_sky_params* p) {
	if (!c) return MIRT_ERR_ARG;
	char msg[160];
	if (const int r = mirt_sun_sky::check(p, msg, sizeof msg)) return fail(c, r, "%s", msg);
	if (!c->have_scene) return fail(c, MIRT_ERR_STATE, "mirt_set_sun_sky replaces the environment of a scene: mirt_set_scene first");
	const mirt_sun_sky::Args a = mirt_sun_sky::args(*p);
	const float amb[3] = { c->scene.ambient[0], c->scene.ambient[1], c->scene.ambient[2] };
	return replace_environment(c, amb, nullptr, p->width, p->height, &a);
}
int mirt_debug_allow_half_boxes(mirt_ctx* c, int allow) { if (!c) return MIRT_ERR_ARG; c->allow_half = allow != 0; return MIRT_OK; }

} // extern "C"

// ---- the Geometry update: spheres moved in place (mirt.h "moving spheres in place") ------------------------------------------------------
namespace {
// The links of the tree in place (refit.hpp), carved from c->refit_links: built by one kernel the first time a tree is refitted.
RefitLinks refit_links_of(mirt_ctx* c) {
	const size_t nr = c->scene.n_recs, np = c->scene.n_spheres;
	RefitLinks l;
	l.parent = c->refit_links.as<uint32_t>(); l.used = l.parent + nr; l.leaf_rec = l.used + nr; l.arrivals = l.leaf_rec + np;
	l.box = reinterpret_cast<mirt_box::Box*>(l.arrivals + nr);
	return l;
}
template <int L> void launch_refit(mirt_ctx* c, const RefitLinks& l, bool links) {
	const SceneDev& s = c->scene;
	uint4* recs = reinterpret_cast<uint4*>(const_cast<float4*>(s.recs));       // c->recs or c->recs_wide: this context's own allocation
	if (links) hipLaunchKernelGGL(k_refit_links<L>, dim3((s.n_recs + kRefitBlock - 1u) / kRefitBlock), dim3(kRefitBlock), 0, c->stream, recs, s.n_recs, s.n_spheres, l);
	else hipLaunchKernelGGL(k_refit<L>, dim3((s.n_spheres + kRefitBlock - 1u) / kRefitBlock), dim3(kRefitBlock), 0, c->stream, recs, s.n_recs, s.spheres, s.n_spheres, l);
}
void launch_refit(mirt_ctx* c, const RefitLinks& l, bool links) {
	if (c->scene.wide) launch_refit<kRefitWide>(c, l, links);
	else if (c->scene.half_boxes) launch_refit<kRefitHalf>(c, l, links);
	else launch_refit<kRefitF32>(c, l, links);
}
} // namespace

extern "C" int mirt_update_spheres(mirt_ctx* c, uint32_t n, const uint32_t* bvh_index, const uint32_t* geometry_index, const float* xyz_rsq) {
	if (!c) return MIRT_ERR_ARG;
	if (!c->have_scene) return fail(c, MIRT_ERR_STATE, "mirt_update_spheres moves spheres of a scene: mirt_set_scene first");
	SceneDev& s = c->scene;
	{ char msg[320];                                                             // before anything changes: a refused call leaves every word in place
	  if (const int r = mirt_scene_update::check(n, bvh_index, geometry_index, xyz_rsq, s.n_spheres, s.half_boxes != 0, msg, sizeof msg)) return fail(c, r, "%s", msg); }
	if (n == 0) return MIRT_OK;
	{ const int fr = flush_and_wait(c); if (fr) return fr; }                      // deferred accumulations and batches in flight see the old geometry
	// the edit list, then the scatter into c->spheres and into the geometry-order table (what mirt_update_materials regenerates the light tables from)
	const size_t index_bytes = (static_cast<size_t>(n) * 8u + 15u) & ~static_cast<size_t>(15u);
	HIP_TRY(c, c->refit_edits.ensure(index_bytes + static_cast<size_t>(n) * sizeof(float4)));
	uint32_t* d_index = c->refit_edits.as<uint32_t>();
	uint32_t* d_geo_index = d_index + n;
	float4* d_packet = reinterpret_cast<float4*>(static_cast<char*>(c->refit_edits.ptr) + index_bytes);
	const size_t nr = s.n_recs, np = s.n_spheres;
	if (!c->refit_links_valid) HIP_TRY(c, c->refit_links.ensure((3u * nr + np) * 4u + nr * sizeof(mirt_box::Box)));
	const RefitLinks l = refit_links_of(c);
	HIP_TRY(c, hipMemcpyAsync(d_index, bvh_index, static_cast<size_t>(n) * 4u, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(c, hipMemcpyAsync(d_geo_index, geometry_index, static_cast<size_t>(n) * 4u, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(c, hipMemcpyAsync(d_packet, xyz_rsq, static_cast<size_t>(n) * sizeof(float4), hipMemcpyHostToDevice, c->stream));
	hipLaunchKernelGGL(k_update_spheres, dim3((n + kRefitBlock - 1u) / kRefitBlock), dim3(kRefitBlock), 0, c->stream, n, d_index, d_geo_index, d_packet, c->spheres.as<float4>(), c->geo_sphere.as<float4>(), s.n_spheres);
	// every box of the records, over the topology in place
	if (nr) {
		if (!c->refit_links_valid) launch_refit(c, l, true);
		HIP_TRY(c, hipMemsetAsync(l.arrivals, 0, nr * 4u, c->stream));
		launch_refit(c, l, false);
	}
	HIP_TRY(c, hipGetLastError());
	// next event estimation reads the lights' spheres from a table of its own
	if (mirt_scene_update::patch_lights(c->light_ids.data(), static_cast<uint32_t>(c->light_ids.size()), n, geometry_index, xyz_rsq, s.n_spheres,
	                                    reinterpret_cast<float*>(c->light_sphere_host.data())))
		{ const int r = upload(c, c->light_sphere, c->light_sphere_host); if (r) return r; }
	HIP_TRY(c, hipStreamSynchronize(c->stream));                                  // host buffers are copied, never retained
	c->refit_links_valid = true;
	c->cand_valid = false;                                                        // the camera-ray lists name the spheres of the old positions
	c->spheres_gen++;                                                             // a history kept under mirt_set_sphere_motion compares its snapshot with the table as it is now
	if (!c->history_motion) drop_history(c);                                      // surfaces moved: nothing of the old view may be reprojected onto them
	return MIRT_OK;
}

// ---- the Material update: materials edited in place (mirt.h "updating materials in place") ------------------------------------------------
namespace {
// light_sphere / light_emit, light_ids and scene.n_lights from the geometry-order table and the emission rows in place: the reference's
// LightingAcceleration constructor as an ordered compaction on the device (light_list.hpp).  No batch is in flight (the caller has waited).
int regenerate_lights(mirt_ctx* c) {
	SceneDev& s = c->scene;
	const uint32_t n = s.n_spheres, n_blocks = (n + kLightBlock - 1u) / kLightBlock;
	uint32_t n_lights = 0;
	if (n) {
		const uint64_t mask = mirt_scene_update::emit_mask(reinterpret_cast<const float*>(c->emi_host.data()), s.n_mat);
		HIP_TRY(c, c->light_scan.ensure((static_cast<size_t>(n_blocks) + 1u) * 4u));
		uint32_t* totals = c->light_scan.as<uint32_t>();
		uint32_t* count = totals + n_blocks;
		const GeometryTable geo{ c->geo_sphere.as<float4>(), c->geo_mat.as<int32_t>() };
		hipLaunchKernelGGL(k_light_count, dim3(n_blocks), dim3(kLightBlock), 0, c->stream, geo.material, n, mask, totals);
		hipLaunchKernelGGL(k_light_scan, dim3(1), dim3(kLightScanPass), 0, c->stream, totals, n_blocks, count);
		HIP_TRY(c, hipGetLastError());
		HIP_TRY(c, hipMemcpyAsync(&n_lights, count, 4, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream));
		if (n_lights > n) return fail(c, MIRT_ERR_HIP, "update_materials: the light count read back (%u) exceeds the scene's %u spheres", n_lights, n);
		// the tables grow to the new count before the scatter (nothing reads the old rows: they are rewritten whole)
		HIP_TRY(c, c->light_sphere.ensure(std::max<size_t>(n_lights, 1) * sizeof(float4)));
		HIP_TRY(c, c->light_emit.ensure(std::max<size_t>(n_lights, 1) * sizeof(float4)));
		if (n_lights) {
			hipLaunchKernelGGL(k_light_scatter, dim3(n_blocks), dim3(kLightBlock), 0, c->stream, geo, n, mask, totals, c->mat_emission.as<float4>(),
			                   c->light_sphere.as<float4>(), c->light_emit.as<float4>(), n_lights);
			HIP_TRY(c, hipGetLastError());
		}
	}
	// the ids and the rows, as mirt_update_spheres' patch_lights wants them
	std::vector<float4> emit(n_lights);
	c->light_sphere_host.resize(n_lights);
	c->light_ids.resize(n_lights);
	if (n_lights) {
		HIP_TRY(c, hipMemcpyAsync(emit.data(), c->light_emit.ptr, static_cast<size_t>(n_lights) * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(c, hipMemcpyAsync(c->light_sphere_host.data(), c->light_sphere.ptr, static_cast<size_t>(n_lights) * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream));
	}
	for (uint32_t l = 0; l < n_lights; l++) std::memcpy(&c->light_ids[l], &emit[l].w, 4);
	s.light_sphere = c->light_sphere.as<float4>(); s.light_emit = c->light_emit.as<float4>();
	s.n_lights = n_lights;                                                         // fp.n_lights, fp.mis and the sky's light number follow per launch
	return MIRT_OK;
}
} // namespace

extern "C" int mirt_update_materials(mirt_ctx* c, uint32_t n_rows, const uint32_t* material_index, const mirt_material* rows,
                                     uint32_t n_assign, const uint32_t* bvh_index, const uint32_t* geometry_index, const int32_t* material_ID) {
	if (!c) return MIRT_ERR_ARG;
	if (!c->have_scene) return fail(c, MIRT_ERR_STATE, "mirt_update_materials edits the materials of a scene: mirt_set_scene first");
	SceneDev& s = c->scene;
	{ char msg[320];                                                             // before anything changes: a refused call leaves every word in place
	  if (const int r = mirt_scene_update::check_materials(n_rows, material_index, rows, n_assign, bvh_index, geometry_index, material_ID, s.n_spheres, s.n_mat,
	                                                       c->transmission != 0, reinterpret_cast<const float*>(c->glass_host.data()), msg, sizeof msg)) return fail(c, r, "%s", msg); }
	if (n_rows == 0 && n_assign == 0) return MIRT_OK;
	{ const int fr = flush_and_wait(c); if (fr) return fr; }                      // deferred accumulations and batches in flight see the old materials
	// the kept host rows, as flatten_tables makes them, and the four small tables again (at most 63 rows each: no kernel)
	for (uint32_t i = 0; i < n_rows; i++) {
		const mirt_material& m = rows[i];
		const uint32_t k = material_index[i];
		c->alb_host[k] = make_float4(m.albedo[0], m.albedo[1], m.albedo[2], 0.0f);
		c->emi_host[k] = make_float4(m.emission[0], m.emission[1], m.emission[2], 0.0f);
		c->ggx_host[k] = make_float4(m.F0[0], m.F0[1], m.F0[2], m.roughness);
		c->glass_host[k] = make_float4(m.transmission[0], m.transmission[1], m.transmission[2], 1.0f + m.IOR_minus_one);
	}
	int r;
	if (n_rows && ((r = upload(c, c->mat_albedo, c->alb_host)) || (r = upload(c, c->mat_emission, c->emi_host)) || (r = upload(c, c->mat_ggx, c->ggx_host)) ||
	               (r = upload(c, c->mat_glass, c->glass_host)))) return r;
	// the re-assigned spheres, in both orders
	if (n_assign) {
		const size_t words = static_cast<size_t>(n_assign);
		HIP_TRY(c, c->refit_edits.ensure(3u * words * 4u));
		uint32_t* d_bvh = c->refit_edits.as<uint32_t>();
		uint32_t* d_geo = d_bvh + words;
		int32_t* d_mat = reinterpret_cast<int32_t*>(d_geo + words);
		HIP_TRY(c, hipMemcpyAsync(d_bvh, bvh_index, words * 4u, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipMemcpyAsync(d_geo, geometry_index, words * 4u, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipMemcpyAsync(d_mat, material_ID, words * 4u, hipMemcpyHostToDevice, c->stream));
		hipLaunchKernelGGL(k_assign_materials, dim3((n_assign + kLightBlock - 1u) / kLightBlock), dim3(kLightBlock), 0, c->stream, n_assign, d_bvh, d_geo, d_mat,
		                   c->prim_mat.as<int32_t>(), GeometryTable{ c->geo_sphere.as<float4>(), c->geo_mat.as<int32_t>() }, s.n_spheres);
		HIP_TRY(c, hipGetLastError());
	}
	if ((r = regenerate_lights(c))) return r;
	HIP_TRY(c, hipStreamSynchronize(c->stream));                                  // host buffers are copied, never retained
	c->scene_has_glass = has_glass(c->glass_host);                                // with the transmission switch on, the GLASS kernels start or stop being launched
	c->mat_merged_valid = false;                                                  // the next MIXED launch uploads the new colours
	return MIRT_OK;                                                               // (closure_plan() reads the material count and the closure table: neither changed)
}

extern "C" int mirt_debug_lights(mirt_ctx* c, int32_t* ids_out, float* sphere_rows_out, float* emit_rows_out, size_t capacity_lights, uint32_t info[4]) {
	if (!c) return MIRT_ERR_ARG;
	if (!info) return fail(c, MIRT_ERR_ARG, "debug_lights: info is NULL");
	if (!c->have_scene) return fail(c, MIRT_ERR_STATE, "there are no light tables: mirt_set_scene first");
	const SceneDev& s = c->scene;
	const size_t n = s.n_lights;
	info[0] = s.n_lights; info[1] = kLightBlock; info[2] = kLightScanPass; info[3] = 0u;
	if (!ids_out && !sphere_rows_out && !emit_rows_out) return MIRT_OK;
	if (capacity_lights < n) return fail(c, MIRT_ERR_ARG, "debug_lights: room for %zu lights, the scene has %zu", capacity_lights, n);
	if (n == 0) return MIRT_OK;
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	std::vector<float4> emit(n);
	HIP_TRY(c, hipMemcpy(emit.data(), s.light_emit, n * sizeof(float4), hipMemcpyDeviceToHost));   // the device copies next event estimation samples
	if (emit_rows_out) std::memcpy(emit_rows_out, emit.data(), n * sizeof(float4));
	if (ids_out) for (size_t l = 0; l < n; l++) std::memcpy(&ids_out[l], &emit[l].w, 4);
	if (sphere_rows_out) HIP_TRY(c, hipMemcpy(sphere_rows_out, s.light_sphere, n * sizeof(float4), hipMemcpyDeviceToHost));
	return MIRT_OK;
}
