// mirt_launch.hip — the launch layer of the C-ABI (ctx.hpp): the batch pipeline, the kernel tables and every launch of the kernels in kernels.hpp,
// id_map.hpp, refit.hpp, light_list.hpp and sun_sky.hpp.  It is the only unit that includes those headers, so an edit to the API layer
// (mirt_capi.hip) or the resolve layer (mirt_resolve.hip) recompiles none of their kernels.
//
// Host-side stand-in for the per-tile ray streams of Renderer<Policy> (Renderer.hpp:38-49): one set of frame-wide SoA streams per batch in
// flight (see kernels.hpp).  There is no CPU fallback.
#include "ctx.hpp"
#include "kernels.hpp"
#include "id_map.hpp"
#include "sun_sky.hpp"
#include "refit.hpp"
#include "light_list.hpp"
#include "scene_update_host.hpp"
#include "bvh_layout.hpp"
#include "bvh_build.hpp"
#include "lbvh_build.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>

using namespace mirt;

namespace {

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
constexpr size_t kArenaPlanes = 2 * 10 + 2 + 16;      // two ray streams (40 B), hit (tfar, prim), shadow stream (four 16-B records): in 4-byte planes per ray of capacity
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
} // namespace
uint32_t batch_limit(const mirt_ctx* c) {
	if (c->policy.max_batch) return std::min(c->policy.max_batch, max_slots(c));
	const uint64_t n_pix = static_cast<uint64_t>(c->n_tiles) * kTileSize;
	if (n_pix == 0) return 1;
	const uint64_t b = std::max<uint64_t>((kBatchRays + n_pix / 2) / n_pix, batch_floor(c));
	return static_cast<uint32_t>(std::min<uint64_t>(std::min<uint64_t>(b, max_slots(c)), std::max<uint32_t>(c->batch_mem_cap, 1u)));
}
namespace {

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
	p.wgs_per_cu = std::min(std::max(kLdsPerCu / p.launch_bytes, 1u), c->tune.trace_wgs);
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
} // namespace
uint32_t wanted_slots(const mirt_ctx* c) {
	if (c->policy.streams) return std::min<uint32_t>(c->policy.streams, 8u);
	return static_cast<uint64_t>(c->n_tiles) * kTileSize * batch_limit(c) >= kSerialRays ? 1u : 3u;
}
namespace {
// Device bytes of the batches in flight for the current plan (ray streams + contribution buffers).
uint64_t streams_bytes(const mirt_ctx* c) {
	const uint64_t rays = static_cast<uint64_t>(c->n_tiles) * kTileSize * batch_limit(c);
	return wanted_slots(c) * (rays * 4u * (kArenaPlanes + (c->ggx_pdf ? 2u : 0u)) + rays * 12u);      // mirt_set_ggx_pdf: the closure-pdf plane of both streams, 4 B per ray each
}
} // namespace

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
	while (c->slots.size() > want) c->slots.pop_back();
	while (c->slots.size() < want) {
		PipeSlot sl;
		HIP_TRY(c, hipStreamCreateWithFlags(&sl.stream.s, hipStreamNonBlocking));
		HIP_TRY(c, hipEventCreateWithFlags(&sl.batch_done.e, hipEventDisableTiming));
		HIP_TRY(c, hipEventCreateWithFlags(&sl.merged.e, hipEventDisableTiming));
		c->slots.push_back(std::move(sl));
	}
	const size_t planes = kArenaPlanes;
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

namespace {
// half-angle of a pixel's bundle of camera rays: half a pixel diagonal (0.7072) at distance >= |z|; + 1e-4: a sample's own cone half-width
// (1.38e-3 .. 1.47e-3, from |D|^2 - 1 of its normalised direction) may exceed the axis ray's by 8.5e-5
float bundle_half_angle(const mirt_ctx* c) { return (0.7072f / std::fabs(c->camera.z)) * 1.01f + 1e-4f; }

// mirt_set_sky_sampling changes the kernels launched only where its light can be drawn and can carry something.
bool sky_active(const mirt_ctx* c) { return c->sky_sampling && c->sky.dev.t && c->sky.total > 0.0f && c->policy.mis && c->scene.has_ambient && !c->stream_order; }
} // namespace

// The launch rule of mirt_set_material_closures.  The effective closure of material m is closures[m], or policy.brdf at and beyond the table's end.
// If materials 0 .. n_mat - 1 of the scene all take closure k, the kernels of policy.brdf = k are launched (mixed = false, ggx = k): the same device
// code, hence that policy's words.  Otherwise the MIXED instantiations run with `mask` (bit m = material m is GGX).  The material LIST decides, not
// which materials the spheres use.  Exact stream order excludes a table (both setters), so k_tile_stream only ever sees policy.brdf.
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

namespace {
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
	sc.chunk_max = c->tune.chunk; sc.leaf_batch = c->tune.leaf_batch; sc.refill_idle = c->tune.refill_idle;
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
	if (!c->tables.gloss_decay_dev_valid) {                                                  // (batches in flight on other streams may still read the old table)
		HIP_TRY(c, sync_all(c));
		HIP_TRY(c, c->tables.gloss_decay_dev.ensure(std::max<size_t>(c->gloss_decay.size(), 1) * sizeof(float)));
		if (!c->gloss_decay.empty()) HIP_TRY(c, hipMemcpy(c->tables.gloss_decay_dev.ptr, c->gloss_decay.data(), c->gloss_decay.size() * sizeof(float), hipMemcpyHostToDevice));
		c->tables.gloss_decay_dev_valid = true;
	}
	Bracket t(c, MIRT_K_TRACE, st);
	hipLaunchKernelGGL(kTileStream[c->policy.brdf != 0], dim3(c->n_tiles * batch_n), dim3(kTileSize), 0, st, sc, fp, contrib, ctr, c->tables.mat_ggx.as<float4>(),
	                   c->tables.gloss_decay_dev.as<float>(), static_cast<uint32_t>(c->gloss_decay.size()), count ? 1u : 0u);
	return MIRT_OK;
}

// Builds the context's candidate lists (mirt_ctx::cand ...) for the current scene, camera and tile set: one cone traversal per local pixel
// (kernels.hpp kCollect).  The build runs on the main stream.  Every batch launched so far is ahead of it there — the main stream waits for a
// batch's batch_done before it merges the batch — so a rebuild cannot overtake a batch that still reads the previous lists; batches on
// other streams wait for cand_built (launch_batch).
int build_primary_lists(mirt_ctx* c, const SceneDev& sc, const FrameParams& fp, bool count) {
	HIP_TRY(c, c->lists.cand.ensure(static_cast<size_t>(fp.n_pix) * kCandStride * sizeof(uint32_t)));
	HIP_TRY(c, c->lists.cand_listed.ensure(static_cast<size_t>(fp.n_pix) * sizeof(uint32_t)));        // at most every pixel is without a list
	HIP_TRY(c, c->lists.cand_words.ensure(CandWords::kWords * sizeof(uint32_t)));
	if (!c->lists.cand_built) HIP_TRY(c, hipEventCreateWithFlags(&c->lists.cand_built.e, hipEventDisableTiming));
	const CandWords cw{ c->lists.cand_words.as<uint32_t>() };
	HIP_TRY(c, hipMemsetAsync(cw.w, 0, CandWords::kWords * sizeof(uint32_t), c->stream));
	{ Bracket t(c, MIRT_K_TRACE);
	  const FatList none{ cw.unused_fat_count(), nullptr, 0u };
	  hipLaunchKernelGGL(kPrimaryCand[!count], dim3(trace_grid(c, fp.n_pix)), dim3(kTraceBlock), trace_lds(c), c->stream, sc, fp, c->lists.cand.as<uint32_t>(), bundle_half_angle(c),
	                     cw.work(), none, c->counters.as<DevCounters>(), c->lists.cand_listed.as<uint32_t>(), cw.listed_pixels()); }
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipEventRecord(c->lists.cand_built, c->stream));
	c->lists.cand_gen++;
	c->lists.cand_valid = true;
	return MIRT_OK;
}

// mirt_set_aov(1): the camera rays' hit records of the batch lie in sl.hit (slot * n_pix + pixel) from the bounce-0 trace launches until the
// bounce-1 trace overwrites them; k_first_hit_aov runs in between, on the batch's own stream.  The slab holds running sums and float
// addition does not associate, so batches in flight on different streams must reach it in batch order: each waits for the event recorded
// after the previous batch's kernel.  (One batch at a time: everything is on the main stream already.)
int launch_first_hit_aov(mirt_ctx* c, PipeSlot& sl, hipStream_t st, const SceneDev& sc, const FrameParams& fp) {
	const bool pipelined = c->slots.size() > 1;
	if (pipelined) {
		if (!sl.aov_done) HIP_TRY(c, hipEventCreateWithFlags(&sl.aov_done.e, hipEventDisableTiming));
		if (c->aov_prev && c->aov_prev != sl.aov_done) HIP_TRY(c, hipStreamWaitEvent(st, c->aov_prev, 0));   // (the slot's own previous batch is ahead on this very stream)
	}
	{ Bracket t(c, MIRT_K_RESOLVE, st);
	  const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((static_cast<uint64_t>(fp.n_pix) + kBlock - 1) / kBlock, static_cast<uint64_t>(c->n_cu) * 64u));
	  // the closure colour of the first hit: albedo under Lambertian, F0 under GGX; MIXED: one merged table, per material the row of its closure
	  const ClosurePlan plan = closure_plan(c);
	  if (plan.mixed && !c->tables.mat_merged_valid) {
	    std::vector<float4> merged(c->scene.n_mat);
	    for (uint32_t m = 0; m < c->scene.n_mat; m++) merged[m] = ((plan.mask >> m) & 1ull) ? c->tables.ggx_host[m] : c->tables.alb_host[m];
	    HIP_TRY(c, sync_all(c));                                                  // (batches in flight on other streams may still read the old table)
	    HIP_TRY(c, c->tables.mat_merged.ensure(merged.size() * sizeof(float4)));
	    HIP_TRY(c, hipMemcpy(c->tables.mat_merged.ptr, merged.data(), merged.size() * sizeof(float4), hipMemcpyHostToDevice));
	    c->tables.mat_merged_valid = true;
	  }
	  const float4* colour = plan.mixed ? c->tables.mat_merged.as<float4>() : plan.ggx ? c->tables.mat_ggx.as<float4>() : c->scene.mat_albedo;
	  hipLaunchKernelGGL(first_hit_aov_kernel(lens_on(c), c->freeze.n_frozen != 0), dim3(grid), dim3(kBlock), 0, st, sc, fp, sl.hit, colour, c->aov.as<float>(), c->lens, c->freeze.tile_frozen.as<uint32_t>()); }
	if (pipelined) { HIP_TRY(c, hipEventRecord(sl.aov_done, st)); c->aov_prev = sl.aov_done; }
	return MIRT_OK;
}
} // namespace

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
	const bool sparse = c->freeze.n_frozen != 0;
	const uint32_t* tile_frozen = c->freeze.tile_frozen.as<uint32_t>();
	const uint32_t active_pix = (c->n_tiles - c->freeze.n_frozen) * kTileSize;
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
	const float4* mat_ggx = c->tables.mat_ggx.as<float4>();
	float* contrib = sl.contrib.as<float>();                                      // slot k of the buffer = accumulation acc_base + k + 1
	uint32_t* fat_lists = sl.fat.as<uint32_t>();
	const SceneDev sc = trace_scene(c);
	const bool count = c->policy.count_traffic != 0;
	// k_shade's grid: as many 512-thread workgroups as are resident per CU at the launched form's waves per SIMD (shade_waves: three at 6, four at 8); more only adds passes
	// (tune_shade_wgs, MIRT_TUNE_SHADE_WGS: one figure for every form instead, for sweeps; 0 = follow the form)
	const ClosurePlan plan = closure_plan(c);
	const auto shade_grid = [&](const ShadeForm& f) {
		const uint32_t wgs = c->tune.shade_wgs ? c->tune.shade_wgs : shade_waves(f) * 4u / (kShadeBlock / 64u);
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
		if (!c->lists.cand_valid || count) { const int r = build_primary_lists(c, sc, fp, count); if (r) return r; }
		if (pipelined && sl.cand_gen != c->lists.cand_gen) { HIP_TRY(c, hipStreamWaitEvent(st, c->lists.cand_built, 0)); sl.cand_gen = c->lists.cand_gen; }
		if (sparse) {
			// the listed pixels of the active tiles: made on the main stream behind the lists' build (and, like it, behind every earlier batch's merge
			// wait), again whenever the lists or the mask have changed
			if (c->lists.listed_gen == 0 || c->lists.listed_for_cand != c->lists.cand_gen || c->lists.listed_for_freeze != c->freeze.freeze_gen) {
				HIP_TRY(c, c->lists.listed_active.ensure((static_cast<size_t>(fp.n_pix) + 1) * sizeof(uint32_t)));
				if (!c->lists.listed_built) HIP_TRY(c, hipEventCreateWithFlags(&c->lists.listed_built.e, hipEventDisableTiming));
				uint32_t* la = c->lists.listed_active.as<uint32_t>();
				HIP_TRY(c, hipMemsetAsync(la, 0, sizeof(uint32_t), c->stream));
				const CandWords words{ c->lists.cand_words.as<uint32_t>() };
				hipLaunchKernelGGL(k_listed_active, dim3(grid_for(c, fp.n_pix)), dim3(kBlock), 0, c->stream, c->lists.cand_listed.as<uint32_t>(), words.listed_pixels(), tile_frozen, la + 1, la);
				HIP_TRY(c, hipGetLastError());
				HIP_TRY(c, hipEventRecord(c->lists.listed_built, c->stream));
				c->lists.listed_for_cand = c->lists.cand_gen; c->lists.listed_for_freeze = c->freeze.freeze_gen; c->lists.listed_gen++;
			}
			if (pipelined && sl.listed_gen != c->lists.listed_gen) { HIP_TRY(c, hipStreamWaitEvent(st, c->lists.listed_built, 0)); sl.listed_gen = c->lists.listed_gen; }
		}
	}
	const CandWords cw{ c->lists.cand_words.as<uint32_t>() };
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
			    hipLaunchKernelGGL(primary_hits_kernel(count, wave, sparse), dim3(wave ? wgrid : hgrid), dim3(kBlock), 0, st, sc, fp, c->lists.cand.as<uint32_t>(), sl.hit, ctr, tile_frozen, active_pix);
			  }
			  // the adds of bounce-1 that waited for occlusion land in the paths' contribution words before k_shade adds this bounce's terms;
			  const ShadowSink sink{ contrib, batch_n, fp.pix_bits, nullptr };
			  StreamBuf rays = in;
			  // A listed launch reads nothing else of the stream: camera rays are functions of their index.  kPrimaryList: the pixels without a candidate
			  // list (once a tile is frozen: those of them in the active tiles); kPrimaryActive, a tile frozen and no lists: every pixel of the active tiles.
			  const int primary = bounce != 0 ? kPrimaryNone : lists ? kPrimaryList : sparse ? kPrimaryActive : kPrimaryAll;
			  uint32_t* listed_count = nullptr;
			  const uint32_t* list = nullptr;
			  if (primary == kPrimaryActive) { listed_count = c->freeze.active_list.as<uint32_t>(); list = listed_count + 1; }
			  else if (lists && sparse) { listed_count = c->lists.listed_active.as<uint32_t>(); list = listed_count + 1; }
			  else if (lists) { listed_count = cw.listed_pixels(); list = c->lists.cand_listed.as<uint32_t>(); }
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
			                     form.sky ? c->sky.dev : SkyTable{}, plan.mask, form.pdf ? sl.pdf_plane[bounce & 1u] : nullptr, form.pdf ? sl.pdf_plane[(bounce & 1u) ^ 1u] : nullptr); }
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
	if (c->policy.profile && c->prof.pending.size() > 512) harvest(c);
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

// The sampling table of the scene's environment map, built on the device from c->tables.hdri (kernels.hpp k_sky_importance, k_sky_scan) on the main
// stream, which is synchronised before the total is read.  The caller has validated the texels and no batch is in flight.
int build_sky_table(mirt_ctx* c) {
	const SceneDev& s = c->scene;
	const uint32_t cols = static_cast<uint32_t>(std::max(s.hdri_w, 2) - 1), rows = static_cast<uint32_t>(std::max(s.hdri_h, 2) - 1);
	HIP_TRY(c, c->sky.table.ensure(sky_table_floats(rows, cols) * sizeof(float)));
	float* t = c->sky.table.as<float>();
	hipLaunchKernelGGL(k_sky_importance, dim3(rows), dim3(kSkyBlock), 0, c->stream, s.hdri, s.hdri_w, s.ambient[0], s.ambient[1], s.ambient[2], rows, cols, t);
	hipLaunchKernelGGL(k_sky_scan, dim3(rows), dim3(kSkyBlock), 0, c->stream, rows, cols, t);
	HIP_TRY(c, hipGetLastError());
	float total = 0.0f;
	HIP_TRY(c, hipMemcpyAsync(&total, t + rows - 1, sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	c->sky.dev = SkyTable{ t, rows, cols };
	c->sky.total = total;
	return MIRT_OK;
}

// The records the kernels walk for this scene, uploaded (a host-built tree) or built in place (the GPU LBVH over c->tables.spheres, uploaded by the caller).
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
		HIP_TRY(c, c->tables.recs.ensure(static_cast<size_t>(t.n_recs) * (t.is_half ? 32u : 64u)));
		const bool want_wide = t.is_half && c->tune.wide;                    // the 4-wide binary16 records as well (used when the tree is shallow enough)
		if (want_wide) HIP_TRY(c, c->tables.recs_wide.ensure(static_cast<size_t>(t.n_recs) * 64u));
		std::string why;
		uint32_t n_wide = 0;
		if (!mirt_gpu::build_lbvh(c->stream, c->tables.spheres.as<float4>(), n_spheres, t.is_half ? nullptr : c->tables.recs.as<float>(), t.is_half ? c->tables.recs.as<uint32_t>() : nullptr, &t.depth, &why,
		                          want_wide ? c->tables.recs_wide.as<uint32_t>() : nullptr, &n_wide))
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
	t.is_wide = t.is_half && c->tune.wide && mirt_host::build_wide_half_records(t.f32, t.wide, &wide_levels);
	if (t.is_wide) t.n_recs = static_cast<uint32_t>(t.wide.size() / 16);
	return t.is_wide ? upload(c, c->tables.recs, t.wide) : t.is_half ? upload(c, c->tables.recs, t.half) : upload(c, c->tables.recs, t.f32);
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
	HIP_TRY(c, c->hist.id_words.ensure(2 * sizeof(uint32_t)));
	HIP_TRY(c, hipMemsetAsync(c->hist.id_words.ptr, 0, 2 * sizeof(uint32_t), c->stream));
	const IdMapDev p{ gs->camera, c->width, static_cast<uint32_t>(n), 1.0f / static_cast<float>(c->width) };
	{ Bracket t(c, MIRT_K_RESOLVE);
	  hipLaunchKernelGGL(k_id_map, dim3(trace_grid(gs, n)), dim3(kTraceBlock), trace_lds(gs), c->stream, trace_scene(gs), p, prim_dev, dist_dev, c->hist.id_words.as<uint32_t>()); }
	HIP_TRY(c, hipGetLastError());
	return MIRT_OK;
}

extern "C" {

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

int mirt_debug_math(mirt_ctx* c, int fn, size_t n, const float* in, float* out) {
	if (!c) return MIRT_ERR_ARG;
	static const int n_in[15] = { 1, 2, 1, 2, 2, 6, 8, 3, 10, 9, 1, 6, 2, 3, 7 }, n_out[15] = { 2, 1, 1, 3, 3, 10, 5, 5, 3, 6, 1, 6, 6, 3, 1 };
	if (fn < 0 || fn > 14 || !in || !out || n == 0 || n >= (1u << 28)) return fail(c, MIRT_ERR_ARG, "bad arguments");
	HIP_TRY(c, hipSetDevice(c->device));
	ScopedBuffer din, dout;
	HIP_TRY(c, din.ensure(n * n_in[fn] * 4)); HIP_TRY(c, dout.ensure(n * n_out[fn] * 4));
	HIP_TRY(c, hipMemcpy(din.ptr, in, n * n_in[fn] * 4, hipMemcpyHostToDevice));
	const bool sky_fn = fn == 12 || fn == 13;
	if (sky_fn && !(c->sky.dev.t && c->sky.total > 0.0f)) return fail(c, MIRT_ERR_STATE, "debug_math fn %d reads the sky sampling table: mirt_set_sky_sampling(ctx, 1) over a scene whose table has a total above 0 first", fn);
	if (fn == 14) hipLaunchKernelGGL(k_debug_ggx_pdf, dim3(grid_for(c, n)), dim3(kBlock), 0, c->stream, static_cast<uint32_t>(n), din.as<float>(), dout.as<float>());
	else if (sky_fn) hipLaunchKernelGGL(k_debug_sky, dim3(grid_for(c, n)), dim3(kBlock), 0, c->stream, fn, static_cast<uint32_t>(n), din.as<float>(), dout.as<float>(), c->scene, c->sky.dev);
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
	if (!c->lists.cand_valid && (r = build_primary_lists(c, trace_scene(c), fp, false))) return r;   // (the lists of the current view: the ones the next batch reads)
	std::vector<uint32_t> host(static_cast<size_t>(fp.n_pix));                            // plane 0 of the lists: the counts
	HIP_TRY(c, hipMemcpyAsync(host.data(), c->lists.cand.ptr, host.size() * 4, hipMemcpyDeviceToHost, c->stream));
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
	if (!c->lists.cand_valid && (r = build_primary_lists(c, trace_scene(c), fp, false))) return r;   // (as mirt_debug_primary_lists)
	HIP_TRY(c, hipMemcpyAsync(counts, c->lists.cand.ptr, static_cast<size_t>(fp.n_pix) * 4, hipMemcpyDeviceToHost, c->stream));     // plane 0 of the lists
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

} // extern "C"

// ---- the Geometry update: spheres moved in place (mirt.h "moving spheres in place") ------------------------------------------------------
namespace {
// The links of the tree in place (refit.hpp), carved from c->tables.refit_links: built by one kernel the first time a tree is refitted.
RefitLinks refit_links_of(mirt_ctx* c) {
	const size_t nr = c->scene.n_recs, np = c->scene.n_spheres;
	RefitLinks l;
	l.parent = c->tables.refit_links.as<uint32_t>(); l.used = l.parent + nr; l.leaf_rec = l.used + nr; l.arrivals = l.leaf_rec + np;
	l.box = reinterpret_cast<mirt_box::Box*>(l.arrivals + nr);
	return l;
}
template <int L> void launch_refit(mirt_ctx* c, const RefitLinks& l, bool links) {
	const SceneDev& s = c->scene;
	uint4* recs = reinterpret_cast<uint4*>(const_cast<float4*>(s.recs));       // c->tables.recs or c->tables.recs_wide: this context's own allocation
	if (links) hipLaunchKernelGGL(k_refit_links<L>, dim3((s.n_recs + kRefitBlock - 1u) / kRefitBlock), dim3(kRefitBlock), 0, c->stream, recs, s.n_recs, s.n_spheres, l);
	else hipLaunchKernelGGL(k_refit<L>, dim3((s.n_spheres + kRefitBlock - 1u) / kRefitBlock), dim3(kRefitBlock), 0, c->stream, recs, s.n_recs, s.spheres, s.n_spheres, l);
}
void launch_refit(mirt_ctx* c, const RefitLinks& l, bool links) {
	if (c->scene.wide) launch_refit<kRefitWide>(c, l, links);
	else if (c->scene.half_boxes) launch_refit<kRefitHalf>(c, l, links);
	else launch_refit<kRefitF32>(c, l, links);
}
} // namespace

int launch_update_spheres(mirt_ctx* c, uint32_t n, const uint32_t* bvh_index, const uint32_t* geometry_index, const float* xyz_rsq) {
	SceneDev& s = c->scene;
	// the edit list, then the scatter into c->tables.spheres and into the geometry-order table (what mirt_update_materials regenerates the light tables from)
	const size_t index_bytes = (static_cast<size_t>(n) * 8u + 15u) & ~static_cast<size_t>(15u);
	HIP_TRY(c, c->tables.refit_edits.ensure(index_bytes + static_cast<size_t>(n) * sizeof(float4)));
	uint32_t* d_index = c->tables.refit_edits.as<uint32_t>();
	uint32_t* d_geo_index = d_index + n;
	float4* d_packet = reinterpret_cast<float4*>(static_cast<char*>(c->tables.refit_edits.ptr) + index_bytes);
	const size_t nr = s.n_recs, np = s.n_spheres;
	if (!c->tables.refit_links_valid) HIP_TRY(c, c->tables.refit_links.ensure((3u * nr + np) * 4u + nr * sizeof(mirt_box::Box)));
	const RefitLinks l = refit_links_of(c);
	HIP_TRY(c, hipMemcpyAsync(d_index, bvh_index, static_cast<size_t>(n) * 4u, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(c, hipMemcpyAsync(d_geo_index, geometry_index, static_cast<size_t>(n) * 4u, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(c, hipMemcpyAsync(d_packet, xyz_rsq, static_cast<size_t>(n) * sizeof(float4), hipMemcpyHostToDevice, c->stream));
	hipLaunchKernelGGL(k_update_spheres, dim3((n + kRefitBlock - 1u) / kRefitBlock), dim3(kRefitBlock), 0, c->stream, n, d_index, d_geo_index, d_packet, c->tables.spheres.as<float4>(), c->tables.geo_sphere.as<float4>(), s.n_spheres);
	// every box of the records, over the topology in place
	if (nr) {
		if (!c->tables.refit_links_valid) launch_refit(c, l, true);
		HIP_TRY(c, hipMemsetAsync(l.arrivals, 0, nr * 4u, c->stream));
		launch_refit(c, l, false);
	}
	HIP_TRY(c, hipGetLastError());
	// next event estimation reads the lights' spheres from a table of its own
	if (mirt_scene_update::patch_lights(c->tables.light_ids.data(), static_cast<uint32_t>(c->tables.light_ids.size()), n, geometry_index, xyz_rsq, s.n_spheres,
	                                    reinterpret_cast<float*>(c->tables.light_sphere_host.data())))
		{ const int r = upload(c, c->tables.light_sphere, c->tables.light_sphere_host); if (r) return r; }
	HIP_TRY(c, hipStreamSynchronize(c->stream));                                  // host buffers are copied, never retained
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
		const uint64_t mask = mirt_scene_update::emit_mask(reinterpret_cast<const float*>(c->tables.emi_host.data()), s.n_mat);
		HIP_TRY(c, c->tables.light_scan.ensure((static_cast<size_t>(n_blocks) + 1u) * 4u));
		uint32_t* totals = c->tables.light_scan.as<uint32_t>();
		uint32_t* count = totals + n_blocks;
		const GeometryTable geo{ c->tables.geo_sphere.as<float4>(), c->tables.geo_mat.as<int32_t>() };
		hipLaunchKernelGGL(k_light_count, dim3(n_blocks), dim3(kLightBlock), 0, c->stream, geo.material, n, mask, totals);
		hipLaunchKernelGGL(k_light_scan, dim3(1), dim3(kLightScanPass), 0, c->stream, totals, n_blocks, count);
		HIP_TRY(c, hipGetLastError());
		HIP_TRY(c, hipMemcpyAsync(&n_lights, count, 4, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream));
		if (n_lights > n) return fail(c, MIRT_ERR_HIP, "update_materials: the light count read back (%u) exceeds the scene's %u spheres", n_lights, n);
		// the tables grow to the new count before the scatter (nothing reads the old rows: they are rewritten whole)
		HIP_TRY(c, c->tables.light_sphere.ensure(std::max<size_t>(n_lights, 1) * sizeof(float4)));
		HIP_TRY(c, c->tables.light_emit.ensure(std::max<size_t>(n_lights, 1) * sizeof(float4)));
		if (n_lights) {
			hipLaunchKernelGGL(k_light_scatter, dim3(n_blocks), dim3(kLightBlock), 0, c->stream, geo, n, mask, totals, c->tables.mat_emission.as<float4>(),
			                   c->tables.light_sphere.as<float4>(), c->tables.light_emit.as<float4>(), n_lights);
			HIP_TRY(c, hipGetLastError());
		}
	}
	// the ids and the rows, as mirt_update_spheres' patch_lights wants them
	std::vector<float4> emit(n_lights);
	c->tables.light_sphere_host.resize(n_lights);
	c->tables.light_ids.resize(n_lights);
	if (n_lights) {
		HIP_TRY(c, hipMemcpyAsync(emit.data(), c->tables.light_emit.ptr, static_cast<size_t>(n_lights) * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(c, hipMemcpyAsync(c->tables.light_sphere_host.data(), c->tables.light_sphere.ptr, static_cast<size_t>(n_lights) * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream));
	}
	for (uint32_t l = 0; l < n_lights; l++) std::memcpy(&c->tables.light_ids[l], &emit[l].w, 4);
	s.light_sphere = c->tables.light_sphere.as<float4>(); s.light_emit = c->tables.light_emit.as<float4>();
	s.n_lights = n_lights;                                                         // fp.n_lights, fp.mis and the sky's light number follow per launch
	return MIRT_OK;
}
} // namespace

int launch_update_materials(mirt_ctx* c, uint32_t n_assign, const uint32_t* bvh_index, const uint32_t* geometry_index, const int32_t* material_ID) {
	SceneDev& s = c->scene;
	// the re-assigned spheres, in both orders
	if (n_assign) {
		const size_t words = static_cast<size_t>(n_assign);
		HIP_TRY(c, c->tables.refit_edits.ensure(3u * words * 4u));
		uint32_t* d_bvh = c->tables.refit_edits.as<uint32_t>();
		uint32_t* d_geo = d_bvh + words;
		int32_t* d_mat = reinterpret_cast<int32_t*>(d_geo + words);
		HIP_TRY(c, hipMemcpyAsync(d_bvh, bvh_index, words * 4u, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipMemcpyAsync(d_geo, geometry_index, words * 4u, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipMemcpyAsync(d_mat, material_ID, words * 4u, hipMemcpyHostToDevice, c->stream));
		hipLaunchKernelGGL(k_assign_materials, dim3((n_assign + kLightBlock - 1u) / kLightBlock), dim3(kLightBlock), 0, c->stream, n_assign, d_bvh, d_geo, d_mat,
		                   c->tables.prim_mat.as<int32_t>(), GeometryTable{ c->tables.geo_sphere.as<float4>(), c->tables.geo_mat.as<int32_t>() }, s.n_spheres);
		HIP_TRY(c, hipGetLastError());
	}
	return regenerate_lights(c);
}

// mirt_set_sun_sky: the map is written where it is read (sun_sky.hpp k_sun_sky).
hipError_t bake_sun_sky(mirt_ctx* c, const mirt_sun_sky::Args& a, size_t n_texels, float4* dst) {
	hipLaunchKernelGGL(k_sun_sky, dim3(static_cast<uint32_t>((n_texels + kSunSkyBlock - 1u) / kSunSkyBlock)), dim3(kSunSkyBlock), 0, c->stream, a, dst);
	return hipGetLastError();
}

extern "C" {

int mirt_debug_lights(mirt_ctx* c, int32_t* ids_out, float* sphere_rows_out, float* emit_rows_out, size_t capacity_lights, uint32_t info[4]) {
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


} // extern "C"
