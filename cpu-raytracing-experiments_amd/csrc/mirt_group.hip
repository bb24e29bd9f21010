// mirt_group.hip — multi-GPU inside the library (include/mirt.h, "mirt_group_*").
//
// The reference host is ONE C++ object: `Renderer<> renderer{scene}` (Application.cpp:514) whose Accumulate() is a
// parallel_for over the 16x16 tiles (Renderer.hpp:75).  A group stands for that object on n GPUs of one node:
//   * one mirt_ctx per device, each with the whole scene (a few MB) and its share of the tile ROWS, interleaved: member i renders
//     tile rows i, i+n, i+2n, ... (every GPU sees sky and ground alike; contiguous stripes differ by 1.5x in cost);
//   * no exchange while rendering: tiles are independent and every random draw is keyed on the global LaunchIndex
//     (Renderer.hpp:107,117), so the union of the members' accumulators is the single-GPU accumulator bit for bit;
//   * ONE gather of the accumulator slabs to the first device — RCCL point-to-point (a grouped ncclSend / ncclRecv per peer,
//     i.e. ncclGather) over xGMI, one link per peer — followed by a device-side un-interleave into the full-image
//     AccumulationTile layout, where Render() resolves the whole frame.
// librccl is loaded on first use (dlopen), so single-GPU users of libmirt.so do not pay for it.  Members that name the SAME
// device (a rehearsal on a one-GPU box; RCCL refuses two ranks on one device) exchange their slabs with plain device copies.
// Everything else here goes through the public C-ABI of the contexts.
#include "../../include/mirt.h"
#include "noise_host.hpp"
#include "tile_map.hpp"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <dlfcn.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

struct Rccl {
	void* lib = nullptr;
	ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
	ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
	ncclResult_t (*GroupStart)() = nullptr;
	ncclResult_t (*GroupEnd)() = nullptr;
	ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
	ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
	const char* (*GetErrorString)(ncclResult_t) = nullptr;
	std::string load() {
		if (lib) return "";
		for (const char* name : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so" }) { lib = dlopen(name, RTLD_NOW | RTLD_LOCAL); if (lib) break; }
		if (!lib) return std::string("cannot load librccl: ") + dlerror();
		auto sym = [&](const char* n) { return dlsym(lib, n); };
		CommInitAll = reinterpret_cast<decltype(CommInitAll)>(sym("ncclCommInitAll"));
		CommDestroy = reinterpret_cast<decltype(CommDestroy)>(sym("ncclCommDestroy"));
		GroupStart = reinterpret_cast<decltype(GroupStart)>(sym("ncclGroupStart"));
		GroupEnd = reinterpret_cast<decltype(GroupEnd)>(sym("ncclGroupEnd"));
		Send = reinterpret_cast<decltype(Send)>(sym("ncclSend"));
		Recv = reinterpret_cast<decltype(Recv)>(sym("ncclRecv"));
		GetErrorString = reinterpret_cast<decltype(GetErrorString)>(sym("ncclGetErrorString"));
		if (!CommInitAll || !CommDestroy || !GroupStart || !GroupEnd || !Send || !Recv || !GetErrorString) { dlclose(lib); lib = nullptr; return "librccl lacks a required symbol"; }
		return "";
	}
};
Rccl g_rccl;
thread_local std::string g_group_create_error;

// Member r's slab holds its tile rows r, r+n, ... in ascending order: local row j is tile row r + j*n of the image.
// One thread per float4 of the slab; a tile row is h_tiles * buckets * 3 * 256 floats in both layouts (AOV slabs: h_tiles * 7 * 256).
__global__ __launch_bounds__(256) void k_uninterleave(float4* __restrict__ full, const float4* __restrict__ slab, size_t quads_per_row, uint32_t rows, uint32_t member, uint32_t n_members) {
	const size_t total = quads_per_row * rows;
	for (size_t q = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; q < total; q += static_cast<size_t>(gridDim.x) * 256) {
		const size_t j = q / quads_per_row, within = q - j * quads_per_row;
		full[(member + j * n_members) * quads_per_row + within] = slab[q];
	}
}

} // namespace

struct mirt_group {
	std::vector<int> devices;
	std::vector<mirt_ctx*> members;
	mirt_ctx* full = nullptr;              // on devices[0]: the gathered full-image accumulator and its Render()
	std::vector<ncclComm_t> comms;         // one per member, distinct devices only
	bool distinct = true;                  // every member on a device of its own (RCCL); otherwise plain device copies
	std::vector<void*> staging;            // on devices[0]: where member r's slab lands (r >= 1)
	std::vector<size_t> staging_bytes;
	std::vector<void*> aov_staging;        // likewise for the members' AOV slabs (mirt_group_set_aov)
	std::vector<size_t> aov_staging_bytes;
	uint32_t aov = 0;
	uint32_t width = 0, height = 0, buckets = 5;
	bool gathered = false;                 // `full` holds the members' current accumulators
	double last_gather_ms = 0.0;
	std::string error;
};

namespace {

int gfail(mirt_group* g, int code, const char* fmt, ...) {
	char buf[512];
	va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
	if (g) g->error = buf; else g_group_create_error = buf;
	return code;
}
// Runs `call` on every member; the first failure is reported with the member's own error text.
#define FOR_MEMBERS(g, what, call) do { for (size_t _i = 0; _i < (g)->members.size(); _i++) { mirt_ctx* ctx = (g)->members[_i]; const int _rc = (call); \
	if (_rc < 0) return gfail((g), _rc, "%s on member %zu (device %d): %s", (what), _i, (g)->devices[_i], mirt_last_error(ctx)); } } while (0)
#define FULL_TRY(g, what, call) do { const int _rc = (call); if (_rc < 0) return gfail((g), _rc, "%s on the gather context: %s", (what), mirt_last_error((g)->full)); } while (0)
// Runs `call` on every member, then on the gather context if the group has one.
#define FOR_MEMBERS_AND_FULL(g, what, call) do { FOR_MEMBERS(g, what, call); if ((g)->full) { mirt_ctx* ctx = (g)->full; FULL_TRY(g, what, call); } } while (0)
// An entry point that does nothing but that: mirt_group_<name> with the parameter list `params` runs mirt_<name> with `args` (ctx = the context).
#define GROUP_FORWARD(name, params, args) int mirt_group_##name params { if (!g) return MIRT_ERR_ARG; FOR_MEMBERS_AND_FULL(g, "mirt_" #name, mirt_##name args); return MIRT_OK; }
// A group of one is its member: `call` on it is the whole entry point, and the member's error text the group's.
#define RETURN_IF_SINGLE(g, call) do { if ((g)->members.size() == 1) { mirt_ctx* ctx = (g)->members[0]; const int _rc = (call); return _rc < 0 ? gfail((g), _rc, "%s", mirt_last_error(ctx)) : _rc; } } while (0)
#define GHIP(g, expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return gfail((g), MIRT_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); } while (0)
#define GNCCL(g, expr) do { ncclResult_t _r = (expr); if (_r != ncclSuccess) return gfail((g), MIRT_ERR_HIP, "%s: %s", #expr, g_rccl.GetErrorString(_r)); } while (0)
// Per-tile values between the image's LaunchIndex order and member i's local order: its local tile row j is tile row i + j * n of the image
// (mirt_group_resize), h_tiles tiles each — the split the tile records of mirt_group_noise use.
template <class T> void rows_to_member(const T* image, T* local, uint32_t h_tiles, uint32_t rows, uint32_t i, uint32_t n, uint32_t per_tile = 1) {
	for (uint32_t j = 0; j < rows; j++) std::memcpy(local + static_cast<size_t>(j) * h_tiles * per_tile, image + static_cast<size_t>(i + j * n) * h_tiles * per_tile, static_cast<size_t>(h_tiles) * per_tile * sizeof(T));
}
template <class T> void rows_to_image(const T* local, T* image, uint32_t h_tiles, uint32_t rows, uint32_t i, uint32_t n, uint32_t per_tile = 1) {
	for (uint32_t j = 0; j < rows; j++) std::memcpy(image + static_cast<size_t>(i + j * n) * h_tiles * per_tile, local + static_cast<size_t>(j) * h_tiles * per_tile, static_cast<size_t>(h_tiles) * per_tile * sizeof(T));
}
// One per-tile read-out of every member, un-interleaved into LaunchIndex order.
template <class T, class Call> int per_tile_read(mirt_group* g, T* out, size_t capacity, const char* what, Call call) {
	const uint32_t n = static_cast<uint32_t>(g->members.size()), h_tiles = g->width / MIRT_TILE_ROOT, v_tiles = g->height / MIRT_TILE_ROOT;
	if (!out || capacity < static_cast<size_t>(h_tiles) * v_tiles) return gfail(g, MIRT_ERR_ARG, "%s: room for %zu tiles, the image has %zu", what, capacity, static_cast<size_t>(h_tiles) * v_tiles);
	std::vector<T> local;
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t rows = mirt::TileMap::tile_rows_owned(v_tiles, i, n);
		local.assign(static_cast<size_t>(rows) * h_tiles + 1, T(0));
		const int rc = call(g->members[i], local.data(), static_cast<size_t>(rows) * h_tiles);
		if (rc != MIRT_OK) return gfail(g, rc < 0 ? rc : MIRT_ERR_STATE, "%s on member %u (device %d): %s", what, i, g->devices[i], rc < 0 ? mirt_last_error(g->members[i]) : "not ready");
		rows_to_image(local.data(), out, h_tiles, rows, i, n);
	}
	return MIRT_OK;
}
uint32_t accumulations_of(const mirt_group* g) { uint32_t acc = 0; (void)mirt_get_accumulations(g->members[0], &acc); return acc; }   // every member holds the same count

} // namespace

extern "C" {

const char* mirt_group_last_error(const mirt_group* g) { return g ? g->error.c_str() : g_group_create_error.c_str(); }

int mirt_group_create(const int* devices, int n, mirt_group** out) {
	if (!out) return gfail(nullptr, MIRT_ERR_ARG, "out is NULL");
	*out = nullptr;
	if (!devices || n < 1 || n > 64) return gfail(nullptr, MIRT_ERR_ARG, "need 1..64 devices");
	mirt_group* g = new mirt_group();
	g->devices.assign(devices, devices + n);
	for (int i = 0; i < n; i++) for (int j = 0; j < i; j++) if (devices[i] == devices[j]) g->distinct = false;
	auto bail = [&](int rc, const std::string& why) { g_group_create_error = why; for (mirt_ctx* c : g->members) mirt_destroy(c); if (g->full) mirt_destroy(g->full); delete g; return rc; };
	for (int i = 0; i < n; i++) {
		mirt_ctx* c = nullptr;
		const int rc = mirt_create(devices[i], &c);
		if (rc != MIRT_OK) return bail(rc, std::string("mirt_create(device ") + std::to_string(devices[i]) + "): " + mirt_last_error(nullptr));
		g->members.push_back(c);
	}
	if (n > 1) {
		const int rc = mirt_create(devices[0], &g->full);
		if (rc != MIRT_OK) return bail(rc, std::string("mirt_create(gather context): ") + mirt_last_error(nullptr));
		(void)mirt_set_motion_geometry(g->full, g->members[0]);                   // the gather context holds no geometry: its id map (mirt_set_sphere_motion) is made from the first member's, on the same device
		g->staging.assign(n, nullptr); g->staging_bytes.assign(n, 0);
		g->aov_staging.assign(n, nullptr); g->aov_staging_bytes.assign(n, 0);
		if (g->distinct) {
			const std::string why = g_rccl.load();
			if (!why.empty()) return bail(MIRT_ERR_HIP, why);
			g->comms.assign(n, nullptr);
			const ncclResult_t r = g_rccl.CommInitAll(g->comms.data(), n, devices);      // rccl.h:236 — one communicator per device, this process drives them all
			if (r != ncclSuccess) { g->comms.clear(); return bail(MIRT_ERR_HIP, std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(r)); }
		}
	}
	*out = g;
	return MIRT_OK;
}

int mirt_group_destroy(mirt_group* g) {
	if (!g) return MIRT_ERR_ARG;
	for (ncclComm_t c : g->comms) if (c) (void)g_rccl.CommDestroy(c);
	if (!g->staging.empty()) { (void)hipSetDevice(g->devices[0]); for (void* p : g->staging) if (p) (void)hipFree(p); for (void* p : g->aov_staging) if (p) (void)hipFree(p); }
	for (mirt_ctx* c : g->members) mirt_destroy(c);
	if (g->full) mirt_destroy(g->full);
	delete g;
	return MIRT_OK;
}

int mirt_group_size(const mirt_group* g, int* n) { if (!g || !n) return MIRT_ERR_ARG; *n = static_cast<int>(g->members.size()); return MIRT_OK; }
int mirt_group_member(mirt_group* g, int index, mirt_ctx** ctx) {
	if (!g || !ctx || index < 0 || index >= static_cast<int>(g->members.size())) return MIRT_ERR_ARG;
	*ctx = g->members[index];
	return MIRT_OK;
}

int mirt_group_set_scene(mirt_group* g, const mirt_sphere* geometry, const mirt_sphere* bvh_prims, uint32_t n_spheres, const mirt_bvh_node* nodes, uint32_t n_nodes,
                         const mirt_material* materials, uint32_t n_materials, const int32_t* lights, uint32_t n_lights,
                         const float ambient_color[3], const float* hdri_rgba, uint32_t hdri_w, uint32_t hdri_h) {
	if (!g) return MIRT_ERR_ARG;
	FOR_MEMBERS(g, "mirt_set_scene", mirt_set_scene(ctx, geometry, bvh_prims, n_spheres, nodes, n_nodes, materials, n_materials, lights, n_lights, ambient_color, hdri_rgba, hdri_w, hdri_h));
	// the gather context only resolves frames, but mirt_render wants a scene: the sky and materials are tiny, the geometry is not needed
	if (g->full) FULL_TRY(g, "mirt_set_scene", mirt_set_scene(g->full, nullptr, nullptr, 0, nullptr, 0, materials, n_materials, nullptr, 0, ambient_color, hdri_rgba, hdri_w, hdri_h));
	return MIRT_OK;
}
GROUP_FORWARD(set_camera, (mirt_group* g, const float pos[3], const float orient_xyzw[4], float half_width, float half_height, float z, float exposure), (ctx, pos, orient_xyzw, half_width, half_height, z, exposure))
GROUP_FORWARD(set_gloss_decay, (mirt_group* g, const float* decay, uint32_t n), (ctx, decay, n))
GROUP_FORWARD(set_stream_order, (mirt_group* g, uint32_t exact), (ctx, exact))
GROUP_FORWARD(set_lens, (mirt_group* g, float aperture_radius, float focus_depth), (ctx, aperture_radius, focus_depth))
GROUP_FORWARD(set_light_ris, (mirt_group* g, uint32_t candidates), (ctx, candidates))
GROUP_FORWARD(set_transmission, (mirt_group* g, uint32_t on), (ctx, on))
GROUP_FORWARD(set_sky_sampling, (mirt_group* g, uint32_t on), (ctx, on))                         // every member builds its own table, word for word the same (a fixed summation order)
GROUP_FORWARD(set_ggx_pdf, (mirt_group* g, uint32_t on), (ctx, on))
GROUP_FORWARD(set_environment, (mirt_group* g, const float ambient_color[3], const float* hdri_rgba, uint32_t w, uint32_t h), (ctx, ambient_color, hdri_rgba, w, h))
GROUP_FORWARD(set_sun_sky, (mirt_group* g, const mirt_sun_sky_params* params), (ctx, params))     // every member bakes its own map, word for word the same (a fixed order, no atomics)
// The members only: the gather context was handed a scene without geometry (mirt_group_set_scene), so there is nothing of it to move.
int mirt_group_update_spheres(mirt_group* g, uint32_t n, const uint32_t* bvh_index, const uint32_t* geometry_index, const float* xyz_rsq) {
	if (!g) return MIRT_ERR_ARG;
	FOR_MEMBERS(g, "mirt_update_spheres", mirt_update_spheres(ctx, n, bvh_index, geometry_index, xyz_rsq));
	uint32_t motion = 0;
	if (g->full) (void)mirt_get_sphere_motion(g->full, &motion);
	if (g->full && n && !motion) FULL_TRY(g, "mirt_drop_history", mirt_drop_history(g->full));   // its history shows the surfaces where they were (mirt_set_sphere_motion: it follows them)
	return MIRT_OK;
}
// Every member, and the material rows on the gather context too: mirt_group_set_scene handed it the material tables (its first-hit AOV colour
// and its glass check read them) but no geometry, so there is no sphere of its to re-assign.
int mirt_group_update_materials(mirt_group* g, uint32_t n_rows, const uint32_t* material_index, const mirt_material* rows,
                                uint32_t n_assign, const uint32_t* bvh_index, const uint32_t* geometry_index, const int32_t* material_ID) {
	if (!g) return MIRT_ERR_ARG;
	FOR_MEMBERS(g, "mirt_update_materials", mirt_update_materials(ctx, n_rows, material_index, rows, n_assign, bvh_index, geometry_index, material_ID));
	if (g->full && n_rows) FULL_TRY(g, "mirt_update_materials", mirt_update_materials(g->full, n_rows, material_index, rows, 0, nullptr, nullptr, nullptr));
	return MIRT_OK;
}
GROUP_FORWARD(set_material_closures,(mirt_group* g, const uint8_t* closure, uint32_t n), (ctx, closure, n))   // the gather context too: its first-hit AOV colour follows the table
int mirt_group_pick_focus(mirt_group* g, uint32_t x, uint32_t y, float* distance, float* depth) {
	if (!g) return MIRT_ERR_ARG;
	mirt_ctx* ctx = g->members[0];                                                   // one ray: every member holds the whole scene
	const int rc = mirt_pick_focus(ctx, x, y, distance, depth);
	if (rc < 0) return gfail(g, rc, "mirt_pick_focus on member 0 (device %d): %s", g->devices[0], mirt_last_error(ctx));
	return rc;
}
int mirt_group_set_aov(mirt_group* g, uint32_t on) {
	if (!g) return MIRT_ERR_ARG;
	FOR_MEMBERS(g, "mirt_set_aov", mirt_set_aov(ctx, on));
	if (g->full) {
		// the gather context counts the accumulations of the last gather; the members (accepted above) hold none, so neither does it any more
		if (on) FULL_TRY(g, "mirt_reset", mirt_reset(g->full));
		FULL_TRY(g, "mirt_set_aov", mirt_set_aov(g->full, on));
	}
	g->aov = on;
	g->gathered = false;
	return MIRT_OK;
}
int mirt_group_set_policy(mirt_group* g, const mirt_policy* p) {
	if (!g || !p) return MIRT_ERR_ARG;
	FOR_MEMBERS_AND_FULL(g, "mirt_set_policy", mirt_set_policy(ctx, p));
	g->buckets = p->buckets;
	g->gathered = false;
	return MIRT_OK;
}
int mirt_group_resize(mirt_group* g, uint32_t width, uint32_t height) {
	if (!g) return MIRT_ERR_ARG;
	const uint32_t n = static_cast<uint32_t>(g->members.size());
	FOR_MEMBERS(g, "mirt_resize", mirt_resize(ctx, width, height));
	if (n > 1) {
		for (uint32_t i = 0; i < n; i++) {
			const int rc = mirt_set_tile_rows(g->members[i], i, n);                   // Renderer.hpp:75: the parallel_for range, split by tile row
			if (rc < 0) return gfail(g, rc, "mirt_set_tile_rows on member %u: %s", i, mirt_last_error(g->members[i]));
		}
		FULL_TRY(g, "mirt_resize", mirt_resize(g->full, width, height));
	}
	g->width = width; g->height = height; g->gathered = false;
	return MIRT_OK;
}
int mirt_group_reset(mirt_group* g) {
	if (!g) return MIRT_ERR_ARG;
	FOR_MEMBERS(g, "mirt_reset", mirt_reset(ctx));
	g->gathered = false;
	return MIRT_OK;
}
int mirt_group_accumulate_async(mirt_group* g, uint32_t n_calls) {
	if (!g) return MIRT_ERR_ARG;
	FOR_MEMBERS(g, "mirt_accumulate_async", mirt_accumulate_async(ctx, n_calls));     // every device gets its launches before anyone is waited for
	g->gathered = false;
	return MIRT_OK;
}
int mirt_group_synchronize(mirt_group* g) {
	if (!g) return MIRT_ERR_ARG;
	FOR_MEMBERS(g, "mirt_synchronize", mirt_synchronize(ctx));
	return MIRT_OK;
}
int mirt_group_accumulate(mirt_group* g, uint32_t n_calls) {
	const int rc = mirt_group_accumulate_async(g, n_calls);
	return rc ? rc : mirt_group_synchronize(g);
}
int mirt_group_get_accumulations(const mirt_group* g, uint32_t* a) { if (!g || g->members.empty()) return MIRT_ERR_ARG; return mirt_get_accumulations(g->members[0], a); }

int mirt_group_get_counters(mirt_group* g, mirt_counters* out) {
	if (!g || !out) return MIRT_ERR_ARG;
	std::memset(out, 0, sizeof *out);
	for (size_t i = 0; i < g->members.size(); i++) {
		mirt_counters c{};
		const int rc = mirt_get_counters(g->members[i], &c);
		if (rc < 0) return gfail(g, rc, "mirt_get_counters on member %zu: %s", i, mirt_last_error(g->members[i]));
		out->rays += c.rays; out->shadow_rays += c.shadow_rays; out->nodes += c.nodes; out->spheres += c.spheres;
		out->shadow_nodes += c.shadow_nodes; out->shadow_spheres += c.shadow_spheres; out->terminated += c.terminated; out->dropped += c.dropped;
	}
	return MIRT_OK;
}

// The one exchange of the path: every member's slab to the first device, then the un-interleave into the full-image layout.
int mirt_group_gather(mirt_group* g) {
	if (!g) return MIRT_ERR_ARG;
	const uint32_t n = static_cast<uint32_t>(g->members.size());
	if (n == 1 || g->gathered) return MIRT_OK;
	if (g->width == 0) return gfail(g, MIRT_ERR_STATE, "mirt_group_resize has not been called");
	const uint32_t h_tiles = g->width / MIRT_TILE_ROOT, v_tiles = g->height / MIRT_TILE_ROOT;
	// What the exchange moves: the accumulator slabs and, with AOVs on, the AOV slabs — the same tile rows, another row size.
	struct Part { std::vector<void*> slab; std::vector<size_t> bytes; void* full_ptr; size_t row_bytes; std::vector<void*>* staging; std::vector<size_t>* staging_bytes; };
	std::vector<Part> parts;
	parts.push_back(Part{ std::vector<void*>(n, nullptr), std::vector<size_t>(n, 0), nullptr, static_cast<size_t>(h_tiles) * g->buckets * 3 * MIRT_TILE_SIZE * sizeof(float), &g->staging, &g->staging_bytes });
	if (g->aov) parts.push_back(Part{ std::vector<void*>(n, nullptr), std::vector<size_t>(n, 0), nullptr, static_cast<size_t>(h_tiles) * MIRT_AOV_PLANES * MIRT_TILE_SIZE * sizeof(float), &g->aov_staging, &g->aov_staging_bytes });
	std::vector<void*> stream(n, nullptr);
	for (uint32_t i = 0; i < n; i++) {
		int rc = mirt_accumulator_device(g->members[i], &parts[0].slab[i], &parts[0].bytes[i]);   // launches anything deferred and waits for the member's GPU
		if (rc >= 0 && g->aov) rc = mirt_aov_device(g->members[i], &parts[1].slab[i], &parts[1].bytes[i]);
		if (rc >= 0) rc = mirt_get_stream(g->members[i], &stream[i]);
		if (rc < 0) return gfail(g, rc, "accumulator of member %u: %s", i, mirt_last_error(g->members[i]));
	}
	size_t full_bytes = 0; void* full_stream = nullptr;
	FULL_TRY(g, "mirt_accumulator_device", mirt_accumulator_device(g->full, &parts[0].full_ptr, &full_bytes));
	if (full_bytes != parts[0].row_bytes * v_tiles) return gfail(g, MIRT_ERR_STATE, "gather context holds %zu bytes, the image needs %zu", full_bytes, parts[0].row_bytes * v_tiles);
	if (g->aov) {
		FULL_TRY(g, "mirt_aov_device", mirt_aov_device(g->full, &parts[1].full_ptr, &full_bytes));
		if (full_bytes != parts[1].row_bytes * v_tiles) return gfail(g, MIRT_ERR_STATE, "gather context holds %zu bytes of AOVs, the image needs %zu", full_bytes, parts[1].row_bytes * v_tiles);
	}
	FULL_TRY(g, "mirt_get_stream", mirt_get_stream(g->full, &full_stream));
	GHIP(g, hipSetDevice(g->devices[0]));
	for (Part& p : parts) for (uint32_t i = 1; i < n; i++) if ((*p.staging_bytes)[i] < p.bytes[i]) {
		if ((*p.staging)[i]) (void)hipFree((*p.staging)[i]);
		(*p.staging)[i] = nullptr; (*p.staging_bytes)[i] = 0;
		if (p.bytes[i]) { GHIP(g, hipMalloc(&(*p.staging)[i], p.bytes[i])); (*p.staging_bytes)[i] = p.bytes[i]; }
	}
	// From here on every failure is recorded in `rc` and the sequence runs to its end: an ncclGroupStart is always matched by its
	// ncclGroupEnd and both events are destroyed whatever happened in between.
	int rc = MIRT_OK;
	auto hstep = [&](hipError_t e, const char* what) { if (rc == MIRT_OK && e != hipSuccess) rc = gfail(g, MIRT_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); return rc == MIRT_OK; };
	auto nstep = [&](ncclResult_t r, const char* what) { if (rc == MIRT_OK && r != ncclSuccess) rc = gfail(g, MIRT_ERR_HIP, "%s: %s", what, g_rccl.GetErrorString(r)); return rc == MIRT_OK; };
	hipEvent_t t0 = nullptr, t1 = nullptr;
	hipStream_t root = static_cast<hipStream_t>(full_stream);
	hstep(hipEventCreate(&t0), "hipEventCreate"); hstep(hipEventCreate(&t1), "hipEventCreate");
	if (rc == MIRT_OK) hstep(hipEventRecord(t0, root), "hipEventRecord");
	if (rc == MIRT_OK && g->distinct) {
		// ncclGather spelled as its point-to-point form (rccl.h:700,722): the root posts one receive per peer and slab, every peer one send
		// per slab, in the same order on both sides; each transfer rides the xGMI link between that peer and the root
		if (nstep(g_rccl.GroupStart(), "ncclGroupStart")) {
			for (uint32_t i = 1; i < n && rc == MIRT_OK; i++) for (const Part& p : parts) {
				if (!p.bytes[i] || rc != MIRT_OK) continue;
				if (hstep(hipSetDevice(g->devices[0]), "hipSetDevice"))
					nstep(g_rccl.Recv((*p.staging)[i], p.bytes[i] / sizeof(float), ncclFloat, static_cast<int>(i), g->comms[0], root), "ncclRecv");
				if (rc == MIRT_OK && hstep(hipSetDevice(g->devices[i]), "hipSetDevice"))
					nstep(g_rccl.Send(p.slab[i], p.bytes[i] / sizeof(float), ncclFloat, 0, g->comms[i], static_cast<hipStream_t>(stream[i])), "ncclSend");
			}
			const ncclResult_t end = g_rccl.GroupEnd();                              // always: an open group would swallow every later RCCL call of this thread
			nstep(end, "ncclGroupEnd");
		}
		for (uint32_t i = 1; i < n && rc == MIRT_OK; i++) if (hstep(hipSetDevice(g->devices[i]), "hipSetDevice")) hstep(hipStreamSynchronize(static_cast<hipStream_t>(stream[i])), "hipStreamSynchronize");
		(void)hipSetDevice(g->devices[0]);
	} else if (rc == MIRT_OK) {
		for (const Part& p : parts) for (uint32_t i = 1; i < n && rc == MIRT_OK; i++) if (p.bytes[i]) hstep(hipMemcpyAsync((*p.staging)[i], p.slab[i], p.bytes[i], hipMemcpyDeviceToDevice, root), "hipMemcpyAsync");
	}
	for (const Part& p : parts) {
		const size_t quads_per_row = p.row_bytes / sizeof(float4);
		for (uint32_t i = 0; i < n && rc == MIRT_OK; i++) {
			const uint32_t rows = static_cast<uint32_t>(p.bytes[i] / p.row_bytes);
			if (!rows) continue;
			const float4* src = static_cast<const float4*>(i == 0 ? p.slab[0] : (*p.staging)[i]);
			const size_t total = quads_per_row * rows;
			const uint32_t grid = static_cast<uint32_t>(std::min<size_t>((total + 255) / 256, 256u * 16u));
			hipLaunchKernelGGL(k_uninterleave, dim3(grid), dim3(256), 0, root, static_cast<float4*>(p.full_ptr), src, quads_per_row, rows, i, n);
		}
	}
	if (rc == MIRT_OK) hstep(hipGetLastError(), "k_uninterleave");
	if (rc == MIRT_OK) hstep(hipEventRecord(t1, root), "hipEventRecord");
	if (rc == MIRT_OK) hstep(hipStreamSynchronize(root), "hipStreamSynchronize");
	if (rc == MIRT_OK) { float ms = 0.0f; (void)hipEventElapsedTime(&ms, t0, t1); g->last_gather_ms = ms; }
	if (t0) (void)hipEventDestroy(t0);
	if (t1) (void)hipEventDestroy(t1);
	if (rc != MIRT_OK) return rc;
	FULL_TRY(g, "mirt_load_accumulator", mirt_load_accumulator(g->full, static_cast<const float*>(parts[0].full_ptr), 1, accumulations_of(g)));   // in place: only `accumulations` changes
	{	// the members' per-tile counts (mirt_freeze_tiles), so that the gather context resolves every tile at its own count; nothing to load while no tile is behind
		std::vector<uint32_t> counts(static_cast<size_t>(h_tiles) * v_tiles);
		const int cr = mirt_group_tile_counts(g, counts.data(), counts.size());
		if (cr < 0) return cr;
		bool behind = false;
		for (uint32_t c : counts) behind = behind || c != accumulations_of(g);
		if (behind) FULL_TRY(g, "mirt_load_tile_counts", mirt_load_tile_counts(g->full, counts.data(), counts.size()));
	}
	g->gathered = true;
	return MIRT_OK;
}
// The noise estimate of the whole image without a gather: every member reads its own slab (mirt_noise); what comes back is small (16 B per
// tile, 8 KB of histogram) and is merged here on the host.
int mirt_group_noise(mirt_group* g, float floor, float* map_out, float* tile_out, uint32_t* hist_out, mirt_noise_stats* stats) {
	if (!g) return MIRT_ERR_ARG;
	const uint32_t n = static_cast<uint32_t>(g->members.size());
	RETURN_IF_SINGLE(g, mirt_noise(ctx, floor, map_out, tile_out, hist_out, stats));
	char why[256];
	if (const int bad = mirt_noise_host::check_noise_args(floor, g->buckets, why, sizeof why)) return gfail(g, bad, "%s", why);
	if (g->width == 0) return gfail(g, MIRT_ERR_STATE, "mirt_group_resize has not been called");
	uint32_t acc = 0;
	{ const int rc = mirt_get_accumulations(g->members[0], &acc); if (rc < 0) return gfail(g, rc, "mirt_get_accumulations on member 0 failed"); }
	if (acc == 0 || acc % g->buckets != 0) return MIRT_NOT_READY;                          // before any member is asked: every output untouched
	const uint32_t h_tiles = g->width / MIRT_TILE_ROOT, v_tiles = g->height / MIRT_TILE_ROOT;
	std::vector<float> rec(static_cast<size_t>(h_tiles) * v_tiles * 4, 0.0f), part;
	std::vector<uint32_t> hist(MIRT_NOISE_BINS, 0u), part_hist(MIRT_NOISE_BINS);
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t rows = mirt::TileMap::tile_rows_owned(v_tiles, i, n);               // member i renders tile rows i, i + n, ... (mirt_group_resize)
		part.assign(static_cast<size_t>(rows) * h_tiles * 4, 0.0f);
		const int rc = mirt_noise(g->members[i], floor, map_out, part.data(), part_hist.data(), nullptr);   // writes its own tiles of map_out
		if (rc != MIRT_OK) return gfail(g, rc < 0 ? rc : MIRT_ERR_STATE, "mirt_noise on member %u (device %d): %s", i, g->devices[i], rc < 0 ? mirt_last_error(g->members[i]) : "not ready");
		for (uint32_t j = 0; j < rows; j++)                                                 // its local tile row j is tile row i + j * n of the image
			std::memcpy(&rec[static_cast<size_t>(i + j * n) * h_tiles * 4], &part[static_cast<size_t>(j) * h_tiles * 4], static_cast<size_t>(h_tiles) * 4 * sizeof(float));
		for (uint32_t b = 0; b < MIRT_NOISE_BINS; b++) hist[b] += part_hist[b];
	}
	if (tile_out && !rec.empty()) std::memcpy(tile_out, rec.data(), rec.size() * sizeof(float));
	if (hist_out) std::memcpy(hist_out, hist.data(), MIRT_NOISE_BINS * sizeof(uint32_t));
	if (stats) mirt_noise_host::stats_from_tiles(rec.data(), static_cast<size_t>(h_tiles) * v_tiles, stats);
	return MIRT_OK;
}
int mirt_group_accumulate_until(mirt_group* g, const mirt_stop_rule* rule, mirt_noise_stats* last, uint32_t* issued) {
	if (!g) return MIRT_ERR_ARG;
	RETURN_IF_SINGLE(g, mirt_accumulate_until(ctx, rule, last, issued));
	const uint32_t k = g->buckets;
	uint32_t acc = 0;
	{ const int rc = mirt_get_accumulations(g->members[0], &acc); if (rc < 0) return gfail(g, rc, "mirt_get_accumulations on member 0 failed"); }
	char why[256];
	if (const int bad = mirt_noise_host::check_stop_rule(rule, k, acc, why, sizeof why)) return gfail(g, bad, "%s", why);
	std::vector<uint32_t> hist(MIRT_NOISE_BINS);
	return mirt_noise_host::accumulate_until(rule, k,
		[&](uint32_t* a) { return mirt_group_get_accumulations(g, a); },
		[&](uint32_t c) { return mirt_group_accumulate(g, c); },
		[&](float floor, uint32_t* h, mirt_noise_stats* st) { return mirt_group_noise(g, floor, nullptr, nullptr, h, st); },
		[&](int code, const char* text) { return gfail(g, code, "%s", text); },
		last, issued, hist.data());
}
// ---- per-tile adaptive sampling: masks and counts in LaunchIndex order, split and un-interleaved on the host; no gather ----
int mirt_group_freeze_tiles(mirt_group* g, const uint8_t* freeze, size_t n_tiles) {
	if (!g) return MIRT_ERR_ARG;
	RETURN_IF_SINGLE(g, mirt_freeze_tiles(ctx, freeze, n_tiles));
	const uint32_t n = static_cast<uint32_t>(g->members.size()), h_tiles = g->width / MIRT_TILE_ROOT, v_tiles = g->height / MIRT_TILE_ROOT;
	if (n_tiles != static_cast<size_t>(h_tiles) * v_tiles || (!freeze && n_tiles)) return gfail(g, MIRT_ERR_ARG, "freeze_tiles: a mask of %zu tiles, the image has %zu", n_tiles, static_cast<size_t>(h_tiles) * v_tiles);
	const uint32_t acc = accumulations_of(g);
	if (acc == 0 || acc % g->buckets != 0) return gfail(g, MIRT_ERR_STATE, "%u accumulations so far: tiles freeze at a positive multiple of buckets (%u)", acc, g->buckets);   // before any member is asked
	std::vector<uint8_t> local;
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t rows = mirt::TileMap::tile_rows_owned(v_tiles, i, n);
		local.assign(static_cast<size_t>(rows) * h_tiles + 1, 0);
		rows_to_member(freeze, local.data(), h_tiles, rows, i, n);
		const int rc = mirt_freeze_tiles(g->members[i], local.data(), static_cast<size_t>(rows) * h_tiles);
		if (rc < 0) return gfail(g, rc, "mirt_freeze_tiles on member %u (device %d): %s", i, g->devices[i], mirt_last_error(g->members[i]));
	}
	g->gathered = false;                                                             // the gather context's counts are stale
	return MIRT_OK;
}
int mirt_group_tile_counts(mirt_group* g, uint32_t* counts_out, size_t capacity) {
	if (!g) return MIRT_ERR_ARG;
	RETURN_IF_SINGLE(g, mirt_tile_counts(ctx, counts_out, capacity));
	return per_tile_read(g, counts_out, capacity, "mirt_tile_counts", [](mirt_ctx* c, uint32_t* o, size_t cap) { return mirt_tile_counts(c, o, cap); });
}
int mirt_group_frozen_tiles(mirt_group* g, uint8_t* mask_out, size_t capacity) {
	if (!g) return MIRT_ERR_ARG;
	RETURN_IF_SINGLE(g, mirt_frozen_tiles(ctx, mask_out, capacity));
	return per_tile_read(g, mask_out, capacity, "mirt_frozen_tiles", [](mirt_ctx* c, uint8_t* o, size_t cap) { return mirt_frozen_tiles(c, o, cap); });
}
int mirt_group_tile_above(mirt_group* g, float floor, float target, uint32_t* above_out, size_t capacity) {
	if (!g) return MIRT_ERR_ARG;
	RETURN_IF_SINGLE(g, mirt_tile_above(ctx, floor, target, above_out, capacity));
	char why[256];
	if (const int bad = mirt_noise_host::check_noise_args(floor, g->buckets, why, sizeof why)) return gfail(g, bad, "%s", why);
	if (!mirt_noise_host::finite_nonneg(target)) return gfail(g, MIRT_ERR_ARG, "target %g is not a finite value >= 0", static_cast<double>(target));
	const uint32_t acc = accumulations_of(g);
	if (acc == 0 || acc % g->buckets != 0) return MIRT_NOT_READY;                          // before any member is asked: above_out untouched
	return per_tile_read(g, above_out, capacity, "mirt_tile_above", [&](mirt_ctx* c, uint32_t* o, size_t cap) { return mirt_tile_above(c, floor, target, o, cap); });
}
int mirt_group_accumulate_adaptive(mirt_group* g, const mirt_stop_rule* rule, uint32_t min_accumulations, mirt_adaptive_report* report) {
	if (!g) return MIRT_ERR_ARG;
	RETURN_IF_SINGLE(g, mirt_accumulate_adaptive(ctx, rule, min_accumulations, report));
	char why[256];
	if (const int bad = mirt_noise_host::check_stop_rule(rule, g->buckets, accumulations_of(g), why, sizeof why)) return gfail(g, bad, "%s", why);
	const size_t n_tiles = static_cast<size_t>(g->width / MIRT_TILE_ROOT) * (g->height / MIRT_TILE_ROOT);
	return mirt_noise_host::accumulate_adaptive(rule, g->buckets, min_accumulations, n_tiles,
		[&](uint32_t* a) { return mirt_group_get_accumulations(g, a); },
		[&](uint32_t c) { return mirt_group_accumulate(g, c); },
		[&](float floor, float target, float* rec, uint32_t* above, mirt_noise_stats* st) {
			const int rc = mirt_group_noise(g, floor, nullptr, rec, nullptr, st);
			return rc != MIRT_OK ? rc : mirt_group_tile_above(g, floor, target, above, n_tiles); },
		[&](uint8_t* mask) { return mirt_group_frozen_tiles(g, mask, n_tiles); },
		[&](const uint8_t* mask) { return mirt_group_freeze_tiles(g, mask, n_tiles); },
		[&](uint32_t* counts) { return mirt_group_tile_counts(g, counts, n_tiles); },
		[&](int code, const char* text) { return gfail(g, code, "%s", text); },
		report);
}
// Diagnostic: is RCCL usable from this process?  Loads librccl, makes a one-device communicator on `device` and sends n_floats to
// itself through a grouped ncclSend / ncclRecv pair (the calls mirt_group_gather makes between distinct devices); 0 = the data arrived intact.
int mirt_group_rccl_selftest(int device, size_t n_floats) {
	const std::string why = g_rccl.load();
	if (!why.empty()) return gfail(nullptr, MIRT_ERR_HIP, "%s", why.c_str());
	if (n_floats == 0) return gfail(nullptr, MIRT_ERR_ARG, "n_floats is 0");
	GHIP(nullptr, hipSetDevice(device));
	ncclComm_t comm = nullptr;
	GNCCL(nullptr, g_rccl.CommInitAll(&comm, 1, &device));
	float *src = nullptr, *dst = nullptr;
	hipStream_t st = nullptr;
	std::vector<float> host(n_floats), back(n_floats, 0.0f);
	for (size_t i = 0; i < n_floats; i++) host[i] = static_cast<float>(i % 8191) * 0.5f;
	int rc = MIRT_OK;
	auto step = [&](hipError_t e, const char* what) { if (rc == MIRT_OK && e != hipSuccess) rc = gfail(nullptr, MIRT_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); };
	auto nstep = [&](ncclResult_t r, const char* what) { if (rc == MIRT_OK && r != ncclSuccess) rc = gfail(nullptr, MIRT_ERR_HIP, "%s: %s", what, g_rccl.GetErrorString(r)); };
	step(hipMalloc(&src, n_floats * 4), "hipMalloc"); step(hipMalloc(&dst, n_floats * 4), "hipMalloc"); step(hipStreamCreate(&st), "hipStreamCreate");
	if (rc == MIRT_OK) step(hipMemcpy(src, host.data(), n_floats * 4, hipMemcpyHostToDevice), "hipMemcpy");
	if (rc == MIRT_OK) {
		nstep(g_rccl.GroupStart(), "ncclGroupStart");
		nstep(g_rccl.Recv(dst, n_floats, ncclFloat, 0, comm, st), "ncclRecv");
		nstep(g_rccl.Send(src, n_floats, ncclFloat, 0, comm, st), "ncclSend");
		nstep(g_rccl.GroupEnd(), "ncclGroupEnd");
		step(hipStreamSynchronize(st), "hipStreamSynchronize");
	}
	if (rc == MIRT_OK) step(hipMemcpy(back.data(), dst, n_floats * 4, hipMemcpyDeviceToHost), "hipMemcpy");
	if (rc == MIRT_OK && std::memcmp(host.data(), back.data(), n_floats * 4) != 0) rc = gfail(nullptr, MIRT_ERR_HIP, "data sent through RCCL came back changed");
	if (st) (void)hipStreamDestroy(st);
	if (src) (void)hipFree(src);
	if (dst) (void)hipFree(dst);
	(void)g_rccl.CommDestroy(comm);
	return rc;
}
int mirt_group_last_gather_ms(const mirt_group* g, double* ms) { if (!g || !ms) return MIRT_ERR_ARG; *ms = g->last_gather_ms; return MIRT_OK; }

int mirt_group_accumulator_floats(const mirt_group* g, size_t* n) {
	if (!g || !n) return MIRT_ERR_ARG;
	*n = static_cast<size_t>(g->width / MIRT_TILE_ROOT) * (g->height / MIRT_TILE_ROOT) * g->buckets * 3 * MIRT_TILE_SIZE;
	return MIRT_OK;
}
int mirt_group_read_accumulator(mirt_group* g, float* host_dst) {
	if (!g || !host_dst) return MIRT_ERR_ARG;
	RETURN_IF_SINGLE(g, mirt_read_accumulator(ctx, host_dst));
	const int rc = mirt_group_gather(g);
	if (rc) return rc;
	FULL_TRY(g, "mirt_read_accumulator", mirt_read_accumulator(g->full, host_dst));
	return MIRT_OK;
}
int mirt_group_aov_floats(const mirt_group* g, size_t* n) {
	if (!g || !n) return MIRT_ERR_ARG;
	*n = g->aov ? static_cast<size_t>(g->width / MIRT_TILE_ROOT) * (g->height / MIRT_TILE_ROOT) * MIRT_AOV_PLANES * MIRT_TILE_SIZE : 0;
	return MIRT_OK;
}
int mirt_group_read_aov(mirt_group* g, float* host_dst) {
	if (!g || !host_dst) return MIRT_ERR_ARG;
	RETURN_IF_SINGLE(g, mirt_read_aov(ctx, host_dst));
	if (!g->aov) return gfail(g, MIRT_ERR_STATE, "AOVs are off (mirt_group_set_aov)");
	const int rc = mirt_group_gather(g);
	if (rc) return rc;
	FULL_TRY(g, "mirt_read_aov", mirt_read_aov(g->full, host_dst));
	return MIRT_OK;
}
int mirt_group_render_aov(mirt_group* g, int which, float* out) {
	if (!g) return MIRT_ERR_ARG;
	RETURN_IF_SINGLE(g, mirt_render_aov(ctx, which, out));
	if (!g->aov) return gfail(g, MIRT_ERR_STATE, "AOVs are off (mirt_group_set_aov)");
	if (!out) return gfail(g, MIRT_ERR_ARG, "out is NULL");
	if (accumulations_of(g) == 0) return MIRT_NOT_READY;                                             // nothing is gathered for it
	const int rc = mirt_group_gather(g);
	if (rc) return rc;
	const int rr = mirt_render_aov(g->full, which, out);
	return rr < 0 ? gfail(g, rr, "mirt_render_aov on the gather context: %s", mirt_last_error(g->full)) : rr;
}
int mirt_group_render(mirt_group* g, float* rgba_host) {
	if (!g || !rgba_host) return MIRT_ERR_ARG;
	RETURN_IF_SINGLE(g, mirt_render(ctx, rgba_host));
	const uint32_t acc = accumulations_of(g);
	if (acc == 0 || acc % g->buckets != 0) return MIRT_NOT_READY;       // Renderer.hpp:437: nothing is gathered for a frame that is not due
	const int rc = mirt_group_gather(g);
	if (rc) return rc;
	const int rr = mirt_render(g->full, rgba_host);
	return rr < 0 ? gfail(g, rr, "mirt_render on the gather context: %s", mirt_last_error(g->full)) : rr;
}
// Gathers as mirt_group_render does; the gather context then holds the accumulator, the AOV slab and the counts of the whole image.
int mirt_group_render_atrous(mirt_group* g, const mirt_denoise_params* params, float* rgba_host) {
	if (!g || !params || !rgba_host) return MIRT_ERR_ARG;
	RETURN_IF_SINGLE(g, mirt_render_atrous(ctx, params, rgba_host));
	if (!g->aov) return gfail(g, MIRT_ERR_STATE, "denoise: AOVs are off (mirt_group_set_aov)");
	if (g->buckets < 2u) return gfail(g, MIRT_ERR_STATE, "denoise: the variance guide needs buckets >= 2, the policy has %u", g->buckets);
	const uint32_t acc = accumulations_of(g);
	if (acc == 0 || acc % g->buckets != 0) return MIRT_NOT_READY;       // as mirt_group_render: nothing is gathered for a frame that is not due
	const int rc = mirt_group_gather(g);
	if (rc) return rc;
	const int rr = mirt_render_atrous(g->full, params, rgba_host);      // the argument rules are the gather context's
	return rr < 0 ? gfail(g, rr, "mirt_render_atrous on the gather context: %s", mirt_last_error(g->full)) : rr;
}
// Likewise; the history is the gather context's own state (a group of one: its member's).
int mirt_group_render_temporal(mirt_group* g, const mirt_denoise_params* params, const mirt_temporal_params* temporal, float* rgba_host, float* history_len, mirt_temporal_stats* stats) {
	if (!g || !params || !temporal || !rgba_host) return MIRT_ERR_ARG;
	RETURN_IF_SINGLE(g, mirt_render_temporal(ctx, params, temporal, rgba_host, history_len, stats));
	if (!g->aov) return gfail(g, MIRT_ERR_STATE, "temporal: AOVs are off (mirt_group_set_aov)");
	if (g->buckets < 2u) return gfail(g, MIRT_ERR_STATE, "temporal: the variance guide needs buckets >= 2, the policy has %u", g->buckets);
	const uint32_t acc = accumulations_of(g);
	if (acc == 0 || acc % g->buckets != 0) return MIRT_NOT_READY;       // as mirt_group_render: nothing is gathered for a frame that is not due
	const int rc = mirt_group_gather(g);
	if (rc) return rc;
	const int rr = mirt_render_temporal(g->full, params, temporal, rgba_host, history_len, stats);
	return rr < 0 ? gfail(g, rr, "mirt_render_temporal on the gather context: %s", mirt_last_error(g->full)) : rr;
}
int mirt_group_drop_history(mirt_group* g) {
	if (!g) return MIRT_ERR_ARG;
	mirt_ctx* ctx = g->full ? g->full : g->members[0];
	const int rc = mirt_drop_history(ctx);
	return rc < 0 ? gfail(g, rc, "mirt_drop_history: %s", mirt_last_error(ctx)) : rc;
}
int mirt_group_history_info(const mirt_group* g, uint32_t* valid, uint64_t* bytes) {
	if (!g) return MIRT_ERR_ARG;
	return mirt_history_info(g->full ? g->full : g->members[0], valid, bytes);
}
GROUP_FORWARD(set_sphere_motion, (mirt_group* g, uint32_t on), (ctx, on))
int mirt_group_id_map(mirt_group* g, int32_t* prim_out, float* distance_out) {
	if (!g) return MIRT_ERR_ARG;
	mirt_ctx* ctx = g->full ? g->full : g->members[0];                               // the context mirt_group_render_temporal resolves on
	const int rc = mirt_id_map(ctx, prim_out, distance_out);
	return rc < 0 ? gfail(g, rc, "mirt_id_map: %s", mirt_last_error(ctx)) : rc;
}

} // extern "C"
