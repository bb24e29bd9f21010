// mirt_capi.hip — the API layer of the C-ABI (include/mirt.h): every entry point that validates its arguments, edits the state of the
// context (ctx.hpp) and calls the launch layer (mirt_launch.hip).  It includes no header that defines a kernel: editing it rebuilds none.
// The entry points that read a finished accumulator are the resolve layer's (mirt_resolve.hip).
//
// Host-side stand-in for the state Renderer<Policy> keeps (Renderer.hpp:38-49): scene reference,
// accumulator, width/height, accumulations, h_tiles/v_tiles — with the scene copied to HBM, the
// accumulator resident in HBM in the reference's AccumulationTile layout, and the per-tile ray
// streams replaced by one set of frame-wide SoA streams (see kernels.hpp).
//
// There is no CPU fallback: every entry point that computes needs a gfx950 device and fails with
// MIRT_ERR_NO_DEVICE / MIRT_ERR_HIP otherwise.
#include "ctx.hpp"
#include "scene_update_host.hpp"
#include "sun_sky_host.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>

using namespace mirt;

namespace {

size_t accumulator_floats(const mirt_ctx* c) { return static_cast<size_t>(c->n_tiles) * c->policy.buckets * 3 * kTileSize; }
// What the accumulator's and the AOV slab's read_* / *_device / load_* entry points share, after their own preambles: `floats` of `slab`
// to the host, as a device pointer, or overwritten from `src` (src == the slab itself, filled in place by mirt_group_gather: nothing is copied).
int read_slab(mirt_ctx* c, const DeviceBuffer& slab, size_t floats, float* dst) {
	if (floats) HIP_TRY(c, hipMemcpy(dst, slab.ptr, floats * sizeof(float), hipMemcpyDeviceToHost));
	return MIRT_OK;
}
int slab_device(const DeviceBuffer& slab, size_t floats, void** ptr, size_t* bytes) { *ptr = slab.ptr; *bytes = floats * sizeof(float); return MIRT_OK; }
int load_slab(mirt_ctx* c, const DeviceBuffer& slab, size_t floats, const float* src, int src_is_device) {
	if (floats && src != slab.ptr) HIP_TRY(c, hipMemcpy(slab.ptr, src, floats * sizeof(float), src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
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

int alloc_accumulator(mirt_ctx* c) {
	const size_t floats = accumulator_floats(c);
	HIP_TRY(c, sync_all(c));
	HIP_TRY(c, c->accumulator.ensure(floats * sizeof(float)));
	if (floats) HIP_TRY(c, hipMemsetAsync(c->accumulator.ptr, 0, floats * sizeof(float), c->stream));
	if (c->aov_on) { const int r = alloc_aov(c); if (r) return r; }
	HIP_TRY(c, hipMemsetAsync(c->counters.ptr, 0, sizeof(DevCounters), c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	for (PipeSlot& sl : c->slots) sl.in_use = false;
	c->accumulations = 0;
	c->freeze.drop();
	return MIRT_OK;
}

// The camera's +x, +y and -z in world space, for lens_ray: binary32, the quat * vec3 formula of camera_ray_dir (device_math.hpp camera_axis).
void update_lens_axes(mirt_ctx* c) {
	const f3 r = camera_axis(c->camera.orient, f3{ 1.0f, 0.0f, 0.0f }), u = camera_axis(c->camera.orient, f3{ 0.0f, 1.0f, 0.0f }), f = camera_axis(c->camera.orient, f3{ 0.0f, 0.0f, -1.0f });
	c->lens.right[0] = r.x; c->lens.right[1] = r.y; c->lens.right[2] = r.z;
	c->lens.up[0] = u.x; c->lens.up[1] = u.y; c->lens.up[2] = u.z;
	c->lens.fwd[0] = f.x; c->lens.fwd[1] = f.y; c->lens.fwd[2] = f.z;
}
void set_tile_map(mirt_ctx* c, const TileMap& m, uint32_t n_tiles) { c->first_tile = m.first_tile; c->run_tiles = m.run_tiles; c->stride_tiles = m.stride_tiles; c->n_tiles = n_tiles; }

// ---- mirt_set_scene, step by step --------------------------------------------------------------
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

void commit_scene(mirt_ctx* c, const SceneArgs& a, const SceneRecords& t) {
	SceneDev& s = c->scene;
	s.recs = t.in_recs_wide ? c->tables.recs_wide.as<float4>() : c->tables.recs.as<float4>(); s.spheres = c->tables.spheres.as<float4>(); s.prim_mat = c->tables.prim_mat.as<int32_t>();
	s.light_sphere = c->tables.light_sphere.as<float4>(); s.light_emit = c->tables.light_emit.as<float4>();
	s.mat_albedo = c->tables.mat_albedo.as<float4>(); s.mat_emission = c->tables.mat_emission.as<float4>();
	s.hdri = c->tables.hdri.as<float4>(); s.mat_glass = c->tables.mat_glass.as<float4>();
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

// ---- what exact stream order excludes (DESIGN.md "One switch table in the host layers") ------------------------------------------
// One row per feature that mirt_set_stream_order(ctx, 1) cannot run with.  The exclusion is a rule about pairs, and both directions of every
// pair read this table and nothing else: mirt_set_stream_order(ctx, 1) refuses with the first row that is on (refuse_exact_order), and a
// feature's entry point asked to turn the feature on under exact order refuses with its own row (refuse_under_exact_order).
struct ExactExcludes {
	uint32_t (*on)(const mirt_ctx*);   // 0 = off in this context; otherwise how much of it there is
	const char* why;                   // the message is "exact stream order <why>: <the call that lifts the refusal> first"
	const char* off;                   // what turns the feature off: a format that may print on()
};
const ExactExcludes kExactExcludes[X_ROWS] = {
	/* X_LENS */         { [](const mirt_ctx* c) -> uint32_t { return lens_on(c); }, "replays the reference, which has no lens (Camera.hpp:80-88 ignores it)", "call mirt_set_lens(ctx, 0, 0)" },
	/* X_FROZEN */       { [](const mirt_ctx* c) { return c->freeze.n_frozen; }, "runs a tile's whole bounce loop in one launch and has no form that skips frozen tiles", "%u are frozen, mirt_reset" },
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
} // namespace
int refuse_under_exact_order(mirt_ctx* c, ExactRow row) {
	return c->stream_order ? fail(c, MIRT_ERR_STATE, "exact stream order %s: call mirt_set_stream_order(ctx, 0) first", kExactExcludes[row].why) : MIRT_OK;
}
namespace {

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
	if (const char* e = std::getenv("MIRT_TUNE_CHUNK")) c->tune.chunk = static_cast<uint32_t>(std::min(std::max(std::atoi(e), 64), 65536)) & ~63u;
	if (const char* e = std::getenv("MIRT_TUNE_REFILL_IDLE")) c->tune.refill_idle = static_cast<uint32_t>(std::min(std::max(std::atoi(e), 1), 64));
	if (const char* e = std::getenv("MIRT_TUNE_DENOISE_STAGED")) c->tune.denoise_staged = static_cast<uint32_t>(std::min(std::max(std::atoi(e), 0), static_cast<int>(kAtrousStagedMaxStep)));
	if (const char* e = std::getenv("MIRT_TUNE_WIDE")) c->tune.wide = std::atoi(e) != 0 ? 1u : 0u;
	if (const char* e = std::getenv("MIRT_TUNE_LEAF_BATCH")) c->tune.leaf_batch = static_cast<uint32_t>(std::min(std::max(std::atoi(e), 1), 64));
	if (const char* e = std::getenv("MIRT_TUNE_TRACE_WGS")) c->tune.trace_wgs = std::atoi(e) == 1 ? 1u : 2u;
	if (const char* e = std::getenv("MIRT_TUNE_SHADE_WGS")) c->tune.shade_wgs = static_cast<uint32_t>(std::min(std::max(std::atoi(e), 1), 16));
	if (const char* e = std::getenv("MIRT_DEBUG_POISON_CONTRIB")) c->debug_poison_contrib = std::atoi(e) != 0;
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	e = hipStreamCreateWithFlags(&c->stream.s, hipStreamNonBlocking);
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
	if ((r = upload(c, c->tables.spheres, t.sph)) || (r = build_scene_records(c, a, t.sph, tree)) || (r = upload(c, c->tables.prim_mat, t.pm)) ||
	    (r = upload(c, c->tables.light_sphere, t.lsp)) || (r = upload(c, c->tables.light_emit, t.lem)) || (r = upload(c, c->tables.mat_albedo, t.alb)) ||
	    (r = upload(c, c->tables.mat_emission, t.emi)) || (r = upload(c, c->tables.mat_ggx, t.ggx)) || (r = upload(c, c->tables.mat_glass, t.gls)) || (r = upload(c, c->tables.hdri, t.sky)) ||
	    (r = upload(c, c->tables.geo_sphere, t.gsp)) || (r = upload(c, c->tables.geo_mat, t.gpm))) return r;
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	c->lists.cand_valid = false;                                                             // spheres or tree changed (a node-only update included)
	commit_scene(c, a, tree);
	c->hist.drop();                                                                   // other surfaces: nothing of the old view may be reprojected onto them
	c->tables.glass_host = t.gls; c->scene_has_glass = has_glass(t.gls);
	c->tables.alb_host = t.alb; c->tables.ggx_host = t.ggx; c->tables.emi_host = t.emi; c->tables.mat_merged_valid = false;
	if (c->sky_sampling) { HIP_TRY(c, sync_all(c)); if ((r = build_sky_table(c))) return r; }      // (a batch in flight on another stream may read the old table)
	if ((r = plan_trace_lds(c))) return r;
	c->have_scene = true;
	c->env_baked = false;
	c->tables.refit_links_valid = false;                                                      // another tree
	c->tables.light_ids.assign(lights, lights + n_lights); c->tables.light_sphere_host = t.lsp;      // what mirt_update_spheres patches
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
	c->lists.cand_valid = false;                                                             // every cone has moved
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
		c->lists.cand_valid = false;
	if (p->brdf != c->policy.brdf) c->tables.mat_merged_valid = false;                     // (the closure of the materials beyond the table's end)
	c->policy = *p;
	if (replan) c->planned_for = 0;
	if (realloc_acc) c->hist.drop();                                               // its lengths count samples of another bucket layout
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
	c->tables.gloss_decay_dev_valid = false;
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
	             [](mirt_ctx* c, uint32_t on) { return on && c->have_scene ? check_glass(c, c->tables.glass_host) : MIRT_OK; });
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
	c->tables.mat_merged_valid = false;
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
		if (r || (r = build_sky_table(c))) { c->sky.drop(); return r; }       // the switch stays off
	}
	if (!on) {
		c->sky.drop();
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
	c->lists.cand_valid = false;                                                             // other pixels
	c->dn.drop();                                                                      // mirt_render_atrous allocates them again at the new size
	c->hist.drop();                                                                   // another image
	c->hist.id_out.release();
	c->h_tiles = width / MIRT_TILE_ROOT; c->v_tiles = height / MIRT_TILE_ROOT;          // Renderer.hpp:59-60
	set_tile_map(c, TileMap::of_range(0u, c->h_tiles, width), c->h_tiles * c->v_tiles);
	HIP_TRY(c, c->framebuffer.ensure(std::max<size_t>(static_cast<size_t>(width) * height, 1) * sizeof(float4)));
	HIP_TRY(c, hipMemsetAsync(c->framebuffer.ptr, 0, c->framebuffer.bytes, c->stream));
	if (c->frame_host.bytes < c->framebuffer.bytes) {
		if (c->frame_host.ptr) (void)hipHostFree(c->frame_host.ptr);
		c->frame_host.ptr = nullptr; c->frame_host.bytes = 0;
		HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->frame_host.ptr), c->framebuffer.bytes, hipHostMallocDefault));
		c->frame_host.bytes = c->framebuffer.bytes;
	}
	return alloc_accumulator(c);                                                      // Renderer.hpp:61-62
}

int mirt_set_tile_range(mirt_ctx* c, uint32_t first_tile, uint32_t n_tiles) {
	if (!c) return MIRT_ERR_ARG;
	const uint64_t all = static_cast<uint64_t>(c->h_tiles) * c->v_tiles;
	if (static_cast<uint64_t>(first_tile) + n_tiles > all) return fail(c, MIRT_ERR_ARG, "tile range [%u,+%u) exceeds %llu tiles", first_tile, n_tiles, (unsigned long long)all);
	{ const int dr = drop_and_wait(c); if (dr) return dr; }                         // zeroes the accumulator
	set_tile_map(c, TileMap::of_range(first_tile, c->h_tiles, c->width), n_tiles);
	c->hist.drop();
	c->lists.cand_valid = false;                                                             // other local pixels
	return alloc_accumulator(c);
}

int mirt_set_tile_rows(mirt_ctx* c, uint32_t first_row, uint32_t row_stride) {
	if (!c) return MIRT_ERR_ARG;
	if (row_stride == 0) return fail(c, MIRT_ERR_ARG, "row_stride must be at least 1");
	{ const int dr = drop_and_wait(c); if (dr) return dr; }                         // zeroes the accumulator
	set_tile_map(c, TileMap::of_rows(first_row, row_stride, c->h_tiles, c->width), TileMap::tile_rows_owned(c->v_tiles, first_row, row_stride) * c->h_tiles);
	c->hist.drop();
	c->lists.cand_valid = false;                                                             // other local pixels
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

int mirt_accumulator_floats(const mirt_ctx* c, size_t* n) { if (!c || !n) return MIRT_ERR_ARG; *n = accumulator_floats(c); return MIRT_OK; }
int mirt_read_accumulator(mirt_ctx* c, float* dst) {
	if (!c || !dst) return MIRT_ERR_ARG;
	{ const int fr = flush_and_wait(c); if (fr) return fr; }
	return read_slab(c, c->accumulator, accumulator_floats(c), dst);
}
int mirt_accumulator_device(mirt_ctx* c, void** ptr, size_t* bytes) {
	if (!c || !ptr || !bytes) return MIRT_ERR_ARG;
	{ const int fr = flush_and_wait(c); if (fr) return fr; }                        // the caller reads the slab on a stream of its own (RCCL gather): everything enqueued here has landed
	return slab_device(c->accumulator, accumulator_floats(c), ptr, bytes);
}
int mirt_load_accumulator(mirt_ctx* c, const float* src, int src_is_device, uint32_t accumulations) {
	if (!c || !src) return MIRT_ERR_ARG;
	{ const int dr = drop_and_wait(c); if (dr) return dr; }                         // overwritten below: what is deferred is dropped, not launched
	{ const int r = load_slab(c, c->accumulator, accumulator_floats(c), src, src_is_device); if (r) return r; }   // src == the slab itself: only `accumulations` changes
	c->accumulations = accumulations;
	c->freeze.drop();                                                                  // every tile at `accumulations`; mirt_load_tile_counts applies per-tile counts
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
// The AOV entry points refuse while the AOVs are off, and flush where the accumulator's load drops: the deferred accumulations' AOV sums are
// overwritten by a load, their accumulator adds are not.
int mirt_read_aov(mirt_ctx* c, float* dst) {
	if (!c || !dst) return MIRT_ERR_ARG;
	if (!c->aov_on) return fail(c, MIRT_ERR_STATE, "AOVs are off (mirt_set_aov)");
	{ const int fr = flush_and_wait(c); if (fr) return fr; }
	return read_slab(c, c->aov, aov_floats(c), dst);
}
int mirt_aov_device(mirt_ctx* c, void** ptr, size_t* bytes) {
	if (!c || !ptr || !bytes) return MIRT_ERR_ARG;
	if (!c->aov_on) return fail(c, MIRT_ERR_STATE, "AOVs are off (mirt_set_aov)");
	{ const int fr = flush_and_wait(c); if (fr) return fr; }
	return slab_device(c->aov, aov_floats(c), ptr, bytes);
}
int mirt_load_aov(mirt_ctx* c, const float* src, int src_is_device) {
	if (!c || !src) return MIRT_ERR_ARG;
	if (!c->aov_on) return fail(c, MIRT_ERR_STATE, "AOVs are off (mirt_set_aov)");
	{ const int fr = flush_and_wait(c); if (fr) return fr; }                        // (their sums are overwritten below; their accumulator adds are not)
	return load_slab(c, c->aov, aov_floats(c), src, src_is_device);
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
	*out = c->prof.times;
	if (reset) c->prof.times = mirt_kernel_times{};
	return MIRT_OK;
}
int mirt_get_stream(mirt_ctx* c, void** s) { if (!c || !s) return MIRT_ERR_ARG; *s = c->stream; return MIRT_OK; }

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
	if (!c->sky.dev.t) return fail(c, MIRT_ERR_STATE, "there is no sky sampling table: mirt_set_sky_sampling(ctx, 1) and mirt_set_scene first");
	const size_t floats = sky_table_floats(c->sky.dev.rows, c->sky.dev.cols);
	info[0] = c->sky.dev.rows; info[1] = c->sky.dev.cols; std::memcpy(&info[2], &c->sky.total, 4); info[3] = static_cast<uint32_t>(floats);
	if (!dst) return MIRT_OK;
	if (capacity < floats) return fail(c, MIRT_ERR_ARG, "debug_sky_table: room for %zu floats, the table takes %zu", capacity, floats);
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	HIP_TRY(c, hipMemcpy(dst, c->sky.dev.t, floats * sizeof(float), hipMemcpyDeviceToHost));
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
		DeviceBuffer& dst = n * sizeof(float4) > c->tables.hdri.bytes ? fresh : c->tables.hdri;
		HIP_TRY(c, dst.ensure(n * sizeof(float4)));
		hipError_t e = hipSuccess;
		if (bake) {
			e = bake_sun_sky(c, *bake, n, dst.as<float4>());
		} else e = hipMemcpyAsync(dst.ptr, texels, n * sizeof(float4), hipMemcpyHostToDevice, c->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(c->stream);                 // host buffers are copied, never retained
		if (e != hipSuccess) { fresh.release(); return fail(c, MIRT_ERR_HIP, "environment map: %s", hipGetErrorString(e)); }
		if (&dst == &fresh) c->tables.hdri = std::move(fresh);
		SceneDev& s = c->scene;
		s.hdri = c->tables.hdri.as<float4>();
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

extern "C" int mirt_update_spheres(mirt_ctx* c, uint32_t n, const uint32_t* bvh_index, const uint32_t* geometry_index, const float* xyz_rsq) {
	if (!c) return MIRT_ERR_ARG;
	if (!c->have_scene) return fail(c, MIRT_ERR_STATE, "mirt_update_spheres moves spheres of a scene: mirt_set_scene first");
	SceneDev& s = c->scene;
	{ char msg[320];                                                             // before anything changes: a refused call leaves every word in place
	  if (const int r = mirt_scene_update::check(n, bvh_index, geometry_index, xyz_rsq, s.n_spheres, s.half_boxes != 0, msg, sizeof msg)) return fail(c, r, "%s", msg); }
	if (n == 0) return MIRT_OK;
	{ const int fr = flush_and_wait(c); if (fr) return fr; }                      // deferred accumulations and batches in flight see the old geometry
	{ const int r = launch_update_spheres(c, n, bvh_index, geometry_index, xyz_rsq); if (r) return r; }   // the scatter, the refit and the light rows: mirt_launch.hip
	c->tables.refit_links_valid = true;
	c->lists.cand_valid = false;                                                        // the camera-ray lists name the spheres of the old positions
	c->spheres_gen++;                                                             // a history kept under mirt_set_sphere_motion compares its snapshot with the table as it is now
	if (!c->history_motion) c->hist.drop();                                      // surfaces moved: nothing of the old view may be reprojected onto them
	return MIRT_OK;
}

extern "C" int mirt_update_materials(mirt_ctx* c, uint32_t n_rows, const uint32_t* material_index, const mirt_material* rows,
                                     uint32_t n_assign, const uint32_t* bvh_index, const uint32_t* geometry_index, const int32_t* material_ID) {
	if (!c) return MIRT_ERR_ARG;
	if (!c->have_scene) return fail(c, MIRT_ERR_STATE, "mirt_update_materials edits the materials of a scene: mirt_set_scene first");
	SceneDev& s = c->scene;
	{ char msg[320];                                                             // before anything changes: a refused call leaves every word in place
	  if (const int r = mirt_scene_update::check_materials(n_rows, material_index, rows, n_assign, bvh_index, geometry_index, material_ID, s.n_spheres, s.n_mat,
	                                                       c->transmission != 0, reinterpret_cast<const float*>(c->tables.glass_host.data()), msg, sizeof msg)) return fail(c, r, "%s", msg); }
	if (n_rows == 0 && n_assign == 0) return MIRT_OK;
	{ const int fr = flush_and_wait(c); if (fr) return fr; }                      // deferred accumulations and batches in flight see the old materials
	// the kept host rows, as flatten_tables makes them, and the four small tables again (at most 63 rows each: no kernel)
	for (uint32_t i = 0; i < n_rows; i++) {
		const mirt_material& m = rows[i];
		const uint32_t k = material_index[i];
		c->tables.alb_host[k] = make_float4(m.albedo[0], m.albedo[1], m.albedo[2], 0.0f);
		c->tables.emi_host[k] = make_float4(m.emission[0], m.emission[1], m.emission[2], 0.0f);
		c->tables.ggx_host[k] = make_float4(m.F0[0], m.F0[1], m.F0[2], m.roughness);
		c->tables.glass_host[k] = make_float4(m.transmission[0], m.transmission[1], m.transmission[2], 1.0f + m.IOR_minus_one);
	}
	int r;
	if (n_rows && ((r = upload(c, c->tables.mat_albedo, c->tables.alb_host)) || (r = upload(c, c->tables.mat_emission, c->tables.emi_host)) || (r = upload(c, c->tables.mat_ggx, c->tables.ggx_host)) ||
	               (r = upload(c, c->tables.mat_glass, c->tables.glass_host)))) return r;
	if ((r = launch_update_materials(c, n_assign, bvh_index, geometry_index, material_ID))) return r;          // the re-assigned spheres and the light tables again: mirt_launch.hip
	HIP_TRY(c, hipStreamSynchronize(c->stream));                                  // host buffers are copied, never retained
	c->scene_has_glass = has_glass(c->tables.glass_host);                                // with the transmission switch on, the GLASS kernels start or stop being launched
	c->tables.mat_merged_valid = false;                                                  // the next MIXED launch uploads the new colours
	return MIRT_OK;                                                               // (closure_plan() reads the material count and the closure table: neither changed)
}
