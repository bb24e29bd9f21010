// mirt_host.hpp — C++ host-side mirror of the reference's Renderer / Scene interface over the C-ABI (mirt.h).
//
// The reference host is C++ (Application.cpp); this header gives it the same names with the same meaning:
//   mirt::Sphere / Material / Node      Primitives.hpp:7-27, BVH.hpp:18-31 (byte-identical)
//   mirt::Camera                        Camera.hpp:5-89 (fields the path reads + Projection::Resize/UpdateLens + quatLookAt)
//   mirt::Scene                         Scene.hpp:19-26 (geometry, material, lighting_acceleration, camera, sky, acceleration_structure)
//   mirt::Renderer                      Renderer.hpp:28-68,73,436: Resize / ResetAccumulator / Accumulate / Render / GetFrame
// Failures surface as std::runtime_error carrying mirt_last_error() (the reference asserts / terminates instead).
#pragma once
#include "../../include/mirt.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace mirt {

using Sphere = mirt_sphere;
using Material = mirt_material;
using Node = mirt_bvh_node;
static_assert(sizeof(Sphere) == 32 && sizeof(Material) == 96 && sizeof(Node) == 32, "reference layouts");

struct vec3 { float x = 0, y = 0, z = 0; };
struct quat { float x = 0, y = 0, z = 0, w = 1; };

// Camera.hpp:5-89.  The aperture / focus fields are carried by the reference and read by nothing on its path (Q18): here they drive the
// thin lens of mirt_set_lens, through Renderer::SetLens / RendererPolicy::lens only — a Renderer made without them is the pinhole camera.
struct Camera {
	vec3 pos;
	quat orient;
	float half_width = 0.5f, half_height = 0.5f, z = 0.0f;
	float focal_length = 50.0f, exp = 1.0f;
	float focus_distance = 1.0f;                                           // Camera.hpp:64; world units (the pick stores a hit distance here, Application.cpp:298)
	float f_number = 16.0f;                                                // Camera.hpp:64
	float unit_mm = 1000.0f;                                               // one world unit in millimetres: the reference never connects focal_length's mm to the scene
	float aperture_radius() const { return (focal_length / (2.0f * f_number)) / unit_mm; }   // Projection::calc_aperture, Camera.hpp:17-19,24, in world units

	Camera() { Resize(1, 1); }
	Camera(vec3 eye, vec3 direction, float focal_length_mm = 50.0f, float exposure = 1.0f) : pos(eye), focal_length(focal_length_mm), exp(exposure) {
		const float inv = 1.0f / std::sqrt(direction.x * direction.x + direction.y * direction.y + direction.z * direction.z);
		orient = look_at(vec3{ direction.x * inv, direction.y * inv, direction.z * inv });
		Resize(1, 1);
	}
	void Resize(uint32_t width, uint32_t height) {                         // Projection::Resize + UpdateLens, Camera.hpp:20-31
		half_height = static_cast<float>(height) * 0.5f;
		half_width = static_cast<float>(width) * 0.5f;
		z = half_height * ((-2.0f / 24.0f) * focal_length);
	}
	static quat look_at(vec3 d) {                                          // glm::quatLookAt(direction, up = +y), right-handed
		const vec3 c2{ -d.x, -d.y, -d.z }, up{ 0, 1, 0 };
		vec3 r{ up.y * c2.z - c2.y * up.z, up.z * c2.x - c2.z * up.x, up.x * c2.y - c2.x * up.y };
		const float rr = r.x * r.x + r.y * r.y + r.z * r.z;
		const float s = 1.0f / std::sqrt(rr > 0.00001f ? rr : 0.00001f);
		const vec3 c0{ r.x * s, r.y * s, r.z * s };
		const vec3 c1{ c2.y * c0.z - c0.y * c2.z, c2.z * c0.x - c0.z * c2.x, c2.x * c0.y - c0.x * c2.y };
		const float m00 = c0.x, m01 = c0.y, m02 = c0.z, m10 = c1.x, m11 = c1.y, m12 = c1.z, m20 = c2.x, m21 = c2.y, m22 = c2.z;
		const float fx = m00 - m11 - m22, fy = m11 - m00 - m22, fz = m22 - m00 - m11, fw = m00 + m11 + m22;
		int idx = 0; float big = fw;
		if (fx > big) { big = fx; idx = 1; }
		if (fy > big) { big = fy; idx = 2; }
		if (fz > big) { big = fz; idx = 3; }
		const float b = std::sqrt(big + 1.0f) * 0.5f, mult = 0.25f / b;
		switch (idx) {
		case 0: return quat{ (m12 - m21) * mult, (m20 - m02) * mult, (m01 - m10) * mult, b };
		case 1: return quat{ b, (m01 + m10) * mult, (m20 + m02) * mult, (m12 - m21) * mult };
		case 2: return quat{ (m01 + m10) * mult, b, (m12 + m21) * mult, (m20 - m02) * mult };
		default: return quat{ (m20 + m02) * mult, (m12 + m21) * mult, b, (m01 - m10) * mult };
		}
	}
};

struct Sky {                                                               // Primitives.hpp:29-47
	float ambient_color[3] = { 0, 0, 0 };
	int32_t hdri_width = 1, hdri_height = 1;
	std::vector<float> hdri_data = { 1, 1, 1, 1 };                         // RGBA f32 (synthetic 1x1 texel by default)
};

struct BoundingVolumeHierarchy {                                           // BVH.hpp:85-86,90
	std::vector<Node> nodes;
	std::vector<Sphere> prims;
	BoundingVolumeHierarchy() = default;
	explicit BoundingVolumeHierarchy(const std::vector<Sphere>& primitives) {
		nodes.resize(primitives.size() * 2 + 1);
		prims.resize(primitives.size());
		uint32_t n = 0;
		if (mirt_bvh_build(primitives.data(), static_cast<uint32_t>(primitives.size()), nodes.data(), &n, prims.data()) != MIRT_OK)
			throw std::runtime_error("mirt_bvh_build failed");
		nodes.resize(n);
	}
};
struct LightingAcceleration {                                              // Scene.hpp:9-17
	std::vector<int32_t> prims;
	LightingAcceleration() = default;
	LightingAcceleration(const std::vector<Sphere>& src, const std::vector<Material>& material) {
		prims.resize(src.size() + 1);
		uint32_t n = 0;
		if (mirt_light_list(src.data(), static_cast<uint32_t>(src.size()), material.data(), static_cast<uint32_t>(material.size()), prims.data(), &n) != MIRT_OK)
			throw std::runtime_error("mirt_light_list failed (material_ID out of range?)");
		prims.resize(n);
	}
};
struct Scene {                                                             // Scene.hpp:19-26
	std::vector<Sphere> geometry;
	std::vector<Material> material;
	LightingAcceleration lighting_acceleration;
	Camera camera;
	Sky sky;
	BoundingVolumeHierarchy acceleration_structure;
	void RebuildAcceleration() {                                           // Application.cpp:233-234, 508-509
		acceleration_structure = BoundingVolumeHierarchy{ geometry };
		lighting_acceleration = LightingAcceleration{ geometry, material };
	}
};

struct RendererPolicy {                                                    // Renderer.hpp:19-26 (+ the path's #defines)
	uint32_t max_bounces = 16;
	uint32_t buckets = 5;                                                  // AccumulationBuckets, Renderer.hpp:41
	bool mis = true;                                                       // #define MIS true, Renderer.hpp:71
	bool use_bvh = true;                                                   // reference ships USEBVH false (BVH.hpp:307); results are identical
	bool reference_tree = false;                                           // true: traverse scene.acceleration_structure.nodes as is instead of the internal SAH tree
	bool gpu_build = false;                                                // true: internal tree built on the GPU (LBVH) at SceneChanged(): faster rebuild, slower rays
	uint32_t brdf = 0;                                                     // #define BRDF, Renderer.hpp:70: 0 = Lambertian, 1 = GGX (F0, roughness; SetGlossDecay)
	bool lens = false;                                                     // true: scene.camera's f_number / focus_distance / unit_mm drive a thin lens (CameraChanged re-sends it)
};

class Renderer {
public:
	static constexpr size_t RequiredTiling() { return MIRT_TILE_ROOT; }    // Renderer.hpp:36

	// One renderer object, as in the reference (Application.cpp:514) — on one GPU or on several of the node: `devices` lists the HIP
	// ordinals; the library splits the tile rows over them and gathers the accumulator with one RCCL exchange (mirt.h, mirt_group_*).
	explicit Renderer(const Scene& scene_ref, RendererPolicy policy = {}, std::vector<int> devices = { 0 }) : scene(scene_ref) {
		if (mirt_group_create(devices.data(), static_cast<int>(devices.size()), &group_) != MIRT_OK) throw std::runtime_error(std::string("mirt_group_create: ") + mirt_group_last_error(nullptr));
		mirt_policy& p = policy_;
		p.max_bounces = policy.max_bounces; p.buckets = policy.buckets; p.mis = policy.mis; p.use_bvh = policy.use_bvh; p.reference_tree = policy.reference_tree; p.gpu_build = policy.gpu_build;
		p.brdf = policy.brdf;
		lens_follows_camera_ = policy.lens;
		if (mirt_group_set_policy(group_, &p) < 0) {                           // no destructor runs for a constructor that throws: release the group here
			const std::string why = std::string("mirt_group_set_policy: ") + mirt_group_last_error(group_);
			mirt_group_destroy(group_); group_ = nullptr;
			throw std::runtime_error(why);
		}
	}
	~Renderer() { if (group_) mirt_group_destroy(group_); }
	Renderer(const Renderer&) = delete;
	Renderer& operator=(const Renderer&) = delete;

	// The reference reads `scene` live; a copy in HBM has to be told about edits (Application.cpp:508-510).
	void SceneChanged() {
		const auto& s = scene;
		check(mirt_group_set_scene(group_, s.geometry.data(), s.acceleration_structure.prims.data(), static_cast<uint32_t>(s.geometry.size()),
		                           s.acceleration_structure.nodes.data(), static_cast<uint32_t>(s.acceleration_structure.nodes.size()),
		                           s.material.data(), static_cast<uint32_t>(s.material.size()),
		                           s.lighting_acceleration.prims.data(), static_cast<uint32_t>(s.lighting_acceleration.prims.size()),
		                           s.sky.ambient_color, s.sky.hdri_data.data(), static_cast<uint32_t>(s.sky.hdri_width), static_cast<uint32_t>(s.sky.hdri_height)),
		      "mirt_group_set_scene");
		CameraChanged();
	}
	void CameraChanged() {
		const Camera& c = scene.camera;
		check(mirt_group_set_camera(group_, &c.pos.x, &c.orient.x, c.half_width, c.half_height, c.z, c.exp), "mirt_group_set_camera");
		if (lens_follows_camera_) SetLens(c.aperture_radius(), c.focus_distance);     // UpdateLens, Camera.hpp:21-26
	}
	// Thin-lens depth of field (mirt.h, mirt_set_lens): lens radius and axial depth of the plane of focus in world units; radius 0 = pinhole.
	// Like the reference's lens widgets (Application.cpp:413-417) the caller resets the accumulator afterwards.
	void SetLens(float aperture_radius, float focus_depth) { check(mirt_group_set_lens(group_, aperture_radius, focus_depth), "mirt_group_set_lens"); }
	// The right-click pick (Application.cpp:271-304): the un-jittered pinhole ray of pixel (x, y); distance is INFINITY on a miss, depth is the
	// axial depth to hand to SetLens.
	struct Pick { float distance, depth; };
	Pick PickFocus(uint32_t x, uint32_t y) { Pick p{}; check(mirt_group_pick_focus(group_, x, y, &p.distance, &p.depth), "mirt_group_pick_focus"); return p; }
	void Resize(uint32_t new_width, uint32_t new_height) {                 // Renderer.hpp:53-63
		width = new_width; height = new_height;
		framebuffer.assign(static_cast<size_t>(width) * height * 4, 0.0f);
		check(mirt_group_resize(group_, width, height), "mirt_group_resize");
	}
	void ResetAccumulator() { check(mirt_group_reset(group_), "mirt_group_reset"); }    // Renderer.hpp:64-67
	// The closure the reference picks with #define BRDF (Renderer.hpp:70) and its gloss_decay_table (:212), switchable at run time.
	void SetBRDF(uint32_t brdf) {
		mirt_policy p = policy_; p.brdf = brdf;
		check(mirt_group_set_policy(group_, &p), "mirt_group_set_policy");
		policy_ = p;
	}
	void SetGlossDecay(const std::vector<float>& decay) {
		check(mirt_group_set_gloss_decay(group_, decay.data(), static_cast<uint32_t>(decay.size())), "mirt_group_set_gloss_decay");
	}
	// The reference's stream slots and scalar intersection tail (BVH.hpp:270-286) instead of the wavefront order (mirt.h, mirt_set_stream_order):
	// brute-force traversal, for comparisons against the shipped binary.
	void SetStreamOrder(bool exact) { check(mirt_group_set_stream_order(group_, exact ? 1u : 0u), "mirt_group_set_stream_order"); }
	// The NEE light picked among `candidates` uniform draws by the reference's unused RIS<count> (Sampling.hpp:25-54; mirt.h, mirt_set_light_ris):
	// 0 = off, the uniform draw of Renderer.hpp:259.  Same expectation, so the accumulator is not reset.
	void SetLightRis(uint32_t candidates) { check(mirt_group_set_light_ris(group_, candidates), "mirt_group_set_light_ris"); }
	// Transmissive materials (max(transmission) > 0) take a smooth dielectric interface of index 1 + IOR_minus_one (mirt.h, mirt_set_transmission); off by
	// default, as in the reference, whose closures read neither field.  Another estimand: Reset() is the caller's to call.  Not in exact stream order.
	void SetTransmission(bool on) { check(mirt_group_set_transmission(group_, on ? 1u : 0u), "mirt_group_set_transmission"); }
	// The environment map as one more light of next event estimation (mirt.h, mirt_set_sky_sampling): off by default, as in the reference, where the
	// sky is met by extension rays only.  Same expectation, so the accumulator is not reset.  Not in exact stream order.
	void SetSkySampling(bool on) { check(mirt_group_set_sky_sampling(group_, on ? 1u : 0u), "mirt_group_set_sky_sampling"); }
	// SceneUpdate::Ambient (Application.cpp:335-347,503; mirt.h, mirt_set_environment): scene.sky alone is handed over again — no tree rebuild, the
	// camera-ray lists and the temporal history stay.  The environment is part of the estimand: ResetAccumulator() is the caller's to call.
	void SetEnvironment() {
		const Sky& k = scene.sky;
		check(mirt_group_set_environment(group_, k.ambient_color, k.hdri_data.data(), static_cast<uint32_t>(k.hdri_width), static_cast<uint32_t>(k.hdri_height)), "mirt_group_set_environment");
	}
	// A Preetham sky and a sun disc baked on the device into the environment map, under scene.sky.ambient_color as last handed over (mirt.h,
	// mirt_set_sun_sky).  scene.sky's own texels are not touched: SceneChanged() hands them over again.
	static mirt_sun_sky_params SunSkyDefaults() { mirt_sun_sky_params p{}; mirt_sun_sky_defaults(&p); return p; }
	void SetSunSky(const mirt_sun_sky_params& params) { check(mirt_group_set_sun_sky(group_, &params), "mirt_group_set_sun_sky"); }
	// The map the kernels read (the first member's; every member holds the same words), RGBA f32 rows (mirt.h, mirt_read_environment).
	struct Environment { uint32_t width = 0, height = 0; bool baked = false; std::vector<float> rgba; };
	Environment ReadEnvironment() {
		mirt_ctx* ctx = nullptr;
		check(mirt_group_member(group_, 0, &ctx), "mirt_group_member");
		uint32_t info[4] = {};
		Environment e;
		if (mirt_read_environment(ctx, nullptr, 0, info) < 0) throw std::runtime_error(std::string("mirt_read_environment: ") + mirt_last_error(ctx));
		e.width = info[0]; e.height = info[1]; e.baked = info[2] != 0;
		e.rgba.resize(static_cast<size_t>(e.width) * e.height * 4);
		if (mirt_read_environment(ctx, e.rgba.data(), e.rgba.size(), info) < 0) throw std::runtime_error(std::string("mirt_read_environment: ") + mirt_last_error(ctx));
		return e;
	}
	// SceneUpdate::Geometry for spheres that keep their place (Application.cpp:466-468; mirt.h, mirt_update_spheres): the caller has written the new
	// centre and radius_sq into scene.geometry[geometry_index[i]] and into scene.acceleration_structure.prims[bvh_index[i]], the same sphere in the
	// order hit.primID refers to (BvhIndexOf finds it); those rows alone are handed over and the tree in place is refitted on the GPU — no
	// RebuildAcceleration(), no SceneChanged().  Geometry is part of the estimand: ResetAccumulator() is the caller's to call.
	void UpdateSpheres(const std::vector<uint32_t>& bvh_index, const std::vector<uint32_t>& geometry_index) {
		if (bvh_index.size() != geometry_index.size()) throw std::runtime_error("UpdateSpheres: one bvh_index per geometry_index");
		std::vector<float> packet;
		packet.reserve(4 * geometry_index.size());
		for (const uint32_t g : geometry_index) {
			const Sphere& s = scene.geometry.at(g);
			packet.insert(packet.end(), { s.position[0], s.position[1], s.position[2], s.radius_sq });
		}
		check(mirt_group_update_spheres(group_, static_cast<uint32_t>(geometry_index.size()), bvh_index.data(), geometry_index.data(), packet.data()), "mirt_group_update_spheres");
	}
	// SceneUpdate::Material (Application.cpp:470-485,509; mirt.h, mirt_update_materials): the caller has edited scene.material[material_index[i]] and
	// written the new material_ID into scene.geometry[geometry_index[i]] and scene.acceleration_structure.prims[bvh_index[i]] (the same sphere;
	// BvhIndexOf finds it BEFORE the id is written); those rows and ids alone are handed over, and the light list is regenerated on the GPU by the
	// reference's rule — no RebuildAcceleration(), no SceneChanged().  scene.lighting_acceleration is the caller's: it is not read here and goes
	// stale until the caller rebuilds it.  Materials are part of the estimand: ResetAccumulator() is the caller's to call; the temporal history is kept.
	void UpdateMaterials(const std::vector<uint32_t>& material_index, const std::vector<uint32_t>& bvh_index = {}, const std::vector<uint32_t>& geometry_index = {}) {
		if (bvh_index.size() != geometry_index.size()) throw std::runtime_error("UpdateMaterials: one bvh_index per geometry_index");
		std::vector<Material> rows;
		rows.reserve(material_index.size());
		for (const uint32_t m : material_index) rows.push_back(scene.material.at(m));
		std::vector<int32_t> ids;
		ids.reserve(geometry_index.size());
		for (const uint32_t g : geometry_index) ids.push_back(scene.geometry.at(g).material_ID);
		check(mirt_group_update_materials(group_, static_cast<uint32_t>(rows.size()), material_index.data(), rows.data(),
		                                  static_cast<uint32_t>(ids.size()), bvh_index.data(), geometry_index.data(), ids.data()), "mirt_group_update_materials");
	}
	// Where scene.geometry[g] sits in scene.acceleration_structure.prims: the first row with the same 32 bytes (identical rows are interchangeable).
	uint32_t BvhIndexOf(uint32_t g) const {
		const std::vector<Sphere>& prims = scene.acceleration_structure.prims;
		for (size_t b = 0; b < prims.size(); b++) if (std::memcmp(&prims[b], &scene.geometry.at(g), sizeof(Sphere)) == 0) return static_cast<uint32_t>(b);
		throw std::runtime_error("BvhIndexOf: scene.acceleration_structure.prims does not hold that sphere (RebuildAcceleration() first)");
	}
	// The GGX closure's pdf in the MIS weights (mirt.h, mirt_set_ggx_pdf): off by default, as in the reference, whose Closure<GGX>::pdf returns 0.
	// On: emitters and (under sky sampling) the sky are weighed two ways on GGX surfaces.  Formally another estimator: Reset() is the caller's to call.
	// Not in exact stream order.
	void SetGgxPdf(bool on) { check(mirt_group_set_ggx_pdf(group_, on ? 1u : 0u), "mirt_group_set_ggx_pdf"); }
	// Per-material closures (mirt.h, mirt_set_material_closures): closure[m] = 0 (Lambertian) or 1 (GGX) for material m; an empty table (the default)
	// leaves every material on policy.brdf, as do the materials beyond its end.  Another estimand: Reset() is the caller's to call.  Not in exact stream order.
	void SetMaterialClosures(const std::vector<uint8_t>& closure) {
		check(mirt_group_set_material_closures(group_, closure.data(), static_cast<uint32_t>(closure.size())), "mirt_group_set_material_closures");
	}
	// Renderer.hpp:73-434.  Asynchronous: Render() / counters() / the destructor wait for the GPUs; called once per frame the library
	// still batches the frames between two Render()s that are due (mirt.h, mirt_accumulate_async).
	void Accumulate(uint32_t n_calls = 1) { check(mirt_group_accumulate_async(group_, n_calls), "mirt_group_accumulate_async"); }
	void Synchronize() { check(mirt_group_synchronize(group_), "mirt_group_synchronize"); }
	bool Render() {                                                        // Renderer.hpp:436-478; false = frame unchanged (:437)
		const int rc = mirt_group_render(group_, framebuffer.data());
		check(rc, "mirt_group_render");
		return rc == MIRT_OK;
	}
	const std::vector<float>& GetFrame() const { return framebuffer; }     // RGBA f32 rows, row 0 = y 0 (Renderer.hpp:40,68)
	uint32_t accumulations() const { uint32_t a = 0; mirt_group_get_accumulations(group_, &a); return a; }
	mirt_counters counters() { mirt_counters c{}; check(mirt_group_get_counters(group_, &c), "mirt_group_get_counters"); return c; }
	std::vector<float> accumulator() {                                     // the whole image's AccumulationTile slab (Renderer.hpp:43-46)
		size_t n = 0; mirt_group_accumulator_floats(group_, &n);
		std::vector<float> acc(n);
		check(mirt_group_read_accumulator(group_, acc.data()), "mirt_group_read_accumulator");
		return acc;
	}
	// First-hit AOVs (mirt.h): the reference's compiled-out FIRST BOUNCE OUTPUTS (Renderer.hpp:216-231) summed beside the accumulator.
	// SetAOV(true) only before the first Accumulate(); RenderAOV returns width * height * (1 for MIRT_AOV_DEPTH, else 3) floats,
	// row 0 = y 0, empty before the first accumulation.
	void SetAOV(bool on) { check(mirt_group_set_aov(group_, on ? 1u : 0u), "mirt_group_set_aov"); }
	std::vector<float> aov() {                                             // the whole image's [tile][plane 0..6][256] sums
		size_t n = 0; mirt_group_aov_floats(group_, &n);
		std::vector<float> sums(n);
		check(mirt_group_read_aov(group_, sums.data()), "mirt_group_read_aov");
		return sums;
	}
	std::vector<float> RenderAOV(int which) {
		std::vector<float> img(static_cast<size_t>(width) * height * (which == MIRT_AOV_DEPTH ? 1 : 3), 0.0f);
		const int rc = mirt_group_render_aov(group_, which, img.data());
		check(rc, "mirt_group_render_aov");
		if (rc != MIRT_OK) img.clear();
		return img;
	}
	// Variance-guided à-trous denoised resolve (mirt.h, mirt_render_atrous): the frame Render() resolves, filtered under the guidance of the first-hit
	// AOVs and each pixel's own bucket variance.  Needs SetAOV(true) and buckets >= 2; changes no state.  width * height * 4 floats, row 0 = y 0;
	// empty while Render() would return false.
	static mirt_denoise_params DenoiseDefaults() { mirt_denoise_params p{}; mirt_atrous_defaults(&p); return p; }
	std::vector<float> RenderDenoised(const mirt_denoise_params& params = DenoiseDefaults()) {
		std::vector<float> img(static_cast<size_t>(width) * height * 4, 0.0f);
		const int rc = mirt_group_render_atrous(group_, &params, img.data());
		check(rc, "mirt_group_render_atrous");
		if (rc != MIRT_OK) img.clear();
		return img;
	}
	// Temporal history for the denoised resolve (mirt.h, mirt_render_temporal): RenderDenoised() through a history that survives ResetAccumulator() and
	// camera moves — reprojected through the first-hit depth, rejected where depth or normal disagree, blended by sample count, then filtered.
	// history_len / stats may be NULL.  The shading switches do not drop the history: after changing the estimand call DropHistory().
	static mirt_temporal_params TemporalDefaults() { mirt_temporal_params p{}; mirt_temporal_defaults(&p); return p; }
	std::vector<float> RenderTemporal(const mirt_denoise_params& params = DenoiseDefaults(), const mirt_temporal_params& temporal = TemporalDefaults(),
	                                  std::vector<float>* history_len = nullptr, mirt_temporal_stats* stats = nullptr) {
		std::vector<float> img(static_cast<size_t>(width) * height * 4, 0.0f);
		if (history_len) history_len->assign(static_cast<size_t>(width) * height, 0.0f);
		const int rc = mirt_group_render_temporal(group_, &params, &temporal, img.data(), history_len ? history_len->data() : nullptr, stats);
		check(rc, "mirt_group_render_temporal");
		if (rc != MIRT_OK) img.clear();
		return img;
	}
	void DropHistory() { check(mirt_group_drop_history(group_), "mirt_group_drop_history"); }
	// Keeping the history across sphere moves (mirt.h, mirt_set_sphere_motion): on, UpdateSpheres() no longer drops the history; it carries the id
	// map and the sphere table it was taken under, and RenderTemporal() carries a moved sphere's pixels back to where the sphere was.  A change drops it.
	void SetHistoryMotion(bool on) { check(mirt_group_set_sphere_motion(group_, on ? 1u : 0u), "mirt_group_set_sphere_motion"); }
	// First-hit id map (mirt.h, mirt_id_map): per pixel of the whole image, row 0 = y 0, the BVH-order sphere (scene.acceleration_structure.prims) the
	// un-jittered pinhole ray through the pixel centre meets first, -1 for none, and its distance (INFINITY on a miss).  Changes no state.
	struct IdMapResult { std::vector<int32_t> prim; std::vector<float> distance; };
	IdMapResult IdMap() {
		IdMapResult m;
		m.prim.assign(static_cast<size_t>(width) * height, -1);
		m.distance.assign(static_cast<size_t>(width) * height, 0.0f);
		check(mirt_group_id_map(group_, m.prim.data(), m.distance.data()), "mirt_group_id_map");
		return m;
	}
	// Per-pixel noise estimate from the buckets (mirt.h, mirt_noise): the relative standard error of the mean of the bucket means, read from the
	// members' own slabs without a gather.  ready = false (and nothing filled) while accumulations is 0 or not a multiple of `buckets`.
	struct NoiseResult {
		bool ready = false;
		mirt_noise_stats stats{};
		std::vector<float> map;                                            // width * height, row 0 = y 0 (want_map)
		std::vector<float> tiles;                                          // 4 per tile in LaunchIndex order: {max, mean, usable, non-finite}
		std::vector<uint32_t> hist;                                        // MIRT_NOISE_BINS
	};
	NoiseResult Noise(float floor = 0.0f, bool want_map = false) {
		NoiseResult r;
		if (want_map) r.map.assign(static_cast<size_t>(width) * height, 0.0f);
		r.tiles.assign(static_cast<size_t>(width / MIRT_TILE_ROOT) * (height / MIRT_TILE_ROOT) * 4, 0.0f);
		r.hist.assign(MIRT_NOISE_BINS, 0u);
		const int rc = mirt_group_noise(group_, floor, want_map ? r.map.data() : nullptr, r.tiles.empty() ? nullptr : r.tiles.data(), r.hist.data(), &r.stats);
		check(rc, "mirt_group_noise");
		r.ready = rc == MIRT_OK;
		return r;
	}
	// Upper edge of the histogram bin that holds the q-quantile (mirt_noise_quantile; host code); NaN for an empty histogram.
	static float NoiseQuantile(const std::vector<uint32_t>& hist, double q) {
		float v = 0.0f;
		if (hist.size() != MIRT_NOISE_BINS) throw std::runtime_error("NoiseQuantile: the histogram must hold MIRT_NOISE_BINS words");
		const int rc = mirt_noise_quantile(hist.data(), q, &v);
		if (rc < 0) throw std::runtime_error("mirt_noise_quantile: q is not in (0, 1]");
		return rc == MIRT_OK ? v : std::nanf("");
	}
	// Render until converged (mirt_accumulate_until): synchronous; converged = false when max_accumulations was reached first.
	struct UntilResult { bool converged; uint32_t issued; mirt_noise_stats last; };
	UntilResult AccumulateUntil(const mirt_stop_rule& rule) {
		UntilResult r{};
		const int rc = mirt_group_accumulate_until(group_, &rule, &r.last, &r.issued);
		check(rc, "mirt_group_accumulate_until");
		r.converged = rc == MIRT_OK;
		return r;
	}
	// Per-tile adaptive sampling (mirt.h): frozen tiles take no more samples; masks, counts and `above` hold one entry per tile of the image in
	// LaunchIndex order.  A tile whose count is n holds what n plain Accumulate() calls leave in it.
	size_t Tiles() const { return static_cast<size_t>(width / MIRT_TILE_ROOT) * (height / MIRT_TILE_ROOT); }
	void FreezeTiles(const std::vector<uint8_t>& mask) { check(mirt_group_freeze_tiles(group_, mask.data(), mask.size()), "mirt_group_freeze_tiles"); }
	std::vector<uint32_t> TileCounts() {
		std::vector<uint32_t> counts(Tiles());
		check(mirt_group_tile_counts(group_, counts.data(), counts.size()), "mirt_group_tile_counts");
		return counts;
	}
	std::vector<uint32_t> NoiseAbove(float target, float floor = 0.0f) {   // usable pixels per tile with e > target; empty while Noise() is not ready
		std::vector<uint32_t> above(Tiles());
		const int rc = mirt_group_tile_above(group_, floor, target, above.data(), above.size());
		check(rc, "mirt_group_tile_above");
		if (rc != MIRT_OK) above.clear();
		return above;
	}
	// The freeze rule (mirt_adaptive_select; host code): `frozen` may be empty (none).
	static std::vector<uint8_t> AdaptiveSelect(const std::vector<float>& tiles, const std::vector<uint32_t>& above, const std::vector<uint8_t>& frozen, double quantile) {
		if (tiles.size() != above.size() * 4 || (!frozen.empty() && frozen.size() != above.size())) throw std::runtime_error("AdaptiveSelect: tiles, above and frozen must describe the same tiles");
		std::vector<uint8_t> out(above.size());
		if (mirt_adaptive_select(tiles.data(), above.data(), frozen.empty() ? nullptr : frozen.data(), above.size(), quantile, out.data()) < 0) throw std::runtime_error("mirt_adaptive_select: quantile is not in (0, 1]");
		return out;
	}
	// The adaptive loop (mirt_accumulate_adaptive): synchronous; converged = every tile froze before max_accumulations.
	struct AdaptiveResult { bool converged; mirt_adaptive_report report; };
	AdaptiveResult AccumulateAdaptive(const mirt_stop_rule& rule, uint32_t min_accumulations = 0) {
		AdaptiveResult r{};
		const int rc = mirt_group_accumulate_adaptive(group_, &rule, min_accumulations, &r.report);
		check(rc, "mirt_group_accumulate_adaptive");
		r.converged = rc == MIRT_OK;
		return r;
	}
	double gather_ms() const { double ms = 0; mirt_group_last_gather_ms(group_, &ms); return ms; }
	mirt_group* handle() { return group_; }

	const Scene& scene;
	std::vector<float> framebuffer;
	uint32_t width = 0, height = 0;

private:
	void check(int rc, const char* what) const {
		if (rc < 0) throw std::runtime_error(std::string(what) + ": " + mirt_group_last_error(group_));
	}
	mirt_group* group_ = nullptr;
	mirt_policy policy_{};
	bool lens_follows_camera_ = false;
};

} // namespace mirt
