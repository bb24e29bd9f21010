/* mirt.h — C-ABI of the MI355X-native replacement for the reference's
 * Renderer<Policy>::{Resize, ResetAccumulator, Accumulate, Render} hot path
 * (Borx25/CPU-Raytracing-experiments, Renderer.hpp:53-67,73-434,436-478).
 *
 * The reference has no FFI/plugin layer: the boundary is the C++ class `Renderer`
 * holding `const Scene&` (Renderer.hpp:38,51; instantiated Application.cpp:514).
 * Each entry point below names the reference member it stands in for.  Structs are
 * passed in the reference's exact byte layout so a host can hand over its
 * std::vector<Sphere>/<Material>/<Node> storage unchanged.
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every call returns an
 * int status (0 = MIRT_OK, >0 informational, <0 error) and never aborts
 * (the reference returns void and asserts/terminates: App.cpp:43-48, Application.cpp:226-229);
 * one context = one caller thread at a time; calls are synchronous unless named *_async;
 * host buffers are copied, never retained.
 */
#ifndef MIRT_H
#define MIRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIRT_OK              0
#define MIRT_NOT_READY       1   /* mirt_render before accumulations % buckets == 0 (Renderer.hpp:437) */
#define MIRT_ERR_ARG        -1
#define MIRT_ERR_HIP        -2
#define MIRT_ERR_STATE      -3
#define MIRT_ERR_NO_DEVICE  -4

#define MIRT_TILE_ROOT     16u   /* Renderer.hpp:32  (Policy.log_tile = 4) */
#define MIRT_TILE_SIZE    256u   /* Renderer.hpp:33 */
#define MIRT_MAX_MATERIALS 63u   /* Renderer.hpp:23,92 (max_materialID = 64, key -1 = miss) */
#define MIRT_MAX_BUCKETS   16u
#define MIRT_BVH_STACK     64u   /* DataStructures.hpp:26-44, BVH.hpp:127,321 */

/* Primitives.hpp:7-17 — alignas(16) {vec3 position; float radius_sq; int32 material_ID} = 32 B */
typedef struct mirt_sphere {
	float   position[3];
	float   radius_sq;
	int32_t material_ID;
	int32_t _pad[3];
} mirt_sphere;

/* Primitives.hpp:18-27 — alignas(32), 96 B.  The path reads albedo and emission with policy.brdf = 0 (Lambertian), F0, roughness
 * and emission with policy.brdf = 1 (GGX).  No closure of the reference reads F80, transmission or IOR_minus_one; transmission and
 * IOR_minus_one are read by this library's dielectric interface once mirt_set_transmission(ctx, 1) is called (below) and by nothing
 * otherwise; F80 is read by nothing. */
typedef struct mirt_material {
	float albedo[3];
	float F0[3];
	float F80[3];
	float emission[3];
	float transmission[3];
	float roughness;
	float IOR_minus_one;
	float _pad[7];
} mirt_material;

/* BVH.hpp:18-31 — alignas(32) {alignas(16) vec3 min; u32 first_id; alignas(16) vec3 max; u32 prim_count} = 32 B.
 * Leaf iff prim_count != 0 (prims [first_id, first_id+prim_count) of the BVH-order array);
 * inner: children at first_id and first_id+1. */
typedef struct mirt_bvh_node {
	float    min_bound[3];
	uint32_t first_id;
	float    max_bound[3];
	uint32_t prim_count;
} mirt_bvh_node;

/* RendererPolicy (Renderer.hpp:19-26) + the compile-time switches of the path, made runtime. */
typedef struct mirt_policy {
	uint32_t max_bounces;   /* Policy.max_bounces, Renderer.hpp:24 (bounce-loop iterations; seed stride 2*max_bounces+1, :107) */
	uint32_t buckets;       /* AccumulationBuckets, Renderer.hpp:41 (reference: 5; 1..16 accepted) */
	uint32_t mis;           /* #define MIS, Renderer.hpp:71 */
	uint32_t use_bvh;       /* #define USEBVH, BVH.hpp:307 (reference ships 0 = brute force) */
	uint32_t count_traffic; /* 1: kernels also count BVH nodes / spheres visited (slower; for the roofline's algorithmic bytes) */
	uint32_t profile;       /* 1: bracket every kernel launch with HIP events (mirt_get_kernel_times) */
	uint32_t max_batch;     /* Accumulate() calls traced together as one batch: 1..256, clamped to what the context's path ids and stream slots hold —
	                           2^30 / (its pixel count rounded up to a power of two), and pixels x batch + 12288 <= 2^30 (a context that owns all 2^24 pixels of a
	                           4096 x 4096 image: 63); 0 = auto, about 1 G primary rays per batch within the free device memory.  mirt_get_policy
	                           reports the value in effect.  Results do not depend on it: adds reach every bucket in accumulation order. */
	uint32_t reference_tree;/* 0 (default): traverse a GPU-internal SAH tree built over the same BVH-order prims; 1: traverse the caller's
	                         * nodes as handed over.  Results are identical either way (DESIGN.md "Traversal semantics"); read at mirt_set_scene. */
	uint32_t streams;       /* batches of accumulations kept in flight on separate HIP streams (0 = default 3, 1 = one kernel at a time).
	                         * Each in-flight batch renders into its own contribution buffer; the buffers are added to the accumulator in
	                         * accumulation order, so results do not depend on this value. */
	uint32_t gpu_build;     /* 1: the GPU-internal traversal tree is built on the GPU at mirt_set_scene (Morton-order LBVH, milliseconds) instead of
	                         * the host SAH sweep (better tree, 0.3 s per 100 k spheres): for the edit-rebuild loop (Application.cpp:508).  Results
	                         * are identical either way; ignored with reference_tree = 1 or fewer than 2 spheres.  Read at mirt_set_scene. */
	uint32_t trace_primary_rays; /* 0 (default): within a batch, the camera rays of a pixel (one jittered sample per accumulation of the batch, up to 256) share ONE cone traversal that lists the
	                         * spheres they can hit; each sample then tests only those, with the reference's arithmetic.  1: every primary ray walks the
	                         * tree by itself (measurements; the traversal-twin counter checks).  Results are identical either way. */
	uint32_t brdf;          /* #define BRDF, Renderer.hpp:70: 0 (default) = Closure<LambertianDiffuse>, 1 = Closure<GGX> for every hit
	                         * (DataStreams.hpp:184-219) with alpha = roughness^2 + (1 - roughness^2) * gloss decay of the bounce
	                         * (mirt_set_gloss_decay).  Its pdf() is 0 as in the reference: lights are reached by next-event estimation
	                         * only (an emitter hit by a sampled ray weighs powerHeuristic(0, .) = 0).  Other values: MIRT_ERR_ARG. */
} mirt_policy;

typedef struct mirt_counters {
	uint64_t rays;            /* rays handed to closest-hit traversal: primary + extension (Renderer.hpp:165) */
	uint64_t shadow_rays;     /* rays handed to any-hit traversal (Renderer.hpp:302) */
	uint64_t nodes;           /* BVH nodes box-tested by closest-hit traversal (count_traffic) */
	uint64_t spheres;         /* spheres tested by closest-hit traversal (count_traffic) */
	uint64_t shadow_nodes;
	uint64_t shadow_spheres;
	uint64_t terminated;      /* paths added into the accumulator (Renderer.hpp:424-430) */
	uint64_t dropped;         /* paths still alive after the last bounce, radiance dropped (Q5) */
} mirt_counters;

/* Kernel classes for mirt_get_kernel_times.  MIRT_K_TRACE includes the shadow rays and their deferred adds (traced in the
 * same launches); MIRT_K_SHADOW is kept for ABI stability and stays 0. */
enum { MIRT_K_RAYGEN = 0, MIRT_K_TRACE = 1, MIRT_K_SHADE = 2, MIRT_K_SHADOW = 3, MIRT_K_RESOLVE = 4, MIRT_K_COUNT = 5 };
typedef struct mirt_kernel_times {
	double   ms[MIRT_K_COUNT];        /* summed HIP-event time per kernel class since the last reset of the timers */
	uint64_t launches[MIRT_K_COUNT];
} mirt_kernel_times;

typedef struct mirt_ctx mirt_ctx;

/* Renderer(const Scene&) ctor, Renderer.hpp:51.  device = HIP device ordinal. */
int mirt_create(int device, mirt_ctx** out);
int mirt_destroy(mirt_ctx* ctx);
/* Last error text of ctx (or of the failed mirt_create when ctx == NULL). */
const char* mirt_last_error(const mirt_ctx* ctx);

/* BoundingVolumeHierarchy<Sphere> ctor, BVH.hpp:90-206 (host, runs on every scene edit, Application.cpp:233,508).
 * nodes_out capacity >= 2*n; prims_out capacity n (BVH-order copy of geometry, BVH.hpp:201-205). */
int mirt_bvh_build(const mirt_sphere* geometry, uint32_t n, mirt_bvh_node* nodes_out, uint32_t* n_nodes_out, mirt_sphere* prims_out);
/* LightingAcceleration ctor, Scene.hpp:12-16: geometry-order indices with dot(emission,emission) > 0. lights_out capacity n. */
int mirt_light_list(const mirt_sphere* geometry, uint32_t n, const mirt_material* materials, uint32_t n_materials,
                    int32_t* lights_out, uint32_t* n_lights_out);

/* The `const Scene& scene` the renderer reads (Scene.hpp:19-26): geometry (authoring order, used by NEE
 * Renderer.hpp:262), acceleration_structure.{nodes,prims}, material, lighting_acceleration.prims, sky
 * (Primitives.hpp:29-47; hdri_rgba = RGBA f32 texels, >= 1x1).  Call again after any scene edit
 * (Application.cpp:508-510); it does not reset the accumulator. */
int mirt_set_scene(mirt_ctx* ctx,
                   const mirt_sphere* geometry, const mirt_sphere* bvh_prims, uint32_t n_spheres,
                   const mirt_bvh_node* nodes, uint32_t n_nodes,
                   const mirt_material* materials, uint32_t n_materials,
                   const int32_t* lights, uint32_t n_lights,
                   const float ambient_color[3], const float* hdri_rgba, uint32_t hdri_w, uint32_t hdri_h);

/* scene.camera fields the path reads (Camera.hpp:80-88; Renderer.hpp:439): view.pos, view.orient (x,y,z,w),
 * projection.half_width / half_height / z, exp.
 * orient may be any finite quaternion and is used as handed over (glm's quat * vec3, then normalize: for |q| = s that is the
 * map (1 - s^2) I + s^2 R, a shear unless s = 1; the reference's own look-at returns one of norm sqrt(1/2) for a direction
 * parallel to up).  The camera rays' candidate lists bound a pixel's samples by a cone that assumes a rotation, with 1 % to
 * spare: a camera with ||q|^2 - 1| >= 1e-4 gets no lists — its camera rays walk the tree, as with trace_primary_rays = 1 —
 * and below that the stretch stays under 2.1e-4.  Results are identical to trace_primary_rays = 1 either way
 * (tests/test_views_and_scales.py). */
int mirt_set_camera(mirt_ctx* ctx, const float pos[3], const float orient_xyzw[4],
                    float half_width, float half_height, float z, float exposure);

/* ---- thin lens: depth of field and focus picking ------------------------------------------------------------------------
 * The reference's camera carries focus_distance, f_number and aperture_radius (Camera.hpp:6-45), its UI edits them (Application.cpp:413-417) and
 * a right-click picks the focus distance (Application.cpp:271-304), but generate_ray ignores all of it (Camera.hpp:80-88): the reference defines
 * no lens, so this mode has no reference text behind it (the test oracle carries the project's own: DESIGN.md section 2).  Here: a thin lens of radius aperture_radius around view.pos in the camera's x/y plane, focused on the
 * plane perpendicular to the optical axis at axial depth focus_depth, both in WORLD units (hosts convert the reference's millimetres; see
 * mirt_host.hpp / scene.py `unit_mm`).  Per sample: the pinhole direction d of Camera::generate_ray, unchanged; a lens point from two draws at the
 * seed offset the reference reserves and never uses (2 * max_bounces, Renderer.hpp:107) through its own disk mapping (Sampling.hpp:85-104);
 * the ray runs from the lens point through pos + d * (focus_depth / dot(d, forward)).  Arithmetic: csrc/device_math.hpp lens_ray.
 * aperture_radius = 0 (the default) IS the pinhole path: the same kernels and the same words as a context that never called this.
 * With a lens every camera ray walks the tree (the policy.trace_primary_rays = 1 route; mirt_get_policy still reports the caller's value).
 * Both arguments finite, aperture_radius >= 0, focus_depth > 0 when aperture_radius > 0: else MIRT_ERR_ARG.  Not available in exact stream
 * order (that mode replays the reference): aperture_radius > 0 under stream order 1, and mirt_set_stream_order(ctx, 1) with a lens on, return
 * MIRT_ERR_STATE.  Deferred mirt_accumulate_async calls are launched first, under the old lens; the accumulator is NOT reset (the caller
 * does, as Application.cpp:510). */
int mirt_set_lens(mirt_ctx* ctx, float aperture_radius, float focus_depth);
int mirt_get_lens(const mirt_ctx* ctx, float* aperture_radius, float* focus_depth);
/* The right-click pick, Application.cpp:271-304: one un-jittered (samples = {0.5, 0.5}) PINHOLE ray through pixel (x, y), lens or no lens, through the closest-hit traversal the context is configured with.  distance = tfar, INFINITY on a miss (:298); depth = distance * min(dot(d, forward), 1) is the axial depth of the hit, the value to hand to mirt_set_lens.  Changes no state; any pixel of the image, owned by this context or not; x >= width or y >= height: MIRT_ERR_ARG. */
int mirt_pick_focus(mirt_ctx* ctx, uint32_t x, uint32_t y, float* distance, float* depth);

int mirt_set_policy(mirt_ctx* ctx, const mirt_policy* policy);
int mirt_get_policy(const mirt_ctx* ctx, mirt_policy* policy);   /* with the values in effect for max_batch / streams left at 0 */
/* gloss_decay_table of Renderer.hpp:212 (policy.brdf = 1): decay[b] is mixed into the GGX alpha of the hits of bounce b; bounces at
 * or beyond n use 0.  n <= 1024; every value finite and in [0, 1], else MIRT_ERR_ARG.  decay = NULL or n = 0: all zeros (the
 * default).  Deferred mirt_accumulate_async calls are launched first, with the table they were issued under. */
int mirt_set_gloss_decay(mirt_ctx* ctx, const float* decay, uint32_t n);
/* Stream order (Q14).  exact = 0 (default): the wavefront pipeline; a path has no stream slot and every closest-hit test uses the FMA
 * form of BVH.hpp:250-268.  exact = 1: a fidelity mode that replays the reference's 256-ray stream of every (tile, accumulation) —
 * slot ID of bounce 0 is pixel ID, the hits are ordered by the stable counting sort on matID (DataStreams.hpp:221-253), the survivors
 * of Russian roulette are compacted in that order (Renderer.hpp:357-404) — and tests the last `active_rays % 8` slots of a stream
 * with the unfused scalar tail of BVH.hpp:270-286, as the shipped binary does.  Traversal is brute force over all spheres in this
 * mode (the reference as shipped, USEBVH false): policy.use_bvh, reference_tree, gpu_build and trace_primary_rays are accepted and
 * change nothing.  Everything else — closures, NEE, MIS, roulette, buckets, batching, policy.streams, tile ranges — is as in mode 0.
 * Several times slower than the default path; never the benched one.  Other values: MIRT_ERR_ARG.  Deferred mirt_accumulate_async
 * calls are launched first, in the mode they were issued under; the accumulator is not reset. */
int mirt_set_stream_order(mirt_ctx* ctx, uint32_t exact);
int mirt_get_stream_order(const mirt_ctx* ctx, uint32_t* exact);

/* ---- the NEE light by resampled importance sampling ------------------------------------------------------------------------
 * Next event estimation draws ONE light per hit, uniformly (Renderer.hpp:259; its author's note at :260 asks for something better), and with many
 * lights most draws are wasted: below the horizon, behind the surface, too far.  The reference ships RIS<count> and Reservoir::Update
 * (Sampling.hpp:25-54) and never calls them.  candidates = M > 0: per hit, M candidates are drawn from the NEE stream exactly as the plain
 * draw is (u0, u1, light; the stream just continues), each is carried to its MIS-weighted radiance rad_i by the unchanged NEE text, its weight is
 * w_i = max(rad_i.rgb) (0 if it left the text early; it still counts), and a weighted reservoir keeps one (one more draw per candidate:
 * replace when w_i > 0 and r < w_i / sum; the first candidate with w_i > 0 is taken whatever r, because the generator's r reaches 1.0f).  Still ONE shadow ray per hit, carrying rad_sel * (sum / (M * w_sel)); none if every w_i = 0.
 * Every candidate is distributed as the plain draw, so the estimator's expectation is exactly the plain path's: only the variance changes,
 * and the accumulator is NOT reset.  The emissive-hit MIS weight, the closure sample and the roulette are untouched: `rays` and `terminated`
 * do not change, `shadow_rays` does.  M = 1 is the plain path word for word (the one candidate is taken, sum / (1 * w) = 1), computed by the
 * RIS kernels.
 * candidates = 0 (the default): off — the same device code as a context that never called this.  1 .. MIRT_MAX_LIGHT_RIS: on.  Above:
 * MIRT_ERR_ARG.  Accepted and without effect with policy.mis = 0 or a scene without lights.  Not available in exact stream order (that mode
 * replays the reference): candidates > 0 under stream order 1, and mirt_set_stream_order(ctx, 1) with candidates > 0, return MIRT_ERR_STATE.
 * Deferred mirt_accumulate_async calls are launched first, under the old setting; the camera-ray candidate lists stay valid. */
#define MIRT_MAX_LIGHT_RIS 32u
int mirt_set_light_ris(mirt_ctx* ctx, uint32_t candidates);
int mirt_get_light_ris(const mirt_ctx* ctx, uint32_t* candidates);

/* ---- transmission: a smooth dielectric interface for the materials that carry one -----------------------------------------------
 * The reference's glass materials (Application.cpp:73-74,89-90: transmission, IOR_minus_one) are read by none of its closures, so by default
 * they render as the Lambertian or GGX balls their other fields describe.  on = 1: a material with tmax = max(transmission.rgb) > 0 is
 * transmissive, and a hit on it is shaded like this (the definition is this library's own: device_math.hpp dielectric_interface,
 * shade_hit_body.inc; float64 twin in tests/glass_definitions.py):
 *   - lobe: a hit reached from INSIDE its sphere (the geometric normal had to be flipped) always takes the interface; one from outside takes
 *     it when s0 < tmax; otherwise the hit is shaded by the unchanged text (NEE, emissive MIS, the policy's closure, roulette) with no
 *     reweighting — selection probability and lobe weight cancel, so transmission sweeps continuously from the opaque material to glass.
 *     s0, s1 are the 4th and 5th draws of the bounce's closure stream hash_2d(acc, seed + 2 * bounce + 1); a hit on any other material
 *     draws exactly what it draws with the switch off.
 *   - interface: no next event estimation (a delta closure).  n = 1 + IOR_minus_one, r = entering ? 1 / n : n, c = cos of incidence,
 *     sin2_t = r^2 (1 - c^2).  sin2_t >= 1: total internal reflection, weight 1.  Else unpolarised Fresnel F = (rs^2 + rp^2) / 2; s1 < F reflects
 *     (weight 1), otherwise the ray refracts by Snell's law, with weight transmission / tmax when ENTERING and 1 when leaving: the tint is a
 *     surface tint applied once per pass through the ball, not an absorption along the path inside.  The next origin is the hit moved 1e-4
 *     along the facing normal (reflection) or against it (refraction).  n == 1 in binary32: F = 0 and the ray keeps its direction bit for bit.
 *     All of it on world-space vectors: the hit's tangent frame is ill-conditioned near N.z = -1 and is not used here.
 *     The roulette then runs as ever on the new throughput, with the same third draw.
 *   - an emitter hit by a ray that left an interface weighs 1 under MIS (E = throughput * emission): no light sample could have made that
 *     path.  (policy.mis = 0 keeps Q9: E = emission.)  The miss shader is unchanged (Q10).
 * Not physical, on purpose: no 1 / eta^2 radiance scaling (it cancels for every path that enters a ball and leaves it; a camera inside glass
 * is not modelled); no medium stack — overlapping spheres are judged by the flipped normal alone; SHADOW RAYS TREAT GLASS AS OPAQUE, as every
 * sphere: light behind glass arrives only through extension rays (the item above), so there are no caustics by NEE; no roughness, no F80.
 * The first-hit AOVs are unchanged (albedo / F0 of the first hit).
 * on = 0 (the default): the same device code as a context that never called this.  on = 1 over a scene WITHOUT a transmissive material
 * launches that same code too.  Validation, with the switch on only: every transmission component must lie in [0, 1] and a transmissive
 * material needs a finite IOR_minus_one > -1, else MIRT_ERR_ARG — from mirt_set_scene, and from this call over the current scene (the
 * switch then stays off).  on > 1: MIRT_ERR_ARG.  Exact stream order and the switch exclude each other: MIRT_ERR_STATE both ways.
 * Deferred mirt_accumulate_async calls are launched first, under the old setting.  The estimand changes and the accumulator is NOT
 * reset: the caller does that (mirt_reset).  Combines with the lens, light RIS, AOVs, frozen tiles, the noise estimate, groups and both closures. */
int mirt_set_transmission(mirt_ctx* ctx, uint32_t on);
int mirt_get_transmission(const mirt_ctx* ctx, uint32_t* on);

/* ---- per-material closures: Lambertian and GGX materials in one scene ---------------------------------------------------------------
 * policy.brdf mirrors the reference's `#define BRDF` (Renderer.hpp:70): a frame is all Closure<LambertianDiffuse> or all Closure<GGX>, although
 * every mirt_material carries the fields of both.  closure[m], for material m, is 0 (Lambertian) or 1 (GGX); n <= MIRT_MAX_MATERIALS.  Any other
 * value, or a larger n, returns MIRT_ERR_ARG and changes nothing.  closure = NULL or n = 0 removes the table — the default: the same device
 * code as a context that never called this, every material taking policy.brdf.  Materials at index n or above take policy.brdf.  The table
 * survives mirt_set_scene and mirt_set_policy, like the gloss decay table.
 * Shading rule: a hit on material m is shaded, draw for draw, as policy.brdf = closure[m] shades it —
 *   - colour and set-up: albedo (Lambertian); F0 with alpha = r^2 + (1 - r^2) gloss_decay[bounce] (GGX);
 *   - the closure's eval in next event estimation, for sphere lights and the sky, under light RIS too;
 *   - the closure's pdf in the light sample's MIS weight: cos / pi (Lambertian), 0 (GGX);
 *   - the closure sample;
 *   - with sky sampling, the miss weight: the Lambertian heuristic, or 0 for GGX.
 *   The roulette and the dielectric interface of mirt_set_transmission are untouched.  No new estimator: every term is one of the two texts.
 *   pdf_in of an emitter hit (Q8) belongs to the closure that SAMPLED the ray: (1 / pi) max(0, D.z) after a Lambertian hit, 0 after a GGX hit —
 *   whatever the emitter's own material says.  "Sampled by GGX" travels with the surviving ray (bit 30 of the stream's path word).
 * Launch rule: if the effective closures of materials 0 .. n_materials - 1 of the current scene all equal k, the kernels of policy.brdf = k are
 *   launched — the same device code, that policy's words — and *mixed = 0.  Otherwise the MIXED kernels run (both branches in one wave, no
 *   sorting by material) and *mixed = 1.  The material LIST decides, not which materials the spheres use: an unused material of the other kind
 *   forces MIXED.  Without a scene *mixed = 0.
 * First-hit AOVs: the albedo plane holds albedo for a Lambertian material and F0 for a GGX one.
 * The estimand changes and the accumulator is NOT reset: the caller does that (mirt_reset).  Deferred mirt_accumulate_async calls are launched
 * first, under the old table.  Exact stream order and a non-empty table exclude each other: a non-empty table under stream order 1, and
 * mirt_set_stream_order(ctx, 1) with a non-empty table, return MIRT_ERR_STATE.  Combines with the lens, frozen tiles, light RIS, transmission,
 * sky sampling, AOVs, the noise estimate and groups; the camera-ray candidate lists stay valid.
 * mirt_get_material_closures: *n = entries of the table, *mixed as above; the table is copied to closure_out when capacity >= *n (closure_out
 * = NULL asks for the two numbers only; a non-NULL closure_out that is too small is MIRT_ERR_ARG). */
int mirt_set_material_closures(mirt_ctx* ctx, const uint8_t* closure, uint32_t n);
int mirt_get_material_closures(const mirt_ctx* ctx, uint8_t* closure_out, uint32_t capacity, uint32_t* n, uint32_t* mixed);

/* ---- sampling the environment map: the sky as one more light of next event estimation ---------------------------------------------
 * By default light from the environment map (hdri_rgba x ambient_color) reaches a surface only through an extension ray that misses every
 * sphere (the miss shader, thr.r x sky: Q10); the reference does no better, and its author's note at Renderer.hpp:260 asks for better light
 * sampling.  A map with a small bright sun then renders as fireflies.  on = 1, under ambient light and policy.mis = 1: THE SKY IS LIGHT NUMBER
 * n_lights.  This is this library's own definition (float64 twin: tests/sky_definitions.py).  The expectation is the plain path's; only the
 * variance changes, so the accumulator is NOT reset.
 *   The table.  Sky::operator() scales by w - 1 and h - 1 and truncates, so the image is seen through cols = max(w - 1, 1) by rows =
 *     max(h - 1, 1) CELLS; cell (r, c) is ex in [c, c + 1), ey in [r, r + 1) and shows texel (r, c); the last texel row and column have measure
 *     zero, and a 1 x 1 map is one cell that covers every direction.  Importance I = max(t.r amb.r, t.g amb.g, t.b amb.b) x Omega(r) (light
 *     RIS's weight rule times the cell's solid angle), Omega(r) = (2 pi / cols) (sin el(r) - sin el(r + 1)), el(r) = pi (0.5 - r / rows).  Stored:
 *     running sums of the row sums, running sums within each row, and per cell the density p = I / (Omega x total) in 1 / sr.  Two HIP kernels
 *     build it at mirt_set_scene while the switch is on, and when the switch is turned on over the current scene: a fixed summation order, no
 *     floating-point atomics — two builds of one map give the same words, so the members of a group hold identical tables.  Freed by on = 0.
 *   sky_sample(u0, u1) -> (dir, q): the row by inverting the marginal running sums at u0 x total, the column by inverting the row's at u1 x its
 *     sum; the rescaled remainders place the sample in the cell uniformly in sin(elevation) and in azimuth, so q = p(cell) is constant over it;
 *     dir is the inverse of the latitude-longitude map (u = 1/2 + atan2(z, x) / 2 pi, v = 1/2 - asin(y) / pi).  A row or cell whose running sum
 *     does not rise (below 2^-24 of what precedes it) is never drawn.
 *   sky_pdf(dir) -> p~: the density of the cell that the LOOKUP's own arithmetic (fast_atan2 / fast_asin, as the miss shader's) names for dir.
 *     Within the approximations' error of a cell edge this may be the neighbour of the cell that was drawn.  That is intended: the estimator
 *     divides by q, the density it sampled with, and WEIGHS by p~, a function of the direction alone that next event estimation and the miss
 *     shader both evaluate — the two MIS weights of any direction add to one, and the estimator is unbiased whatever those bands do.
 *   Next event estimation draws its light among n_lights + 1 (the same draws: u0, u1, the light, light RIS's r), light_selection_pdf is
 *     1 / (n_lights + 1) wherever it is read (the emissive-hit weight included), and a scene without a sphere light runs it too.  The sky draw:
 *     Ld, q = sky_sample(u0, u1); nothing below the shading horizon; radiance sky(Ld).rgb x (thr.r x f.r) — Q10 carried over — times
 *     w(sel p~, closure pdf) / (sel q) with w the reference's power heuristic; one shadow ray with tfar = FLT_MAX.  Under light RIS a sky candidate
 *     competes with the sphere candidates by its largest channel: the remedy for "a thousand lights and one sun".
 *   The miss shader weighs thr.r x sky by the power heuristic of the closure's LOCAL pdf of the direction, (1/pi) max(0, local z), against
 *     sel x p~: 0 under GGX (its pdf is 0, as for emitters), 1 after a dielectric interface and for camera rays.  The heuristic's 1e-6 floor
 *     (Sampling.hpp:241-247) loses at most about (pi x 1e-3)^2 of the cosine-weighted energy, where both pdfs are tiny; it is not worked round.
 * on = 0 (the default): the same device code as a context that never called this.  An all-zero table (a black map, ambient_color = 0),
 * policy.mis = 0 or no ambient light: accepted, no effect, that same code.  Validation, with the switch on only: a texel that owns a cell and
 * whose importance is negative or not finite (or a total beyond binary32) is MIRT_ERR_ARG — from mirt_set_scene, and from this call over the
 * current scene (the switch then stays off).  on > 1: MIRT_ERR_ARG.  Exact stream order and the switch exclude each other: MIRT_ERR_STATE both
 * ways.  Deferred mirt_accumulate_async calls are launched first, under the old setting.  rays and terminated do not change with the switch;
 * shadow_rays does.  Combines with both closures, light RIS, transmission, the lens, AOVs, frozen tiles, the noise estimate and groups; the
 * camera-ray candidate lists stay valid. */
int mirt_set_sky_sampling(mirt_ctx* ctx, uint32_t on);
int mirt_get_sky_sampling(const mirt_ctx* ctx, uint32_t* on);

/* ---- the GGX closure's pdf: two-way MIS for emitters and the sky on GGX surfaces ----------------------------------------------------
 * Closure<GGX>::pdf returns 0 in the reference ("TODO", DataStreams.hpp:196-198), and so it does here by default: on a GGX surface a ray the
 * closure sampled weighs powerHeuristic(0, .) = 0 at the emitter it hits — and, under sky sampling, at the sky it misses into — so every photon
 * arrives through next event estimation alone, weighted 1 / light_pdf.  On a low-roughness lobe that is the firefly case MIS exists for.
 * on = 1: wherever a hit is shaded by Closure<GGX> (policy.brdf = 1, or the material's closure under mirt_set_material_closures) the closure's
 * pdf is, in binary32 on local-frame vectors (normal = +z),
 *     p~(alpha, L, V) = (L.z > 0 && V.z > 0 && H.z > 0) ? G1_GGX(alpha^2, V.z^2) GGX_D(max(1e-5, alpha^2), H.z^2) / (4 V.z) : 0,   H = normalize(L + V)
 *   — Heitz 2018 eq. 17 with the D-floor microfacet_brdf already applies; float64 statement: tests/definitions.py ggx_vndf_pdf_of_direction.
 *   A V.z whose square underflows counts as V.z = 0.  Three places read it, and nothing else changes:
 *   1. next event estimation, sphere lights and the sky row: the closure pdf in the light sample's power heuristic is p~(alpha, Ll, Vl).  Light
 *      RIS reads nothing new (its weights come from the weighted radiance).
 *   2. the emitter hit: pdf_in of a ray that a GGX hit sampled is p~(alpha, sampled direction, Vl) of THAT hit.  It travels with the ray, in a
 *      4-byte plane per ray stream that is allocated only while the switch is on (the automatic batch plan counts it).  A Lambertian-sampled ray
 *      keeps Q8's word, (1 / pi) max(0, D.z) in world z, bit for bit; after a dielectric interface the weight stays 1.
 *   3. under sky sampling, the miss weight of a ray a GGX hit sampled: powerHeuristic(p~, sel x sky_pdf(dir)) instead of 0.
 *   p~ is a function of the direction alone and all three evaluate it, so each pair of MIS weights adds to one — the sky_pdf argument above —
 *   although the reference's sampler (turned axes and a clamp: DESIGN.md D7) is not exactly the visible-normal density, and also at alpha = 0,
 *   where the floor makes p~ large and finite: the mirror needs no special case.
 * The closure's sample, its estimator F G2 / G1, its eval, the roulette and the traversal read nothing new: rays, terminated and dropped are
 * word for word those of the switch off; shadow_rays may differ (a light sample whose weighted radiance rounds to 0 casts no ray).  The
 * estimand moves only by what the heuristic's 1e-6 floor and D7 allow, but it is formally another estimator, and the accumulator is NOT
 * reset: the caller does that (mirt_reset).
 * on = 0 (the default): the same device code as a context that never called this.  on = 1 while no material of the current scene ends up
 * GGX (policy.brdf = 0 without a table, or a table that makes every material Lambertian): that same code too.  on > 1: MIRT_ERR_ARG.  Exact
 * stream order and the switch exclude each other: MIRT_ERR_STATE both ways.  Deferred mirt_accumulate_async calls are launched first, under the
 * old setting.  Combines with the lens, frozen tiles, light RIS, transmission, sky sampling, per-material closures, AOVs, the noise estimate
 * and groups; the camera-ray candidate lists stay valid. */
int mirt_set_ggx_pdf(mirt_ctx* ctx, uint32_t on);
int mirt_get_ggx_pdf(const mirt_ctx* ctx, uint32_t* on);

/* ---- replacing the environment map on its own: the reference's SceneUpdate::Ambient ---------------------------------------------------
 * The reference tracks an edit of the sky apart from Geometry and Material (Application.cpp:335-347,503).  mirt_set_environment replaces the
 * environment map, its size and ambient_color exactly as mirt_set_scene would set them, and touches NOTHING else: the tree is not rebuilt, the
 * camera-ray candidate lists stay valid, the LDS plan stays, the temporal history is NOT dropped.  After it, accumulator, frame, AOVs and counters
 * equal, word for word, those of a fresh mirt_set_scene with the same scene and this environment — with sky sampling off and on (the table is
 * rebuilt: the same words).  The environment is part of the estimand and the accumulator is NOT reset: as with the shading switches, the caller
 * calls mirt_reset, and mirt_drop_history where it keeps a history.
 * hdri_rgba = NULL with w = h = 0 keeps the map and changes only ambient_color; otherwise hdri_rgba is w x h RGBA f32 texels, >= 1 x 1, copied.
 * Needs an earlier mirt_set_scene: else MIRT_ERR_STATE.  Deferred mirt_accumulate_async calls are launched first, under the old environment, and
 * every stream is waited for before the map is overwritten.  With sky sampling on the new texels (the kept ones under the new ambient_color) pass
 * mirt_set_sky_sampling's validation BEFORE anything is changed: on MIRT_ERR_ARG the old environment is in place, bit for bit.  Allowed in exact
 * stream order: the map is data. */
int mirt_set_environment(mirt_ctx* ctx, const float ambient_color[3], const float* hdri_rgba, uint32_t w, uint32_t h);
/* The map the kernels read, copied from the device after the context's stream has been synchronised.  info[0] width, info[1] height, info[2] 1 if
 * the map was baked by mirt_set_sun_sky and 0 if a caller handed it over, info[3] 0.  rgba_out == NULL: only `info` is filled.  MIRT_ERR_ARG when
 * capacity_floats < 4 * width * height; MIRT_ERR_STATE before mirt_set_scene. */
int mirt_read_environment(mirt_ctx* ctx, float* rgba_out, size_t capacity_floats, uint32_t info[4]);

/* ---- analytic sun and sky: a Preetham daylight sky and a sun disc, baked on the device into the environment map -------------------------
 * mirt_set_sun_sky is mirt_set_environment with the context's current ambient_color and a map of width x height texels that kernel k_sun_sky
 * (csrc/sun_sky.hpp) writes straight into the context's buffer: no host image, no upload.  Everything above holds (nothing else is touched; the
 * caller resets).  The reference has no procedural sky; nothing of it is replayed.  Model: Preetham, Shirley, Smits 1999 for the sky; for the disc
 * an extraterrestrial radiance of 1.9e6 kcd/m^2 behind Rayleigh and aerosol optical depths at the Kasten-Young air mass.
 * THE DEFINITION — this text is the authority; float64 statement and binary32 numpy twin: tests/sun_sky_definitions.py.
 *   Cells.  They are sky_eval's own (see "sampling the environment map"): cols = w - 1, rows = h - 1.  Texel (r, c), r < rows, c < cols, is seen
 *     through azimuth phi in 2 pi (c / cols - 1/2) + [0, 2 pi / cols) and elevation between el(r) and el(r + 1), el(k) = pi (1/2 - k / rows).  Texel
 *     column w - 1 is computed as column 0 and texel row h - 1 as row rows - 1 (what sky_eval reads when ex == fw or ey == fh): the same words.
 *   Sub-samples.  A texel is the mean of a fixed 4 x 4 grid, midpoints in sin(el) and in phi, so each carries the same solid angle: i = 0..3 from
 *     the upper edge down (outer), j = 0..3 in rising phi (inner); sum = (((v_00 + v_01) + v_02) + ...), texel = sum * 0.0625f, alpha = 1.
 *     phi_j = PI_F * ((float)(8 c + 2 j + 1 - 4 cols) / (float)(4 cols))            (the integer is exact; PI_F = 3.14159274f)
 *     edge(k) = 2.0f * (h * h), h = sinf(1.57079637f * ((float)k / (float)rows))     (= 1 - sin el(k), the distance from the pole)
 *     a cell with 2 r + 1 <= rows is measured from y = +1: ta = edge(r), tb = edge(r + 1), t_i = ta + ((2 i + 1) / 8) * (tb - ta), y = 1.0f - t_i;
 *     any other from y = -1: ta = edge(rows - r), tb = edge(rows - r - 1), the same t_i, y = t_i - 1.0f.   ce = sqrtf(t_i * (2.0f - t_i)).
 *     d = (ce * cosf(phi_j), y, ce * sinf(phi_j)): the inverse of sky_eval's map u = 1/2 + fast_atan2(d.z, d.x) / 2 pi, v = 1/2 - fast_asin(d.y) / pi;
 *     fast_atan2(z, x) is the angle of (x, z) from +x towards +z, in (-pi, pi].
 *   Sky.  e = d above the horizon; where y < 0, e = (cosf(phi_j), 0, sinf(phi_j)), the foot of d on the horizon, and the result is multiplied by
 *     `ground`: the lower hemisphere is the horizon ring, tinted.  ct = max(e.y, 1/64).  gamma = 2.0f * atan2f(|e - sun|, |e + sun|) (lengths by
 *     dot3 and sqrtf: the angle between e and the sun without the cancellation of acos near 0 and pi); cg = dot3(e, sun).  For each of Y, x, y,
 *     with A..E the Perez coefficients:  F = (1.0f + A * expf(B / ct)) * ((1.0f + C * expf(D * gamma)) + E * (cg * cg));  value = (zenith * F) * inv_F0,
 *     inv_F0 = 1 / F(0, theta_s).  X = (x / y) * Y;  Z = (((1.0f - x) - y) / y) * Y;  linear Rec.709:
 *       R = (3.2404542f X + -1.5371385f Y) + -0.4985314f Z;  G = (-0.9692660f X + 1.8760108f Y) + 0.0415560f Z;  B = (0.0556434f X + -0.2040259f Y) + 1.0572252f Z
 *     each clamped below at 0, times sky_scale, times ground where y < 0.
 *     Coefficients, linear in the turbidity T:
 *       Y: A = 0.1787 T - 1.4630, B = -0.3554 T + 0.4275, C = -0.0227 T + 5.3251, D = 0.1206 T - 2.5771, E = -0.0670 T + 0.3703
 *       x: A = -0.0193 T - 0.2592, B = -0.0665 T + 0.0008, C = -0.0004 T + 0.2125, D = -0.0641 T - 0.8989, E = -0.0033 T + 0.0452
 *       y: A = -0.0167 T - 0.2608, B = -0.0950 T + 0.0092, C = -0.0079 T + 0.2102, D = -0.0441 T - 1.6537, E = -0.0109 T + 0.0529
 *     Zenith: Y_z = (4.0453 T - 4.9710) tan(chi) - 0.2155 T + 2.4192 kcd/m^2, chi = (4/9 - T/120)(pi - 2 theta_s);  x_z = [T^2 T 1] M_x [theta_s^3
 *       theta_s^2 theta_s 1]^T, y_z likewise, with rows
 *       M_x: (0.00166, -0.00375, 0.00209, 0), (-0.02903, 0.06377, -0.03202, 0.00394), (0.11693, -0.21196, 0.06052, 0.25886)
 *       M_y: (0.00275, -0.00610, 0.00317, 0), (-0.04214, 0.08970, -0.04153, 0.00516), (0.15346, -0.26756, 0.06670, 0.26688)
 *   Sun.  L_rgb = sun_scale * 1.9e6 * exp(-tau m) at 0.68, 0.55, 0.44 um, tau = 0.008735 lambda^-4.08 + (0.04608 T - 0.04586) lambda^-1.3,
 *     m = 1 / (cos theta_s + 0.50572 (96.07995 - theta_s in degrees)^-1.6364).  Added to EVERY sub-sample, below the horizon too and untinted, with weight
 *     clamp((cos g - cos a) / (cos 0.9 a - cos a), 0, 1), a = sun_radius, g the angle between d and the sun, evaluated as
 *       wgt = min(max(0, (edge_a - 0.5f * dot3(d - sun, d - sun)) * ramp_inv), 1),   edge_a = 1 - cos a,  ramp_inv = 1 / (cos 0.9 a - cos a)
 *     (1 - cos g = |d - sun|^2 / 2 for unit vectors: the ramp is 34 binary32 steps of cos g wide at the default radius, and this form does not
 *     lose them).  The linear limb is deliberate: a hard edge would let one rounding flip a sub-sample between the kernel and its float64
 *     statement; with the ramp every texel is a continuous function of its inputs and one bound holds for all of them.
 *   Host.  Everything that depends on the sun alone is computed once on the host in float64, rounded to binary32 once and passed to the kernel: the
 *     unit sun_dir, the fifteen coefficients, the three inv_F0, Y_z, x_z, y_z, L_rgb, edge_a and ramp_inv (csrc/sun_sky_host.hpp).  The device needs
 *     no pow and no tan: per texel eight sinf / cosf for phi and two sinf for the edges, per sub-sample one atan2f, six expf, three sqrtf and the
 *     divisions — the device library's full-precision functions, IEEE division and square root, nothing fused.
 * One thread per texel, a fixed order, no atomics: two bakes of the same parameters give the same words, on every device of a group.
 * MIRT_ERR_ARG, nothing changed: params NULL, a field not finite, sun_dir of zero length or with y < 0 (twilight is not modelled), turbidity outside
 * [2, 10], sun_radius outside (0, 0.1], a negative scale, width or height below 2 or above 32768.  MIRT_ERR_STATE before mirt_set_scene.
 * mirt_sun_sky_defaults (pure host code, no context): sun_dir (0.3, 0.9, 0.3), turbidity 3, sun_radius 0.00465, sky_scale = sun_scale = 0.1 (one
 * render unit per 10 kcd/m^2), ground 0.1, 1025 x 513 texels.  Starting values and design choices, not measurements. */
typedef struct mirt_sun_sky_params {
	float    sun_dir[3];     /* towards the sun, world space, y up as sky_eval has it; normalised by the library; y >= 0 */
	float    turbidity;      /* 2 .. 10 */
	float    sun_radius;     /* angular radius in rad, in (0, 0.1]; default 0.00465 */
	float    sky_scale;      /* render units per kcd/m^2 of sky luminance, >= 0 */
	float    sun_scale;      /* the same for the disc; 0 = no disc */
	float    ground[3];      /* tint of the lower hemisphere */
	uint32_t width, height;  /* texels of the baked map, each in [2, 32768] */
} mirt_sun_sky_params;
int mirt_sun_sky_defaults(mirt_sun_sky_params* out);
int mirt_set_sun_sky(mirt_ctx* ctx, const mirt_sun_sky_params* params);

/* ---- moving spheres in place: the reference's SceneUpdate::Geometry without a rebuild ---------------------------------------------------
 * The reference's editor drags or resizes a sphere (Application.cpp:466-468) and rebuilds its BVH on the host (:508).  mirt_update_spheres is
 * that edit for spheres that keep their place in both arrays: sphere bvh_index[i] of the BVH-order array hit.primID refers to — the same sphere
 * as geometry_index[i] of the authoring-order geometry — takes centre and radius_sq xyz_rsq[4 i .. 4 i + 3].  NOTHING else changes: the order of
 * both arrays, the material ids, the materials, the light list and the environment stay; no other sphere is uploaded again, no tree is built, no
 * environment map is uploaded.  THE CALLER'S BVH ORDER IS KEPT.  The order is part of the result (Renderer.hpp:261-263 compares hit.primID with
 * geometry-order light ids), so the update renders the scene "old order, new spheres" — a valid Scene, not necessarily the order the
 * reference's builder would pick after the move.  After it, accumulator, frame, AOVs and the rays, shadow_rays, terminated and dropped counters
 * equal, word for word, those of a fresh context given mirt_set_scene with the edited geometry and bvh_prims IN THE SAME ORDER, the same nodes and
 * everything else unchanged — under every policy and in exact stream order.  The nodes and spheres counters of count_traffic may differ: they
 * describe the tree, and the tree in place keeps its topology (DESIGN.md "Traversal semantics": results do not depend on it).
 * Geometry is part of the estimand and the accumulator is NOT reset: the caller calls mirt_reset, as Application.cpp:510 does.
 * Deferred mirt_accumulate_async calls are launched first, under the old geometry, and every stream is waited for.  Then: the edited rows of
 * the sphere table are scattered (k_update_spheres); EVERY box of the records the kernels walk is recomputed on the device over the topology in
 * place (k_refit, csrc/refit.hpp) — leaf boxes as mirt_set_scene makes them, r = sqrt(radius_sq), pad = 2^-18 (max|c| + r), one binary32 step
 * outward; inner boxes their unions; binary16 planes rounded outward — which are the words a fresh build over that topology writes; the row of
 * every light whose geometry id is edited is replaced; the camera-ray candidate lists are rebuilt by the next batch; the temporal history is
 * dropped (surfaces moved) unless mirt_set_sphere_motion is on, which follows the move instead.  Not touched: the material tables, the environment and its sampling table, the LDS plan, the switches.
 * How far a tree may be refitted before mirt_set_scene pays is the caller's decision (DESIGN.md section 4 has measurements).
 * Everything is checked BEFORE anything changes — a refused call leaves every word in place:  MIRT_ERR_STATE before mirt_set_scene;
 * MIRT_ERR_ARG for a NULL array with n > 0, an index >= n_spheres, a bvh_index or a geometry_index that occurs twice in one call, a value that
 * is not finite or radius_sq < 0 (mirt_set_scene's rules);  MIRT_ERR_STATE when the records in place are binary16 (child-pair or 4-wide) and an
 * edited sphere does not fit them — a coordinate beyond 60000 or a diameter under 8 binary16 steps at its magnitude, the rule mirt_set_scene
 * applies per sphere when it chooses the layout: a refit does not change layouts, call mirt_set_scene.  With f32 records the same edit is
 * accepted.  n = 0: MIRT_OK, nothing done. */
int mirt_update_spheres(mirt_ctx* ctx, uint32_t n,
                        const uint32_t* bvh_index,       /* index into the BVH-order prims hit.primID refers to */
                        const uint32_t* geometry_index,  /* index of the same sphere in the authoring-order geometry */
                        const float*    xyz_rsq);        /* n x {position.x, .y, .z, radius_sq} */

/* ---- updating materials in place: the reference's SceneUpdate::Material without a rebuild ---------------------------------------------
 * Every colour picker and slider of the reference's material panel (Application.cpp:477-485: albedo, F0, emission, transmission, roughness,
 * IOR) and the sphere's material selector (:470, geometry[i].material_ID) raise SceneUpdate::Material, on which the reference rebuilds its
 * LightingAcceleration (:347,509; Scene.hpp:12-16).  mirt_update_materials is that edit:  material material_index[i] := rows[i] (n_rows of
 * them), and sphere bvh_index[i] of the BVH-order array — the same sphere as geometry_index[i] of the authoring-order geometry, as in
 * mirt_update_spheres — takes material material_ID[i] (n_assign of them).  Either half may be empty.  THE NUMBER OF MATERIALS CANNOT CHANGE.
 * After it, accumulator, frame, AOVs and the rays, shadow_rays, terminated and dropped counters equal, word for word, those of a fresh
 * context given mirt_set_scene with the edited materials, the edited material_IDs in geometry and bvh_prims IN THE SAME ORDER, the same nodes,
 * the same environment and lights = mirt_light_list(edited geometry, edited materials) — under every policy, both closures, a closure table,
 * transmission, sky sampling, light RIS, the GGX pdf, the lens, frozen tiles, and in exact stream order.  THE LIGHT LIST IS ALWAYS REPLACED BY
 * THE REFERENCE'S RULE, even if mirt_set_scene was handed another list: an edited emission or material_ID creates and removes lights, so the
 * two per-light tables of next event estimation are regenerated on the device in geometry order (csrc/light_list.hpp: an ordered stream
 * compaction over a geometry-order copy of the spheres that mirt_set_scene uploads and both updates keep current; whether a material emits
 * is decided per material on the host by the expression of mirt_light_list, (e0 e0 + e1 e1) + e2 e2 > 0 in binary32), and n_lights moves —
 * with it the Q12 MIS guard, the sky's light number under sky sampling and light RIS's candidate range.
 * Materials are part of the estimand and the accumulator is NOT reset: the caller calls mirt_reset, as Application.cpp:510 does.  Deferred
 * mirt_accumulate_async calls are launched first, under the old materials, and every stream is waited for.
 * Not touched: the spheres' positions, the records, the refit links, the camera-ray candidate lists (they name spheres, not materials), the
 * LDS plan, the environment and its sampling table, the closure table (mirt_set_material_closures).  KEPT: the temporal history — surfaces did
 * not move; as with the environment and the shading switches the caller calls mirt_drop_history beside mirt_reset.
 * Everything is checked BEFORE anything changes — a refused call leaves every word in place:  MIRT_ERR_STATE before mirt_set_scene;
 * MIRT_ERR_ARG for a NULL array with a non-zero count, a material_index >= n_materials or one that occurs twice in one call, a bvh_index or
 * geometry_index >= n_spheres or one that occurs twice in one call, a material_ID outside [0, n_materials), and, with mirt_set_transmission
 * on, a RESULTING material table that breaks its rules (transmission in [0, 1], a finite IOR above 0 for a transmissive material).  Material
 * values are otherwise not validated, as in mirt_set_scene.  Both counts 0: MIRT_OK, nothing done. */
int mirt_update_materials(mirt_ctx* ctx,
                          uint32_t n_rows,   const uint32_t* material_index, const mirt_material* rows,   /* material material_index[i] := rows[i] */
                          uint32_t n_assign, const uint32_t* bvh_index, const uint32_t* geometry_index,   /* the same sphere in both orders */
                                             const int32_t*  material_ID);                                /* ... takes this material */

/* Renderer::Resize, Renderer.hpp:53-63: h_tiles = w/16, v_tiles = h/16 (truncating), allocates and zeroes
 * the accumulator, accumulations = 0.  Owns all tiles until mirt_set_tile_range says otherwise. */
int mirt_resize(mirt_ctx* ctx, uint32_t width, uint32_t height);
/* Multi-GPU sharding of the parallel_for range (Renderer.hpp:75): this context renders LaunchIndex in
 * [first_tile, first_tile + n_tiles).  RNG seeds use the global LaunchIndex (Renderer.hpp:107), so any
 * partition reproduces the single-context result bit for bit.  Reallocates and zeroes the accumulator. */
int mirt_set_tile_range(mirt_ctx* ctx, uint32_t first_tile, uint32_t n_tiles);
/* The same with interleaved tile rows: this context renders the tile rows first_row, first_row + row_stride, ... (a tile row =
 * width/16 consecutive LaunchIndices).  With rank r of N taking (r, N) every GPU sees the whole image height, sky and ground
 * alike: contiguous eighths of the weak-scaling image differ by 1.5x in cost (profiles/experiments/shard_balance.py).  The
 * accumulator slab holds the owned rows in ascending order.  Reallocates and zeroes the accumulator. */
int mirt_set_tile_rows(mirt_ctx* ctx, uint32_t first_row, uint32_t row_stride);
/* Renderer::ResetAccumulator, Renderer.hpp:64-67 */
int mirt_reset(mirt_ctx* ctx);

/* n_calls x Renderer::Accumulate(), Renderer.hpp:73-434 (each call = 1 sample per pixel, ++accumulations first). */
int mirt_accumulate(mirt_ctx* ctx, uint32_t n_calls);
/* Same, without waiting for the GPU.  Whole batches (policy.max_batch) are enqueued on the context's HIP streams at once; a
 * remainder is kept until later calls complete the batch or something needs it — mirt_synchronize, mirt_render when a frame
 * is due, any read of results, any change of scene / camera / policy (the deferred calls are launched with the state they
 * were issued under).  A host that calls this once per frame, as the reference's UI loop calls Accumulate() (Application.cpp:379),
 * therefore still gets full-size launches: 2.1 ms -> 0.8 ms per 1024x1024 frame with Render() called every frame (due every 5th). */
int mirt_accumulate_async(mirt_ctx* ctx, uint32_t n_calls);
/* Launches anything deferred and waits for the GPU. */
int mirt_synchronize(mirt_ctx* ctx);
/* Accumulate() calls issued so far (launched or deferred). */
int mirt_get_accumulations(const mirt_ctx* ctx, uint32_t* accumulations);

/* `accumulator` member, Renderer.hpp:43-46: [local tile][bucket][r,g,b][256] f32. */
int mirt_accumulator_floats(const mirt_ctx* ctx, size_t* n_floats);
int mirt_read_accumulator(mirt_ctx* ctx, float* host_dst);
/* Device address of that slab (for an RCCL gather by the caller); valid until the next resize / tile-range call.
 * Launches anything deferred and waits for the GPU first, so the slab is complete whatever stream the caller reads it on. */
int mirt_accumulator_device(mirt_ctx* ctx, void** device_ptr, size_t* bytes);
/* Checkpoint/resume and post-gather resolve: overwrite the slab (src on host or device) and set `accumulations`. */
int mirt_load_accumulator(mirt_ctx* ctx, const float* src, int src_is_device, uint32_t accumulations);

/* Renderer::Render, Renderer.hpp:436-478: median over buckets * exposure/(accumulations/buckets), ACES tonemap,
 * RGBA f32 row-major width*height (row 0 = y 0), A = 1.  Returns MIRT_NOT_READY and leaves rgba_host untouched
 * when accumulations % buckets != 0.  Only the context's own tiles are written: pixels of other contexts' tiles, and the pixels no
 * tile owns when width or height is no multiple of 16 (columns 16 (width / 16) .. width - 1, rows 16 (height / 16) .. height - 1), are
 * left as the caller handed them.  That is the rule of every resolve below (mirt_render_aov, mirt_noise's map, mirt_render_atrous,
 * mirt_render_temporal's frame and history_len, and their mirt_group_* namesakes); mirt_id_map alone covers all width x height pixels. */
int mirt_render(mirt_ctx* ctx, float* rgba_host);

/* ---- first-hit AOVs: depth, normal and albedo of the camera rays, summed beside the accumulator ---------------------
 * The reference's `FIRST BOUNCE OUTPUTS` (Renderer.hpp:216-231, written down but compiled out): on bounce 0 every pixel adds its hit
 * distance (1e4 on a miss), its world-space shading normal (flipped to face the ray, as the closest-hit shader leaves it) and the
 * colour its closure is set up with (Renderer.hpp:208-210: material.albedo with policy.brdf = 0, material.F0 with brdf = 1; nothing
 * on a miss) into extra planes.  Slab: [local tile][plane 0..6][256] f32 — plane 0 depth, 1-3 normal, 4-6 albedo; the shape of
 * AccumulationTile with seven planes instead of buckets x 3.  Not bucketed: ONE f32 sum over the accumulations 1, 2, 3, ... since the
 * last reset, added in that order, so the words do not depend on policy.max_batch / streams / trace_primary_rays / use_bvh /
 * reference_tree / gpu_build, on mirt_accumulate vs mirt_accumulate_async, or on the tile partition.  The accumulator, the frame and
 * the counters are the same with AOVs on or off; off (the default) costs nothing.
 * Not available in exact stream order: that mode runs a tile's whole bounce loop in one launch and keeps no hit records to read, so
 * mirt_set_aov(ctx, 1) with stream order 1, and mirt_set_stream_order(ctx, 1) with AOVs on, return MIRT_ERR_STATE. */
enum { MIRT_AOV_DEPTH = 0, MIRT_AOV_NORMAL = 1, MIRT_AOV_ALBEDO = 2 };
#define MIRT_AOV_PLANES 7u
/* on = 1: allocates and zeroes the slab; accepted only while accumulations == 0 (the sums would cover fewer samples than the frame:
 * MIRT_ERR_STATE; mirt_reset first).  on = 0: any time; deferred mirt_accumulate_async calls are launched first, under the old
 * setting, then the slab is freed.  Other values: MIRT_ERR_ARG.  mirt_reset zeroes the slab; mirt_resize, mirt_set_tile_range,
 * mirt_set_tile_rows (and a mirt_set_policy that changes `buckets`) reallocate and zero it with the accumulator. */
int mirt_set_aov(mirt_ctx* ctx, uint32_t on);
int mirt_get_aov(const mirt_ctx* ctx, uint32_t* on);
int mirt_aov_floats(const mirt_ctx* ctx, size_t* n_floats);       /* local tiles x 7 x 256; 0 while AOVs are off */
/* The raw sums.  Launches anything deferred and waits for the GPU first.  MIRT_ERR_STATE while AOVs are off (as the three below). */
int mirt_read_aov(mirt_ctx* ctx, float* host_dst);
/* Device address of the slab, as mirt_accumulator_device (mirt_group_gather uses it). */
int mirt_aov_device(mirt_ctx* ctx, void** device_ptr, size_t* bytes);
/* Companion of mirt_load_accumulator (checkpoint/resume, post-gather resolve): overwrites the slab, src on host or device. */
int mirt_load_aov(mirt_ctx* ctx, const float* src, int src_is_device);
/* One AOV resolved row-major over width x height (row 0 = y 0); only the context's own tiles are written.
 *   MIRT_AOV_DEPTH   1 float per pixel    sum / (float)accumulations
 *   MIRT_AOV_NORMAL  3 floats per pixel   normalize(sum) — v * (1 / sqrt(dot(v, v))), dot = (x*x + y*y) + z*z — or (0,0,0) where dot is 0
 *   MIRT_AOV_ALBEDO  3 floats per pixel   sum / (float)accumulations
 * IEEE division and square root.  Unlike mirt_render it needs no multiple of `buckets`; returns MIRT_NOT_READY and leaves `out`
 * untouched while accumulations == 0. */
int mirt_render_aov(mirt_ctx* ctx, int which, float* out);

/* ---- per-pixel noise estimate from the buckets, and render-until-converged -------------------------------------------------
 * The `buckets` sub-images that Render() takes a median of (Renderer.hpp:41,453-455) are k independent estimates of every pixel, so their
 * spread estimates the pixel's error.  The reference has no such read-out (its UI plots frame times); nothing of it is replayed here.
 * THE QUANTITY, for a pixel of an owned tile, when accumulations % buckets == 0 and buckets = k >= 2; r_j, g_j, b_j the raw accumulator
 * words of bucket j; scale = exposure / (float)(accumulations / k), the value mirt_render uses; every operation binary32, in this order,
 * unfused, IEEE division and square root:
 *     y_j  = scale * ((0.2126f * r_j + 0.7152f * g_j) + 0.0722f * b_j)            j = 0 .. k-1
 *     mean = (((y_0 + y_1) + y_2) + ...) / (float)k
 *     var  = (((d_0*d_0 + d_1*d_1) + d_2*d_2) + ...) / (float)(k - 1),            d_j = y_j - mean
 *     se   = sqrt(var / (float)k)
 *     e    = (mean + floor == 0) ? 0 : se / (mean + floor)
 * `floor` (finite, >= 0, in exposure-scaled radiance units) keeps black pixels from dominating.  e is the relative standard error of the
 * MEAN of the bucket means, before tonemapping — deliberately the error of the mean and not of the median that mirt_render shows: a
 * firefly in one bucket raises e although the median ignores it, so e is conservative there, the safe side for a stopping rule.
 * A pixel is USABLE when the word of e is below 0x7f800000, i.e. e is finite and its sign bit is clear.  Any non-finite bucket word
 * gives a non-finite e; a negative mean + floor (negative radiance, which no path produces) gives an e with the sign bit set.  Such
 * pixels keep their e in the map and are counted as non-finite; they never enter the maximum, the tile means or the histogram.
 * Reads only the accumulator slab, so it works in every mode (either closure, lens, AOVs, exact stream order, any tile partition). */
#define MIRT_NOISE_BINS 2048u    /* histogram bin of a usable e: its word >> 20 — eight linear sub-bins per binary octave */
#define MIRT_NOT_CONVERGED 2     /* mirt_accumulate_until reached max_accumulations */
typedef struct mirt_noise_stats {
	uint64_t owned_pixels;       /* 256 x the context's tiles */
	uint64_t finite_pixels;      /* usable pixels */
	uint64_t nonfinite_pixels;   /* owned - usable */
	float    max;                /* largest usable e (0 when there is none) */
	uint32_t _pad;
	double   mean;               /* of the usable e: formed on the host in double from the tile records, sum of mean[t] * count[t] over the local
	                                tiles t in ascending order, divided by finite_pixels (0 when there is none) */
} mirt_noise_stats;
/* Any of map_out, tile_out, hist_out may be NULL.  map_out: width * height floats, row-major (row 0 = y 0); only the context's own tiles
 * are written, the rest of the caller's buffer is left untouched (the rule of mirt_render_aov).  tile_out: 4 floats per local tile,
 * {max, mean over the usable pixels, usable count, non-finite count} (counts as floats, exact; max and mean 0 for a tile without a usable
 * pixel).  hist_out: MIRT_NOISE_BINS words.  Launches anything deferred and waits for the GPU first; changes no state (accumulator, frame,
 * counters); kernel time is booked under MIRT_K_RESOLVE.
 * MIRT_NOT_READY with every output untouched when accumulations == 0 or accumulations % buckets != 0; MIRT_ERR_STATE when buckets < 2;
 * MIRT_ERR_ARG when floor is negative or not finite.  A context that owns no tile returns MIRT_OK with zero counts (and a zero histogram). */
int mirt_noise(mirt_ctx* ctx, float floor, float* map_out, float* tile_out, uint32_t* hist_out, mirt_noise_stats* stats);
/* Pure host code: no context, no GPU.  *value = the UPPER EDGE of the bin that holds the q-quantile of the usable pixels — the pixel of
 * rank ceil(q * n) among the n sorted values (rank at least 1).  It overstates the quantile by at most one sub-bin, 12.5 % relative: the
 * safe side for a stopping rule.  q in (0, 1], else MIRT_ERR_ARG; an empty histogram: MIRT_NOT_READY, *value untouched. */
int mirt_noise_quantile(const uint32_t* hist, double q, float* value);
typedef struct mirt_stop_rule {
	float    target;             /* stop when the quantile's bin edge is <= target ... */
	float    quantile;           /* ... for this q in (0, 1] of the usable pixels (0.95: nineteen pixels in twenty are below target) */
	float    floor;              /* mirt_noise's */
	uint32_t check_every;        /* accumulations between two checks: a positive multiple of `buckets` */
	uint32_t max_accumulations;  /* total (not additional) accumulations at which to give up */
} mirt_stop_rule;
/* A host loop: mirt_accumulate(check_every), then mirt_noise.  MIRT_OK as soon as the quantile is <= target and no pixel is non-finite;
 * MIRT_NOT_CONVERGED once accumulations >= max_accumulations (the last step is shortened to land on the largest multiple of `buckets`
 * that does not pass it).  *last: the stats of the last check (zeros if none ran), *issued: accumulations added by this call; either
 * may be NULL.  MIRT_ERR_ARG unless check_every is a positive multiple of `buckets`, target and floor are finite and >= 0 and quantile
 * is in (0, 1]; MIRT_ERR_STATE when buckets < 2 or the current count is not a multiple of `buckets`.  The accumulator afterwards is,
 * word for word, that of the same number of plain mirt_accumulate calls. */
int mirt_accumulate_until(mirt_ctx* ctx, const mirt_stop_rule* rule, mirt_noise_stats* last, uint32_t* issued);

/* ---- per-tile adaptive sampling: converged tiles stop taking samples --------------------------------------------------------------
 * mirt_accumulate_until samples the whole image until its quantile is quiet; most 16 x 16 tiles are quiet long before the last few.  A FROZEN
 * tile takes no more samples: the bounce-0 kernels emit no camera ray for it, the merge neither reads nor writes it (HIP twins of those
 * kernels, launched only once a tile is frozen: a context that never freezes one runs exactly what it ran before).  Frozen sets only grow —
 * there is no un-freeze; mirt_reset, mirt_resize, mirt_set_tile_range, mirt_set_tile_rows, a mirt_set_policy that changes `buckets` and
 * mirt_load_accumulator clear every freeze — so every tile still active has the same count, the context's `accumulations`, and a frozen tile's
 * count is the value `accumulations` had when it froze.  THE CONTRACT, with no tolerance anywhere: a tile whose count is n holds, word for word,
 * what n plain mirt_accumulate calls leave in that tile — accumulator and AOV slab (random draws are keyed on the global LaunchIndex and the
 * accumulation index).  mirt_render, mirt_render_aov, mirt_noise and mirt_tile_above resolve every tile at its own count: on the device,
 * scale = exposure / (float)(count / buckets) (AOVs: (float)count), the binary32 operations of the whole-image scale; their MIRT_NOT_READY
 * rules stay on the global `accumulations`.  mirt_accumulate* with every tile frozen only counts calls, as a context without tiles does.
 * Counters count what ran: `rays` only the samples of active tiles.  The owned pixel space is not compacted: batch size and stream memory stay
 * sized by the owned pixels, and the sparse bounce-0 kernels still sweep every owned pixel.  Frozen tiles and exact stream order exclude each
 * other (MIRT_ERR_STATE both ways).
 * BIAS: stopping a tile on an estimate made from the very samples it holds keeps the tiles whose estimate came out low by chance — like every
 * such rule it biases the frame dark, the more the earlier it may stop.  min_accumulations is the guard: nothing freezes before it. */
/* ORs freeze[t] != 0 into the mask (n_local_tiles = the context's tiles, in local order = ascending LaunchIndex).  Deferred calls are launched
 * first, under the old mask.  MIRT_ERR_ARG on a wrong length; MIRT_ERR_STATE when accumulations == 0, when accumulations % buckets != 0 (a
 * frozen tile must stay resolvable), and in exact stream order. */
int mirt_freeze_tiles(mirt_ctx* ctx, const uint8_t* freeze, size_t n_local_tiles);
/* counts_out[t]: `accumulations` for an active tile, the frozen value for a frozen one.  MIRT_ERR_ARG when capacity is below the tiles. */
int mirt_tile_counts(mirt_ctx* ctx, uint32_t* counts_out, size_t capacity);
/* mask_out[t] = 1 for a frozen tile, else 0 (a tile frozen at the current count has the count of an active one: the counts do not tell). */
int mirt_frozen_tiles(mirt_ctx* ctx, uint8_t* mask_out, size_t capacity);
/* Companion of mirt_load_accumulator (checkpoint / resume): call it after that one, which sets every tile's count to its `accumulations` and
 * clears all freezes.  Every count must be a positive multiple of `buckets` and <= accumulations (else MIRT_ERR_ARG, nothing changed); a tile
 * below `accumulations` is frozen at its count. */
int mirt_load_tile_counts(mirt_ctx* ctx, const uint32_t* counts, size_t n_local_tiles);
/* (Named without the word of the noise section: that section's set of entry points is closed, and pinned by its interface test.)
 * above_out[t] = usable pixels of local tile t with e > target (e, usable: mirt_noise's; the tile at its own count): one more ballot beside
 * the kernel's own.  Statuses as mirt_noise; target finite and >= 0, capacity at least the context's tiles, else MIRT_ERR_ARG. */
int mirt_tile_above(mirt_ctx* ctx, float floor, float target, uint32_t* above_out, size_t capacity);
/* Pure host code: no context, no GPU.  From mirt_noise's tile records {max, mean, usable, nonfinite} and mirt_tile_above's counts: a tile not
 * yet frozen freezes (freeze_out[t] = 1) when nonfinite == 0 and above <= (uint32_t)floor((1.0 - quantile) * usable), in double — at least
 * the quantile of its usable pixels is at or below the target; a tile without a usable and without a non-finite pixel freezes (0 <= 0).
 * A tile with frozen[t] != 0 is passed through as 1 (frozen may be NULL: none).  quantile in (0, 1], else MIRT_ERR_ARG. */
int mirt_adaptive_select(const float* tile_records, const uint32_t* above, const uint8_t* frozen, size_t n_tiles, double quantile, uint8_t* freeze_out);
typedef struct mirt_adaptive_report {
	uint32_t issued;              /* accumulations added by this call (to the context's count; a frozen tile took fewer) */
	uint32_t checks;              /* noise checks run */
	uint32_t frozen_tiles;        /* at return */
	uint32_t owned_tiles;
	uint64_t tile_accumulations;  /* sum of the tiles' counts at return: 256 x this = camera rays the frame holds */
	mirt_noise_stats last;        /* of the last check (zeros if none ran) */
} mirt_adaptive_report;
/* A host loop: mirt_accumulate(check_every), mirt_noise with mirt_tile_above(target), mirt_adaptive_select(quantile), mirt_freeze_tiles — the
 * select and freeze only once accumulations >= min_accumulations.  MIRT_OK when every owned tile is frozen; MIRT_NOT_CONVERGED at
 * max_accumulations (last step shortened as in mirt_accumulate_until).  Argument and state rules: mirt_accumulate_until's, and MIRT_ERR_STATE
 * in exact stream order.  report may be NULL. */
int mirt_accumulate_adaptive(mirt_ctx* ctx, const mirt_stop_rule* rule, uint32_t min_accumulations, mirt_adaptive_report* report);

/* ---- variance-guided à-trous denoised resolve from the buckets and the first-hit AOVs ------------------------------------------------
 * A second resolve beside mirt_render: an edge-avoiding à-trous wavelet filter (Dammertz et al. 2010) over the median-of-buckets frame, guided
 * by the first-hit AOVs and, as in SVGF (Schied et al. 2017), by each pixel's own variance — here the spread of its buckets, the quantity of
 * mirt_noise — so that a converged pixel is left alone and a noisy one is smoothed.  The reference has no denoiser; nothing of it is replayed.
 * It READS the accumulator slab, the AOV slab and the per-tile counts and changes no state (accumulator, AOVs, counters, frozen tiles; what
 * mirt_render returns afterwards).  It writes what mirt_render writes: RGBA f32, row-major, row 0 = y 0, ACES applied last, A = 1.
 * THE DEFINITION.  Every operation binary32, one rounding each, unfused, in the stated order, IEEE division and square root; the exponentials
 * of the two papers are replaced by Cauchy falloffs 1 / (1 + t t), so that no operation is left to a library.  lum(r, g, b) =
 * (0.2126f * r + 0.7152f * g) + 0.0722f * b.  "The image" is the w x h pixels its tiles cover (w = 16 (width / 16), h = 16 (height / 16)).
 * For pixel p, n = its tile's sample count (mirt_tile_counts), k = buckets, scale = exposure / (float)(n / k):
 *   1. signal     s_c = scale * median_k(the k bucket words of channel c): mirt_render's operations up to, not including, the tonemapping.
 *   2. variance   y_j, mean and var exactly as mirt_noise defines them (above); v = var / (float)k, the variance of the mean.
 *   3. guides     mirt_render_aov's three outputs: z = depth_sum / (float)n;  N = normalize(normal_sum), (0,0,0) where the sum has no length;
 *                 a_c = albedo_sum_c / (float)n.
 *   4. modulator  m_c = (demodulate && a_c >= albedo_floor) ? a_c : 1.0f;   x_c = s_c / m_c;   lm = lum(m_r, m_g, m_b);   v = v / (lm * lm).
 *   5. usability  p is USABLE when x_r, x_g, x_b, v, z, N.x, N.y, N.z are all finite and v >= 0.  Decided here, once; it never changes.  An
 *                 unusable pixel is never taken as a tap, and as a centre it passes through every step: its output is tonemapping(s), the word
 *                 mirt_render writes.
 *   6. iteration  i = 0 .. iterations - 1, step = 1 << i, from buffer A (x, v) into buffer B, then the two swap.  For a usable centre p:
 *        gv   the smoothed variance: the kernel (1/16 1/8 1/16; 1/8 1/4 1/8; 1/16 1/8 1/16) over the current v of the pixels at distance 1 —
 *             never at distance `step` — that are inside the image, usable and, the centre aside, turned the same way (nn > 0, or all six normal
 *             components zero; nn as below: variance does not cross a crease or a silhouette), dy = -1 .. 1 outside, dx = -1 .. 1 inside:
 *             G = (((g_0 v_0) + g_1 v_1) + ...), K = ((g_0 + g_1) + ...), each sum starting from the first pixel taken; gv = G / K.
 *        sd   = sigma_lum * sqrt(gv) + lum_floor;      l_p = lum(x_p).
 *        taps (dy, dx), dy = -2 .. 2 outside, dx = -2 .. 2 inside, q = p + step * (dx, dy); a q outside the image or unusable is skipped.
 *             h = (1/16, 1/4, 3/8, 1/4, 1/16).  The centre tap: w = 9/64.  Any other tap:
 *               nn = (N_p.x * N_q.x + N_p.y * N_q.y) + N_p.z * N_q.z
 *               wn = 1 when all six normal components are zero (two miss pixels); else wn = (nn > 0 ? nn : 0), then normal_squarings times wn = wn * wn
 *               tz = fabsf(z_p - z_q) / (sigma_depth * ((z_p < z_q ? z_q : z_p) * (float)(step * max(|dx|, |dy|))) + FLT_MIN)
 *               tl = fabsf(l_p - lum(x_q)) / sd
 *               w  = (((h[dy] * h[dx]) * wn) * (1.0f / (1.0f + tz * tz))) * (1.0f / (1.0f + tl * tl))
 *             W = ((w_0 + w_1) + ...),  X_c = ((w_0 x_0c + w_1 x_1c) + ...),  V = (((w_0 w_0) v_0 + (w_1 w_1) v_1) + ...), each sum starting
 *             from the first tap taken.  x'_c = X_c / W;  v' = V / (W * W).  W >= 9/64: the centre tap is always taken.
 *   7. output     out_c = x_c * m_c, tonemapping(out), A = 1.
 * sigma_depth is the relative change of depth allowed per pixel of tap distance; sigma_lum counts standard deviations of the pixel.
 * TWO CONSEQUENCES the tests rest on: (a) iterations = 0 with demodulate = 0 writes mirt_render's frame word for word (m = 1: s / 1 and s * 1
 * are s).  (b) The result is a function of the two slabs and the counts alone: it does not depend on policy.max_batch / streams, on the tree,
 * or on how the slabs got there — rendered, loaded (mirt_load_accumulator, mirt_load_aov, mirt_load_tile_counts) or gathered by a group.
 * iterations and normal_squarings in 0 .. 8, demodulate 0 or 1, sigma_lum and sigma_depth finite and >= 0, lum_floor finite and > 0, albedo_floor
 * finite, no NULL pointer: else MIRT_ERR_ARG.  MIRT_ERR_STATE while AOVs are off, with buckets < 2, and for a context that does not own every
 * tile of the image: a 5 x 5 stencil at step 16 reads 32 pixels into its neighbours' tiles, so a partial context is refused, not approximated
 * (a group resolves on its gather context).  Exact stream order has no AOVs, hence MIRT_ERR_STATE there too.  Then MIRT_NOT_READY, with rgba_host
 * untouched, under mirt_render's condition.  Pixels outside "the image" of the definition (no tile owns them) are never read as taps and never
 * written: rgba_host keeps there what the caller handed over.  Launches anything deferred and waits for the GPU first; kernel time is booked under MIRT_K_RESOLVE.
 * Scratch: four float4 images (x and v twice, the guides, the modulator), allocated by the first call, released by mirt_resize and mirt_destroy —
 * 4 x 268 MB at 4096 x 4096.  Kernels: csrc/denoise.hpp; binary32 numpy twin: tests/denoise_twin.py. */
typedef struct mirt_denoise_params {
	uint32_t iterations;        /* 0..8 à-trous passes, step 1, 2, 4, ...; 0 = no filtering */
	uint32_t normal_squarings;  /* 0..8: normal weight = max(0, n_p.n_q)^(2^this) */
	uint32_t demodulate;        /* 0 / 1: filter colour / albedo, multiply back afterwards */
	float    sigma_lum;         /* luminance stop, in standard deviations of the pixel */
	float    sigma_depth;       /* depth stop: relative depth change allowed per pixel of tap distance */
	float    lum_floor;         /* > 0: added to the luminance denominator */
	float    albedo_floor;      /* a channel is demodulated only where its albedo >= this */
} mirt_denoise_params;
/* (The entry points are named after the filter, not after what it removes: the noise section's set of entry points is closed and pinned by its
 * interface test, as mirt_tile_above's note says.  The host layers call them render_denoised / denoise_defaults.)
 * Pure host code, no context: iterations 5, normal_squarings 5, demodulate 1, sigma_lum 4, sigma_depth 0.05, lum_floor 1e-4, albedo_floor 1/256. */
int mirt_atrous_defaults(mirt_denoise_params* out);
int mirt_render_atrous(mirt_ctx* ctx, const mirt_denoise_params* params, float* rgba_host);

/* ---- temporal history for the denoised resolve: reproject the last view's result across a camera move -----------------------------------
 * A third resolve.  The reference calls Accumulate(); Render(); once per frame and resets the accumulator on every camera move
 * (Application.cpp:309-333,379-380): after each move the frame holds `buckets` samples again, although most surfaces it shows were seen before.
 * This resolve keeps the last call's demodulated signal, its variance and its guides as a HISTORY, reprojects it through the first-hit depth
 * into the new view, rejects what does not match, blends the survivors with the new samples by sample count, and runs the à-trous passes above
 * on the blend (the temporal half of SVGF, Schied et al. 2017).  The reference has none of this; nothing of it is replayed.
 * It READS the accumulator slab, the AOV slab and the per-tile counts, as mirt_render_atrous does, and changes no renderer state except its own
 * history (accumulator, AOVs, counters, frozen tiles and what mirt_render returns afterwards are untouched).
 * THE DEFINITION.  Every operation binary32, one rounding each, unfused, in the stated order, IEEE division and square root.  dot(a, b) =
 * (a.x * b.x + a.y * b.y) + a.z * b.z.  w, h, "the image", n (the pixel's tile count), x_c, v, N, z, m_c, usable: as in the à-trous definition.
 *   1. prepare    steps 1-5 of mirt_render_atrous, unchanged.
 *   2. reproject  The history holds hx = (x, v), hg = (N, z) and usability, hn = its length in samples, per pixel, the camera `prev` it was taken
 *                 under, and the demodulate / albedo_floor it was taken with.  THE CALL TAKES THE HISTORY when one exists, max_ratio > 0, the
 *                 history is of this image size, of these demodulate / albedo_floor words and of this camera's exposure word (x is in exposure-scaled
 *                 units), and both cameras satisfy | |q|^2 - 1 | < 1e-4
 *                 (|q|^2 = ((x x + y y) + z z) + w w: the condition of the candidate lists).  Otherwise every usable pixel is `no_history`.
 *                 For a usable centre p = (px, py) whose N is not all zero (a miss has no surface to follow; it is `no_history`), cam = this call's camera:
 *        d  = camera_ray_dir(cam, px, py, 0.5f, 0.5f)       (Camera.hpp:80-88 as device_math.hpp spells it)
 *        P  = cam.pos + d * z          (per component: one product, one sum);      r = P - prev.pos;      z' = sqrt(dot(r, r))
 *        q  = the rotation of camera_ray_dir, inverted: r + ((uv * w) + uuv) * 2 per component with qv = -prev.orient.xyz, w = prev.orient.w,
 *             uv = cross(qv, r), uuv = cross(qv, uv)    (device_math.hpp camera_axis with the vector part negated)
 *        q.z / prev.z <= 0: the point lies behind the history's camera, p is `outside`.  Else t = prev.z / q.z,
 *        fx = (q.x * t + prev.half_width) - 0.5f,   fy = (q.y * t + prev.half_height) - 0.5f.
 *        EXCEPTION: when cam equals prev word for word (all eleven words) the map is the identity by definition: fx = (float)px, fy = (float)py, z' = z.
 *        ix = floorf(fx), wx = fx - ix, ux = 1.0f - wx; likewise iy, wy, uy.  Taps (i, j) = (0,0), (1,0), (0,1), (1,1) at pixel (ix + i, iy + j) with
 *        b = (i ? wx : ux) * (j ? wy : uy).  (No tap is in the image unless -1 <= ix <= w - 1 and -1 <= iy <= h - 1; a NaN or infinite fx, fy fails that.)
 *        A tap is TAKEN when it is inside the image, usable in the history with hn > 0, fabsf(z_tap - z') <= depth_tol * z', and
 *        dot(N_p, N_tap) >= normal_min.  B = ((b_0 + b_1) + ...), X_c = ((b_0 x_0c + b_1 x_1c) + ...), V = ((b_0 v_0 + ...)), L = ((b_0 hn_0 + ...)),
 *        each sum starting from the first tap taken.  xh_c = X_c / B, vh = V / B, nh = L / B.
 *        Class: no tap inside the image: `outside`; else no tap taken, or B == 0: `rejected`; else `reprojected`.
 *   3. blend      for a reprojected pixel: cap = max_ratio * (float)n; nh = cap < nh ? cap : nh; a = (float)n / ((float)n + nh);
 *                 x_c = xh_c + a * (x_c - xh_c);  v = (a * a) * v + ((1.0f - a) * (1.0f - a)) * vh;  len = (float)n + nh.
 *                 Every other usable pixel keeps x, v and has len = (float)n.  An unusable pixel passes through as in the à-trous definition; len = 0.
 *   4. history    with update = 1 the blended (x, v), this call's guides and usability, len, cam and demodulate / albedo_floor become the history
 *                 — the blend BEFORE any filtering, so that spatial blur never compounds over frames.  A call that returns an error or
 *                 MIRT_NOT_READY leaves the history as it was — with one exception: MIRT_ERR_HIP from a call with update = 1 and iterations >= 2 may
 *                 come after the old history's image was used as scratch; that return drops the history (mirt_history_info: valid = 0).
 *   5. filter     steps 6-7 of the à-trous definition on the blend.
 * CONSEQUENCES the tests rest on: (a) a call that takes no history writes mirt_render_atrous's frame word for word.  (b) Under the identity map over
 * the slabs the history was taken from, xh = x (b_0 = 1: x * 1 / 1), so x is unchanged word for word and len = n + min(hn, max_ratio n).  (c) The
 * result is a function of the two slabs, the counts, the camera and the history alone.
 * LIFETIME.  The history is allocated by the first call with update = 1 and is kept across mirt_reset, mirt_set_camera and mirt_set_lens — that is
 * its purpose.  It is dropped by mirt_drop_history, mirt_set_scene, mirt_resize, mirt_set_tile_range, mirt_set_tile_rows, a mirt_set_policy that
 * changes `buckets`, and mirt_destroy.  THE SHADING SWITCHES DO NOT DROP IT (light RIS, transmission, sky sampling, closures, the GGX pdf, the
 * gloss decay table, the lens): a caller who changes the estimand calls mirt_drop_history, as it calls mirt_reset.  Under a thin lens the
 * reprojection still follows the pinhole centre ray of the pixel and the summed first-hit depth: out of focus it reprojects a blur, not a surface.
 * A change of exposure needs no drop: a history of another exposure word is ignored for the call, as one of another demodulation is.  Memory: two float4 images and
 * one float image while a history is held (36 B per pixel: 604 MB at 4096 x 4096), one more float image of scratch for a call's lengths (67 MB),
 * beside the four scratch images of mirt_render_atrous.
 * Errors and preconditions are exactly mirt_render_atrous's (arguments, then AOVs on, buckets >= 2, the whole image in one context, hence no exact
 * stream order, then MIRT_NOT_READY under mirt_render's condition, rgba_host untouched); in addition MIRT_ERR_ARG when max_ratio or depth_tol is
 * negative or not finite, normal_min is outside [-1, 1], update > 1, or temporal is NULL.  Kernel time is booked under MIRT_K_RESOLVE.
 * history_len (or NULL): width * height floats, row-major, `len` of every pixel of the image (pixels no tile covers are left untouched, in
 * history_len and in rgba_host alike; a point that projects onto such a pixel of the history is `outside`: the history's image is w x h too).
 * Kernel: csrc/temporal.hpp (k_reproject); binary32 numpy twin: tests/temporal_twin.py; float64 definition: tests/temporal_definitions.py. */
typedef struct mirt_temporal_params {
	float    max_ratio;     /* >= 0: history may weigh at most max_ratio x the pixel's own sample count; 0 = take no history */
	float    depth_tol;     /* >= 0: a tap is taken when |z_tap - z'| <= depth_tol * z' */
	float    normal_min;    /* in [-1, 1]: ... and dot(N_p, N_tap) >= normal_min */
	uint32_t update;        /* 0 / 1: write this call's blend as the new history */
} mirt_temporal_params;
typedef struct mirt_temporal_stats {   /* pixels of the image; the five sum to w * h */
	uint64_t reprojected;   /* blended with history */
	uint64_t no_history;    /* usable, but step 2 does not apply: the call takes no history, or the centre is a miss (N all zero) */
	uint64_t outside;       /* every tap outside the history's image, or the point behind its camera */
	uint64_t rejected;      /* some tap inside the image, none taken (depth, normal, unusable or empty history there), or B == 0 */
	uint64_t unusable;      /* step 5 of the à-trous definition */
} mirt_temporal_stats;
int mirt_temporal_defaults(mirt_temporal_params* out);   /* pure host code, no context: max_ratio 7, depth_tol 0.02, normal_min 0.9, update 1 */
int mirt_render_temporal(mirt_ctx* ctx, const mirt_denoise_params* params, const mirt_temporal_params* temporal,
                         float* rgba_host, float* history_len, mirt_temporal_stats* stats /* or NULL */);
int mirt_drop_history(mirt_ctx* ctx);
/* *valid = 1 while a history is held; *bytes = device bytes of its three images (0 after a drop). */
int mirt_history_info(const mirt_ctx* ctx, uint32_t* valid, uint64_t* bytes);

/* ---- first-hit id map: which sphere every pixel shows ---------------------------------------------------------------------------------
 * What mirt_pick_focus finds for one pixel, for every pixel of the image in one launch: pixel (x, y), row-major in rows of `width`, over the
 * WHOLE image whether this context owns the tile or not, holds the first hit of the un-jittered pinhole ray through the pixel centre (samples
 * 0.5, 0.5; lens or no lens) through the closest-hit traversal the context is configured with (every record layout, f32 records, use_bvh = 0,
 * reference_tree = 1; a non-unit quaternion is fine: the ray walks the tree).  prim_out: the BVH-order id hit.primID refers to, -1 on a miss;
 * distance_out: tfar, INFINITY on a miss.  Either may be NULL.  The editor's "active sphere" (Application.cpp:466-470) is prim_out at the
 * cursor; mirt_update_spheres takes that id as its bvh_index.
 * It changes no state: accumulator, AOVs, counters (`rays` included), lists and history are untouched; it only reads, so exact stream order
 * allows it.  MIRT_ERR_STATE before a scene, a camera or a size is set; MIRT_ERR_ARG when width * height does not fit 31 bits.  Kernel time
 * is booked under MIRT_K_RESOLVE.  Kernel: csrc/id_map.hpp (k_id_map): the rays are generated from the pixel index, no ray stream exists. */
int mirt_id_map(mirt_ctx* ctx, int32_t* prim_out /* w*h or NULL */, float* distance_out /* w*h or NULL */);

/* ---- keeping the history across sphere moves: id map and object motion -----------------------------------------------------------------
 * mirt_update_spheres drops the temporal history, because the reprojection above follows the camera only.  With this switch on (0 / 1, default
 * 0; another value: MIRT_ERR_ARG) it does not (it still does everything else it does), and the history carries two more things: an ID PLANE
 * (int32 per pixel: the id map of the call that wrote it) and a SPHERE SNAPSHOT (the BVH-order {pos, radius_sq} table the history was taken
 * under, 16 B per sphere, as it already carries the camera).  mirt_render_temporal then computes the id map of the current camera before step 2
 * and runs k_reproject<MOTION>.  With the switch off every kernel launched and every word written is what it is without this section.
 * THE DEFINITION, in the style of step 2 above: binary32, one rounding per operation, unfused, in this order.  For a usable centre p with guides
 * (N, z) and i = the id map's word at p, P = cam.pos + d * z as in step 2.  now = spheres[i] = (c, rsq), then = snapshot[i] = (c0, rsq0).  The
 * sphere has MOVED when i >= 0 and any of the four words differ.
 *   not moved, or i < 0:  the map is step 2's, the identity exception included.
 *   moved:                o = P - c per component;  if the rsq words differ and rsq > 0: s = sqrtf(rsq0 / rsq), o = o * s per component;
 *                         P' = c0 + o per component;  r = P' - prev.pos, and on from there exactly as step 2 (z', q, behind, t, fx, fy).  The
 *                         identity exception does NOT apply.  Normals need no map: translation and uniform scale keep them.
 *   taps:                 a tap is taken when step 2's four conditions hold AND the history's id word at the tap equals i (-1 equals -1).  What
 *                         a moving ball uncovers therefore does not inherit the ball's history: those pixels are `rejected`.  THIS HOLDS WITH
 *                         THE SWITCH ON EVEN WHEN NOTHING MOVED: a tap across a silhouette, which depth and normal might let pass, is not taken.
 *   history write:        with update = 1 the call's id map becomes the history's id plane (renamed as the guides are, not copied), and the
 *                         snapshot is copied device to device from the table in place — skipped while no mirt_update_spheres came since the last
 *                         copy.  Several updates between two history writes need no bookkeeping: the map compares "now" with "then".  A call with
 *                         update = 0 changes neither.
 * Blend, filter and the statistics classes are unchanged.  Consequence (b) stands (the id plane of the history equals the id map there).
 * Consequence (c) becomes: the result is a function of the two slabs, the counts, the two cameras, the history, the id map and the two sphere
 * tables alone.
 * LIFETIME.  Any change of the switch drops the history; mirt_set_scene drops it as ever (ids change meaning); mirt_update_materials keeps it.
 * mirt_history_info counts the id plane and the snapshot (4 B per pixel + 16 B per sphere) only while the switch is on.  One more int32 image of
 * scratch holds a call's own id map.  The preconditions of mirt_render_temporal are unchanged.
 * mirt_set_motion_geometry: the context whose scene, traversal settings and sphere table the id map of `ctx` is made from (NULL or ctx itself:
 * its own, the default).  For a context that resolves frames it does not trace — the gather context of a group holds no geometry — ; both must
 * be on one device and show the same camera words when a call needs the map (MIRT_ERR_STATE otherwise).  `geometry` must outlive `ctx` or be
 * reset first.  A change drops the history.
 * Kernel: csrc/temporal.hpp (k_reproject<true>); binary32 numpy twin: tests/temporal_motion_twin.py; float64 definition:
 * tests/temporal_motion_definitions.py. */
int mirt_set_sphere_motion(mirt_ctx* ctx, uint32_t on);
int mirt_get_sphere_motion(const mirt_ctx* ctx, uint32_t* on);
int mirt_set_motion_geometry(mirt_ctx* ctx, mirt_ctx* geometry);

int mirt_get_counters(mirt_ctx* ctx, mirt_counters* out);
int mirt_get_kernel_times(mirt_ctx* ctx, mirt_kernel_times* out, int reset);
/* HIP stream the context launches on (hipStream_t), for callers that time with their own events. */
int mirt_get_stream(mirt_ctx* ctx, void** hip_stream);

/* ---- multi-GPU: the same renderer on n devices of one node ------------------------------------------------------
 * The reference host is ONE object, `Renderer<> renderer{scene}` (Application.cpp:514), whose Accumulate() is a parallel_for over
 * the tiles (Renderer.hpp:75).  A group is that object on n GPUs, driven by one host thread of one process: one context per
 * device with the whole scene and an interleaved share of the tile rows (member i: rows i, i+n, ...; mirt_set_tile_rows), no
 * exchange while rendering, and ONE gather of the accumulator slabs to devices[0] — RCCL point-to-point over xGMI (librccl is loaded
 * on first use) — with a device-side un-interleave into the full-image AccumulationTile layout, where Render() resolves the whole
 * frame.  Results equal the single-context ones bit for bit (random draws are keyed on the global LaunchIndex, Renderer.hpp:107).
 * Entries mirror their mirt_* namesakes; errors: mirt_group_last_error.  devices[] may name one device more than once (rehearsal on
 * a one-GPU box: slabs are then exchanged with device copies, RCCL needs distinct devices).
 * (One process PER GPU — torch.distributed / MPI ranks — uses plain contexts with mirt_set_tile_rows + mirt_accumulator_device instead.) */
typedef struct mirt_group mirt_group;
int mirt_group_create(const int* devices, int n, mirt_group** out);
int mirt_group_destroy(mirt_group* group);
const char* mirt_group_last_error(const mirt_group* group);       /* NULL: of the failed mirt_group_create / selftest */
int mirt_group_size(const mirt_group* group, int* n);
int mirt_group_member(mirt_group* group, int index, mirt_ctx** ctx);   /* borrowed: counters, kernel times, debug entry points */
int mirt_group_set_scene(mirt_group* group,
                         const mirt_sphere* geometry, const mirt_sphere* bvh_prims, uint32_t n_spheres,
                         const mirt_bvh_node* nodes, uint32_t n_nodes,
                         const mirt_material* materials, uint32_t n_materials,
                         const int32_t* lights, uint32_t n_lights,
                         const float ambient_color[3], const float* hdri_rgba, uint32_t hdri_w, uint32_t hdri_h);
int mirt_group_set_camera(mirt_group* group, const float pos[3], const float orient_xyzw[4], float half_width, float half_height, float z, float exposure);
int mirt_group_set_lens(mirt_group* group, float aperture_radius, float focus_depth);   /* mirt_set_lens on every member */
int mirt_group_set_light_ris(mirt_group* group, uint32_t candidates);             /* mirt_set_light_ris on every member */
int mirt_group_set_transmission(mirt_group* group, uint32_t on);                   /* mirt_set_transmission on every member (and the gather context) */
int mirt_group_set_sky_sampling(mirt_group* group, uint32_t on);                   /* mirt_set_sky_sampling on every member (and the gather context) */
int mirt_group_set_ggx_pdf(mirt_group* group, uint32_t on);                        /* mirt_set_ggx_pdf on every member (and the gather context) */
int mirt_group_set_material_closures(mirt_group* group, const uint8_t* closure, uint32_t n);   /* mirt_set_material_closures on every member (and the gather context) */
int mirt_group_set_environment(mirt_group* group, const float ambient_color[3], const float* hdri_rgba, uint32_t w, uint32_t h);   /* mirt_set_environment on every member (and the gather context) */
int mirt_group_set_sun_sky(mirt_group* group, const mirt_sun_sky_params* params);   /* mirt_set_sun_sky on every member (and the gather context): each bakes its own map, the same words */
int mirt_group_update_spheres(mirt_group* group, uint32_t n, const uint32_t* bvh_index, const uint32_t* geometry_index, const float* xyz_rsq);   /* mirt_update_spheres on every member (the gather context holds no geometry) */
int mirt_group_update_materials(mirt_group* group, uint32_t n_rows, const uint32_t* material_index, const mirt_material* rows,
                                uint32_t n_assign, const uint32_t* bvh_index, const uint32_t* geometry_index, const int32_t* material_ID);   /* mirt_update_materials on every member; the material rows on the gather context too (it holds the material tables, no geometry) */
int mirt_group_pick_focus(mirt_group* group, uint32_t x, uint32_t y, float* distance, float* depth);   /* mirt_pick_focus on the first member */
int mirt_group_set_policy(mirt_group* group, const mirt_policy* policy);
int mirt_group_set_gloss_decay(mirt_group* group, const float* decay, uint32_t n);
int mirt_group_set_stream_order(mirt_group* group, uint32_t exact);             /* mirt_set_stream_order on every member */
int mirt_group_resize(mirt_group* group, uint32_t width, uint32_t height);      /* Renderer::Resize + the tile-row split */
int mirt_group_reset(mirt_group* group);                                         /* Renderer::ResetAccumulator */
int mirt_group_accumulate(mirt_group* group, uint32_t n_calls);                  /* n x Renderer::Accumulate on every device, then waits */
int mirt_group_accumulate_async(mirt_group* group, uint32_t n_calls);
int mirt_group_synchronize(mirt_group* group);
int mirt_group_get_accumulations(const mirt_group* group, uint32_t* accumulations);
int mirt_group_get_counters(mirt_group* group, mirt_counters* out);              /* summed over the members */
/* The one exchange: slabs -> devices[0] (ncclSend / ncclRecv per peer, rccl.h:700,722), un-interleaved there.  Implied by the two
 * reads below; a no-op for one member or when nothing was accumulated since the last gather. */
int mirt_group_gather(mirt_group* group);
int mirt_group_last_gather_ms(const mirt_group* group, double* ms);              /* device time of the last gather incl. un-interleave */
int mirt_group_accumulator_floats(const mirt_group* group, size_t* n_floats);    /* of the whole image */
int mirt_group_read_accumulator(mirt_group* group, float* host_dst);             /* whole image, [tile][bucket][r,g,b][256] in LaunchIndex order */
int mirt_group_render(mirt_group* group, float* rgba_host);                      /* Renderer::Render of the whole frame; MIRT_NOT_READY as mirt_render; pixels no tile owns are left as handed over, as by mirt_render */
/* First-hit AOVs of the whole image.  mirt_group_gather moves the members' AOV slabs in the same exchange as their accumulator slabs
 * and un-interleaves them with the same tile-row mapping; the sums equal the single-context ones bit for bit.  Both branches of the
 * exchange carry them — device copies when one device is named several times, RCCL between distinct devices — but only the first
 * can be run on a one-GPU box: the RCCL branch for the AOV slabs is built and has not been run. */
int mirt_group_set_aov(mirt_group* group, uint32_t on);                          /* mirt_set_aov on every member (and the gather context) */
int mirt_group_aov_floats(const mirt_group* group, size_t* n_floats);            /* of the whole image: tiles x 7 x 256; 0 while off */
int mirt_group_read_aov(mirt_group* group, float* host_dst);                     /* whole image, [tile][plane 0..6][256] in LaunchIndex order */
int mirt_group_render_aov(mirt_group* group, int which, float* out);             /* mirt_render_aov of the whole frame */
/* mirt_render_atrous of the whole frame: gathers as mirt_group_render does, then resolves on the gather context, which holds the accumulator,
 * the AOV slab and the per-tile counts of the whole image — the single context's words.  MIRT_ERR_STATE (AOVs off, buckets < 2) and MIRT_NOT_READY
 * are decided before the gather; the argument rules are then the gather context's. */
int mirt_group_render_atrous(mirt_group* group, const mirt_denoise_params* params, float* rgba_host);
/* mirt_render_temporal of the whole frame, likewise: the history lives on the gather context (a group of one: on its member), which follows
 * mirt_group_set_camera as the members do, so the words are the single context's.  mirt_group_set_scene, mirt_group_resize and a
 * mirt_group_set_policy that changes `buckets` drop it, as their namesakes do; mirt_group_drop_history and mirt_group_history_info act on it. */
int mirt_group_render_temporal(mirt_group* group, const mirt_denoise_params* params, const mirt_temporal_params* temporal,
                               float* rgba_host, float* history_len, mirt_temporal_stats* stats);
int mirt_group_drop_history(mirt_group* group);
int mirt_group_history_info(const mirt_group* group, uint32_t* valid, uint64_t* bytes);
/* mirt_set_sphere_motion on every member and the gather context (whose id map is made from the first member's geometry: mirt_set_motion_geometry);
 * mirt_group_update_spheres then keeps the history.  mirt_group_id_map: mirt_id_map on the context mirt_group_render_temporal resolves on. */
int mirt_group_set_sphere_motion(mirt_group* group, uint32_t on);
int mirt_group_id_map(mirt_group* group, int32_t* prim_out, float* distance_out);
/* mirt_noise / mirt_accumulate_until of the whole image.  NO gather: every member runs mirt_noise on its own slab; histograms and counts add
 * as integers, the maximum is exact, the members' tile records are un-interleaved on the host into LaunchIndex order (tile_out: 4 floats per
 * tile of the image), each member writes its own tiles of map_out, and the mean is the double sum over those records in LaunchIndex order.
 * Counts, histogram, max, tile records and map equal the single-context ones bit for bit, the mean as the same double sum.  Statuses as the
 * namesakes'; MIRT_NOT_READY is decided before any member is asked, with every output untouched. */
int mirt_group_noise(mirt_group* group, float floor, float* map_out, float* tile_out, uint32_t* hist_out, mirt_noise_stats* stats);
int mirt_group_accumulate_until(mirt_group* group, const mirt_stop_rule* rule, mirt_noise_stats* last, uint32_t* issued);
/* Per-tile adaptive sampling of the whole image (namesakes: "per-tile adaptive sampling" above).  Masks, counts and `above` are in LaunchIndex
 * order, one entry per tile of the image; they are split over the members' tile rows and un-interleaved on the host, as the tile records of
 * mirt_group_noise are — NO gather, also not in the loop.  mirt_group_gather loads the members' counts into the gather context, so
 * mirt_group_render, mirt_group_render_aov resolve every tile at its own count.  Status rules as the namesakes', decided before any member is
 * asked.  (mirt_group_tile_above: the group twin of mirt_tile_above.) */
int mirt_group_freeze_tiles(mirt_group* group, const uint8_t* freeze, size_t n_tiles);
int mirt_group_tile_counts(mirt_group* group, uint32_t* counts_out, size_t capacity);
int mirt_group_frozen_tiles(mirt_group* group, uint8_t* mask_out, size_t capacity);
int mirt_group_tile_above(mirt_group* group, float floor, float target, uint32_t* above_out, size_t capacity);
int mirt_group_accumulate_adaptive(mirt_group* group, const mirt_stop_rule* rule, uint32_t min_accumulations, mirt_adaptive_report* report);
/* Diagnostic: one-device RCCL communicator on `device`, n_floats sent to itself through a grouped ncclSend / ncclRecv. */
int mirt_group_rccl_selftest(int device, size_t n_floats);

/* ---- stage-level entry points (parity tests of single kernels) -------------------------------------
 * SoA planes: p_xyz / dir_xyz hold x[n], y[n], z[n] back to back. */
/* RAY GENERATION, Renderer.hpp:113-127 for Accumulate() number `accumulations`; ray order tile*256 + ID over local tiles. */
int mirt_debug_raygen(mirt_ctx* ctx, uint32_t accumulations, float* p_xyz, float* dir_xyz);
/* Traverse (BVH.hpp:309-360): tfar starts at FLT_MAX, primID at -1 (BVH-order index). */
int mirt_debug_trace_closest(mirt_ctx* ctx, size_t n, const float* p_xyz, const float* dir_xyz, float* tfar_out, int32_t* primID_out);
/* Traverse_shadow (BVH.hpp:362-404): occluded_out[i] in {0,1}. */
int mirt_debug_trace_shadow(mirt_ctx* ctx, size_t n, const float* p_xyz, const float* dir_xyz, const float* tfar, uint8_t* occluded_out);
/* Device math used by the shading kernels, evaluated on the GPU for n inputs.
 * fn: 0 fast_sincos(x)->(sin,cos)  [VectorMath.hpp:644-662]   in: x[n]            out: 2n
 *     1 fast_atan2(y,x)            [VectorMath.hpp:632-642]   in: y[n],x[n]       out: n
 *     2 fast_asin(x)               [VectorMath.hpp:625-630]   in: x[n]            out: n
 *     3 1/x, sqrt(x), a/b checks                               in: a[n],b[n]       out: 3n (1/a, sqrt(|a|), a/b)
 *     4 hemisphere(t,s)            [Sampling.hpp:92-94]       in: t[n],s[n]       out: 3n
 *     5 tangent_space(N)+to_local/to_world round trip [Sampling.hpp:150-179]  in: N(3n),v(3n)  out: 10n (T xyzw, local xyz, world xyz)
 *     6 sample_direction_to_sphere [Sampling.hpp:220-239]     in: Wc(3n),sin2[n],dist[n],r2[n],t[n],s[n]  out: 5n (L xyz, distance, pdf)
 *     7 rng: hash_2d(x,y) then 3 pcg draws as float + bounded int  [Random.hpp:5-50]  in: x[n],y[n],range[n] as u32 bits  out: 5n (hash bits, f0,f1,f2, bounded bits)
 *     8 Closure<GGX>::eval         [DataStreams.hpp:189-195, Sampling.hpp:272-296]  in: F0(3n),alpha[n],Llocal(3n),Vlocal(3n)  out: 3n
 *     9 Closure<GGX>::sample       [DataStreams.hpp:200-218, Sampling.hpp:254-270,297-309]  in: F0(3n),alpha[n],Vlocal(3n),u0[n],u1[n]  out: 6n (dir, estimator)
 *    10 the sphere tests' sqrt (kernels.hpp sqrt_trav) — must equal IEEE sqrt for every input >= 0   in: x[n]  out: n
 *    11 dielectric_interface (device_math.hpp; mirt_set_transmission)   in: Vl.x[n], Vl.y[n], Vl.z[n], n_ior[n], entering[n] (!= 0), s1[n]
 *                                                           out: dir.x, dir.y, dir.z (local), F, reflected (0 / 1), tir (0 / 1)   (6n)
 *    12 sky_sample (kernels.hpp; mirt_set_sky_sampling on over a scene, else MIRT_ERR_STATE)   in: u0[n], u1[n]   out: dir.x, dir.y, dir.z, q, row, column (6n; row and column as floats)
 *    13 sky_pdf    (likewise)                                                                   in: dir.x[n], dir.y[n], dir.z[n]   out: p~, row, column (3n)
 *    14 ggx_pdf    (device_math.hpp; mirt_set_ggx_pdf — needs no switch)                         in: alpha[n], Llocal(3n), Vlocal(3n)   out: p~ (n)
 *       (8, 9: the defined part of the reference's compiled-out GGX closure; not used by the path — DESIGN.md §7)
 */
int mirt_debug_math(mirt_ctx* ctx, int fn, size_t n, const float* in, float* out);
/* Introspection of the GPU-internal BVH layout (tests, bench, DESIGN.md numbers):
 * out[0] records, out[1] records staged in LDS, out[2] spheres staged in LDS, out[3] tree depth, out[4] bit 0: binary16
 * records are in use, bit 1: they are the 64-B records of up to four children (else 32-B child pairs), out[5] dynamic LDS
 * bytes of a trace workgroup, out[6] trace workgroups per CU, out[7] CUs. */
int mirt_debug_info(mirt_ctx* ctx, uint32_t out[8]);
/* Read-back of the records the trace kernels walk, copied from the device after the context's stream has been synchronised
 * (a host-built tree as uploaded, a GPU-built one as built).  info[0] records, info[1] bytes per record (64 / 32 / 64),
 * info[2] layout: 0 f32 child pairs, 1 binary16 child pairs, 2 binary16 records of up to four children, info[3] tree depth.
 * dst == NULL: only `info` is filled.  MIRT_ERR_ARG when capacity_bytes < info[0] * info[1]. */
int mirt_debug_tree(mirt_ctx* ctx, void* dst, size_t capacity_bytes, uint32_t info[4]);
/* Read-back of the sky sampling table (mirt_set_sky_sampling), copied from the device after the context's stream has been synchronised.
 * info[0] rows, info[1] columns (of CELLS), info[2] the bits of the total (the last marginal running sum), info[3] floats in the table.
 * Layout, in floats: marg[rows], rowsum[rows], tn[rows + 1] (1 - sin el(k)), ts[rows + 1] (1 + sin el(k)), cond[rows][cols], dens[rows][cols].
 * dst == NULL: only `info` is filled.  `capacity` is in floats: MIRT_ERR_ARG when below info[3].  MIRT_ERR_STATE while there is no table
 * (the switch is off, or no scene has been set). */
int mirt_debug_sky_table(mirt_ctx* ctx, float* dst, size_t capacity, uint32_t info[4]);
/* Read-back of the two per-light tables next event estimation samples, copied from the device after the context's stream has been synchronised
 * (as mirt_set_scene flattened the caller's list, or as mirt_update_materials regenerated them).  ids_out[l]: the geometry id of light l;
 * sphere_rows_out: 4 floats per light {centre, radius_sq}; emit_rows_out: 4 floats per light {emission.rgb of its material, the bits of its id}.
 * info[0] n_lights, info[1] spheres per workgroup of the compaction, info[2] workgroups one pass of its totals scan covers, info[3] 0.
 * All three pointers NULL: only `info` is filled; any of them may be NULL.  MIRT_ERR_ARG when capacity_lights < n_lights; MIRT_ERR_STATE before
 * mirt_set_scene. */
int mirt_debug_lights(mirt_ctx* ctx, int32_t* ids_out, float* sphere_rows_out, float* emit_rows_out, size_t capacity_lights, uint32_t info[4]);
/* Length histogram of the per-pixel candidate lists of the current scene / camera / size (policy.trace_primary_rays = 0 path):
 * hist[n] = local pixels whose bundle of camera rays can hit n spheres for n = 0..7, hist[8] = 8 or more (lists hold up to 31), hist[9] = pixels without a list (traced normally). */
int mirt_debug_primary_lists(mirt_ctx* ctx, uint32_t hist[10]);
/* The lists' lengths pixel by pixel, in local pixel order (tile-major, 256 per tile, as every per-pixel buffer of the context): counts[i] = spheres
 * listed for local pixel i (0..31), 0xffffffff for a pixel without a list.  MIRT_ERR_ARG when `capacity` (in counts) is below the local pixels. */
int mirt_debug_primary_counts(mirt_ctx* ctx, uint32_t* counts, size_t capacity);
/* Test knob: forbid (0) / allow (1, default) the binary16 records; takes effect at the next mirt_set_scene. */
int mirt_debug_allow_half_boxes(mirt_ctx* ctx, int allow);

#ifdef __cplusplus
}
#endif
#endif /* MIRT_H */
