// mirt_headless.cpp — headless stand-in for RaytracingApp (Application.cpp:32-235, 361-386): builds a scene the way
// the reference's constructor does, then drives the renderer with the reference's call protocol
// (Resize -> [Accumulate, Render] per frame) through mirt_host.hpp, and writes the resolved frame in the reference's own screenshot
// format — Radiance .hdr, flipped vertically like Image::Store (Image.cpp:71-74) — or as a PFM (by the extension of --out).  --hdri loads the
// environment map the way the constructor does (stbi_loadf(..., 4), Application.cpp:225-231); --ambient sets sky.ambient_color, which scales it.
//
//   mirt_headless --scene default9|furnace|bvh_test|brdf_test|synthetic:N [--size WxH] [--spp N | --frames N] [--bounces B] [--buckets K] [--brute] [--devices 0,1,..]
//                 [--hdri env.hdr] [--ambient A] [--brdf 0|1] [--gloss-decay a,b,...] [--exact-stream-order] [--out frame.hdr|frame.pfm] [--aov PREFIX] [--light-ris M] [--transmission] [--sky-sampling] [--closures 0,1,1,...] [--ggx-pdf]
//                 [--f-number F] [--focus-distance D] [--unit-mm U] [--focus-pixel X,Y]
//                 [--until-noise T] [--noise-quantile Q] [--noise-floor F] [--check-every N] [--max-accumulations M] [--noise-out map.pfm]
//                 [--adaptive T] [--min-accumulations N] [--counts-out counts.pfm] [--denoise [ITERATIONS]] [--denoise-plain-out plain.hdr|plain.pfm] [--temporal [MAX_RATIO]] [--orbit DEG] [--history-motion] [--ids-out ids.pfm]
// --denoise writes to --out the variance-guided à-trous denoised resolve of the last frame (mirt_render_atrous with its defaults; ITERATIONS, 0 .. 8,
// replaces their pass count) instead of the plain one; it implies the first-hit AOVs, which guide it.  --denoise-plain-out writes the plain frame beside it.
// --adaptive T renders with per-tile adaptive sampling (mirt_accumulate_adaptive): like --until-noise, but every 16 x 16 tile stops taking samples
// as soon as ITS Q-quantile is <= T (not before --min-accumulations, default 0); ends when every tile has stopped or at --max-accumulations.
// --counts-out writes the per-pixel sample count (each tile's count, painted over its pixels) as a one-channel PFM.  Adds a line
// {"adaptive": {"converged": ..., "issued": ..., "checks": ..., "frozen_tiles": ..., "owned_tiles": ..., "tile_accumulations": ...}}
// --until-noise T renders until converged instead of a fixed --spp (mirt_accumulate_until): N accumulations at a time (--check-every, default 4 x
// buckets) until the Q-quantile (--noise-quantile, default 0.95) of the per-pixel noise estimate — the relative standard error of the mean of the
// bucket means over (mean + F), F = --noise-floor — is <= T, or M accumulations (--max-accumulations, default 1000) are reached.  --noise-out writes
// the estimate of the final accumulator as a one-channel PFM (`Pf`).  Any of these options adds ONE line to stdout after the report:
// (converged and issued are null unless --until-noise ran the stopping loop; quantile_value is -1 when it is not finite)
// {"noise": {"converged": ..., "issued": ..., "quantile": Q, "quantile_value": ..., "max": ..., "mean": ..., "finite_pixels": ..., "nonfinite_pixels": ...}}
// Any of the four lens options turns the thin lens on (mirt_set_lens): camera.f_number / focus_distance / unit_mm as in Camera.hpp:64 (unit_mm =
// millimetres per world unit, default 1000); --focus-pixel X,Y is the right-click pick (Application.cpp:271-304): it prints the picked distance and
// focuses on its axial depth (a pick that meets the sky leaves the focus distance as given).
// --brdf 1 renders every hit with the GGX closure (#define BRDF 1, Renderer.hpp:70), --gloss-decay gives its per-bounce table (:212).
// --exact-stream-order replays the reference's stream slots and its scalar intersection tail (BVH.hpp:270-286; brute force, mirt_set_stream_order).
// --light-ris M picks the NEE light among M uniform candidates by resampled importance sampling (mirt_set_light_ris; 0 = off, at most 32).
// --transmission renders the materials that carry a transmission as glass: a smooth dielectric interface of index 1 + IOR_minus_one (mirt_set_transmission).
// --sky-sampling makes the environment map (--hdri, --ambient) one more light of next event estimation, drawn by importance (mirt_set_sky_sampling).
// --ggx-pdf gives the GGX closure its visible-normal pdf in the MIS weights: emitters and the sampled sky are weighed two ways on GGX surfaces (mirt_set_ggx_pdf).
// --closures 0,1,1,... gives the closure per material, 0 Lambertian and 1 GGX, so that both kinds share a scene; materials beyond the list take --brdf (mirt_set_material_closures).
// --aov PREFIX sums the first-hit AOVs beside the frame (mirt_set_aov) and writes PREFIX.depth.pfm (one channel, `Pf`), PREFIX.normal.pfm and
// PREFIX.albedo.pfm (`PF`) after the last frame.
// --devices: the GPUs the one Renderer object uses (tile rows split over them inside the library, one RCCL gather per frame read).
// --frames N is the UI loop itself (Application.cpp:373-380): N frames of { Accumulate(); Render(); }; the report lists the frames on
// which Render() produced output (every `buckets`-th, Renderer.hpp:437) and a hash of the last frame shown.
#include "mirt_host.hpp"
#include "hdr_io.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace mirt;

static Material make_material(float ar, float ag, float ab, float er = 0, float eg = 0, float eb = 0) {
	Material m{};
	m.albedo[0] = ar; m.albedo[1] = ag; m.albedo[2] = ab;
	m.emission[0] = er; m.emission[1] = eg; m.emission[2] = eb;
	return m;
}
// the members only the GGX closure reads (F0, roughness), those only the dielectric interface reads (transmission, IOR_minus_one; --transmission) and F80, which nothing reads
static Material with_ggx(Material m, vec3 F0, vec3 F80, float roughness, vec3 transmission = vec3{ 0, 0, 0 }, float IOR_minus_one = 0.0f) {
	m.F0[0] = F0.x; m.F0[1] = F0.y; m.F0[2] = F0.z;
	m.F80[0] = F80.x; m.F80[1] = F80.y; m.F80[2] = F80.z;
	m.transmission[0] = transmission.x; m.transmission[1] = transmission.y; m.transmission[2] = transmission.z;
	m.roughness = roughness; m.IOR_minus_one = IOR_minus_one;
	return m;
}
static Sphere make_sphere(float x, float y, float z, float radius_sq, int32_t mat) {
	Sphere s{};
	s.position[0] = x; s.position[1] = y; s.position[2] = z; s.radius_sq = radius_sq; s.material_ID = mat;
	return s;
}

// Scenes::Default, Application.cpp:33-101
static void scene_default9(Scene& sc) {
	sc.camera = Camera{ vec3{ -0.2f, 0.3f, 1.0f }, vec3{ 0.1f, -0.4f, -1.0f }, 40.0f, 1.0f };
	const vec3 none{ 0, 0, 0 };
	sc.material = {
		with_ggx(make_material(1, 1, 1), vec3{ 0.8f, 0.8f, 0.8f }, vec3{ 0.9f, 0.9f, 0.9f }, 0.2f),
		with_ggx(make_material(1, 1, 1, 0.1f * 25.0f, 0.1f * 25.0f, 0.1f * 200.0f), none, none, 1.0f),
		with_ggx(make_material(1, 1, 1, 0.1f * 150.0f, 0.1f * 150.0f, 0.1f * 150.0f), none, none, 1.0f),
		with_ggx(make_material(1, 1, 1, 200.0f, 17.0f, 25.0f), none, none, 1.0f),
		with_ggx(make_material(0.793f, 0.793f, 0.664f), vec3{ 0.04f, 0.04f, 0.04f }, vec3{ 0.5f, 0.5f, 0.5f }, 0.85f),
		with_ggx(make_material(0.05f, 0.05f, 0.05f), vec3{ 0.03f, 0.03f, 0.03f }, vec3{ 0.5f, 0.5f, 0.5f }, 0.05f, vec3{ 0.95f, 0.95f, 0.95f }, 0.44f),
		with_ggx(make_material(1, 1, 1), vec3{ 0.944f, 0.776f, 0.373f }, vec3{ 0.8f, 0.8f, 0.6f }, 0.15f),
		with_ggx(make_material(1, 1, 1), vec3{ 0.076288f, 0.077375f, 0.078887f }, vec3{ 0.47990f, 0.48028f, 0.48080f }, 0.1f, vec3{ 0.670f, 0.764f, 0.855f }, 0.762f),
		with_ggx(make_material(1, 1, 1), vec3{ 0.04f, 0.04f, 0.04f }, vec3{ 0.5f, 0.5f, 0.5f }, 0.8f) };
	sc.geometry = {
		make_sphere(0.3f, -1.47f, 0.0f, 1.5f * 1.5f, 0), make_sphere(0.29999f, 0.0801f, 0.0f, 0.05f * 0.05f, 1), make_sphere(0.3302f, 0.36165f, 0.7119f, 0.05f * 0.05f, 2),
		make_sphere(-0.4857f, -0.0242f, -0.41383f, 0.05f * 0.05f, 3), make_sphere(0.3f, 1.7f, 0.0f, 1.5f * 1.5f, 4), make_sphere(0.018f, 0.022f, 0.07f, 0.02f * 0.02f, 5),
		make_sphere(-0.037f, 0.022f, 0.0f, 0.03f * 0.03f, 6), make_sphere(-0.0846f, -0.0334f, 0.283f, 0.012f * 0.012f, 7), make_sphere(0.03863f, -0.00788f, 0.2835f, 0.012f * 0.012f, 8) };
}
// Scenes::BRDF_test, Application.cpp:123-217, the Properties::Roughness case the reference hard-codes (scene.py brdf_test)
static void scene_brdf_test(Scene& sc) {
	const int32_t gradations = 10;
	const float cam_offset = static_cast<float>(gradations) * 2.8f;
	sc.camera = Camera{ vec3{ 0, 0, cam_offset }, vec3{ 0, 0, -1 } };
	Material floor = make_material(0.1f, 0.1f, 0.1f); floor.roughness = 1.0f;
	sc.material = { floor, make_material(0, 0, 0, 100.0f, 100.0f, 100.0f) };
	sc.geometry = { make_sphere(0.0f, -1001.0f, 0.0f, 1000.0f * 1000.0f, 0), make_sphere(0.0f, 10.0f, 0.0f, 5.0f, 1) };
	for (int32_t i = 0; i < gradations; i++) {
		const float t = static_cast<float>(i) / static_cast<float>(gradations - 1);
		const float x = static_cast<float>(i * 2 - gradations) * 1.25f + 1.0f;
		sc.material.push_back(with_ggx(make_material(0, 0, 0), vec3{ 1, 1, 1 }, vec3{ 1, 1, 1 }, t));
		sc.geometry.push_back(make_sphere(x, static_cast<float>(i) * 0.1f, 0.0f, 1.0f, static_cast<int32_t>(sc.material.size()) - 1));
	}
	sc.sky.ambient_color[0] = sc.sky.ambient_color[1] = sc.sky.ambient_color[2] = 1.0f;
}
// Scenes::White_Furnace, Application.cpp:218-223
static void scene_furnace(Scene& sc) {
	sc.camera = Camera{ vec3{ 0, 0, 3 }, vec3{ 0, 0, -1 } };
	sc.material = { make_material(1, 1, 1) };
	sc.geometry = { make_sphere(0, 0, 0, 1.0f, 0) };
	sc.sky.ambient_color[0] = sc.sky.ambient_color[1] = sc.sky.ambient_color[2] = 1.0f;
}
// S(n) of SURVEY.md §8d, generator = the reference's PCG (Random.hpp:5-43) — same scene as scene.py's synthetic()
static uint32_t hash_u32(uint32_t i) { i ^= i >> 16; i *= 0x21f0aaadu; i ^= i >> 15; i *= 0xd35a2d97u; i ^= i >> 15; return i ^ 0xe6fe3bebu; }
static float next_unit(uint32_t& s) {
	uint32_t v = s; s = s * 747796405u + 2891336453u;
	v = ((v >> ((v >> 28u) + 4u)) ^ v) * 277803737u; v = (v >> 22u) ^ v;
	return static_cast<float>(v) * 0x1p-32f;
}
static void scene_synthetic(Scene& sc, uint32_t n, float ambient) {
	const float cb = static_cast<float>(std::cbrt(static_cast<double>(n))), H = cb, L = cb * 2.0f;
	uint32_t st = hash_u32(1);
	sc.material.assign(17, Material{});
	for (int m = 0; m < 16; m++) for (int c = 0; c < 3; c++) sc.material[m].albedo[c] = 0.2f + 0.6f * next_unit(st);
	sc.material[16] = make_material(1, 1, 1, 20, 20, 20);
	sc.geometry.assign(n, Sphere{});
	sc.geometry[0] = make_sphere(0, -1000.0f, 0, 1000.0f * 1000.0f, 0);
	for (uint32_t i = 1; i < n; i++) {
		const float u0 = next_unit(st), u1 = next_unit(st), u2 = next_unit(st), u3 = next_unit(st);
		const float r = 0.3f + 0.7f * u3;
		sc.geometry[i] = make_sphere(-L + (2.0f * L) * u0, 0.2f + (H - 0.2f) * u1, -L + (2.0f * L) * u2, r * r, static_cast<int32_t>(i % 16));
	}
	for (uint32_t i = 0; i < n; i++) if ((i % 64) == 63 || (n < 64 && i == n - 1)) sc.geometry[i].material_ID = 16;
	sc.camera = Camera{ vec3{ 0.0f, H, 3.0f * L }, vec3{ 0.0f, -0.3f, -1.0f }, 40.0f, 1.0f };
	sc.sky.ambient_color[0] = sc.sky.ambient_color[1] = sc.sky.ambient_color[2] = ambient;
}

// Scenes::BVH_test, Application.cpp:102-122, fixed version (see scene.py bvh_test(): the shipped scene has an empty material list and
// a std::mt19937 whose distributions differ between standard libraries): eight Lambertian materials, the reference's PCG seeded with
// hash_u32 of the low 32 bits of the shipped seed, draws per sphere in the shipped order radius, x, y, z, material.
static void scene_bvh_test(Scene& sc) {
	uint32_t st = hash_u32(0x04d15a07u);
	sc.material.assign(8, Material{});
	for (int m = 0; m < 8; m++) for (int c = 0; c < 3; c++) sc.material[m].albedo[c] = 0.2f + 0.7f * next_unit(st);
	sc.geometry.clear();
	for (int i = 0; i < 255; i++) {
		const float r = 0.3f + 19.7f * next_unit(st);
		const float x = -100.0f + 200.0f * next_unit(st);
		const float y = 100.0f * next_unit(st);
		const float z = -100.0f + 200.0f * next_unit(st);
		const uint32_t m = static_cast<uint32_t>(next_unit(st) * 8.0f);
		sc.geometry.push_back(make_sphere(x, y, z, r * r, static_cast<int32_t>(m < 7u ? m : 7u)));
	}
	sc.camera = Camera{ vec3{ 0, 60, 300 }, vec3{ 0, 0, -1 } };
	sc.sky.ambient_color[0] = sc.sky.ambient_color[1] = sc.sky.ambient_color[2] = 1.0f;
}

static uint64_t fnv1a(const std::vector<float>& v) {
	uint64_t hsh = 1469598103934665603ull;
	for (float f : v) { uint32_t u; std::memcpy(&u, &f, 4); for (int b = 0; b < 4; b++) { hsh ^= (u >> (8 * b)) & 0xffu; hsh *= 1099511628211ull; } }
	return hsh;
}

// An AOV image as mirt_render_aov leaves it: `channels` (1: `Pf`, 3: `PF`) floats per pixel, row 0 = y 0 = the bottom row PFM starts with.
static bool write_pfm_planes(const std::string& path, const std::vector<float>& img, uint32_t w, uint32_t h, uint32_t channels) {
	FILE* f = std::fopen(path.c_str(), "wb");
	if (!f) return false;
	std::fprintf(f, "%s\n%u %u\n-1.0\n", channels == 1 ? "Pf" : "PF", w, h);
	const bool ok = img.size() == static_cast<size_t>(w) * h * channels && std::fwrite(img.data(), sizeof(float), img.size(), f) == img.size();
	return (std::fclose(f) == 0) && ok;
}

static bool write_pfm(const std::string& path, const std::vector<float>& rgba, uint32_t w, uint32_t h) {
	FILE* f = std::fopen(path.c_str(), "wb");
	if (!f) return false;
	std::fprintf(f, "PF\n%u %u\n-1.0\n", w, h);                 // little-endian; PFM rows run bottom-to-top = framebuffer order (y 0 = bottom)
	std::vector<float> row(static_cast<size_t>(w) * 3);
	for (uint32_t y = 0; y < h; y++) {
		for (uint32_t x = 0; x < w; x++) for (int c = 0; c < 3; c++) row[x * 3 + c] = rgba[(static_cast<size_t>(y) * w + x) * 4 + c];
		std::fwrite(row.data(), sizeof(float), row.size(), f);
	}
	std::fclose(f);
	return true;
}

int main(int argc, char** argv) {
	std::string scene_name = "default9", out, hdri, aov_prefix;
	uint32_t w = 512, h = 512, spp = 10, n = 0;
	RendererPolicy policy;
	float ambient = 0.0f;
	bool ambient_set = false;
	std::vector<int> devices = { 0 };
	std::vector<float> gloss_decay;
	bool exact_stream_order = false;
	float f_number = 16.0f, focus_distance = 1.0f, unit_mm = 1000.0f;          // Camera.hpp:64
	bool lens = false, pick = false;
	uint32_t pick_x = 0, pick_y = 0;
	std::string noise_out;
	bool until_noise = false, noise_report = false;
	float noise_target = 0.0f, noise_quantile = 0.95f, noise_floor = 0.0f;
	uint32_t check_every = 0, max_accumulations = 1000;
	bool adaptive = false;
	uint32_t min_accumulations = 0, light_ris = 0;
	bool transmission = false, sky_sampling = false, ggx_pdf = false;
	std::vector<uint8_t> closures;
	std::string counts_out, plain_out;
	bool denoise = false;
	int denoise_iterations = -1;                                               // -1: the default
	bool temporal = false, history_motion = false;
	std::string ids_out;
	float temporal_ratio = -1.0f, orbit_deg = 0.0f;                            // -1: the default max_ratio
	bool sun_sky = false;
	float sun_elevation = 0.0f, sun_azimuth = 0.0f, sun_turbidity = -1.0f, sun_orbit_deg = 0.0f;   // turbidity -1: the default
	uint32_t env_w = 0, env_h = 0;                                             // 0: the default map size
	std::string env_out;
	struct SphereMove { uint32_t index; float step[3]; };                       // --move-sphere: geometry-order sphere `index` moves by `step` between frames
	std::vector<SphereMove> moves;
	struct EmissionEdit { uint32_t material; float rgb[3]; };                   // --set-emission: material `material` emits `rgb` from the second frame on
	struct MaterialAssign { uint32_t index; uint32_t material; };               // --sphere-material: geometry-order sphere `index` takes material `material`
	std::vector<EmissionEdit> emissions;
	std::vector<MaterialAssign> assigns;
	if (argc == 4 && std::string(argv[1]) == "--convert-hdr") {
		// file-format check without a GPU: read a picture like stbi_loadf does (top-down) and store it again like Image::Store does (which
		// flips, so the rows are handed over bottom-up): the output decodes to the same texels
		std::vector<float> texels; int32_t iw = 0, ih = 0;
		const std::string why = mirt_hdr::read(argv[2], texels, iw, ih);
		if (!why.empty()) { std::fprintf(stderr, "mirt_headless: %s: %s\n", argv[2], why.c_str()); return 1; }
		std::vector<float> flipped(texels.size());
		for (int32_t y = 0; y < ih; y++) std::memcpy(&flipped[static_cast<size_t>(y) * iw * 4], &texels[static_cast<size_t>(ih - 1 - y) * iw * 4], static_cast<size_t>(iw) * 16);
		return mirt_hdr::write_flipped(argv[3], flipped.data(), static_cast<uint32_t>(iw), static_cast<uint32_t>(ih)) ? 0 : 1;
	}
	for (int i = 1; i < argc; i++) {
		const std::string a = argv[i];
		auto next = [&]() -> const char* { if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", a.c_str()); std::exit(2); } return argv[++i]; };
		if (a == "--help") {             // before any device is touched
			std::puts("mirt_headless --scene default9|furnace|bvh_test|brdf_test|synthetic:N [--size WxH] [--spp N | --frames N] [--bounces B] [--buckets K] [--brute] [--devices 0,1,..]\n"
			          "              [--hdri env.hdr] [--ambient A] [--brdf 0|1] [--gloss-decay a,b,...] [--exact-stream-order] [--out frame.hdr|frame.pfm] [--aov PREFIX]\n"
			          "              [--light-ris M] [--transmission] [--sky-sampling] [--closures 0,1,1,...] [--ggx-pdf]\n"
			          "              [--f-number F] [--focus-distance D] [--unit-mm U] [--focus-pixel X,Y]\n"
			          "              [--until-noise T] [--noise-quantile Q] [--noise-floor F] [--check-every N] [--max-accumulations M] [--noise-out map.pfm]\n"
			          "              [--adaptive T] [--min-accumulations N] [--counts-out counts.pfm] [--denoise [ITERATIONS]] [--denoise-plain-out FILE]\n"
			          "              [--temporal [MAX_RATIO]] [--orbit DEG] [--history-motion] [--ids-out ids.pfm]\n"
		          "              [--sun-sky ELEVATION_DEG,AZIMUTH_DEG[,TURBIDITY]] [--env-size WxH] [--env-out env.hdr] [--sun-orbit DEG]\n"
		          "              [--move-sphere I:DX,DY,DZ]... [--set-emission M:R,G,B]... [--sphere-material I:M]...\n"
			          "mirt_headless --convert-hdr in.hdr out.hdr\n"
			          "  --sky-sampling  the environment map (--hdri, --ambient) is one more light of next event estimation, drawn by importance (mirt_set_sky_sampling)\n"
			          "  --ggx-pdf  the GGX closure's visible-normal pdf in the MIS weights: emitters and the sampled sky are weighed two ways on GGX surfaces (mirt_set_ggx_pdf)\n"
			          "  --light-ris M   the NEE light is picked among M candidates by resampled importance sampling (mirt_set_light_ris)\n"
			          "  --transmission  materials that carry a transmission render as glass (mirt_set_transmission)\n"
			          "  --denoise [N]   --out receives the variance-guided a-trous denoised resolve (N passes, default 5; implies the first-hit AOVs); --denoise-plain-out FILE: the plain frame\n"
			          "  --temporal [R]  every frame of --frames is `buckets` accumulations resolved through the temporal history (mirt_render_temporal; R = max_ratio, default 7; implies the AOVs); --out receives the last one\n"
			          "  --history-motion  with --temporal and --move-sphere: the history survives the moves; it carries the id map and the sphere table it was taken under (mirt_set_sphere_motion)\n"
		          "  --ids-out FILE  the first-hit id map of the last view as a one-channel .pfm: the BVH-order sphere every pixel centre shows, as a float, -1 for none (mirt_id_map)\n"
		          "  --orbit DEG     after every frame the camera yaws DEG degrees about the scene's centre and the accumulator is reset, as the reference does on a camera move (frames of `buckets` accumulations)\n"
			          "  --sun-sky E,A[,T]  the environment map is a Preetham sky of turbidity T with a sun disc at elevation E and azimuth A degrees, baked on the GPU under --ambient (mirt_set_sun_sky)\n"
		          "  --env-size WxH  texels of the map --sun-sky bakes (mirt_sun_sky_defaults: 1025x513)\n"
		          "  --env-out FILE  the environment map the kernels read, written as Radiance .hdr (mirt_read_environment)\n"
		          "  --sun-orbit DEG with --sun-sky and --frames: after every frame of `buckets` accumulations the sun turns DEG degrees about the vertical and the accumulator is reset (mirt_set_sun_sky alone: no mirt_set_scene)\n"
		          "  --move-sphere I:DX,DY,DZ  with --frames: before every frame after the first, geometry-order sphere I moves by (DX, DY, DZ) and the accumulator is reset; the tree in place is refitted on the GPU (mirt_update_spheres alone: no mirt_set_scene).  Repeatable\n"
		          "  --set-emission M:R,G,B  with --frames: before every frame after the first, material M emits (R, G, B) and the accumulator is reset; the material tables are replaced and the light list is regenerated on the GPU (mirt_update_materials alone: no mirt_set_scene).  Repeatable\n"
		          "  --sphere-material I:M  likewise: geometry-order sphere I takes material M (mirt_update_materials).  Repeatable\n"
		          "  --closures LIST the closure of material 0, 1, ...: 0 Lambertian, 1 GGX; materials beyond the list take --brdf (mirt_set_material_closures)");
			return 0;
		}
		else if (a == "--scene") scene_name = next();
		else if (a == "--size") { if (std::sscanf(next(), "%ux%u", &w, &h) != 2) return 2; }
		else if (a == "--spp" || a == "--frames") spp = static_cast<uint32_t>(std::atoi(next()));
		else if (a == "--bounces") policy.max_bounces = static_cast<uint32_t>(std::atoi(next()));
		else if (a == "--buckets") policy.buckets = static_cast<uint32_t>(std::atoi(next()));
		else if (a == "--ambient") { ambient = static_cast<float>(std::atof(next())); ambient_set = true; }
		else if (a == "--hdri") hdri = next();
		else if (a == "--brute") policy.use_bvh = false;
		else if (a == "--brdf") policy.brdf = static_cast<uint32_t>(std::atoi(next()));
		else if (a == "--gloss-decay") { for (const char* p = next(); *p;) { gloss_decay.push_back(static_cast<float>(std::atof(p))); while (*p && *p != ',') p++; if (*p == ',') p++; } }
		else if (a == "--exact-stream-order") exact_stream_order = true;
		else if (a == "--out") out = next();
		else if (a == "--aov") aov_prefix = next();
		else if (a == "--light-ris") light_ris = static_cast<uint32_t>(std::atoi(next()));
		else if (a == "--transmission") transmission = true;
		else if (a == "--sky-sampling") sky_sampling = true;
		else if (a == "--ggx-pdf") ggx_pdf = true;
		else if (a == "--closures") { for (const char* p = next(); *p;) { const int v = std::atoi(p); closures.push_back(static_cast<uint8_t>(v < 0 || v > 255 ? 255 : v)); while (*p && *p != ',') p++; if (*p == ',') p++; } }
		else if (a == "--f-number") { f_number = static_cast<float>(std::atof(next())); lens = true; }
		else if (a == "--focus-distance") { focus_distance = static_cast<float>(std::atof(next())); lens = true; }
		else if (a == "--unit-mm") { unit_mm = static_cast<float>(std::atof(next())); lens = true; }
		else if (a == "--focus-pixel") { if (std::sscanf(next(), "%u,%u", &pick_x, &pick_y) != 2) return 2; lens = pick = true; }
		else if (a == "--until-noise") { noise_target = static_cast<float>(std::atof(next())); until_noise = noise_report = true; }
		else if (a == "--noise-quantile") { noise_quantile = static_cast<float>(std::atof(next())); noise_report = true; }
		else if (a == "--noise-floor") { noise_floor = static_cast<float>(std::atof(next())); noise_report = true; }
		else if (a == "--check-every") { check_every = static_cast<uint32_t>(std::atoi(next())); noise_report = true; }
		else if (a == "--max-accumulations") { max_accumulations = static_cast<uint32_t>(std::atoi(next())); noise_report = true; }
		else if (a == "--noise-out") { noise_out = next(); noise_report = true; }
		else if (a == "--adaptive") { noise_target = static_cast<float>(std::atof(next())); adaptive = noise_report = true; }
		else if (a == "--min-accumulations") min_accumulations = static_cast<uint32_t>(std::atoi(next()));
		else if (a == "--counts-out") counts_out = next();
		else if (a == "--denoise") { denoise = true; if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') denoise_iterations = std::atoi(argv[++i]); }
		else if (a == "--denoise-plain-out") { plain_out = next(); denoise = true; }
		else if (a == "--temporal") { temporal = true; if (i + 1 < argc && ((argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') || argv[i + 1][0] == '.')) temporal_ratio = static_cast<float>(std::atof(argv[++i])); }
		else if (a == "--history-motion") history_motion = true;
		else if (a == "--ids-out") ids_out = next();
		else if (a == "--orbit") orbit_deg = static_cast<float>(std::atof(next()));
		else if (a == "--sun-sky") { const int got = std::sscanf(next(), "%f,%f,%f", &sun_elevation, &sun_azimuth, &sun_turbidity); if (got < 2) return 2; sun_sky = true; }
		else if (a == "--env-size") { if (std::sscanf(next(), "%ux%u", &env_w, &env_h) != 2) return 2; }
		else if (a == "--env-out") env_out = next();
		else if (a == "--move-sphere") { SphereMove m{}; if (std::sscanf(next(), "%u:%f,%f,%f", &m.index, &m.step[0], &m.step[1], &m.step[2]) != 4) return 2; moves.push_back(m); }
		else if (a == "--set-emission") { EmissionEdit e{}; if (std::sscanf(next(), "%u:%f,%f,%f", &e.material, &e.rgb[0], &e.rgb[1], &e.rgb[2]) != 4) return 2; emissions.push_back(e); }
		else if (a == "--sphere-material") { MaterialAssign m{}; if (std::sscanf(next(), "%u:%u", &m.index, &m.material) != 2) return 2; assigns.push_back(m); }
		else if (a == "--sun-orbit") sun_orbit_deg = static_cast<float>(std::atof(next()));
		else if (a == "--devices") { devices.clear(); for (const char* p = next(); *p;) { devices.push_back(std::atoi(p)); while (*p && *p != ',') p++; if (*p == ',') p++; } if (devices.empty()) return 2; }
		else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
	}
	try {
		Scene scene;
		if (scene_name == "default9") scene_default9(scene);
		else if (scene_name == "furnace") scene_furnace(scene);
		else if (scene_name == "brdf_test") scene_brdf_test(scene);
		else if (scene_name == "bvh_test") scene_bvh_test(scene);
		else if (scene_name.rfind("synthetic:", 0) == 0) { n = static_cast<uint32_t>(std::atoi(scene_name.c_str() + 10)); if (n < 2) return 2; scene_synthetic(scene, n, ambient); }
		else { std::fprintf(stderr, "unknown scene %s\n", scene_name.c_str()); return 2; }
		if (ambient_set) scene.sky.ambient_color[0] = scene.sky.ambient_color[1] = scene.sky.ambient_color[2] = ambient;
		if (!hdri.empty()) {                                           // Application.cpp:225-231
			const std::string why = mirt_hdr::read(hdri, scene.sky.hdri_data, scene.sky.hdri_width, scene.sky.hdri_height);
			if (!why.empty()) { std::fprintf(stderr, "mirt_headless: %s: %s\n", hdri.c_str(), why.c_str()); return 1; }
		}
		scene.RebuildAcceleration();                                   // Application.cpp:233-234

		Renderer renderer{ scene, policy, devices };
		renderer.SetGlossDecay(gloss_decay);
		renderer.SetStreamOrder(exact_stream_order);
		if (!aov_prefix.empty() || denoise || temporal) renderer.SetAOV(true);
		renderer.SetLightRis(light_ris);
		renderer.SetTransmission(transmission);
		renderer.SetSkySampling(sky_sampling);
		renderer.SetGgxPdf(ggx_pdf);
		renderer.SetMaterialClosures(closures);
		if (history_motion) renderer.SetHistoryMotion(true);
		// pad the viewport to the tile requirement like UIRender does (Application.cpp:365-372)
		const uint32_t t = static_cast<uint32_t>(Renderer::RequiredTiling());
		w = (w + t - 1) & ~(t - 1); h = (h + t - 1) & ~(t - 1);
		scene.camera.Resize(w, h);                                     // Application.cpp:375-376
		renderer.SceneChanged();
		renderer.Resize(w, h);
		mirt_sun_sky_params sun = Renderer::SunSkyDefaults();
		auto aim_sun = [&]() {                                          // elevation and azimuth in degrees -> the direction towards the sun, y up
			const double el = sun_elevation * 3.14159265358979323846 / 180.0, az = sun_azimuth * 3.14159265358979323846 / 180.0;
			sun.sun_dir[0] = static_cast<float>(std::cos(el) * std::cos(az)); sun.sun_dir[1] = static_cast<float>(std::sin(el)); sun.sun_dir[2] = static_cast<float>(std::cos(el) * std::sin(az));
			if (sun_elevation == 90.0f) { sun.sun_dir[0] = sun.sun_dir[2] = 0.0f; }
			if (sun_elevation == 0.0f) sun.sun_dir[1] = 0.0f;
			renderer.SetSunSky(sun);
		};
		if (sun_sky) {                                                  // the Ambient update: after SceneChanged(), which handed over scene.sky
			if (sun_turbidity >= 0.0f) sun.turbidity = sun_turbidity;
			if (env_w) { sun.width = env_w; sun.height = env_h; }
			aim_sun();
		}
		if (lens) {
			scene.camera.f_number = f_number; scene.camera.focus_distance = focus_distance; scene.camera.unit_mm = unit_mm;
			if (pick) {                                                     // pick, then set (Application.cpp:298-299)
				const Renderer::Pick p = renderer.PickFocus(pick_x, pick_y);
				std::printf("picked focus at pixel (%u, %u): distance %g, depth %g\n", pick_x, pick_y, static_cast<double>(p.distance), static_cast<double>(p.depth));
				if (std::isfinite(p.depth)) scene.camera.focus_distance = p.depth;
			}
			renderer.SetLens(scene.camera.aperture_radius(), scene.camera.focus_distance);
			renderer.ResetAccumulator();
		}

		const auto t0 = std::chrono::steady_clock::now();
		bool have_frame = false;
		std::vector<float> temporal_frame;                             // --temporal: the last frame resolved through the history
		std::string frames_due;                                        // 1-based frame numbers on which Render() produced output
		Renderer::UntilResult until{};
		Renderer::AdaptiveResult adapt{};
		if (adaptive) {                                                // per-tile adaptive sampling: the frame is resolved once, at the end, every tile at its own count
			const mirt_stop_rule rule{ noise_target, noise_quantile, noise_floor, check_every ? check_every : 4u * policy.buckets, max_accumulations };
			adapt = renderer.AccumulateAdaptive(rule, min_accumulations);
			if (renderer.Render()) { have_frame = true; frames_due = std::to_string(renderer.accumulations()); }
		}
		else if (until_noise) {                                        // render until converged: the frame is resolved once, at the end
			const mirt_stop_rule rule{ noise_target, noise_quantile, noise_floor, check_every ? check_every : 4u * policy.buckets, max_accumulations };
			until = renderer.AccumulateUntil(rule);
			if (renderer.Render()) { have_frame = true; frames_due = std::to_string(renderer.accumulations()); }
		}
		else if (sun_sky && sun_orbit_deg != 0.0f) {
			// A moving sun: every frame is `buckets` accumulations; then the sun turns about the vertical through SetSunSky alone — no SceneChanged(),
			// no tree rebuild — and the accumulator is reset, as on any edit (Application.cpp:503-510).
			for (uint32_t frame = 0; frame < spp; frame++) {
				renderer.Accumulate(policy.buckets);
				if (renderer.Render()) { have_frame = true; frames_due += (frames_due.empty() ? "" : ", ") + std::to_string(frame + 1); }
				if (frame + 1 < spp) { sun_azimuth += sun_orbit_deg; aim_sun(); renderer.ResetAccumulator(); }
			}
		}
		else if (!moves.empty() || !emissions.empty() || !assigns.empty()) {
			// A drag: every frame is `buckets` accumulations; then the spheres move in both of the scene's arrays and UpdateSpheres hands those rows over
			// alone — no RebuildAcceleration(), no SceneChanged(): the tree in place is refitted — and the accumulator is reset (Application.cpp:466-468,510).
			std::vector<uint32_t> geometry_index, bvh_index;
			for (const SphereMove& m : moves) {
				if (m.index >= scene.geometry.size()) { std::fprintf(stderr, "--move-sphere %u: the scene has %zu spheres\n", m.index, scene.geometry.size()); return 2; }
				geometry_index.push_back(m.index); bvh_index.push_back(renderer.BvhIndexOf(m.index));
			}
			// A material edit (Application.cpp:470-485): the emissions and the material ids are written into the scene's arrays and UpdateMaterials hands
			// those rows and ids over alone; the light list is regenerated on the GPU.  The edit is absolute: applied again before every later frame.
			std::vector<uint32_t> material_index, assign_geometry, assign_bvh;
			for (const EmissionEdit& e : emissions) {
				if (e.material >= scene.material.size()) { std::fprintf(stderr, "--set-emission %u: the scene has %zu materials\n", e.material, scene.material.size()); return 2; }
				material_index.push_back(e.material);
			}
			for (const MaterialAssign& m : assigns) {
				if (m.index >= scene.geometry.size() || m.material >= scene.material.size()) { std::fprintf(stderr, "--sphere-material %u:%u: the scene has %zu spheres and %zu materials\n", m.index, m.material, scene.geometry.size(), scene.material.size()); return 2; }
				assign_geometry.push_back(m.index); assign_bvh.push_back(renderer.BvhIndexOf(m.index));
			}
			// --temporal resolves each frame through the history; UpdateSpheres drops it unless --history-motion lets it follow the spheres.
			mirt_denoise_params dp = Renderer::DenoiseDefaults();
			if (denoise_iterations >= 0) dp.iterations = static_cast<uint32_t>(denoise_iterations);
			mirt_temporal_params tp = Renderer::TemporalDefaults();
			if (temporal_ratio >= 0.0f) tp.max_ratio = temporal_ratio;
			for (uint32_t frame = 0; frame < spp; frame++) {
				renderer.Accumulate(policy.buckets);
				if (renderer.Render()) { have_frame = true; frames_due += (frames_due.empty() ? "" : ", ") + std::to_string(frame + 1); }
				if (temporal) {
					mirt_temporal_stats st{};
					temporal_frame = renderer.RenderTemporal(dp, tp, nullptr, &st);
					std::printf("{\"temporal\": {\"frame\": %u, \"reprojected\": %llu, \"no_history\": %llu, \"outside\": %llu, \"rejected\": %llu, \"unusable\": %llu, \"frame_fnv1a\": \"%016llx\"}}\n", frame + 1,
					            (unsigned long long)st.reprojected, (unsigned long long)st.no_history, (unsigned long long)st.outside, (unsigned long long)st.rejected, (unsigned long long)st.unusable,
					            (unsigned long long)fnv1a(temporal_frame));
				}
				if (frame + 1 < spp) {
					for (size_t k = 0; k < moves.size(); k++) {
						Sphere& g = scene.geometry[geometry_index[k]];
						for (int a = 0; a < 3; a++) g.position[a] += moves[k].step[a];
						scene.acceleration_structure.prims[bvh_index[k]] = g;
					}
					if (!moves.empty()) renderer.UpdateSpheres(bvh_index, geometry_index);
					if (!material_index.empty() || !assign_geometry.empty()) {
						for (const EmissionEdit& e : emissions) for (int a = 0; a < 3; a++) scene.material[e.material].emission[a] = e.rgb[a];
						for (size_t k = 0; k < assigns.size(); k++) {
							scene.geometry[assign_geometry[k]].material_ID = static_cast<int32_t>(assigns[k].material);
							scene.acceleration_structure.prims[assign_bvh[k]].material_ID = static_cast<int32_t>(assigns[k].material);
						}
						renderer.UpdateMaterials(material_index, assign_bvh, assign_geometry);
					}
					renderer.ResetAccumulator();
				}
			}
		}
		else if (temporal || orbit_deg != 0.0f) {
			// A moving camera: every frame is `buckets` accumulations (the fewest Render() resolves), then the camera yaws about the scene's centre
			// and the accumulator is reset, as the reference does on every move (Application.cpp:309-333).  --temporal resolves each frame through
			// the history, which survives the reset.
			vec3 centre{};
			for (const auto& sp : scene.geometry) { centre.x += sp.position[0]; centre.y += sp.position[1]; centre.z += sp.position[2]; }
			if (!scene.geometry.empty()) { const float inv = 1.0f / static_cast<float>(scene.geometry.size()); centre.x *= inv; centre.y *= inv; centre.z *= inv; }
			const float half = orbit_deg * 0.5f * 3.14159265358979f / 180.0f, sy = std::sin(half), cy = std::cos(half), s2 = 2.0f * sy * cy, c2 = cy * cy - sy * sy;
			mirt_denoise_params dp = Renderer::DenoiseDefaults();
			if (denoise_iterations >= 0) dp.iterations = static_cast<uint32_t>(denoise_iterations);
			mirt_temporal_params tp = Renderer::TemporalDefaults();
			if (temporal_ratio >= 0.0f) tp.max_ratio = temporal_ratio;
			for (uint32_t frame = 0; frame < spp; frame++) {
				renderer.Accumulate(policy.buckets);
				if (renderer.Render()) { have_frame = true; frames_due += (frames_due.empty() ? "" : ", ") + std::to_string(frame + 1); }
				if (temporal) {
					mirt_temporal_stats st{};
					temporal_frame = renderer.RenderTemporal(dp, tp, nullptr, &st);
					std::printf("{\"temporal\": {\"frame\": %u, \"reprojected\": %llu, \"no_history\": %llu, \"outside\": %llu, \"rejected\": %llu, \"unusable\": %llu, \"frame_fnv1a\": \"%016llx\"}}\n", frame + 1,
					            (unsigned long long)st.reprojected, (unsigned long long)st.no_history, (unsigned long long)st.outside, (unsigned long long)st.rejected, (unsigned long long)st.unusable,
					            (unsigned long long)fnv1a(temporal_frame));
				}
				if (orbit_deg != 0.0f && frame + 1 < spp) {                 // yaw by the quaternion (0, sy, 0, cy): the position about the centre, the orientation with it
					Camera& cam = scene.camera;
					const float dx = cam.pos.x - centre.x, dz = cam.pos.z - centre.z;
					cam.pos.x = centre.x + (c2 * dx + s2 * dz); cam.pos.z = centre.z + (c2 * dz - s2 * dx);
					const quat o = cam.orient;
					cam.orient = quat{ cy * o.x + sy * o.z, cy * o.y + sy * o.w, cy * o.z - sy * o.x, cy * o.w - sy * o.y };
					renderer.CameraChanged();
					renderer.ResetAccumulator();
				}
			}
		}
		else for (uint32_t frame = 0; frame < spp; frame++) {          // one UIRender per frame: Accumulate(); Render();  (Application.cpp:379-380)
			renderer.Accumulate();
			if (renderer.Render()) { have_frame = true; frames_due += (frames_due.empty() ? "" : ", ") + std::to_string(frame + 1); }
		}
		const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		Renderer::NoiseResult nz;                                      // read before anything is printed or written: a frame count that gives no estimate fails the run as a whole
		if (noise_report) {
			nz = renderer.Noise(noise_floor, !noise_out.empty());
			if (!nz.ready) { std::fprintf(stderr, "mirt_headless: no noise estimate: %u accumulations are not a positive multiple of %u buckets\n", renderer.accumulations(), policy.buckets); return 1; }
		}
		const mirt_counters c = renderer.counters();

		// FNV-1a over the raw accumulator words: lets a test compare this C++ host against the Python host bit for bit
		const std::vector<float> acc = renderer.accumulator();
		const uint64_t hsh = fnv1a(acc);
		const uint64_t frame_hsh = have_frame ? fnv1a(renderer.GetFrame()) : 0ull;

		std::printf("{\"scene\": \"%s\", \"spheres\": %zu, \"nodes\": %zu, \"lights\": %zu, \"width\": %u, \"height\": %u, \"accumulations\": %u, "
		            "\"rays\": %llu, \"shadow_rays\": %llu, \"terminated\": %llu, \"dropped\": %llu, \"seconds\": %.6f, \"mray_per_s\": %.3f, "
		            "\"accumulator_fnv1a\": \"%016llx\", \"frame_ready\": %s, \"frames_due\": [%s], \"last_frame_fnv1a\": \"%016llx\", \"gpus\": %zu, \"gather_ms\": %.3f}\n",
		            scene_name.c_str(), scene.geometry.size(), scene.acceleration_structure.nodes.size(), scene.lighting_acceleration.prims.size(), w, h,
		            renderer.accumulations(), (unsigned long long)c.rays, (unsigned long long)c.shadow_rays, (unsigned long long)c.terminated,
		            (unsigned long long)c.dropped, sec, c.rays / sec / 1e6, (unsigned long long)hsh, have_frame ? "true" : "false", frames_due.c_str(), (unsigned long long)frame_hsh, devices.size(), renderer.gather_ms());
		auto write_frame = [&](const std::string& path, const std::vector<float>& frame) {
			const bool as_hdr = path.size() >= 4 && path.compare(path.size() - 4, 4, ".hdr") == 0;
			const bool ok = as_hdr ? mirt_hdr::write_flipped(path, frame.data(), w, h) : write_pfm(path, frame, w, h);
			if (!ok) std::fprintf(stderr, "cannot write %s\n", path.c_str());
			return ok;
		};
		if (temporal && !temporal_frame.empty()) { if (!out.empty() && !write_frame(out, temporal_frame)) return 1; }      // --temporal decides what --out receives, --denoise or not
		else if (denoise && have_frame) {                              // the denoised resolve of the accumulator the last frame shows
			mirt_denoise_params dp = Renderer::DenoiseDefaults();
			if (denoise_iterations >= 0) dp.iterations = static_cast<uint32_t>(denoise_iterations);
			const std::vector<float> filtered = renderer.RenderDenoised(dp);
			if (filtered.empty()) { std::fprintf(stderr, "mirt_headless: no denoised frame: %u accumulations are not a positive multiple of %u buckets\n", renderer.accumulations(), policy.buckets); return 1; }
			std::printf("{\"denoise\": {\"iterations\": %u, \"frame_fnv1a\": \"%016llx\"}}\n", dp.iterations, (unsigned long long)fnv1a(filtered));
			if (!out.empty() && !write_frame(out, filtered)) return 1;
			if (!plain_out.empty() && !write_frame(plain_out, renderer.GetFrame())) return 1;
		}
		else if (!out.empty() && have_frame && !write_frame(out, renderer.GetFrame())) return 1;
		if (!ids_out.empty()) {
			const Renderer::IdMapResult ids = renderer.IdMap();
			std::vector<float> img(ids.prim.size());
			for (size_t k = 0; k < img.size(); k++) img[k] = static_cast<float>(ids.prim[k]);
			if (!write_pfm_planes(ids_out, img, w, h, 1)) { std::fprintf(stderr, "cannot write %s\n", ids_out.c_str()); return 1; }
		}
		if (!env_out.empty()) {
			const Renderer::Environment env = renderer.ReadEnvironment();
			std::printf("{\"environment\": {\"width\": %u, \"height\": %u, \"baked\": %s, \"fnv1a\": \"%016llx\"}}\n", env.width, env.height, env.baked ? "true" : "false", (unsigned long long)fnv1a(env.rgba));
			if (!mirt_hdr::write_flipped(env_out, env.rgba.data(), env.width, env.height)) { std::fprintf(stderr, "cannot write %s\n", env_out.c_str()); return 1; }
		}
		if (!aov_prefix.empty()) {
			const struct { int which; const char* name; uint32_t channels; } outputs[3] = { { MIRT_AOV_DEPTH, "depth", 1 }, { MIRT_AOV_NORMAL, "normal", 3 }, { MIRT_AOV_ALBEDO, "albedo", 3 } };
			for (const auto& o : outputs) {
				const std::string path = aov_prefix + "." + o.name + ".pfm";
				if (!write_pfm_planes(path, renderer.RenderAOV(o.which), w, h, o.channels)) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
			}
		}
		if (adaptive)
			std::printf("{\"adaptive\": {\"converged\": %s, \"issued\": %u, \"checks\": %u, \"frozen_tiles\": %u, \"owned_tiles\": %u, \"tile_accumulations\": %llu}}\n", adapt.converged ? "true" : "false",
			            adapt.report.issued, adapt.report.checks, adapt.report.frozen_tiles, adapt.report.owned_tiles, (unsigned long long)adapt.report.tile_accumulations);
		if (!counts_out.empty()) {                                     // every tile's count over its 16 x 16 pixels (rows as in the frame: row 0 = y 0)
			const std::vector<uint32_t> counts = renderer.TileCounts();
			std::vector<float> img(static_cast<size_t>(w) * h, 0.0f);
			const uint32_t h_tiles = w / 16u;
			for (uint32_t y = 0; y < h; y++) for (uint32_t x = 0; x < w; x++) img[static_cast<size_t>(y) * w + x] = static_cast<float>(counts[(y / 16u) * h_tiles + x / 16u]);
			if (!write_pfm_planes(counts_out, img, w, h, 1)) { std::fprintf(stderr, "cannot write %s\n", counts_out.c_str()); return 1; }
		}
		if (noise_report) {
			const float qv = Renderer::NoiseQuantile(nz.hist, static_cast<double>(noise_quantile));
			const std::string loop = until_noise ? std::string(until.converged ? "true" : "false") + ", \"issued\": " + std::to_string(until.issued) : "null, \"issued\": null";   // null: no stopping loop ran
			std::printf("{\"noise\": {\"converged\": %s, \"quantile\": %.9g, \"quantile_value\": %.9g, \"max\": %.9g, \"mean\": %.17g, "
			            "\"finite_pixels\": %llu, \"nonfinite_pixels\": %llu}}\n", loop.c_str(),
			            static_cast<double>(noise_quantile), std::isfinite(qv) ? static_cast<double>(qv) : -1.0, static_cast<double>(nz.stats.max), nz.stats.mean,
			            (unsigned long long)nz.stats.finite_pixels, (unsigned long long)nz.stats.nonfinite_pixels);
			if (!noise_out.empty() && !write_pfm_planes(noise_out, nz.map, w, h, 1)) { std::fprintf(stderr, "cannot write %s\n", noise_out.c_str()); return 1; }
		}
	} catch (const std::exception& e) {
		std::fprintf(stderr, "mirt_headless: %s\n", e.what());
		return 1;
	}
	return 0;
}
