// mirt_resolve.hip — the resolve layer of the C-ABI (ctx.hpp): everything that reads a finished accumulator or AOV slab.  mirt_render and
// mirt_render_aov (resolve.hpp), the denoised resolves with and without the temporal history (denoise.hpp, temporal.hpp), the noise estimate and
// what is built on it: per-tile freezes and counts, mirt_accumulate_adaptive and mirt_accumulate_until.  The id map it needs under
// mirt_set_sphere_motion is the launch layer's (launch_id_map).
#include "ctx.hpp"
#include "denoise.hpp"
#include "temporal.hpp"
#include "resolve.hpp"
#include "noise_host.hpp"

#include <cmath>
#include <cstring>

using namespace mirt;

namespace {

// The mask and the list of active pixels as the sparse kernels read them.  The caller has synchronised every stream.
int upload_freezes(mirt_ctx* c) {
	if (c->freeze.n_frozen == 0) return MIRT_OK;
	std::vector<uint32_t> mask(c->n_tiles), list(1);
	list.reserve(static_cast<size_t>(c->n_tiles - c->freeze.n_frozen) * kTileSize + 1);
	for (uint32_t t = 0; t < c->n_tiles; t++) {
		mask[t] = c->freeze.frozen[t] ? 1u : 0u;
		if (!c->freeze.frozen[t]) for (uint32_t id = 0; id < kTileSize; id++) list.push_back(t * kTileSize + id);
	}
	list[0] = static_cast<uint32_t>(list.size() - 1);
	HIP_TRY(c, c->freeze.tile_frozen.ensure(mask.size() * sizeof(uint32_t)));
	HIP_TRY(c, c->freeze.active_list.ensure((static_cast<size_t>(c->n_tiles) * kTileSize + 1) * sizeof(uint32_t)));
	HIP_TRY(c, hipMemcpy(c->freeze.tile_frozen.ptr, mask.data(), mask.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
	HIP_TRY(c, hipMemcpy(c->freeze.active_list.ptr, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
	c->freeze.freeze_gen++;
	return MIRT_OK;
}
// The per-tile counts for a resolve kernel: NULL while no tile is frozen (the kernels then do what they have always done).  The caller has
// synchronised every stream, and the kernel it launches is on the main stream, behind this copy.
int upload_tile_counts(mirt_ctx* c, const uint32_t** dev) {
	*dev = nullptr;
	if (c->freeze.n_frozen == 0) return MIRT_OK;
	std::vector<uint32_t> counts(c->n_tiles);
	for (uint32_t t = 0; t < c->n_tiles; t++) counts[t] = tile_count(c, t);
	HIP_TRY(c, c->freeze.tile_counts.ensure(counts.size() * sizeof(uint32_t)));
	HIP_TRY(c, hipMemcpy(c->freeze.tile_counts.ptr, counts.data(), counts.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
	*dev = c->freeze.tile_counts.as<uint32_t>();
	return MIRT_OK;
}
} // namespace

extern "C" {

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
	HIP_TRY(c, hipMemcpyAsync(c->frame_host.ptr, c->framebuffer.ptr, frame_floats * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	if (whole) std::memcpy(rgba_host, c->frame_host.ptr, frame_floats * sizeof(float));   // every pixel is this context's
	else copy_owned_tiles(tile_map(c), c->n_tiles, 4u, c->frame_host.ptr, rgba_host);                 // only this context's tiles
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
	for (DeviceBuffer* b : { &c->dn.cv[0], &c->dn.cv[1], &c->dn.gd, &c->dn.mu }) HIP_TRY(c, b->ensure(image_bytes));
	const uint32_t* counts = nullptr;
	if ((r = upload_tile_counts(c, &counts))) return r;
	const TileMap m = tile_map(c);
	{ Bracket t(c, MIRT_K_RESOLVE);
	  hipLaunchKernelGGL(k_denoise_prepare, dim3(c->n_tiles), dim3(kTileSize), 0, c->stream, c->accumulator.as<float>(), c->aov.as<float>(), c->dn.cv[0].as<float4>(),
	                     c->dn.gd.as<float4>(), c->dn.mu.as<float4>(), m, k, scale, static_cast<float>(c->accumulations), counts, c->camera.exposure, p->demodulate, p->albedo_floor); }
	HIP_TRY(c, hipGetLastError());
	// The passes go from `src` to `dst`; the two swap, and the buffer that becomes free after the first pass is `spare`.  Plain: cv[0] -> cv[1] -> cv[0].
	// Temporal: k_reproject writes the blend into cv[1], which the passes only read when it is to become the history (update = 1: the old history's
	// (x, v) image is the spare then, free as soon as k_reproject has read it).
	float4 *src = c->dn.cv[0].as<float4>(), *dst = c->dn.cv[1].as<float4>(), *spare = c->dn.cv[0].as<float4>();
	if (tp) {
		const size_t len_bytes = static_cast<size_t>(c->width) * c->height * sizeof(float);
		HIP_TRY(c, c->hist.len.ensure(len_bytes));
		HIP_TRY(c, c->hist.stats.ensure(kTemporalStatSlots * kTemporalStatPitch * sizeof(unsigned long long)));
		if (tp->update) { HIP_TRY(c, c->hist.x.ensure(image_bytes)); HIP_TRY(c, c->hist.g.ensure(image_bytes)); HIP_TRY(c, c->hist.n.ensure(len_bytes)); }
		HIP_TRY(c, hipMemsetAsync(c->hist.stats.ptr, 0, kTemporalStatSlots * kTemporalStatPitch * sizeof(unsigned long long), c->stream));
		TemporalDev td{};
		td.cam = c->camera; td.prev = c->hist.cam;
		td.max_ratio = tp->max_ratio; td.depth_tol = tp->depth_tol; td.normal_min = tp->normal_min;
		// the call takes the history when there is one, of this image and these demodulation settings, and both cameras rotate
		// (x carries the exposure it was resolved under: a history of another exposure word is in other units)
		td.take = (c->hist.valid && tp->max_ratio > 0.0f && c->hist.width == c->width && c->hist.height == c->height && c->hist.demodulate == p->demodulate &&
		           std::memcmp(&c->hist.albedo_floor, &p->albedo_floor, sizeof(float)) == 0 && std::memcmp(&c->hist.cam.exposure, &c->camera.exposure, sizeof(float)) == 0 &&
		           unit_orient(c->camera) && unit_orient(c->hist.cam)) ? 1u : 0u;
		td.identity = std::memcmp(&c->camera, &c->hist.cam, sizeof(CameraParams)) == 0 ? 1u : 0u;
		if (!td.take) td.prev = c->camera;
		if (c->history_motion) {
			// the id map of this camera first, then the MOTION instantiation: the pixel's sphere, the table now and the table the history was taken under
			const size_t id_bytes = static_cast<size_t>(c->width) * c->height * sizeof(int32_t);
			HIP_TRY(c, c->hist.id_cur.ensure(id_bytes));
			if (tp->update) { HIP_TRY(c, c->hist.id.ensure(id_bytes)); HIP_TRY(c, c->hist.snap.ensure(std::max<size_t>(gs->scene.n_spheres, 1) * sizeof(float4))); }
			if ((r = launch_id_map(c, gs, c->hist.id_cur.as<int32_t>(), nullptr))) return r;
			const MotionDev<true> mo{ c->hist.id_cur.as<int32_t>(), c->hist.id.as<int32_t>(), gs->scene.spheres, c->hist.snap.as<float4>() };
			Bracket t(c, MIRT_K_RESOLVE);
			hipLaunchKernelGGL(k_reproject<true>, dim3(c->h_tiles, c->v_tiles), dim3(kAtrousBlock * kAtrousBlock), 0, c->stream, c->dn.cv[0].as<float4>(), c->dn.gd.as<float4>(),
			                   c->hist.x.as<float4>(), c->hist.g.as<float4>(), c->hist.n.as<float>(), c->dn.cv[1].as<float4>(), c->hist.len.as<float>(), c->hist.stats.as<unsigned long long>(),
			                   c->width, c->h_tiles * kAtrousBlock, c->v_tiles * kAtrousBlock, counts, c->accumulations, td, mo);
		} else {
			Bracket t(c, MIRT_K_RESOLVE);
			hipLaunchKernelGGL(k_reproject<false>, dim3(c->h_tiles, c->v_tiles), dim3(kAtrousBlock * kAtrousBlock), 0, c->stream, c->dn.cv[0].as<float4>(), c->dn.gd.as<float4>(),
			                   c->hist.x.as<float4>(), c->hist.g.as<float4>(), c->hist.n.as<float>(), c->dn.cv[1].as<float4>(), c->hist.len.as<float>(), c->hist.stats.as<unsigned long long>(),
			                   c->width, c->h_tiles * kAtrousBlock, c->v_tiles * kAtrousBlock, counts, c->accumulations, td, MotionDev<false>{});
		}
		HIP_TRY(c, hipGetLastError());
		// the snapshot follows the table once the kernel has read the old one (stream order); skipped while no mirt_update_spheres came since the last copy
		if (c->history_motion && tp->update && gs->scene.n_spheres && (!c->hist.snap_valid || c->hist.snap_gen != gs->spheres_gen))
			HIP_TRY(c, hipMemcpyAsync(c->hist.snap.ptr, gs->scene.spheres, static_cast<size_t>(gs->scene.n_spheres) * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
		src = c->dn.cv[1].as<float4>(); dst = c->dn.cv[0].as<float4>();
		spare = tp->update ? c->hist.x.as<float4>() : c->dn.cv[1].as<float4>();
	}
	// From the second pass on, update = 1 writes into the old history's (x, v) image: a HIP error between here and the renaming below would
	// leave a history that claims to be valid over a scratch image, so such a return drops it (mirt.h, step 4).
	struct DropOnError { mirt_ctx* c; bool armed; ~DropOnError() { if (armed) c->hist.valid = false; } } guard{ c, tp && tp->update && p->iterations >= 2u };
	const DenoiseDev dev{ p->sigma_lum, p->sigma_depth, p->lum_floor, p->normal_squarings };
	for (uint32_t i = 0; i < p->iterations; i++) {
		const uint32_t step = 1u << i;
		const bool staged = step <= c->tune.denoise_staged;
		Bracket t(c, MIRT_K_RESOLVE);
		hipLaunchKernelGGL(staged ? k_atrous<true> : k_atrous<false>, dim3(c->h_tiles, c->v_tiles), dim3(kAtrousBlock * kAtrousBlock), 0, c->stream,
		                   src, c->dn.gd.as<float4>(), dst, c->width, c->h_tiles * kAtrousBlock, c->v_tiles * kAtrousBlock, step, dev);
		float4* const next = i == 0u ? spare : src;
		src = dst; dst = next;
	}
	HIP_TRY(c, hipGetLastError());
	{ Bracket t(c, MIRT_K_RESOLVE);
	  hipLaunchKernelGGL(k_denoise_finish, dim3(grid_for(c, n_pix)), dim3(kBlock), 0, c->stream, src, c->dn.mu.as<float4>(), c->framebuffer.as<float4>(), n_pix, m); }
	HIP_TRY(c, hipGetLastError());
	// the frame leaves as mirt_render's does (the framebuffer is scratch: every resolve writes all of the context's tiles before it is read)
	const size_t frame_floats = static_cast<size_t>(c->width) * c->height * 4;
	const bool whole = c->width == c->h_tiles * MIRT_TILE_ROOT && c->height == c->v_tiles * MIRT_TILE_ROOT;
	HIP_TRY(c, hipMemcpyAsync(c->frame_host.ptr, c->framebuffer.ptr, frame_floats * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	std::vector<float> len_host;
	unsigned long long class_counts[kTemporalClasses] = {};
	std::vector<unsigned long long> count_slots(tp ? kTemporalStatSlots * kTemporalStatPitch : 0u);
	if (tp) {
		if (history_len) { len_host.resize(static_cast<size_t>(c->width) * c->height); HIP_TRY(c, hipMemcpyAsync(len_host.data(), c->hist.len.ptr, len_host.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream)); }
		HIP_TRY(c, hipMemcpyAsync(count_slots.data(), c->hist.stats.ptr, count_slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
	}
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	if (whole) std::memcpy(rgba_host, c->frame_host.ptr, frame_floats * sizeof(float));
	else copy_owned_tiles(m, c->n_tiles, 4u, c->frame_host.ptr, rgba_host);
	if (tp) {
		if (history_len) copy_owned_tiles(m, c->n_tiles, 1u, len_host.data(), history_len);
		for (uint32_t s = 0; s < kTemporalStatSlots; s++) for (uint32_t k = 0; k < kTemporalClasses; k++) class_counts[k] += count_slots[s * kTemporalStatPitch + k];
		if (stats) *stats = mirt_temporal_stats{ class_counts[kTemporalReprojected], class_counts[kTemporalNoHistory], class_counts[kTemporalOutside], class_counts[kTemporalRejected], class_counts[kTemporalUnusable] };
		if (tp->update) {                                                             // step 4: the blend, this call's guides and the lengths ARE the history now; the old ones are scratch
			std::swap(c->hist.x, c->dn.cv[1]); std::swap(c->hist.g, c->dn.gd); std::swap(c->hist.n, c->hist.len);
			c->hist.cam = c->camera; c->hist.demodulate = p->demodulate; c->hist.albedo_floor = p->albedo_floor; c->hist.width = c->width; c->hist.height = c->height;
			if (c->history_motion) { std::swap(c->hist.id, c->hist.id_cur); c->hist.snap_valid = true; c->hist.snap_gen = gs->spheres_gen; }   // this call's id map IS the history's id plane now
			c->hist.valid = true;
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
	c->hist.drop();
	return MIRT_OK;
}
int mirt_history_info(const mirt_ctx* c, uint32_t* valid, uint64_t* bytes) {
	if (!c || !valid || !bytes) return MIRT_ERR_ARG;
	*valid = c->hist.valid ? 1u : 0u;
	*bytes = static_cast<uint64_t>(c->hist.x.bytes) + c->hist.g.bytes + c->hist.n.bytes + c->hist.id.bytes + c->hist.snap.bytes;   // the last two: mirt_set_sphere_motion(1) only
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
	HIP_TRY(c, c->hist.id_out.ensure(n * (sizeof(int32_t) + sizeof(float))));
	int32_t* prim_dev = c->hist.id_out.as<int32_t>();
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
	c->hist.drop();                                                                   // a history without an id plane cannot be taken with one, and the reverse
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
	c->hist.drop();                                                                   // ids of another scene
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
		HIP_TRY(c, c->noise.rec.ensure(rec.size() * sizeof(float)));
		HIP_TRY(c, c->noise.hist.ensure(MIRT_NOISE_BINS * sizeof(uint32_t)));
		if (above_out) HIP_TRY(c, c->noise.above.ensure(static_cast<size_t>(c->n_tiles) * sizeof(uint32_t)));
		const uint32_t* counts = nullptr;
		if ((r = upload_tile_counts(c, &counts))) return r;
		HIP_TRY(c, hipMemsetAsync(c->noise.hist.ptr, 0, MIRT_NOISE_BINS * sizeof(uint32_t), c->stream));
		{ Bracket t(c, MIRT_K_RESOLVE);
		  hipLaunchKernelGGL(k_noise, dim3(c->n_tiles), dim3(kTileSize), 0, c->stream, c->accumulator.as<float>(), map_out ? image.as<float>() : nullptr, c->noise.rec.as<float4>(),
		                     c->noise.hist.as<uint32_t>(), m, k, scale, floor, counts, c->camera.exposure, above_out ? c->noise.above.as<uint32_t>() : nullptr, target); }
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
		HIP_TRY(c, hipMemcpyAsync(rec.data(), c->noise.rec.ptr, rec.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(c, hipMemcpyAsync(hist.data(), c->noise.hist.ptr, MIRT_NOISE_BINS * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		if (above_out) HIP_TRY(c, hipMemcpyAsync(above_out, c->noise.above.ptr, static_cast<size_t>(c->n_tiles) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
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
		if (!freeze[t] || (c->freeze.n_frozen && c->freeze.frozen[t])) continue;
		if (c->freeze.frozen.empty()) { c->freeze.frozen.assign(c->n_tiles, 0); c->freeze.frozen_at.assign(c->n_tiles, 0u); }
		c->freeze.frozen[t] = 1; c->freeze.frozen_at[t] = c->accumulations; c->freeze.n_frozen++;
		changed = true;
	}
	return changed ? upload_freezes(c) : MIRT_OK;
}

int mirt_frozen_tiles(mirt_ctx* c, uint8_t* mask_out, size_t capacity) {
	if (!c) return MIRT_ERR_ARG;
	if (!mask_out && c->n_tiles) return fail(c, MIRT_ERR_ARG, "mask_out is NULL");
	if (capacity < c->n_tiles) return fail(c, MIRT_ERR_ARG, "frozen_tiles: room for %zu tiles, %u local tiles", capacity, c->n_tiles);
	for (uint32_t t = 0; t < c->n_tiles; t++) mask_out[t] = (c->freeze.n_frozen && c->freeze.frozen[t]) ? 1 : 0;
	return MIRT_OK;
}

int mirt_tile_counts(mirt_ctx* c, uint32_t* counts_out, size_t capacity) {
	if (!c) return MIRT_ERR_ARG;
	if (!counts_out) return fail(c, MIRT_ERR_ARG, "counts_out is NULL");
	if (capacity < c->n_tiles) return fail(c, MIRT_ERR_ARG, "tile_counts: room for %zu counts, %u local tiles", capacity, c->n_tiles);
	for (uint32_t t = 0; t < c->n_tiles; t++) counts_out[t] = (c->freeze.n_frozen && c->freeze.frozen[t]) ? c->freeze.frozen_at[t] : c->accumulations + c->deferred;
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
	c->freeze.drop();
	if (!any) return MIRT_OK;
	c->freeze.frozen.assign(c->n_tiles, 0); c->freeze.frozen_at.assign(c->n_tiles, 0u);
	for (uint32_t t = 0; t < c->n_tiles; t++) if (counts[t] < c->accumulations) { c->freeze.frozen[t] = 1; c->freeze.frozen_at[t] = counts[t]; c->freeze.n_frozen++; }
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

} // extern "C"
