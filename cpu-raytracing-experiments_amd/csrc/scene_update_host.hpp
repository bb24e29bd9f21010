// scene_update_host.hpp — the host half of mirt_update_spheres (include/mirt.h, "moving spheres in place"): the argument rules, checked
// before anything is changed, and the patch of the next-event-estimation light table.  Host-only code, no HIP:
// tests/native/scene_update_check.cpp compiles it on its own under sanitizers.
#pragma once
#include "../../include/mirt.h"
#include "bvh_layout.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace mirt_scene_update {

// binary16 records keep a sphere only while its leaf box is adequate: the rule mirt_set_scene's GPU-build branch applies per sphere.
inline bool half_adequate(const float s[4]) {
	const float rad = std::sqrt(s[3]);
	const float amax = std::fmax(std::fmax(std::fabs(s[0]), std::fabs(s[1])), std::fabs(s[2])) + rad * 1.0001f;
	return mirt_host::half_box_adequate(amax, 2.0f * rad, true);
}

// MIRT_OK, or the code of the first rule broken with its reason in `msg`.  n_spheres: of the scene in place; half_records: its records are
// binary16 (child-pair or 4-wide).  Nothing is written but `msg`.
inline int check(uint32_t n, const uint32_t* bvh_index, const uint32_t* geometry_index, const float* xyz_rsq, uint32_t n_spheres, bool half_records,
                 char* msg, size_t msg_bytes) {
	auto say = [&](int code, const char* fmt, auto... args) { if (msg && msg_bytes) std::snprintf(msg, msg_bytes, fmt, args...); return code; };
	if (n == 0) return MIRT_OK;
	if (!bvh_index || !geometry_index || !xyz_rsq) return say(MIRT_ERR_ARG, "update_spheres: bvh_index / geometry_index / xyz_rsq is NULL with n = %u", n);
	std::vector<uint8_t> seen(static_cast<size_t>(n_spheres), 0);          // bit 0: as a bvh_index, bit 1: as a geometry_index
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t b = bvh_index[i], g = geometry_index[i];
		if (b >= n_spheres) return say(MIRT_ERR_ARG, "update_spheres: bvh_index[%u] = %u, the scene has %u spheres", i, b, n_spheres);
		if (g >= n_spheres) return say(MIRT_ERR_ARG, "update_spheres: geometry_index[%u] = %u, the scene has %u spheres", i, g, n_spheres);
		if (seen[b] & 1u) return say(MIRT_ERR_ARG, "update_spheres: bvh_index %u occurs twice (second time at entry %u)", b, i);
		if (seen[g] & 2u) return say(MIRT_ERR_ARG, "update_spheres: geometry_index %u occurs twice (second time at entry %u)", g, i);
		seen[b] |= 1u; seen[g] |= 2u;
		const float* s = xyz_rsq + 4 * static_cast<size_t>(i);
		if (!std::isfinite(s[0]) || !std::isfinite(s[1]) || !std::isfinite(s[2]) || !std::isfinite(s[3]) || s[3] < 0.0f)
			return say(MIRT_ERR_ARG, "update_spheres: entry %u: position / radius_sq must be finite, radius_sq >= 0", i);
	}
	if (half_records)
		for (uint32_t i = 0; i < n; i++)
			if (!half_adequate(xyz_rsq + 4 * static_cast<size_t>(i)))
				return say(MIRT_ERR_STATE, "update_spheres: entry %u (bvh_index %u) does not fit the binary16 records of the tree in place (a coordinate beyond 60000, "
				           "or a diameter under 8 binary16 steps there); a refit keeps the layout: call mirt_set_scene with the edited scene", i, bvh_index[i]);
	return MIRT_OK;
}

// light_sphere[l] = the packet of every light l whose geometry id is edited (rows of 4 floats, as mirt_set_scene flattens them).  Returns
// the number of rows written.  The arguments have passed check().
inline uint32_t patch_lights(const int32_t* light_ids, uint32_t n_lights, uint32_t n, const uint32_t* geometry_index, const float* xyz_rsq, uint32_t n_spheres,
                             float* light_sphere) {
	if (n == 0 || n_lights == 0) return 0;
	uint32_t patched = 0;
	if (static_cast<uint64_t>(n) * n_lights <= 4096u) {                      // a drag: a handful of edits
		for (uint32_t l = 0; l < n_lights; l++)
			for (uint32_t i = 0; i < n; i++)
				if (static_cast<uint32_t>(light_ids[l]) == geometry_index[i]) { for (int k = 0; k < 4; k++) light_sphere[4 * static_cast<size_t>(l) + k] = xyz_rsq[4 * static_cast<size_t>(i) + k]; patched++; }
		return patched;
	}
	std::vector<uint32_t> entry_of(static_cast<size_t>(n_spheres), 0xffffffffu);
	for (uint32_t i = 0; i < n; i++) entry_of[geometry_index[i]] = i;
	for (uint32_t l = 0; l < n_lights; l++) {
		const uint32_t i = entry_of[static_cast<uint32_t>(light_ids[l])];
		if (i == 0xffffffffu) continue;
		for (int k = 0; k < 4; k++) light_sphere[4 * static_cast<size_t>(l) + k] = xyz_rsq[4 * static_cast<size_t>(i) + k];
		patched++;
	}
	return patched;
}

} // namespace mirt_scene_update
