// scene_update_host.hpp — the host half of mirt_update_spheres (include/mirt.h, "moving spheres in place") and of mirt_update_materials
// ("updating materials in place"): the argument rules, checked before anything is changed, the patch of the next-event-estimation light
// table, the glass rule and the per-material emit mask.  Host-only code, no HIP: tests/native/scene_update_check.cpp and
// tests/native/material_update_check.cpp compile it on their own under sanitizers.
#pragma once
#include "../../include/mirt.h"
#include "bvh_build.hpp"
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

// ---- mirt_update_materials ------------------------------------------------------------------------------------------------------------
// What mirt_set_transmission(1) asks of the materials: rows {transmission.rgb, 1 + IOR_minus_one}.  A transmissive material
// (max(transmission) > 0) needs a finite index above 0.  MIRT_OK, or MIRT_ERR_ARG with the reason in `msg`.
inline int check_glass_rows(const float* rows, size_t n, char* msg, size_t msg_bytes) {
	auto say = [&](const char* fmt, auto... args) { if (msg && msg_bytes) std::snprintf(msg, msg_bytes, fmt, args...); return MIRT_ERR_ARG; };
	for (size_t i = 0; i < n; i++) {
		const float* t = rows + 4 * i;
		for (int k = 0; k < 3; k++)
			if (!(t[k] >= 0.0f && t[k] <= 1.0f)) return say("material %zu: transmission[%d] = %g is not in [0, 1] (mirt_set_transmission is on)", i, k, static_cast<double>(t[k]));
		const bool transmissive = t[0] > 0.0f || t[1] > 0.0f || t[2] > 0.0f;
		if (transmissive && !(std::isfinite(t[3]) && t[3] > 0.0f))
			return say("material %zu is transmissive and its IOR_minus_one = %g is not a finite value above -1 (mirt_set_transmission is on)", i, static_cast<double>(t[3]) - 1.0);
	}
	return MIRT_OK;
}

// Bit m: the spheres of material m are lights (bvh_build.hpp emits(), the expression of mirt_light_list).  rows: {emission.rgb, .} per material, at most 64.
inline uint64_t emit_mask(const float* emission_rows, uint32_t n_materials) {
	uint64_t mask = 0;
	for (uint32_t m = 0; m < n_materials && m < 64u; m++) if (mirt_host::emits(emission_rows + 4 * static_cast<size_t>(m))) mask |= 1ull << m;
	return mask;
}

// MIRT_OK, or MIRT_ERR_ARG for the first rule of mirt_update_materials broken, with its reason in `msg`.  n_spheres, n_materials: of the scene
// in place; glass_rows: its {transmission.rgb, 1 + IOR_minus_one} rows, asked about — after the edit — only with `transmission` on.  Nothing
// is written but `msg`.
inline int check_materials(uint32_t n_rows, const uint32_t* material_index, const mirt_material* rows, uint32_t n_assign, const uint32_t* bvh_index,
                           const uint32_t* geometry_index, const int32_t* material_id, uint32_t n_spheres, uint32_t n_materials, bool transmission,
                           const float* glass_rows, char* msg, size_t msg_bytes) {
	auto say = [&](const char* fmt, auto... args) { if (msg && msg_bytes) std::snprintf(msg, msg_bytes, fmt, args...); return MIRT_ERR_ARG; };
	if (n_rows && (!material_index || !rows)) return say("update_materials: material_index / rows is NULL with n_rows = %u", n_rows);
	if (n_assign && (!bvh_index || !geometry_index || !material_id)) return say("update_materials: bvh_index / geometry_index / material_ID is NULL with n_assign = %u", n_assign);
	std::vector<uint8_t> row_seen(static_cast<size_t>(n_materials), 0);
	for (uint32_t i = 0; i < n_rows; i++) {
		const uint32_t m = material_index[i];
		if (m >= n_materials) return say("update_materials: material_index[%u] = %u, the scene has %u materials (their number cannot change)", i, m, n_materials);
		if (row_seen[m]) return say("update_materials: material_index %u occurs twice (second time at entry %u)", m, i);
		row_seen[m] = 1;
	}
	if (n_assign) {
		std::vector<uint8_t> seen(static_cast<size_t>(n_spheres), 0);          // bit 0: as a bvh_index, bit 1: as a geometry_index
		for (uint32_t i = 0; i < n_assign; i++) {
			const uint32_t b = bvh_index[i], g = geometry_index[i];
			if (b >= n_spheres) return say("update_materials: bvh_index[%u] = %u, the scene has %u spheres", i, b, n_spheres);
			if (g >= n_spheres) return say("update_materials: geometry_index[%u] = %u, the scene has %u spheres", i, g, n_spheres);
			if (seen[b] & 1u) return say("update_materials: bvh_index %u occurs twice (second time at entry %u)", b, i);
			if (seen[g] & 2u) return say("update_materials: geometry_index %u occurs twice (second time at entry %u)", g, i);
			seen[b] |= 1u; seen[g] |= 2u;
			if (material_id[i] < 0 || static_cast<uint32_t>(material_id[i]) >= n_materials)
				return say("update_materials: material_ID[%u] = %d, the scene has %u materials", i, material_id[i], n_materials);
		}
	}
	if (transmission && n_rows) {
		std::vector<float> after(glass_rows, glass_rows + 4 * static_cast<size_t>(n_materials));
		for (uint32_t i = 0; i < n_rows; i++) {
			float* g = &after[4 * static_cast<size_t>(material_index[i])];
			for (int k = 0; k < 3; k++) g[k] = rows[i].transmission[k];
			g[3] = 1.0f + rows[i].IOR_minus_one;
		}
		if (check_glass_rows(after.data(), n_materials, msg, msg_bytes)) return MIRT_ERR_ARG;
	}
	return MIRT_OK;
}

} // namespace mirt_scene_update
