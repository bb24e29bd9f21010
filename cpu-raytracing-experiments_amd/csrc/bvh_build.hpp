// bvh_build.hpp — internal entry point of csrc/bvh_build.cpp (the public ones are mirt_bvh_build / mirt_light_list in mirt.h).
#pragma once
#include "../../include/mirt.h"
#include <cstdint>
#include <vector>

namespace mirt_host {
// SAH sweep tree (true half-area cost, one prim per leaf) over `prims`; leaf node k with first_id = s refers to
// prims[prim_of_slot[s]].  Used for the GPU-internal traversal structure only.
void build_sah_tree(const mirt_sphere* prims, uint32_t n, std::vector<mirt_bvh_node>& nodes, std::vector<uint32_t>& prim_of_slot);

// A material with this emission makes its spheres lights: glm::dot(em, em) > 0 in binary32 (Scene.hpp:13-15).  The one statement of the rule,
// for mirt_light_list and for the per-material mask of mirt_update_materials.  An emission whose squares all underflow to 0 does not emit; a
// negative component emits (its square is positive); a NaN component does not (no comparison with a NaN holds).
inline bool emits(const float e[3]) {
	const float energy = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
	return energy > 0.0f;
}
}
