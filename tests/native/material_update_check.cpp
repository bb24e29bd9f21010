// material_update_check.cpp — csrc/scene_update_host.hpp (the argument rules of mirt_update_materials, the glass rule and the per-material emit
// mask) with its own main, for a build under -fsanitize=address,undefined on the CPU.  Without arguments: one line per case of the argument
// rules.  With arguments: each is the hexadecimal bit pattern of one binary32 emission component, three per material; prints the emit mask.
// tests/test_update_materials_cpu.py reads both.
#include "../../cpu-raytracing-experiments_amd/csrc/scene_update_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

namespace su = mirt_scene_update;

namespace {
constexpr uint32_t kSpheres = 5, kMaterials = 4;
// the scene in place: material 2 is glass (transmission 0.5, index 1.5), the others are opaque with IOR_minus_one = 0
const float kGlass[4 * kMaterials] = { 0, 0, 0, 1,  0, 0, 0, 1,  0.5f, 0.5f, 0.5f, 1.5f,  0, 0, 0, 1 };

mirt_material material(float t0 = 0.0f, float t1 = 0.0f, float t2 = 0.0f, float ior_minus_one = 0.0f) {
	mirt_material m{};
	m.transmission[0] = t0; m.transmission[1] = t1; m.transmission[2] = t2; m.IOR_minus_one = ior_minus_one;
	return m;
}

void check_case(const char* label, uint32_t n_rows, const uint32_t* mi, const mirt_material* rows, uint32_t n_assign, const uint32_t* b, const uint32_t* g,
                const int32_t* ids, bool transmission, uint32_t n_spheres = kSpheres) {
	char msg[320] = "";
	const int rc = su::check_materials(n_rows, mi, rows, n_assign, b, g, ids, n_spheres, kMaterials, transmission, kGlass, msg, sizeof msg);
	std::printf("%s rc=%d %s\n", label, rc, msg);
}
} // namespace

int main(int argc, char** argv) {
	if (argc > 1) {
		std::vector<float> rows;
		for (int i = 1; i + 2 < argc; i += 3) {
			for (int k = 0; k < 3; k++) { const uint32_t w = static_cast<uint32_t>(std::strtoul(argv[i + k], nullptr, 16)); float f; std::memcpy(&f, &w, 4); rows.push_back(f); }
			rows.push_back(0.0f);
		}
		std::printf("mask=%llx\n", static_cast<unsigned long long>(su::emit_mask(rows.data(), static_cast<uint32_t>(rows.size() / 4))));
		return 0;
	}
	const uint32_t mi[2] = { 3, 0 }, b[3] = { 0, 2, 1 }, g[3] = { 2, 0, 4 };
	const int32_t ids[3] = { 3, 0, 1 };
	const mirt_material rows[2] = { material(), material() };
	const float nan = std::numeric_limits<float>::quiet_NaN();
	check_case("ok", 2, mi, rows, 3, b, g, ids, false);
	check_case("ok_rows_only", 2, mi, rows, 0, nullptr, nullptr, nullptr, true);
	check_case("ok_assign_only", 0, nullptr, nullptr, 3, b, g, ids, true);
	check_case("empty", 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, true);
	check_case("null_material_index", 1, nullptr, rows, 0, nullptr, nullptr, nullptr, false);
	check_case("null_rows", 1, mi, nullptr, 0, nullptr, nullptr, nullptr, false);
	check_case("null_bvh", 0, nullptr, nullptr, 1, nullptr, g, ids, false);
	check_case("null_geometry", 0, nullptr, nullptr, 1, b, nullptr, ids, false);
	check_case("null_ids", 0, nullptr, nullptr, 1, b, g, nullptr, false);
	{ const uint32_t m[2] = { 3, 4 }; check_case("material_range", 2, m, rows, 0, nullptr, nullptr, nullptr, false); }
	{ const uint32_t m[2] = { 1, 1 }; check_case("material_twice", 2, m, rows, 0, nullptr, nullptr, nullptr, false); }
	{ const uint32_t x[2] = { 0, 5 }; check_case("bvh_range", 0, nullptr, nullptr, 2, x, g, ids, false); }
	{ const uint32_t x[2] = { 0, 0xffffffffu }; check_case("geometry_range", 0, nullptr, nullptr, 2, b, x, ids, false); }
	{ const uint32_t x[3] = { 1, 2, 1 }; check_case("bvh_twice", 0, nullptr, nullptr, 3, x, g, ids, false); }
	{ const uint32_t x[3] = { 1, 2, 2 }; check_case("geometry_twice", 0, nullptr, nullptr, 3, b, x, ids, false); }
	{ const int32_t x[3] = { 3, 4, 1 }; check_case("id_range", 0, nullptr, nullptr, 3, b, g, x, false); }
	{ const int32_t x[3] = { 3, -1, 1 }; check_case("id_negative", 0, nullptr, nullptr, 3, b, g, x, false); }
	check_case("no_spheres_rows", 2, mi, rows, 0, nullptr, nullptr, nullptr, false, 0);              // the gather context of a group: materials, no geometry
	check_case("no_spheres_assign", 0, nullptr, nullptr, 1, b, g, ids, false, 0);
	// a bad half refuses the whole call, whichever half it is
	{ const int32_t x[3] = { 3, 9, 1 }; check_case("good_rows_bad_assign", 2, mi, rows, 3, b, g, x, false); }
	// the glass rule is asked of the RESULTING table, and only with the switch on
	{ const mirt_material r[1] = { material(1.5f) }; const uint32_t m[1] = { 1 };
	  check_case("transmission_range_on", 1, m, r, 0, nullptr, nullptr, nullptr, true); check_case("transmission_range_off", 1, m, r, 0, nullptr, nullptr, nullptr, false); }
	{ const mirt_material r[1] = { material(nan) }; const uint32_t m[1] = { 1 }; check_case("transmission_nan_on", 1, m, r, 0, nullptr, nullptr, nullptr, true); }
	{ const mirt_material r[1] = { material(0.5f, 0, 0, -1.0f) }; const uint32_t m[1] = { 1 };
	  check_case("ior_on", 1, m, r, 0, nullptr, nullptr, nullptr, true); check_case("ior_off", 1, m, r, 0, nullptr, nullptr, nullptr, false); }
	{ const mirt_material r[1] = { material(0.5f, 0, 0, nan) }; const uint32_t m[1] = { 1 }; check_case("ior_nan_on", 1, m, r, 0, nullptr, nullptr, nullptr, true); }
	{ const mirt_material r[1] = { material(0, 0, 0, -1.0f) }; const uint32_t m[1] = { 1 }; check_case("ior_of_an_opaque_row_on", 1, m, r, 0, nullptr, nullptr, nullptr, true); }
	{ const mirt_material r[1] = { material(0.9f, 0.8f, 0.7f, 0.33f) }; const uint32_t m[1] = { 1 }; check_case("new_glass_on", 1, m, r, 0, nullptr, nullptr, nullptr, true); }
	{ const mirt_material r[1] = { material() }; const uint32_t m[1] = { 2 }; check_case("glass_removed_on", 1, m, r, 0, nullptr, nullptr, nullptr, true); }
	// the rows of the table in place are not asked again by an edit that leaves them alone
	check_case("assign_only_on", 0, nullptr, nullptr, 3, b, g, ids, true);
	{ char msg[256] = ""; const float bad[4] = { 0.5f, 0, 0, 0.0f }; std::printf("glass_rows rc=%d", su::check_glass_rows(bad, 1, msg, sizeof msg)); std::printf(" %s\n", msg); }
	std::printf("done\n");
	return 0;
}
