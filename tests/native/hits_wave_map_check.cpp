// Stand-alone check of k_primary_hits_wave's staging map (csrc/hits_wave_map.hpp), meant to be compiled under -fsanitize=address,undefined
// (tests/test_primary_hits_wave.py).  It plays a wave's two phases on heap arrays of the kernel's sizes: every lane stages its slot's record of
// every pixel of the run, then the lanes, remapped, store the records to hit_out[slot][pixel].  Every record of the batch must arrive exactly
// once, a slot's 16 records in 16 neighbouring lanes and words, and nothing may be read before it was staged or touched out of bounds.
#include "../../cpu-raytracing-experiments_amd/csrc/hits_wave_map.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace mirt;

static int fail(const char* what, uint32_t batch_n, uint32_t a, uint32_t b) { std::printf("FAIL batch %u: %s (%u, %u)\n", batch_n, what, a, b); return 1; }

static int check(uint32_t batch_n, uint32_t n_pix, uint32_t base) {
	std::vector<uint64_t> hit_out(static_cast<size_t>(batch_n) * n_pix, ~0ull);
	std::vector<uint32_t> stores(hit_out.size(), 0u);
	const uint32_t n_groups = hits_wave_groups(batch_n);
	if (static_cast<uint64_t>(n_groups) * 64u < batch_n || (n_groups - 1u) * 64u >= batch_n) return fail("groups", batch_n, n_groups, 0);
	for (uint32_t g = 0; g < n_groups; g++) {
		std::vector<uint64_t> stage(kWaveHitsStage, ~0ull);
		std::vector<uint32_t> staged(kWaveHitsStage, 0u);
		for (uint32_t p = 0; p < kWaveHitsRun; p++) {                 // phase 1: lane = slot of the group (lanes beyond batch_n stage a record nobody stores)
			bool pair_used[16] = {};
			for (uint32_t lane = 0; lane < 64; lane++) {
				const uint32_t i = hits_wave_stage_index(p, lane);
				if (i >= kWaveHitsStage) return fail("stage index out of range", batch_n, p, lane);
				if (staged.at(i)++) return fail("two lanes stage into one cell", batch_n, p, lane);
				stage.at(i) = (static_cast<uint64_t>(g * 64u + lane) << 32) | (base + p);
				if (lane < 16) { if (pair_used[i & 15u]) return fail("write: two of 16 neighbouring lanes on one bank pair", batch_n, p, lane); pair_used[i & 15u] = true; }
			}
		}
		const uint32_t n_slots = hits_wave_group_slots(batch_n, g);
		if (n_slots == 0 || n_slots > 64 || g * 64u + n_slots > batch_n || (g + 1 == n_groups && g * 64u + n_slots != batch_n)) return fail("group slots", batch_n, g, n_slots);
		for (uint32_t pass = 0; pass < kWaveHitsPasses; pass++) {        // phase 2
			for (uint32_t lane = 0; lane < 64; lane++) {
				const uint32_t p = hits_wave_out_pixel(lane), s = hits_wave_out_slot(lane, pass);
				if (p >= kWaveHitsRun || s >= 64) return fail("remap out of range", batch_n, lane, pass);
				if ((lane & 15u) != 0 && (hits_wave_out_slot(lane - 1, pass) != s || hits_wave_out_pixel(lane - 1) + 1 != p)) return fail("a slot's records are not in neighbouring lanes", batch_n, lane, pass);
				if ((lane & 15u) != 0 && (hits_wave_stage_index(p, s) & 15u) == (hits_wave_stage_index(hits_wave_out_pixel(lane & ~15u), s) & 15u)) return fail("read: bank pair of the segment's first lane again", batch_n, lane, pass);
				if (s >= n_slots) continue;
				const uint32_t i = hits_wave_stage_index(p, s);
				if (!staged.at(i)) return fail("read of a cell nobody staged", batch_n, lane, pass);
				const size_t o = static_cast<size_t>(g * 64u + s) * n_pix + base + p;
				if (stores.at(o)++) return fail("record stored twice", batch_n, g * 64u + s, p);
				hit_out.at(o) = stage.at(i);
			}
		}
	}
	for (uint32_t slot = 0; slot < batch_n; slot++)
		for (uint32_t pix = 0; pix < n_pix; pix++) {
			const size_t o = static_cast<size_t>(slot) * n_pix + pix;
			const bool in_run = pix >= base && pix < base + kWaveHitsRun;
			if (stores[o] != (in_run ? 1u : 0u)) return fail("store count", batch_n, slot, pix);
			if (in_run && hit_out[o] != ((static_cast<uint64_t>(slot) << 32) | pix)) return fail("record of another (slot, pixel)", batch_n, slot, pix);
		}
	return 0;
}

int main() {
	static_assert(kWaveHitsMinBatch == 32 && kWaveHitsRun == 16 && kWaveHitsStage * 8u == 8192u, "the figures DESIGN.md states");
	int bad = 0;
	for (uint32_t batch_n : { 32u, 33u, 63u, 64u, 65u, 128u, 192u, 256u })
		for (uint32_t base : { 0u, 16u, 240u }) bad += check(batch_n, 256u, base);
	std::printf(bad ? "hits_wave_map: %d failures\n" : "hits_wave_map ok\n", bad);
	return bad ? 1 : 0;
}
