// noise_host.cpp — mirt_noise_quantile and mirt_adaptive_select (include/mirt.h): pure host code, no context and no GPU.  Compiled into libmirt.so, and on its own
// into the sanitizer program of tests/native/noise_sanitize.cpp.
#include "../../include/mirt.h"

#include <cmath>
#include <cstring>

extern "C" int mirt_noise_quantile(const uint32_t* hist, double q, float* value) {
	if (!hist || !value || !(q > 0.0) || !(q <= 1.0)) return MIRT_ERR_ARG;   // (!(q > 0) also refuses NaN)
	uint64_t total = 0;
	for (uint32_t b = 0; b < MIRT_NOISE_BINS; b++) total += hist[b];
	if (total == 0) return MIRT_NOT_READY;
	// rank of the quantile among the sorted values, 1-based: the smallest integer >= q * total (the double product as it rounds), at least 1
	const double want = std::ceil(q * static_cast<double>(total));
	uint64_t rank = want < 1.0 ? 1u : static_cast<uint64_t>(want);
	if (rank > total) rank = total;
	uint64_t seen = 0;
	uint32_t bin = 0;
	for (; bin < MIRT_NOISE_BINS; bin++) { seen += hist[bin]; if (seen >= rank) break; }
	// upper edge of bin b = the value whose word is (b + 1) << 20; from bin 0x7f7 (the last below infinity) upwards that is +infinity
	const uint32_t word = bin >= 0x7f7u ? 0x7f800000u : (bin + 1u) << 20;
	std::memcpy(value, &word, sizeof word);
	return MIRT_OK;
}

// The freeze rule of the adaptive loop, tile by tile (mirt.h "per-tile adaptive sampling").
extern "C" int mirt_adaptive_select(const float* tile_records, const uint32_t* above, const uint8_t* frozen, size_t n_tiles, double quantile, uint8_t* freeze_out) {
	if (!(quantile > 0.0) || !(quantile <= 1.0)) return MIRT_ERR_ARG;              // (!(q > 0) also refuses NaN)
	if (n_tiles && (!tile_records || !above || !freeze_out)) return MIRT_ERR_ARG;
	for (size_t t = 0; t < n_tiles; t++) {
		if (frozen && frozen[t]) { freeze_out[t] = 1; continue; }
		const double usable = static_cast<double>(tile_records[t * 4 + 2]);
		const bool nonfinite = tile_records[t * 4 + 3] != 0.0f;
		const uint32_t cut = static_cast<uint32_t>(std::floor((1.0 - quantile) * usable));      // usable <= 256: the product fits with room to spare
		freeze_out[t] = (!nonfinite && above[t] <= cut) ? 1 : 0;
	}
	return MIRT_OK;
}
