// noise_host.hpp — the host arithmetic of the noise estimate (include/mirt.h, "per-pixel noise estimate"), shared by the single-context
// entry points (mirt_resolve.hip) and their group twins (mirt_group.hip) so that both form the same sums in the same order.  Host-only code.
#pragma once
#include "../../include/mirt.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace mirt_noise_host {

// mirt_noise_stats from tile records {max, mean over the usable pixels, usable count, unusable count} in ascending tile order: counts add as
// integers, the maximum is exact, and the mean is ONE double sum of mean[t] * count[t] over t = 0, 1, 2, ... divided by the total count.
// A group hands over its records in LaunchIndex order — the order a single context that owns the whole image keeps them in.
inline void stats_from_tiles(const float* rec, size_t n_tiles, mirt_noise_stats* st) {
	std::memset(st, 0, sizeof *st);
	st->owned_pixels = static_cast<uint64_t>(n_tiles) * MIRT_TILE_SIZE;
	double sum = 0.0;
	for (size_t t = 0; t < n_tiles; t++) {
		const float* r = rec + t * 4;
		st->finite_pixels += static_cast<uint64_t>(r[2]);
		st->nonfinite_pixels += static_cast<uint64_t>(r[3]);
		if (r[0] > st->max) st->max = r[0];
		sum += static_cast<double>(r[1]) * static_cast<double>(r[2]);
	}
	st->mean = st->finite_pixels ? sum / static_cast<double>(st->finite_pixels) : 0.0;
}

inline bool finite_nonneg(float v) { return std::isfinite(v) && v >= 0.0f; }

// Argument and state rules of mirt_noise / mirt_group_noise and of the two accumulate_until entry points, in the order mirt.h states them:
// MIRT_OK, or the error code with its text in msg (the caller hands both to its own fail()).  One copy for the context and the group.
inline int check_noise_args(float floor, uint32_t buckets, char* msg, size_t n) {
	if (!finite_nonneg(floor)) { std::snprintf(msg, n, "floor %g is not a finite value >= 0", static_cast<double>(floor)); return MIRT_ERR_ARG; }
	if (buckets < 2) { std::snprintf(msg, n, "the noise estimate is the spread of the bucket means: it needs policy.buckets >= 2 (it is %u)", buckets); return MIRT_ERR_STATE; }
	return MIRT_OK;
}
inline int check_stop_rule(const mirt_stop_rule* rule, uint32_t buckets, uint32_t accumulations, char* msg, size_t n) {
	if (!rule) { std::snprintf(msg, n, "rule is NULL"); return MIRT_ERR_ARG; }
	if (buckets < 2) { std::snprintf(msg, n, "the noise estimate is the spread of the bucket means: it needs policy.buckets >= 2 (it is %u)", buckets); return MIRT_ERR_STATE; }
	if (rule->check_every == 0 || rule->check_every % buckets != 0) { std::snprintf(msg, n, "check_every %u is not a positive multiple of buckets (%u)", rule->check_every, buckets); return MIRT_ERR_ARG; }
	if (!finite_nonneg(rule->target) || !finite_nonneg(rule->floor)) { std::snprintf(msg, n, "target and floor must be finite and >= 0"); return MIRT_ERR_ARG; }
	if (!(rule->quantile > 0.0f) || !(rule->quantile <= 1.0f)) { std::snprintf(msg, n, "quantile %g is not in (0, 1]", static_cast<double>(rule->quantile)); return MIRT_ERR_ARG; }
	if (accumulations % buckets != 0) { std::snprintf(msg, n, "%u accumulations so far: not a multiple of buckets (%u)", accumulations, buckets); return MIRT_ERR_STATE; }
	return MIRT_OK;
}

// The loop of mirt_accumulate_until / mirt_group_accumulate_until over a renderer given as three calls:
//   accumulations(uint32_t*)            issued so far
//   accumulate(uint32_t n)              n plain synchronous accumulations
//   noise(float floor, uint32_t* hist, mirt_noise_stats*)
// each returning a mirt status, and report(code, text), the caller's fail().  `buckets` is the policy's.  Negative statuses of the calls are
// returned as they are (the call has set its own error text).
template <class Accumulations, class Accumulate, class Noise, class Report>
int accumulate_until(const mirt_stop_rule* rule, uint32_t buckets, Accumulations accumulations, Accumulate accumulate, Noise noise, Report report,
                     mirt_noise_stats* last, uint32_t* issued, uint32_t* hist /* MIRT_NOISE_BINS words of scratch */) {
	if (last) std::memset(last, 0, sizeof *last);
	if (issued) *issued = 0;
	uint32_t total = 0;
	for (;;) {
		uint32_t acc = 0;
		int rc = accumulations(&acc);
		if (rc < 0) return rc;
		const uint32_t room = rule->max_accumulations > acc ? rule->max_accumulations - acc : 0u;
		const uint32_t step = room < rule->check_every ? room - room % buckets : rule->check_every;
		if (step == 0) return MIRT_NOT_CONVERGED;
		if ((rc = accumulate(step)) < 0) return rc;
		total += step;
		if (issued) *issued = total;
		mirt_noise_stats st;
		if ((rc = noise(rule->floor, hist, &st)) < 0) return rc;
		if (rc != MIRT_OK) return report(MIRT_ERR_STATE, "the noise estimate was not ready after a whole number of bucket rounds: the accumulation count was changed during the loop");
		if (last) *last = st;
		if (st.nonfinite_pixels) continue;
		if (st.finite_pixels == 0) return MIRT_OK;                              // nothing owned: nothing to wait for
		float q = 0.0f;
		if (mirt_noise_quantile(hist, static_cast<double>(rule->quantile), &q) == MIRT_OK && q <= rule->target) return MIRT_OK;
	}
}

// The loop of mirt_accumulate_adaptive / mirt_group_accumulate_adaptive over a renderer given as calls, each returning a mirt status:
//   accumulations(uint32_t*), accumulate(uint32_t n)                       as above
//   check(float floor, float target, float* rec, uint32_t* above, mirt_noise_stats*)   tile records and counts above the target, n_tiles each
//   frozen(uint8_t* mask)                                                   the current mask, n_tiles bytes
//   freeze(const uint8_t* mask), counts(uint32_t*)                          mirt_freeze_tiles, mirt_tile_counts
// Nothing freezes before min_accumulations.  MIRT_OK when every tile is frozen, MIRT_NOT_CONVERGED at max_accumulations.
template <class Accumulations, class Accumulate, class Check, class Frozen, class Freeze, class Counts, class Report>
int accumulate_adaptive(const mirt_stop_rule* rule, uint32_t buckets, uint32_t min_accumulations, size_t n_tiles, Accumulations accumulations, Accumulate accumulate, Check check,
                        Frozen frozen, Freeze freeze, Counts counts, Report report, mirt_adaptive_report* out) {
	mirt_adaptive_report rep;
	std::memset(&rep, 0, sizeof rep);
	float* rec = new float[n_tiles * 4 + 1];
	uint32_t* above = new uint32_t[n_tiles + 1];
	uint8_t* mask = new uint8_t[n_tiles * 2 + 1];
	uint8_t* next = mask + n_tiles;
	int status = MIRT_OK, rc = MIRT_OK;
	for (;;) {
		if ((rc = frozen(mask)) < 0) break;
		size_t n_frozen = 0;
		for (size_t t = 0; t < n_tiles; t++) n_frozen += mask[t] ? 1u : 0u;
		rep.frozen_tiles = static_cast<uint32_t>(n_frozen);
		if (n_frozen == n_tiles) { status = MIRT_OK; break; }                     // every owned tile is frozen (or none is owned)
		uint32_t acc = 0;
		if ((rc = accumulations(&acc)) < 0) break;
		const uint32_t room = rule->max_accumulations > acc ? rule->max_accumulations - acc : 0u;
		const uint32_t step = room < rule->check_every ? room - room % buckets : rule->check_every;   // the last step is shortened, as in accumulate_until
		if (step == 0) { status = MIRT_NOT_CONVERGED; break; }
		if ((rc = accumulate(step)) < 0) break;
		rep.issued += step;
		if ((rc = check(rule->floor, rule->target, rec, above, &rep.last)) < 0) break;
		if (rc != MIRT_OK) { rc = report(MIRT_ERR_STATE, "the noise estimate was not ready after a whole number of bucket rounds: the accumulation count was changed during the loop"); break; }
		rep.checks++;
		if (acc + step < min_accumulations) continue;                             // the guard against stopping on an early, lucky estimate
		if ((rc = mirt_adaptive_select(rec, above, mask, n_tiles, static_cast<double>(rule->quantile), next)) < 0) { rc = report(rc, "adaptive_select refused its arguments"); break; }
		if ((rc = freeze(next)) < 0) break;
	}
	if (rc >= 0) {
		uint32_t* c = above;                                                      // (scratch: the counts)
		rc = counts(c);
		rep.owned_tiles = static_cast<uint32_t>(n_tiles);
		for (size_t t = 0; rc >= 0 && t < n_tiles; t++) rep.tile_accumulations += c[t];
	}
	delete[] rec; delete[] above; delete[] mask;
	if (rc < 0) return rc;
	if (out) *out = rep;
	return status;
}

} // namespace mirt_noise_host
