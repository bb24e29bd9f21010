// Stand-alone driver for the host-only part of the noise estimate (csrc/noise_host.cpp, mirt_noise_quantile), meant to be compiled together
// with it under -fsanitize=address,undefined (tests/test_noise_cpu.py).  The histograms are the crafted ones of that test; every answer is
// printed as the float's word so that the test can compare it with the numpy twin.
#include "../../include/mirt.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static void show(const char* label, const std::vector<uint32_t>& hist, double q) {
	float v = -1.0f;
	const int rc = mirt_noise_quantile(hist.data(), q, &v);
	uint32_t word; std::memcpy(&word, &v, sizeof word);
	std::printf("%s rc=%d word=%08x\n", label, rc, word);
}

int main() {
	std::vector<uint32_t> h(MIRT_NOISE_BINS, 0u);
	show("empty", h, 0.5);
	h[1000] = 7;
	show("single_q0.5", h, 0.5);
	show("single_q1", h, 1.0);
	show("bad_q0", h, 0.0);
	show("bad_q1.5", h, 1.5);
	h[1000] = 50; h[1010] = 50;
	show("two_q0.5", h, 0.5);                       // rank 50: still the lower bin
	show("two_q0.51", h, 0.51);                     // rank 51: the upper bin
	show("two_q1", h, 1.0);
	std::fill(h.begin(), h.end(), 0u);
	h[0] = 1; h[MIRT_NOISE_BINS - 1] = 1; h[0x7f7] = 1;
	show("ends_q0.01", h, 0.01);
	show("ends_q0.5", h, 0.5);                      // the last bin below infinity: its upper edge is +infinity
	show("ends_q1", h, 1.0);
	std::fill(h.begin(), h.end(), 0xffffffffu);    // 2048 x (2^32 - 1): the total needs 64 bits
	show("full_q0.5", h, 0.5);
	float v = 0.0f;
	std::printf("null rc=%d %d\n", mirt_noise_quantile(nullptr, 0.5, &v), mirt_noise_quantile(h.data(), 0.5, nullptr));
	std::printf("done\n");
	return 0;
}
