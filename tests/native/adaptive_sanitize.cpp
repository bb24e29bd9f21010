// Stand-alone program over csrc/noise_host.cpp: mirt_adaptive_select on the crafted cases of tests/test_adaptive_cpu.py, built with
// -fsanitize=address,undefined by test_adaptive_select_under_sanitizers.  Prints one line per case: "<label> rc=<status> <mask as 0/1 digits>".
#include "../../include/mirt.h"

#include <cstdint>
#include <cstdio>
#include <vector>

static void run(const char* label, const std::vector<float>& rec, const std::vector<uint32_t>& above, const std::vector<uint8_t>* frozen, double q) {
	const size_t n = above.size();
	std::vector<uint8_t> out(n, 7);
	const int rc = mirt_adaptive_select(rec.data(), above.data(), frozen ? frozen->data() : nullptr, n, q, out.data());
	std::printf("%s rc=%d ", label, rc);
	for (uint8_t v : out) std::printf("%u", static_cast<unsigned>(v));
	std::printf("\n");
}

int main() {
	// usable 0, 1, 255, 256 with `above` at, one below and one above the cut of each quantile
	const float usable[4] = { 0.0f, 1.0f, 255.0f, 256.0f };
	const double qs[3] = { 1.0, 0.95, static_cast<double>(0.95f) };
	const char* names[3] = { "q1", "q0.95", "q0.95f" };
	for (int qi = 0; qi < 3; qi++) {
		std::vector<float> rec; std::vector<uint32_t> above;
		for (float u : usable) {
			const uint32_t cut = static_cast<uint32_t>((1.0 - qs[qi]) * static_cast<double>(u));      // floor of a non-negative product
			for (int d = -1; d <= 1; d++) {
				if (d < 0 && cut == 0) continue;
				rec.insert(rec.end(), { 0.5f, 0.25f, u, 0.0f });
				above.push_back(cut + d);
			}
		}
		run(names[qi], rec, above, nullptr, qs[qi]);
	}
	{	// a non-finite pixel keeps a tile active; frozen tiles are passed through
		const std::vector<float> rec = { 0.1f, 0.1f, 255.0f, 1.0f,  0.1f, 0.1f, 256.0f, 0.0f,  9.0f, 9.0f, 256.0f, 0.0f,  9.0f, 9.0f, 200.0f, 56.0f };
		const std::vector<uint32_t> above = { 0, 0, 256, 200 };
		const std::vector<uint8_t> frozen = { 0, 0, 1, 1 };
		run("nonfinite", rec, above, nullptr, 0.95);
		run("frozen", rec, above, &frozen, 0.95);
		run("bad_q0", rec, above, nullptr, 0.0);
		run("bad_q1.5", rec, above, nullptr, 1.5);
	}
	std::printf("null rc=%d\n", mirt_adaptive_select(nullptr, nullptr, nullptr, 3, 0.5, nullptr));
	std::printf("empty rc=%d\n", mirt_adaptive_select(nullptr, nullptr, nullptr, 0, 0.5, nullptr));
	std::printf("done\n");
	return 0;
}
