// sun_sky_host.hpp — the host half of mirt_set_sun_sky (include/mirt.h, "analytic sun and sky"): the defaults, the argument rules and everything
// that depends on the sun alone, computed once in float64 and rounded to binary32 for k_sun_sky (sun_sky.hpp).  Host-only code, no HIP:
// tests/native/sun_sky_check.cpp compiles it on its own under sanitizers.
#pragma once
#include "../../include/mirt.h"

#include <cmath>
#include <cstdint>
#include <cstdio>

namespace mirt_sun_sky {

constexpr uint32_t kMaxSide = 32768u;      // width and height of a baked map: the texel index stays below 2^30

// What k_sun_sky is launched with: plain binary32 words, each the float64 value rounded once.
struct Args {
	float perez[3][5];     // A, B, C, D, E of Y, x, y
	float inv_f0[3];       // 1 / F(0, theta_s) of Y, x, y
	float zenith[3];       // Y_z (kcd/m^2), x_z, y_z
	float sun[3];          // towards the sun, unit length
	float sun_rgb[3];      // sun_scale * 1.9e6 * exp(-tau_rgb m)
	float ramp_edge;       // 1 - cos(alpha) = 2 sin^2(alpha / 2)
	float ramp_inv;        // 1 / (cos(0.9 alpha) - cos(alpha))
	float sky_scale;
	float ground[3];
	uint32_t w, h;
};

// Starting values and design choices, not measurements: a high sun a little off the zenith, a clear sky, the sun's mean angular radius, one render
// unit per 10 kcd/m^2 for sky and disc alike, a dark ground, 1024 x 512 cells.
inline int defaults(mirt_sun_sky_params* p) {
	if (!p) return MIRT_ERR_ARG;
	p->sun_dir[0] = 0.3f; p->sun_dir[1] = 0.9f; p->sun_dir[2] = 0.3f;
	p->turbidity = 3.0f;
	p->sun_radius = 0.00465f;
	p->sky_scale = 0.1f;
	p->sun_scale = 0.1f;
	p->ground[0] = p->ground[1] = p->ground[2] = 0.1f;
	p->width = 1025u; p->height = 513u;
	return MIRT_OK;
}

// MIRT_OK, or MIRT_ERR_ARG with its text in msg (the caller hands both to its own fail()).
inline int check(const mirt_sun_sky_params* p, char* msg, size_t n) {
	if (!p) { std::snprintf(msg, n, "params is NULL"); return MIRT_ERR_ARG; }
	const float fields[] = { p->sun_dir[0], p->sun_dir[1], p->sun_dir[2], p->turbidity, p->sun_radius, p->sky_scale, p->sun_scale, p->ground[0], p->ground[1], p->ground[2] };
	for (float v : fields) if (!std::isfinite(v)) { std::snprintf(msg, n, "sun and sky: a field is not finite"); return MIRT_ERR_ARG; }
	const double x = p->sun_dir[0], y = p->sun_dir[1], z = p->sun_dir[2];
	if (!((x * x + y * y) + z * z > 0.0)) { std::snprintf(msg, n, "sun_dir has no length"); return MIRT_ERR_ARG; }
	if (y < 0.0) { std::snprintf(msg, n, "sun_dir.y = %g: a sun below the horizon (twilight) is not modelled", y); return MIRT_ERR_ARG; }
	if (!(p->turbidity >= 2.0f && p->turbidity <= 10.0f)) { std::snprintf(msg, n, "turbidity %g is outside [2, 10]", static_cast<double>(p->turbidity)); return MIRT_ERR_ARG; }
	if (!(p->sun_radius > 0.0f && p->sun_radius <= 0.1f)) { std::snprintf(msg, n, "sun_radius %g is outside (0, 0.1] rad", static_cast<double>(p->sun_radius)); return MIRT_ERR_ARG; }
	if (p->sky_scale < 0.0f || p->sun_scale < 0.0f) { std::snprintf(msg, n, "sky_scale %g / sun_scale %g: a scale is negative", static_cast<double>(p->sky_scale), static_cast<double>(p->sun_scale)); return MIRT_ERR_ARG; }
	if (p->width < 2u || p->height < 2u || p->width > kMaxSide || p->height > kMaxSide) {
		std::snprintf(msg, n, "a baked map of %u x %u texels: each side must be in [2, %u]", p->width, p->height, kMaxSide); return MIRT_ERR_ARG;
	}
	return MIRT_OK;
}

inline double perez(const double c[5], double cos_theta, double gamma) {
	const double cg = std::cos(gamma);
	return (1.0 + c[0] * std::exp(c[1] / cos_theta)) * (1.0 + c[2] * std::exp(c[3] * gamma) + c[4] * cg * cg);
}

// Preetham, Shirley, Smits 1999 (appendix), as include/mirt.h lists the digits; `p` has passed check().
inline Args args(const mirt_sun_sky_params& p) {
	const double pi = 3.14159265358979323846;
	const double T = p.turbidity;
	double s[3] = { p.sun_dir[0], p.sun_dir[1], p.sun_dir[2] };
	const double len = std::sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
	for (double& v : s) v /= len;
	const double cos_s = s[1] > 1.0 ? 1.0 : s[1];
	const double theta_s = std::acos(cos_s);
	const double coef[3][5] = {
		{  0.1787 * T - 1.4630, -0.3554 * T + 0.4275, -0.0227 * T + 5.3251,  0.1206 * T - 2.5771, -0.0670 * T + 0.3703 },
		{ -0.0193 * T - 0.2592, -0.0665 * T + 0.0008, -0.0004 * T + 0.2125, -0.0641 * T - 0.8989, -0.0033 * T + 0.0452 },
		{ -0.0167 * T - 0.2608, -0.0950 * T + 0.0092, -0.0079 * T + 0.2102, -0.0441 * T - 1.6537, -0.0109 * T + 0.0529 } };
	const double mx[3][4] = { { 0.00166, -0.00375, 0.00209, 0.0 }, { -0.02903, 0.06377, -0.03202, 0.00394 }, { 0.11693, -0.21196, 0.06052, 0.25886 } };
	const double my[3][4] = { { 0.00275, -0.00610, 0.00317, 0.0 }, { -0.04214, 0.08970, -0.04153, 0.00516 }, { 0.15346, -0.26756, 0.06670, 0.26688 } };
	const double tv[3] = { T * T, T, 1.0 }, th[4] = { theta_s * theta_s * theta_s, theta_s * theta_s, theta_s, 1.0 };
	double xz = 0.0, yz = 0.0;
	for (int i = 0; i < 3; i++) for (int j = 0; j < 4; j++) { xz += tv[i] * mx[i][j] * th[j]; yz += tv[i] * my[i][j] * th[j]; }
	const double chi = (4.0 / 9.0 - T / 120.0) * (pi - 2.0 * theta_s);
	const double Yz = (4.0453 * T - 4.9710) * std::tan(chi) - 0.2155 * T + 2.4192;
	Args a{};
	const double zen[3] = { Yz, xz, yz };
	for (int k = 0; k < 3; k++) {
		for (int j = 0; j < 5; j++) a.perez[k][j] = static_cast<float>(coef[k][j]);
		a.inv_f0[k] = static_cast<float>(1.0 / perez(coef[k], 1.0, theta_s));
		a.zenith[k] = static_cast<float>(zen[k]);
		a.sun[k] = static_cast<float>(s[k]);
		a.ground[k] = p.ground[k];
	}
	// the disc: extraterrestrial radiance through Rayleigh and aerosol optical depths at the air mass of Kasten and Young 1989
	const double deg = theta_s * 180.0 / pi;
	const double m = 1.0 / (cos_s + 0.50572 * std::pow(96.07995 - deg, -1.6364));
	const double lambda[3] = { 0.68, 0.55, 0.44 };
	for (int k = 0; k < 3; k++) {
		const double tau = 0.008735 * std::pow(lambda[k], -4.08) + (0.04608 * T - 0.04586) * std::pow(lambda[k], -1.3);
		a.sun_rgb[k] = static_cast<float>(static_cast<double>(p.sun_scale) * 1.9e6 * std::exp(-tau * m));
	}
	const double alpha = p.sun_radius;
	const double sh = std::sin(0.5 * alpha), sh9 = std::sin(0.45 * alpha);
	a.ramp_edge = static_cast<float>(2.0 * sh * sh);
	a.ramp_inv = static_cast<float>(1.0 / (2.0 * sh * sh - 2.0 * sh9 * sh9));           // cos(0.9 a) - cos(a) without the cancellation
	a.sky_scale = p.sky_scale;
	a.w = p.width; a.h = p.height;
	return a;
}

} // namespace mirt_sun_sky
