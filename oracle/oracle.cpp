// oracle/oracle.cpp — TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
// CPU restatement of the reference's Renderer::Accumulate / Render hot path
// (Borx25/CPU-Raytracing-experiments), used ONLY by tests/, __graft_entry__.smoke()
// and bench.py's cpu_baseline leg as the checker / reported baseline.  The product
// (cpu-raytracing-experiments_amd/csrc) never links, loads or calls anything here.
//
// PARITY STATUS: "parity unpinned" at the third-party boundary.  The reference has no
// tests, golden vectors or fixtures, and cannot be built in this image (MSVC-only
// constructs; glm / VCL / PPL / Vulkan headers absent).  This file
// therefore *defines* the semantics of the glm / VCL calls the path makes (documented
// at each helper) and is pinned only by (i) the integer KATs re-derived from
// Random.hpp's formulas, (ii) the analytic white-furnace result, (iii) internal
// cross-checks between the three traversal modes below.
//
// Every function cites the reference file:line it follows.  Arithmetic rules:
//   * compiled with -ffp-contract=off; fmaf() appears only where the reference uses
//     FMA intrinsics (BVH.hpp:251-260);
//   * min/max are spelled as the exact ternaries std::/glm:: expand to;
//   * IEEE f32 div / sqrt, round-to-nearest-even conversions, denormals preserved.
//
// Traversal modes (orc_config trav_mode):
//   0  brute force           — the reference as shipped (#define USEBVH false, BVH.hpp:307,312-318)
//   1  stream BVH            — the reference's USEBVH==true path (BVH.hpp:320-358, 367-402)
//   2  robust per-ray BVH    — CPU twin of the traversal the HIP kernels run (trace kernels in
//                              csrc/kernels.hpp): conservatively padded boxes, t in [0, tfar],
//                              near-first order with closest-hit pruning, lowest-prim-index tie
//                              break.  By construction it must return the mode-0 (brute force,
//                              as shipped) answer bit for bit; tests assert mode 2 == mode 0.
//                              Mode 1 is NOT equivalent to mode 0 (Q17 + order dependence of the
//                              stream traversal) and is kept as the reference's own alternative
//                              path for the CPU baseline and to quantify that discrepancy.
//
// Closure (orc_set_brdf): the reference's compile-time `#define BRDF` (Renderer.hpp:70) as oracle state.
//   0  Closure<LambertianDiffuse> — the reference as shipped (DataStreams.hpp:164-182)
//   1  Closure<GGX>               — DataStreams.hpp:184-219, with the gloss decay table Renderer.hpp:212 names
//                                   but never declares supplied by the caller
// Both are one accumulate_tile body, instantiated once per closure.
#include <cstdint>
#include <cstring>
#include <cstdlib>
#include <cmath>
#include <cfloat>
#include <vector>
#include <algorithm>
#include <numeric>
#include <thread>
#include <atomic>
#include <immintrin.h>

namespace {

// ---------------------------------------------------------------------------------
// Data contract (byte layouts of the reference structs)
// ---------------------------------------------------------------------------------
struct alignas(16) Sphere {            // Primitives.hpp:7-17  (32 B, 20 used)
	float px, py, pz;
	float radius_sq;
	int32_t material_ID;
};
static_assert(sizeof(Sphere) == 32, "Sphere layout");

struct alignas(32) Material {          // Primitives.hpp:18-27 (96 B, 68 used)
	float albedo[3];
	float F0[3];
	float F80[3];
	float emission[3];
	float transmission[3];
	float roughness;
	float IOR_minus_one;
};
static_assert(sizeof(Material) == 96, "Material layout");

struct alignas(32) Node {              // BVH.hpp:18-31 (32 B)
	alignas(16) float mn[3];
	uint32_t first_id;
	alignas(16) float mx[3];
	uint32_t prim_count;
};
static_assert(sizeof(Node) == 32, "Node layout");

struct v3 { float x, y, z; };
struct q4 { float x, y, z, w; };       // glm::quat storage order x,y,z,w (ctor order is w,x,y,z)

// ---------------------------------------------------------------------------------
// glm / std semantics this restatement defines
// ---------------------------------------------------------------------------------
static inline float std_max(float a, float b) { return (a < b) ? b : a; }   // std::max
static inline float std_min(float a, float b) { return (b < a) ? b : a; }   // std::min
static inline float glm_max(float x, float y) { return (x < y) ? y : x; }   // glm::max
static inline float glm_min(float x, float y) { return (y < x) ? y : x; }   // glm::min
static inline float dot3(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }  // glm::dot(vec3)
static inline v3 cross3(v3 x, v3 y) {                                                  // glm::cross
	return { x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y };
}
static inline v3 normalize3(v3 v) {    // glm::normalize = v * inversesqrt(dot(v,v)), inversesqrt = 1/sqrt
	float inv = 1.0f / sqrtf(dot3(v, v));
	return { v.x * inv, v.y * inv, v.z * inv };
}
static inline v3 quat_rotate(q4 q, v3 v) {   // glm operator*(quat, vec3)
	v3 qv{ q.x, q.y, q.z };
	v3 uv = cross3(qv, v);
	v3 uuv = cross3(qv, uv);
	return { v.x + ((uv.x * q.w) + uuv.x) * 2.0f,
	         v.y + ((uv.y * q.w) + uuv.y) * 2.0f,
	         v.z + ((uv.z * q.w) + uuv.z) * 2.0f };
}
static const float kPi          = static_cast<float>(3.14159265358979323846264338327950288);
static const float kHalfPi      = static_cast<float>(1.57079632679489661923132169163975144);
static const float kTwoPi       = static_cast<float>(6.28318530717958647692528676655900576);
static const float kOneOverPi   = static_cast<float>(0.318309886183790671537767526745028724);
static const float kOneOver2Pi  = static_cast<float>(0.159154943091895335768883763372514362);

static inline uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// ---------------------------------------------------------------------------------
// Random.hpp:5-50
// ---------------------------------------------------------------------------------
static inline float make_unit_float(uint32_t x) { return static_cast<float>(x) * 0x1p-32f; }   // :5
static inline uint32_t pcg_state_transition(uint32_t v) { return v * 747796405u + 2891336453u; } // :10-13
static inline uint32_t pcg_output(uint32_t v) {                                                 // :14-18
	v = ((v >> ((v >> 28u) + 4u)) ^ v) * 277803737u;
	return (v >> 22u) ^ v;
}
static inline uint32_t pcg_generate(uint32_t* s) { uint32_t p = *s; *s = pcg_state_transition(p); return pcg_output(p); } // :20-24
static inline float rand_unit_float(uint32_t* s) { return make_unit_float(pcg_generate(s)); }   // :26-29
static inline uint32_t rand_bounded_int(uint32_t* s, uint32_t range) {                          // :31-34
	uint32_t v = static_cast<uint32_t>(rand_unit_float(s) * static_cast<float>(range));
	uint32_t hi = range - 1;
	return (v < hi) ? v : hi;   // std::min(range-1, v)
}
static inline uint32_t hash_u32(uint32_t i) {                                                   // :36-43
	i ^= i >> 16; i *= 0x21f0aaadu; i ^= i >> 15; i *= 0xd35a2d97u; i ^= i >> 15;
	return i ^ 0xe6fe3bebu;
}
static inline uint32_t hash_2d(uint32_t x, uint32_t y) {                                        // :45-50
	const uint32_t qx = 0x41c64e6du * ((x >> 1u) ^ y);
	const uint32_t qy = 0x41c64e6du * ((y >> 1u) ^ x);
	return 0x41c64e6du * (qx ^ (qy >> 3u));
}

// ---------------------------------------------------------------------------------
// VectorMath.hpp:581-662 (scalar helpers)
// ---------------------------------------------------------------------------------
static inline float fast_abs(float v) { return u2f(f2u(v) & 0x7fffffffu); }                                   // :581-584
static inline float fast_copysign(float v, float s) { return u2f((f2u(v) & 0x7fffffffu) | (f2u(s) & 0x80000000u)); } // :589-592
static inline float fast_round(float x) { return rintf(x); }              // :593-595 _mm_round_ss nearest-even
static inline float f_xor(float a, float b) { return u2f(f2u(a) ^ f2u(b)); }   // :611-613
static inline float f_and(float a, float b) { return u2f(f2u(a) & f2u(b)); }   // :617-619

static inline float fast_asin(float x) {                                   // :625-630
	float f = fast_abs(x);
	f = (f < 1.0f) ? 1.0f - (1.0f - f) : 1.0f;
	f = kHalfPi - sqrtf(1.0f - f) * (1.5707963267f + f * (-0.213300989f + f * (0.077980478f + f * -0.02164095f)));
	return fast_copysign(f, x);
}
static inline float fast_atan2(float y, float x) {                         // :632-642
	const float a = fast_abs(x); const float b = fast_abs(y);
	float lo = std_min(a, b), hi = std_max(a, b);
	float k = hi == 0.0f ? 0.0f : lo / hi;
	k = 1.0f - (1.0f - k);
	const float k2 = k * k;
	float r = k * (0.43157974f * k2 + 1.0f) / ((0.05831938f * k2 + 0.76443945f) * k2 + 1.0f);
	if (b > a) r = kHalfPi - r;
	if (x < 0.0f) r = kPi - r;
	return fast_copysign(r, y);
}
static inline void fast_sincos(float x, float* sine, float* cosine) {      // :644-662
	const float qf = fast_round(x * kOneOverPi);
	const uint32_t sign_mask = static_cast<uint32_t>(static_cast<int32_t>(qf)) << 31;   // _mm_cvtps_epi32 then <<31
	x += qf * (-0.78515625f * 4);
	x += qf * (-0.00024187564849853515625f * 4);
	x += qf * (-3.7747668102383613586e-08f * 4);
	x += qf * (-1.2816720341285448015e-12f * 4);
	x = kHalfPi - (kHalfPi - x);
	float x2 = x * x;
	x = u2f(f2u(x) ^ sign_mask);
	float su = 2.6083159809786593541503e-06f;     float cu = -2.71811842367242206819355e-07f;
	su = su * x2 - 0.0001981069071916863322258f;  cu = (cu * x2 + 2.47990446951007470488548e-05f);
	su = su * x2 + 0.00833307858556509017944336f; cu = (cu * x2 - 0.00138888787478208541870117f);
	su = su * x2 - 0.166666597127914428710938f;   cu = (cu * x2 + 0.0416666641831398010253906f);
	su = x2 * (su * x) + x;                       cu = (cu * x2 - 0.5f); cu = (cu * x2 + 1.0f);
	cu = u2f(f2u(cu) ^ sign_mask);
	if (fast_abs(su) > 1.0f) { su = 0.0f; }       if (fast_abs(cu) > 1.0f) { cu = 0.0f; }
	*sine = su; *cosine = cu;
}

// ---------------------------------------------------------------------------------
// Sampling.hpp
// ---------------------------------------------------------------------------------
static inline float median3(float a, float b, float c) {                   // :8-12
	return std_max(std_min(a, b), std_min(std_max(a, b), c));
}
static inline float median5(float a, float b, float c, float d, float e) { // :13-21
	return median3(std_max(std_min(a, b), std_min(c, d)), std_min(std_max(a, b), std_max(c, d)), e);
}
static inline v3 spherical_to_cartesian(float phi_over_2pi, float sin_theta, float cos_theta) {   // :77-84
	float cos_phi, sin_phi; fast_sincos(phi_over_2pi * kTwoPi, &sin_phi, &cos_phi);
	return { sin_theta * cos_phi, sin_theta * sin_phi, cos_theta };
}
static inline v3 hemisphere(float t, float s) {                             // :92-94
	return spherical_to_cartesian(s, sqrtf(t), sqrtf(std_max(0.0f, 1.0f - t)));
}
static inline void orthonormal_basis(v3 n, v3* v2, v3* v3_) {               // :116-130
	float sign = f_and(-0.0f, n.z);
	float s = f_xor(1.0f, sign);
	float z = -1.0f / (s + n.z);
	float s_nx = f_xor(sign, n.x);
	float ny_z = n.y * z;
	float t = n.x * ny_z;
	*v2 = { 1.0f + (s_nx * n.x) * z, f_xor(sign, t), -s_nx };
	*v3_ = { t, s + ny_z * n.y, -n.y };
}
static inline q4 tangent_space(v3 N) {                                      // :150-159 (quat ctor order w,x,y,z)
	if (N.z < -1.0f + FLT_EPSILON) {
		return q4{ 0.0f, 1.0f, 0.0f, 0.0f };      // {w=0, x=0, y=1, z=0}
	} else {
		float s = sqrtf(2.0f * (N.z + 1.0f));
		float invs = 1.0f / s;
		return q4{ -N.y * invs, N.x * invs, 0.0f, s * 0.5f };
	}
}
static inline v3 to_local(q4 T, v3 v) {                                     // :161-169
	float temp = 2.0f * (v.z * T.w + v.x * T.y - T.x * v.y);
	return { v.x - T.y * temp, v.y + T.x * temp, temp * T.w - v.z };
}
static inline v3 to_world(q4 T, v3 v) {                                     // :171-179
	float temp = 2.0f * (v.z * T.w - v.x * T.y + T.x * v.y);
	return { v.x + T.y * temp, v.y - T.x * temp, temp * T.w - v.z };
}
static inline float conePdf(float cosThetaMax) {                            // :192-194
	return kOneOver2Pi / std_max(1e-6f, 1.0f - cosThetaMax);
}
static inline float spherePdf(float radius_sq, float dist_sq) {             // :196-200
	float sinThetaMax2 = radius_sq / dist_sq;
	float cosThetaMax = sqrtf(std_max(0.0f, 1.0f - sinThetaMax2));
	return conePdf(cosThetaMax);
}
static inline v3 sample_direction_to_sphere(v3 Wc, float sinThetaMax2, float center_dist, float radius2,
                                            float t, float s, float* out_distance, float* out_pdf) {   // :220-239
	float cosThetaMax = sqrtf(std_max(0.0f, 1.0f - sinThetaMax2));
	*out_pdf = conePdf(cosThetaMax);
	float cosTheta = 1.0f - t * (1.0f - cosThetaMax);
	float sinTheta = sqrtf(sinThetaMax2 * t);
	float src_blend = (sinThetaMax2 < 0.00068523f ? sinTheta : cosTheta);
	float invert = sqrtf(std_max(0.0f, 1.0f - src_blend * src_blend));
	cosTheta = (sinThetaMax2 < 0.00068523f ? invert : cosTheta);
	sinTheta = (sinThetaMax2 < 0.00068523f ? sinTheta : invert);
	float temp = center_dist * sinTheta;
	*out_distance = center_dist * cosTheta - sqrtf(std_max(0.0f, radius2 - temp * temp)) - 1e-5f;
	v3 Ll = spherical_to_cartesian(s, sinTheta, cosTheta);
	v3 wcX, wcY; orthonormal_basis(Wc, &wcX, &wcY);
	return { wcX.x * Ll.x + wcY.x * Ll.y + Wc.x * Ll.z,
	         wcX.y * Ll.x + wcY.y * Ll.y + Wc.y * Ll.z,
	         wcX.z * Ll.x + wcY.z * Ll.y + Wc.z * Ll.z };
}
// ---- GGX closure (DataStreams.hpp:184-219, Sampling.hpp:102-104,254-309) — §8f rank 4, FUNCTION LEVEL ONLY ----------------------
// The reference compiles this path out (`#define BRDF 0`, Renderer.hpp:70): with BRDF 1 it does not build (`gloss_decay_table`,
// Renderer.hpp:212, is declared nowhere) and Closure<GGX>::pdf returns 0 (DataStreams.hpp:198, "TODO").  What IS defined — eval and
// sample of the closure and the functions under them — is restated here so that the device versions can be checked bit for bit.
// glm: mix(x, y, a) = x * (1 - a) + y * a; vec3 * float and vec3 + vec3 componentwise, left to right.
static inline float glm_mix(float x, float y, float a) { return x * (1.0f - a) + y * a; }
static inline float std_clamp(float v, float lo, float hi) { return (v < lo) ? lo : (hi < v) ? hi : v; }
static inline void polar_to_cartesian(float phi_over_2pi, float rho, float* x, float* y) {      // Sampling.hpp:85-91
	float cos_phi, sin_phi; fast_sincos(phi_over_2pi * kTwoPi, &sin_phi, &cos_phi);
	*x = rho * cos_phi; *y = rho * sin_phi;
}
static inline void disk(float t, float s, float* x, float* y) { polar_to_cartesian(s, sqrtf(t), x, y); }   // :102-104
static inline v3 distribution_visible_normals(v3 Vlocal, float alpha, float u, float v) {        // :254-270
	v3 V = normalize3(v3{ alpha * Vlocal.x, alpha * Vlocal.y, Vlocal.z });
	float sx, sy; disk(u, v, &sx, &sy);
	const float t = 1.0f - sx * sx;
	sy = glm_mix(sqrtf(t), sy, V.z * 0.5f + 0.5f);
	v3 X, Y; orthonormal_basis(V, &X, &Y);
	const float k = sqrtf(std_max(0.0f, t - sy * sy));
	v3 H{ (X.x * sx + Y.x * sy) + V.x * k, (X.y * sx + Y.y * sy) + V.y * k, (X.z * sx + Y.z * sy) + V.z * k };
	return normalize3(v3{ alpha * H.x, alpha * H.y, std_max(0.0f, H.z) });
}
static inline float pow5(float x) { float t = x * x; t *= t; return x * t; }                       // :272
static inline v3 Fresnel(v3 F0, float HdotV) {                                                    // :273-275
	const float a = pow5(std_clamp(1.0f - HdotV, 0.0f, 1.0f));
	return { glm_mix(F0.x, 1.0f, a), glm_mix(F0.y, 1.0f, a), glm_mix(F0.z, 1.0f, a) };
}
static inline float GGX_D(float alpha2, float NdotH2) {                                            // :278-281
	float temp = (1.0f + (alpha2 - 1.0f) * NdotH2);
	return alpha2 / (kPi * temp * temp);
}
static inline float Smith_G2_Height_Correlated_GGX_Lagarde(float alpha2, float NdotL, float NdotV) {   // :287-291
	float a = NdotV * sqrtf(alpha2 + NdotL * (NdotL - alpha2 * NdotL));
	float b = NdotL * sqrtf(alpha2 + NdotV * (NdotV - alpha2 * NdotV));
	return 0.5f / (a + b);
}
static inline v3 microfacet_brdf(v3 F0, float alpha, float NdotV, float NdotL, float NdotH, float HdotV) {   // :293-296
	const float alpha2 = alpha * alpha;
	const v3 F = Fresnel(F0, HdotV);
	const float k = NdotL * GGX_D(std_max(0.00001f, alpha2), NdotH * NdotH) * Smith_G2_Height_Correlated_GGX_Lagarde(alpha2, NdotL, NdotV);
	return { F.x * k, F.y * k, F.z * k };
}
static inline float G1_GGX(float alpha2, float NdotS2) { return 2.0f / (1.0f + sqrtf(((alpha2 * (1.0f - NdotS2)) + NdotS2) / NdotS2)); }   // :297-299
static inline float Smith_G2_Over_G1_Height_Correlated(float alpha2, float NdotL, float NdotV) {  // :301-305
	float G1V = G1_GGX(alpha2, NdotV * NdotV);
	float G1L = G1_GGX(alpha2, NdotL * NdotL);
	return G1L / (G1V + G1L - G1V * G1L);
}
static inline v3 vndf_estimator(v3 F0, float alpha, float NdotV, float NdotL, float HdotV) {      // :307-309
	const v3 F = Fresnel(F0, HdotV);
	const float k = Smith_G2_Over_G1_Height_Correlated(alpha * alpha, NdotL, NdotV);
	return { F.x * k, F.y * k, F.z * k };
}
static inline v3 ggx_eval(v3 F0, float alpha, v3 Llocal, v3 Vlocal) {                            // Closure<GGX>::eval, DataStreams.hpp:189-195
	float NdotL = std_max(0.0f, Llocal.z);
	float NdotV = std_max(0.0f, Vlocal.z);
	const v3 Hn = normalize3(v3{ Llocal.x + Vlocal.x, Llocal.y + Vlocal.y, Llocal.z + Vlocal.z });
	float NdotH = std_max(0.0f, Hn.z);
	float HdotV = std_max(0.0f, dot3(Hn, Vlocal));
	return microfacet_brdf(F0, alpha, NdotV, NdotL, NdotH, HdotV);
}
static inline void ggx_sample(v3 F0, float alpha, v3 Vlocal, float u0, float u1, v3* dir, v3* estimator) {   // Closure<GGX>::sample, DataStreams.hpp:200-218
	float NdotV = std_max(0.0f, Vlocal.z);
	float HdotV;
	if (alpha == 0.0f) {
		*dir = v3{ -Vlocal.x, -Vlocal.y, Vlocal.z };
		HdotV = NdotV;
	} else {
		v3 Hlocal = distribution_visible_normals(Vlocal, alpha, u0, u1);
		HdotV = dot3(Hlocal, Vlocal);
		const float k = 2.0f * HdotV;
		*dir = v3{ k * Hlocal.x - Vlocal.x, k * Hlocal.y - Vlocal.y, k * Hlocal.z - Vlocal.z };
		HdotV = std_max(0.0f, HdotV);
	}
	float NdotL = std_max(0.0f, dir->z);
	*estimator = vndf_estimator(F0, alpha, NdotV, NdotL, HdotV);
}

static inline float powerHeuristic(float f, float g) { float f2 = f * f; return f2 / std_max(1e-6f, f2 + g * g); } // :241-244
static inline float powerHeuristic_over_f(float f, float g) { return f / std_max(1e-6f, f * f + g * g); }         // :245-247

// ---------------------------------------------------------------------------------
// Color.hpp:47-49,66-73 (lane-wise; VCL Vec8f ops are IEEE lane ops)
// ---------------------------------------------------------------------------------
static inline float ACES_rtt_odt_fit(float x) {
	return (x * (x + 0.0245786f) - 0.000090537f) / (x * (0.983729f * x + 0.4329510f) + 0.238081f);
}
static inline float vcl_max(float a, float b) { return (a > b) ? a : b; }   // _mm256_max_ps(a,b)
static inline float vcl_min(float a, float b) { return (a < b) ? a : b; }   // _mm256_min_ps(a,b)
static inline void tonemapping(float& r, float& g, float& b) {
	float x = ACES_rtt_odt_fit(r * 0.59719f + g * 0.35458f + b * 0.04823f);
	float y = ACES_rtt_odt_fit(r * 0.07600f + g * 0.90834f + b * 0.01566f);
	float z = ACES_rtt_odt_fit(r * 0.02840f + g * 0.13383f + b * 0.83777f);
	r = vcl_min(1.0f, vcl_max(0.0f, x * 1.604750f + y * -0.53108f + z * -0.07367f));
	g = vcl_min(1.0f, vcl_max(0.0f, x * -0.10208f + y * 1.10813f + z * -0.00605f));
	b = vcl_min(1.0f, vcl_max(0.0f, x * -0.00327f + y * -0.07276f + z * 1.07602f));
}

// ---------------------------------------------------------------------------------
// Camera.hpp:80-88, Primitives.hpp:29-47
// ---------------------------------------------------------------------------------
struct Camera {
	v3 pos{0, 0, 0};
	q4 orient{0, 0, 0, 1};
	float half_width = 0.5f, half_height = 0.5f, z = -1.0f, exposure = 1.0f;
};
static inline v3 generate_ray_dir(const Camera& c, int32_t x, int32_t y, const float* samples) {
	v3 d{ static_cast<float>(x) + samples[0] - c.half_width,
	      static_cast<float>(y) + samples[1] - c.half_height,
	      c.z };
	return normalize3(quat_rotate(c.orient, d));
}
struct Sky {
	float ambient[3] = {0, 0, 0};
	int32_t w = 0, h = 0;
	std::vector<float> hdri;      // RGBA f32
	float fw = 0, fh = 0;
};
static inline v3 sky_eval(const Sky& s, float x, float y, float z) {         // Primitives.hpp:35-46
	float ex = s.fw * (0.5f + kOneOver2Pi * fast_atan2(z, x));
	float ey = s.fh * (0.5f - kOneOverPi * fast_asin(y));
	const float* t = s.hdri.data() + 4 * (static_cast<int32_t>(ey) * s.w + static_cast<int32_t>(ex));
	return { t[0] * s.ambient[0], t[1] * s.ambient[1], t[2] * s.ambient[2] };
}

// ---------------------------------------------------------------------------------
// BVH builder — BVH.hpp:90-206 (quirks Q15, Q16 reproduced)
// ---------------------------------------------------------------------------------
struct Box { float mn[3], mx[3]; };
static inline Box box_empty() { return { { FLT_MAX, FLT_MAX, FLT_MAX }, { -FLT_MAX, -FLT_MAX, -FLT_MAX } }; }  // :28-29
static inline void box_or(Box& a, const Box& b) {                             // :35-39 (glm::min/max(vec3))
	for (int i = 0; i < 3; i++) { a.mn[i] = glm_min(a.mn[i], b.mn[i]); a.mx[i] = glm_max(a.mx[i], b.mx[i]); }
}
static bool g_true_half_area = false;   // true while building the mode-2 internal tree: full half area instead of the reference's Q15 formula
static inline float box_half_area(const Box& b) {                             // :58-67 — Q15: only d.y*d.z
	float d[3] = { b.mx[0] - b.mn[0], b.mx[1] - b.mn[1], b.mx[2] - b.mn[2] };
	if (g_true_half_area) return (d[0] * d[1] + d[1] * d[2]) + d[2] * d[0];      // csrc/bvh_build.cpp sah_area(full)
	float area = 0.0f;
	int32_t i = 2;
	for (float accum = d[i--]; i > 0; i--) { area += d[i] * accum; accum += d[i]; }
	return area;
}
static inline size_t box_largest_axis(const Box& b) {                          // :48-54
	float d[3] = { b.mx[0] - b.mn[0], b.mx[1] - b.mn[1], b.mx[2] - b.mn[2] };
	size_t ret = 0;
	for (size_t i = 1; i < 3; ++i) if (d[ret] < d[i]) ret = i;
	return ret;
}

struct BVH {
	std::vector<Node> nodes;
	std::vector<Sphere> prims;
	std::vector<Box> padded;      // mode 2 only: conservative box per node (same indexing as nodes)
	std::vector<uint32_t> slot_prim;   // mode 2 tree only: leaf slot -> index into the reference tree's prims (empty = identity)
	float pad_rel = 0.0f;
	bool wide = false;                 // mode 2 only: walk the tree as the product's 4-wide records do (csrc/bvh_layout.hpp build_wide_half_records)
};

static void bvh_build(const std::vector<Sphere>& primitives, BVH& out, std::vector<uint32_t>* order_out = nullptr) {
	struct StackFrame { size_t ID, begin, count; };
	struct Split { size_t pos, axis; float cost; };
	const size_t primnum = primitives.size();
	std::vector<uint32_t> primIDs(primnum * 3);
	std::vector<Box> bboxes(primnum);
	std::vector<float> centroids(primnum * 3);
	std::vector<float> accum_cost(primnum);
	std::vector<uint8_t> marks(primnum);
	out.prims.assign(primnum, Sphere{});
	out.nodes.clear();
	out.nodes.reserve(2 * (primnum + 1));
	std::vector<Box> node_box; node_box.reserve(2 * (primnum + 1));
	if (primnum == 0) return;

	for (size_t i = 0; i < primnum; i++) {                                    // :116-117, Primitives.hpp:13-16
		float r = sqrtf(primitives[i].radius_sq);
		const float p[3] = { primitives[i].px, primitives[i].py, primitives[i].pz };
		for (int a = 0; a < 3; a++) {
			bboxes[i].mn[a] = p[a] - r; bboxes[i].mx[a] = p[a] + r;
			centroids[i * 3 + a] = (bboxes[i].mx[a] + bboxes[i].mn[a]) * 0.5f;  // :55-57
		}
	}
	for (size_t axis = 0; axis < 3; ++axis) {                                   // :118-122
		uint32_t* ids = primIDs.data() + axis * primnum;
		std::iota(ids, ids + primnum, 0u);
		// std::ranges::sort is unstable in the reference; ties broken by index here (documented choice).
		std::stable_sort(ids, ids + primnum, [&](uint32_t a, uint32_t b) { return centroids[a * 3 + axis] < centroids[b * 3 + axis]; });
	}
	auto reduce_bboxes = [&](size_t from, size_t to) { Box r = box_empty(); for (size_t i = from; i < to; ++i) box_or(r, bboxes[primIDs[i]]); return r; }; // :109-113 (axis 0 ids)
	auto heur_leaf_cost = [](size_t size, float ha) { return ha * static_cast<float>(size); };               // :77-79 (log_cluster_size 0)
	auto heur_non_split = [](size_t size, float ha) { return ha * (static_cast<float>(size) - 1.0f); };      // :80-82 (cost_ratio 1)
	auto push_node = [&](const Box& b) { Node n; memset(&n, 0, sizeof n); for (int a = 0; a < 3; a++) { n.mn[a] = b.mn[a]; n.mx[a] = b.mx[a]; } out.nodes.push_back(n); node_box.push_back(b); };

	{ Box root = box_empty(); for (size_t i = 0; i < primnum; i++) box_or(root, bboxes[i]); push_node(root); }   // :125
	std::vector<StackFrame> stack; stack.reserve(64);
	stack.push_back({0, 0, primnum});
	while (!stack.empty()) {
		StackFrame item = stack.back(); stack.pop_back();
		if (item.count <= 1) {                                                 // :133-137
			out.nodes[item.ID].first_id = static_cast<uint32_t>(item.begin);
			out.nodes[item.ID].prim_count = static_cast<uint32_t>(item.count);
			continue;
		}
		const size_t first_child = out.nodes.size();
		out.nodes[item.ID].first_id = static_cast<uint32_t>(first_child);
		const size_t begin = item.begin, end = item.begin + item.count;
		const Box nb = node_box[item.ID];
		Split best{ begin + (item.count + 1) / 2, box_largest_axis(nb), heur_non_split(item.count, box_half_area(nb)) };   // :144
		for (size_t axis = 0; axis < 3; ++axis) {                               // :146-171 (Q16: full sweeps)
			size_t first_right = 0;
			Box right_bbox = box_empty();
			for (size_t i = end - 1; i > begin;) {
				float right_cost = 0.0f;
				for (; i > i - std::min<size_t>(i - begin, 32); --i) {
					box_or(right_bbox, bboxes[primIDs[axis * primnum + i]]);
					accum_cost[i] = right_cost = heur_leaf_cost(end - i, box_half_area(right_bbox));
				}
				if (right_cost > best.cost) { first_right = i; break; }
			}
			Box left_bbox = box_empty();
			for (size_t i = begin; i < end - 1; i++) {
				box_or(left_bbox, bboxes[primIDs[axis * primnum + i]]);
				if (i < first_right) break;
				float left_cost = heur_leaf_cost(i + 1 - begin, box_half_area(left_bbox));
				if (left_cost > best.cost) break;
				float cost = left_cost + accum_cost[i + 1];
				if (cost < best.cost) best = Split{ i + 1, axis, cost };
			}
		}
		for (size_t i = begin; i < best.pos; ++i) marks[primIDs[best.axis * primnum + i]] = 1;   // :174-175
		for (size_t i = best.pos; i < end; ++i) marks[primIDs[best.axis * primnum + i]] = 0;
		for (size_t axis = 0; axis < 3; ++axis) {                               // :176-183
			if (axis == best.axis) continue;
			std::stable_partition(primIDs.begin() + axis * primnum + begin, primIDs.begin() + axis * primnum + end,
			                      [&](uint32_t id) { return marks[id] != 0; });
		}
		struct Range { size_t begin, end; };                                    // :186-197
		const Range ranges[2] = { { begin, best.pos }, { best.pos, end } };
		const Box children[2] = { reduce_bboxes(ranges[0].begin, ranges[0].end), reduce_bboxes(ranges[1].begin, ranges[1].end) };
		size_t sort_area = static_cast<size_t>(box_half_area(children[0]) < box_half_area(children[1]));
		size_t sort_size = static_cast<size_t>(ranges[0].end - ranges[0].begin < ranges[1].end - ranges[1].begin);
		size_t combined = sort_area ^ sort_size;
		push_node(children[sort_area]);
		push_node(children[1 - sort_area]);
		stack.push_back({ first_child + combined, ranges[sort_size].begin, ranges[sort_size].end - ranges[sort_size].begin });
		stack.push_back({ first_child + (1 - combined), ranges[1 - sort_size].begin, ranges[1 - sort_size].end - ranges[1 - sort_size].begin });
	}
	for (size_t i = 0; i < primnum; i++) out.prims[i] = primitives[primIDs[i]];   // :201-205
	if (order_out) order_out->assign(primIDs.begin(), primIDs.begin() + primnum);
}

// ---------------------------------------------------------------------------------
// Stream containers — DataStreams.hpp:74-157 (StreamSize = 256)
// ---------------------------------------------------------------------------------
constexpr size_t TileRoot = 16, TileSize = 256, N = 256;     // Renderer.hpp:32-34, policy log_tile=4
constexpr size_t MaxMaterialID = 64;                         // Renderer.hpp:23

struct Bitset256 {                                            // DataStreams.hpp:6-57
	uint64_t block[4];
	bool test(size_t i) const { return (block[i / 64] >> (i % 64)) & 1ull; }
	void set(size_t i) { block[i / 64] |= (1ull << (i % 64)); }
	void zero() { memset(block, 0, sizeof block); }
};
struct Buffer {                                               // :75-88
	struct { float x[N], y[N], z[N]; } p, dir;
	struct { float r[N], g[N], b[N]; } radiance, throughput;
	float pdf[N];
	uint32_t pixelID[N];
};
struct Hit { float tfar[N]; int32_t primID[N]; int32_t matID[N]; };               // :106-112
struct ShadowStream {                                                               // :113-126
	struct { float x[N], y[N], z[N]; } p, dir;
	float tfar[N];
	struct { float r[N], g[N], b[N]; } radiance;
	Bitset256 occluded;
};
struct alignas(64) RayStream {
	Buffer buffers[2];
	Bitset256 termination, has_shadowray;
	uint32_t seed[N];
	uint32_t RayID[N];
	Hit hit;
	ShadowStream shadow_rays;
};
struct ShaderData {                                                                 // :142-157; closure[ID] of either type, DataStreams.hpp:164-219
	float albedo[N][3];                                                             // Closure<LambertianDiffuse>
	float F0[N][3];                                                                 // Closure<GGX>
	float alpha[N];
	struct { float x[N], y[N], z[N]; } P, V;
	struct { float x[N], y[N], z[N], w[N]; } T;
	Bitset256 is_emissive;
};

struct Counters {
	std::atomic<uint64_t> rays{0}, shadow_rays{0};
	std::atomic<uint64_t> nodes{0}, spheres{0}, shadow_nodes{0}, shadow_spheres{0};
	std::atomic<uint64_t> terminated{0};
};
struct LocalCounters { uint64_t rays = 0, shadow_rays = 0, nodes = 0, spheres = 0, shadow_nodes = 0, shadow_spheres = 0, terminated = 0; };

// ---------------------------------------------------------------------------------
// Intersection — BVH.hpp:219-305
// ---------------------------------------------------------------------------------
// One ray × one sphere with the SIMD body's FMA formula (BVH.hpp:251-267).  Q14: the scalar
// tail's unfused formula is NOT used; every ray takes the FMA form (the one deliberate normalisation).
static inline void sphere_closest(const Sphere& s, int32_t prim_ID, float px, float py, float pz,
                                  float dx, float dy, float dz, float* tfar, int32_t* primID) {
	float tx = s.px - px;
	float b = dx * tx;
	float disc = fmaf(-tx, tx, s.radius_sq);
	float ty = s.py - py;
	b = fmaf(dy, ty, b);
	disc = fmaf(-ty, ty, disc);
	float tz = s.pz - pz;
	b = fmaf(dz, tz, b);
	disc = fmaf(-tz, tz, disc);
	disc = fmaf(b, b, disc);
	// :261-265 — sqrt of a negative gives the sign-set NaN, so "sign(sqrt) clear" is the disc>=0 test
	// (restated explicitly; -0.0 discriminant: sqrt(-0)=-0 has its sign set -> rejected, as in the SIMD body).
	if (f2u(disc) & 0x80000000u) return;
	float sq = sqrtf(disc);
	float dist = b - sq;
	if (f2u(dist) & 0x80000000u) dist = b + sq;        // blendv on the sign bit of dist
	if ((dist < *tfar) && !(f2u(dist) & 0x80000000u)) { *tfar = dist; *primID = prim_ID; }
}
// The scalar tail of intersect_prims exactly as written (BVH.hpp:270-286): separate multiply and add, dimension by
// dimension, `disc < 0` / `dist < 0 || dist >= tfar` tests.  Used only with orc_set_exact_tail(1) (trav_mode 0), to measure how
// far the Q14 normalisation above is from the reference's own mixed SIMD-body / scalar-tail arithmetic.
static inline void sphere_closest_scalar_tail(const Sphere& s, int32_t prim_ID, float px, float py, float pz,
                                              float dx, float dy, float dz, float* tfar, int32_t* primID) {
	const float c[3] = { s.px, s.py, s.pz }, p[3] = { px, py, pz }, d[3] = { dx, dy, dz };
	float b = 0.0f;
	float disc = s.radius_sq;
	for (int dim = 0; dim < 3; dim++) {
		const float temp = c[dim] - p[dim];
		b += d[dim] * temp;
		disc -= temp * temp;
	}
	disc += b * b;
	if (disc < 0.0f) return;
	disc = sqrtf(disc);
	const float dist = (b >= disc ? b - disc : b + disc);
	if (dist < 0.0f || dist >= *tfar) return;
	*tfar = dist; *primID = prim_ID;
}
static bool g_exact_tail = false;
// Shadow any-hit, scalar formula (BVH.hpp:294-300)
static inline bool sphere_occludes(const Sphere& s, float px, float py, float pz, float dx, float dy, float dz, float tfar) {
	v3 P{ s.px - px, s.py - py, s.pz - pz };
	float b = dot3(v3{dx, dy, dz}, P);
	float disc = b * b - dot3(P, P) + s.radius_sq;
	if (disc < 0.0f) return false;
	disc = sqrtf(disc);
	float dist = (b >= disc ? b - disc : b + disc);
	if (dist < 0.0f || dist >= tfar) return false;
	return true;
}

#if defined(__AVX2__) && defined(__FMA__)
// 8 rays × 1 sphere, BVH.hpp:250-268 — lane-for-lane the arithmetic of sphere_closest().
static inline void sphere_closest8(const Sphere& s, int32_t prim_ID, const Buffer& in, Hit& out, size_t ID) {
	const __m256 cx = _mm256_set1_ps(s.px), cy = _mm256_set1_ps(s.py), cz = _mm256_set1_ps(s.pz), r2 = _mm256_set1_ps(s.radius_sq);
	__m256 tx = _mm256_sub_ps(cx, _mm256_loadu_ps(&in.p.x[ID]));
	__m256 b = _mm256_mul_ps(_mm256_loadu_ps(&in.dir.x[ID]), tx);
	__m256 disc = _mm256_fnmadd_ps(tx, tx, r2);
	__m256 ty = _mm256_sub_ps(cy, _mm256_loadu_ps(&in.p.y[ID]));
	b = _mm256_fmadd_ps(_mm256_loadu_ps(&in.dir.y[ID]), ty, b);
	disc = _mm256_fnmadd_ps(ty, ty, disc);
	__m256 tz = _mm256_sub_ps(cz, _mm256_loadu_ps(&in.p.z[ID]));
	b = _mm256_fmadd_ps(_mm256_loadu_ps(&in.dir.z[ID]), tz, b);
	disc = _mm256_fnmadd_ps(tz, tz, disc);
	disc = _mm256_fmadd_ps(b, b, disc);
	if (_mm256_movemask_ps(disc) == 0xFF) return;
	__m256 neg = disc;                                   // sign of disc before sqrt == sign of sqrt result (NaN keeps it)
	__m256 sq = _mm256_sqrt_ps(disc);
	__m256 dist = _mm256_sub_ps(b, sq);
	dist = _mm256_blendv_ps(dist, _mm256_add_ps(b, sq), dist);
	__m256 lt = _mm256_cmp_ps(dist, _mm256_loadu_ps(&out.tfar[ID]), _CMP_LT_OS);
	__m256 mask = _mm256_andnot_ps(_mm256_or_ps(neg, dist), lt);
	_mm256_maskstore_ps(&out.tfar[ID], _mm256_castps_si256(mask), dist);
	_mm256_maskstore_epi32(&out.primID[ID], _mm256_castps_si256(mask), _mm256_set1_epi32(prim_ID));
}
#endif

static void intersect_prims(const BVH& bvh, const Buffer& in, Hit& out, size_t begin_ray, size_t end_ray,
                            size_t begin_prim, size_t end_prim, LocalCounters& lc) {        // BVH.hpp:236-288
	for (size_t prim = begin_prim; prim < end_prim; prim++) {
		const Sphere& s = bvh.prims[prim];
		size_t ID = begin_ray;
#if defined(__AVX2__) && defined(__FMA__)
		for (; (ID + 7) < end_ray; ID += 8) sphere_closest8(s, static_cast<int32_t>(prim), in, out, ID);
#endif
		for (; ID < end_ray; ID++) {                       // the last (end_ray - begin_ray) % 8 rays of the stream
			if (g_exact_tail) sphere_closest_scalar_tail(s, static_cast<int32_t>(prim), in.p.x[ID], in.p.y[ID], in.p.z[ID], in.dir.x[ID], in.dir.y[ID], in.dir.z[ID], &out.tfar[ID], &out.primID[ID]);
			else sphere_closest(s, static_cast<int32_t>(prim), in.p.x[ID], in.p.y[ID], in.p.z[ID], in.dir.x[ID], in.dir.y[ID], in.dir.z[ID], &out.tfar[ID], &out.primID[ID]);
		}
	}
	lc.spheres += (end_prim - begin_prim) * (end_ray - begin_ray);
}
static void intersect_prims_shadow(const BVH& bvh, ShadowStream& in, size_t begin_ray, size_t end_ray,
                                   size_t begin_prim, size_t end_prim, LocalCounters& lc) {  // BVH.hpp:290-305
	for (size_t ID = begin_ray; ID < end_ray; ID++) {
		for (size_t prim = begin_prim; prim < end_prim; prim++) {
			lc.shadow_spheres++;
			if (sphere_occludes(bvh.prims[prim], in.p.x[ID], in.p.y[ID], in.p.z[ID], in.dir.x[ID], in.dir.y[ID], in.dir.z[ID], in.tfar[ID])) {
				in.occluded.set(ID);
				break;
			}
		}
	}
}

struct RayAccel { float mx, my, mz, nx, ny, nz, t; };          // AABB_acceleration_struct, BVH.hpp:208-216
static inline RayAccel make_accel(float px, float py, float pz, float dx, float dy, float dz, float t) {   // :326-333
	RayAccel a;
	a.mx = 1.0f / dx; a.nx = px * a.mx;
	a.my = 1.0f / dy; a.ny = py * a.my;
	a.mz = 1.0f / dz; a.nz = pz * a.mz;
	a.t = t;
	return a;
}
static inline bool test_AABB(const RayAccel& a, const Node& node) {                                        // :219-234
	float lo = node.mn[0] * a.mx - a.nx;
	float hi = node.mx[0] * a.mx - a.nx;
	float tmin = glm_max(1e-4f, glm_min(lo, hi));
	float tmax = glm_min(a.t, glm_max(lo, hi));
	lo = node.mn[1] * a.my - a.ny;
	hi = node.mx[1] * a.my - a.ny;
	tmin = glm_max(tmin, glm_min(lo, hi));
	tmax = glm_min(tmax, glm_max(lo, hi));
	lo = node.mn[2] * a.mz - a.nz;
	hi = node.mx[2] * a.mz - a.nz;
	tmin = glm_max(tmin, glm_min(lo, hi));
	tmax = glm_min(tmax, glm_max(lo, hi));
	return tmax >= tmin;
}

// mode 1: BVH.hpp:320-358
static void traverse_stream(const BVH& bvh, const Buffer& in, Hit& out, size_t size, LocalCounters& lc) {
	struct Frame { size_t ID, head; };
	Frame stack[64]; size_t sp = 0;
	Frame frame{0, 0};
	static thread_local RayAccel accel[N];
	for (size_t i = 0; i < size; i++) accel[i] = make_accel(in.p.x[i], in.p.y[i], in.p.z[i], in.dir.x[i], in.dir.y[i], in.dir.z[i], out.tfar[i]);
	for (;;) {
		const Node& node = bvh.nodes[frame.ID];
		bool descended = false;
		for (; frame.head < size; frame.head++) {
			lc.nodes++;
			if (test_AABB(accel[frame.head], node)) {
				if (node.prim_count == 0) {
					if (sp >= 64) abort();                                      // DataStructures.hpp:36 assert
					stack[sp++] = Frame{ static_cast<size_t>(node.first_id) + 1, frame.head };
					frame.ID = node.first_id;
					descended = true;
					break;
				}
				intersect_prims(bvh, in, out, frame.head, size, node.first_id, node.first_id + node.prim_count, lc);
				break;
			}
		}
		if (descended) continue;
		if (sp == 0) return;
		frame = stack[--sp];
	}
}
// mode 1 shadow: BVH.hpp:367-402
static void traverse_stream_shadow(const BVH& bvh, ShadowStream& in, size_t size, LocalCounters& lc) {
	struct Frame { size_t ID, head; };
	Frame stack[64]; size_t sp = 0;
	Frame frame{0, 0};
	static thread_local RayAccel accel[N];
	for (size_t i = 0; i < size; i++) accel[i] = make_accel(in.p.x[i], in.p.y[i], in.p.z[i], in.dir.x[i], in.dir.y[i], in.dir.z[i], in.tfar[i]);
	for (;;) {
		const Node& node = bvh.nodes[frame.ID];
		bool descended = false;
		for (; frame.head < size; frame.head++) {
			lc.shadow_nodes++;
			if (test_AABB(accel[frame.head], node)) {
				if (node.prim_count == 0) {
					if (sp >= 64) abort();
					stack[sp++] = Frame{ static_cast<size_t>(node.first_id) + 1, frame.head };
					frame.ID = node.first_id;
					descended = true;
					break;
				}
				intersect_prims_shadow(bvh, in, frame.head, size, node.first_id, node.first_id + node.prim_count, lc);
				break;
			}
		}
		if (descended) continue;
		if (sp == 0) return;
		frame = stack[--sp];
	}
}

// mode 2: robust per-ray traversal — CPU twin of node_step() / node_step_wide() / leaf_step() in csrc/kernels.hpp.
// Boxes: every leaf box is the sphere's bbox grown by pad = pad_rel * (max|centre coord| + radius)
// and rounded outward; inner boxes are unions of their children.  The padding absorbs the rounding of
// the slab test and the "fuzz" of the reference's sphere test (BVH.hpp:251-267), so a sphere the
// brute-force loop would accept is never culled; with the (dist, prim index) lexicographic minimum as
// the closest-hit rule the result is then independent of visiting order and equals mode 0.
static inline float next_up(float x) { return nextafterf(x, INFINITY); }
static inline float next_dn(float x) { return nextafterf(x, -INFINITY); }
static void bvh_pad(BVH& bvh, const std::vector<Sphere>& prims, float pad_rel) {
	const size_t n = bvh.nodes.size();
	bvh.padded.assign(n, box_empty());
	bvh.pad_rel = pad_rel;
	for (size_t k = n; k-- > 0;) {
		const Node& nd = bvh.nodes[k];
		Box b = box_empty();
		if (nd.prim_count != 0) {
			for (uint32_t slot = nd.first_id; slot < nd.first_id + nd.prim_count; slot++) {
				const Sphere& s = prims[bvh.slot_prim.empty() ? slot : bvh.slot_prim[slot]];
				const float c[3] = { s.px, s.py, s.pz };
				const float r = sqrtf(s.radius_sq);
				const float amax = std_max(std_max(fabsf(c[0]), fabsf(c[1])), fabsf(c[2]));
				const float pad = pad_rel * (amax + r);
				for (int a = 0; a < 3; a++) {
					b.mn[a] = glm_min(b.mn[a], next_dn((c[a] - r) - pad));
					b.mx[a] = glm_max(b.mx[a], next_up((c[a] + r) + pad));
				}
			}
		} else {
			b = bvh.padded[nd.first_id];
			box_or(b, bvh.padded[nd.first_id + 1]);
		}
		bvh.padded[k] = b;
	}
}
// Optional: round every padded box outward to IEEE binary16 (lo toward -inf, hi toward +inf), as the product's 32-B
// half-precision records do (csrc/bvh_layout.hpp build_half_records); the values the slab test sees are then identical.
static void bvh_quantize_half(BVH& bvh) {
	for (Box& b : bvh.padded) for (int a = 0; a < 3; a++) {
		b.mn[a] = _cvtsh_ss(_cvtss_sh(b.mn[a], _MM_FROUND_TO_NEG_INF | _MM_FROUND_NO_EXC));
		b.mx[a] = _cvtsh_ss(_cvtss_sh(b.mx[a], _MM_FROUND_TO_POS_INF | _MM_FROUND_NO_EXC));
	}
}
// Conservative "cone" slab test.  The reference's sphere tests assume a unit direction (disc = b^2 - |oc|^2 + r^2,
// BVH.hpp:251-260,295-296), but its tangent frame is ill-conditioned near N.z = -1 (Sampling.hpp:150-159) and can hand
// back stretched directions; for such a ray a sphere the ray geometrically misses can still pass the test.  Algebra:
// with d the reported hit parameter, |p + d*D - c|^2 = r^2 + d^2 (|D|^2 - 1) (+ rounding), i.e. the reported hit point
// lies within d*sqrt(|D|^2-1) of the sphere.  So the boxes are tested against the ray inflated by alpha*t (L-inf) at
// parameter t, alpha^2 = max(|D|^2-1,0)*(1+2^-10) + g_cone_fuzz (rounding of the sphere arithmetic, relative to distance):
//     lo_i - alpha t <= p_i + t d_i <= hi_i + alpha t   <=>   t (d_i+alpha) >= lo_i - p_i  and  t (d_i-alpha) <= hi_i - p_i
// which is the usual slab test with reciprocal 1/(d_i+alpha) for the lo plane and 1/(d_i-alpha) for the hi plane; an
// axis with |d_i| <= alpha gives two lower bounds and is dropped (lo -> -inf, hi -> +inf).
static float g_cone_fuzz = 0x1p-19f;
struct RaySlab { float ia[3], na[3], ib[3], nb[3], c[3]; };
// Rays with alpha > kAlphaFat skip the tree: the product hands them to k_trace_fat, which runs the brute-force loops
// over all prims (csrc/kernels.hpp trav_begin / k_trace_fat); counters then grow by the prim count, no boxes.
static constexpr float kAlphaFat = 0.03f;
static inline RaySlab make_slab(float px, float py, float pz, float dx, float dy, float dz, bool* fat) {
	RaySlab s;
	const float L2 = (dx * dx + dy * dy) + dz * dz;
	const float a2 = fmaxf(L2 - 1.0f, 0.0f) * 1.0009765625f + g_cone_fuzz;
	const float alpha = sqrtf(a2) * 1.0009765625f;
	*fat = alpha > kAlphaFat;
	const float p[3] = { px, py, pz }, d[3] = { dx, dy, dz };
	for (int a = 0; a < 3; a++) {
		const float prod = (d[a] - alpha) * (d[a] + alpha);                // as slab_axis() in csrc/kernels.hpp
		if (prod == 0.0f) { s.ia[a] = 0.0f; s.ib[a] = 0.0f; s.na[a] = -INFINITY; s.nb[a] = INFINITY; }
		else {
			const float r = 1.0f / prod;
			s.ia[a] = (d[a] - alpha) * r; s.ib[a] = (d[a] + alpha) * r; s.na[a] = -(p[a] * s.ia[a]); s.nb[a] = -(p[a] * s.ib[a]);
		}
		s.c[a] = (prod < 0.0f) ? INFINITY : -INFINITY;                      // |d| < alpha: both planes bound t from below, no upper bound
	}
	return s;
}
// slab test on [0, tfar]; per axis enter = med3(l, h, c), leave = max3(l, h, c) with c = -inf (ordinary axis) or +inf
// (|d| < alpha), see kernels.hpp slab_hit(); no NaN reaches the selections
static inline float med3(float a, float b, float c) { return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c)); }
static inline bool slab_test(const RaySlab& s, const Box& b, float tfar, float* tnear) {
	const float lx = fmaf(b.mn[0], s.ia[0], s.na[0]), hx = fmaf(b.mx[0], s.ib[0], s.nb[0]);
	const float ly = fmaf(b.mn[1], s.ia[1], s.na[1]), hy = fmaf(b.mx[1], s.ib[1], s.nb[1]);
	const float lz = fmaf(b.mn[2], s.ia[2], s.na[2]), hz = fmaf(b.mx[2], s.ib[2], s.nb[2]);
	const float ex = med3(lx, hx, s.c[0]), ey = med3(ly, hy, s.c[1]), ez = med3(lz, hz, s.c[2]);
	const float ox = fmaxf(fmaxf(lx, hx), s.c[0]), oy = fmaxf(fmaxf(ly, hy), s.c[1]), oz = fmaxf(fmaxf(lz, hz), s.c[2]);
	const float tmin = fmaxf(fmaxf(ex, ey), fmaxf(ez, 0.0f));
	const float tmax = fminf(fminf(ox, oy), fminf(oz, tfar));
	*tnear = tmin;
	return tmin <= tmax;
}
// sphere_closest() with the order-independent acceptance rule
static inline void sphere_closest_tie(const Sphere& s, int32_t prim_ID, float px, float py, float pz,
                                      float dx, float dy, float dz, float* tfar, int32_t* primID) {
	float t = FLT_MAX; int32_t id = -1;
	sphere_closest(s, prim_ID, px, py, pz, dx, dy, dz, &t, &id);       // candidate against an open tfar
	if (id < 0) return;
	if (t < *tfar || (t == *tfar && (*primID < 0 || prim_ID < *primID))) { *tfar = t; *primID = prim_ID; }
}
// Same per-ray order as node_step() / leaf_step() in csrc/kernels.hpp: a depth-first walk whose stack items are inner nodes AND
// leaves.  At an inner node both child boxes are tested against the current tfar; of the hit children (leaf or not) the nearer
// is visited next and the other pushed; a leaf is intersected when it is visited, then the next item is popped.  (The root box
// itself is not tested.)
static inline void traverse_ray(const BVH& bvh, const std::vector<Sphere>& prims, float px, float py, float pz, float dx, float dy, float dz,
                                float* tfar, int32_t* primID, LocalCounters& lc) {
	bool fat;
	const RaySlab rs = make_slab(px, py, pz, dx, dy, dz, &fat);
	if (fat) {
		for (size_t p = 0; p < prims.size(); p++) sphere_closest_tie(prims[p], static_cast<int32_t>(p), px, py, pz, dx, dy, dz, tfar, primID);
		lc.spheres += prims.size();
		return;
	}
	auto leaf = [&](const Node& n) {
		for (uint32_t slot = n.first_id; slot < n.first_id + n.prim_count; slot++) {
			const uint32_t p = bvh.slot_prim.empty() ? slot : bvh.slot_prim[slot];
			lc.spheres++;
			sphere_closest_tie(prims[p], static_cast<int32_t>(p), px, py, pz, dx, dy, dz, tfar, primID);
		}
	};
	if (bvh.nodes[0].prim_count != 0) {            // single-leaf tree: the GPU record holds the leaf's box as child 0
		float t0; lc.nodes += bvh.wide ? 1 : 2;    // (the wide layout counts the slots in use, the binary one both children)
		if (slab_test(rs, bvh.padded[0], *tfar, &t0)) leaf(bvh.nodes[0]);
		return;
	}
	uint32_t stack[64]; size_t sp = 0;
	uint32_t id = 0;
	for (;;) {
		if (bvh.nodes[id].prim_count != 0) leaf(bvh.nodes[id]);
		else if (bvh.wide) {
			// node_step_wide() of csrc/kernels.hpp: the node stands for itself and its inner children — up to four kids, in the order
			// [children of c0 ..., children of c1 ...]; all are tested against the current tfar, the nearest hit one (lowest slot on ties)
			// is visited next, the other hit ones are pushed in slot order
			uint32_t kids[4]; int nk = 0;
			for (uint32_t c = bvh.nodes[id].first_id; c <= bvh.nodes[id].first_id + 1; c++) {
				if (bvh.nodes[c].prim_count == 0) { kids[nk++] = bvh.nodes[c].first_id; kids[nk++] = bvh.nodes[c].first_id + 1; }
				else kids[nk++] = c;
			}
			lc.nodes += static_cast<uint64_t>(nk);
			float t[4]; bool h[4]; int m = -1;
			for (int k = 0; k < nk; k++) { h[k] = slab_test(rs, bvh.padded[kids[k]], *tfar, &t[k]); if (h[k] && (m < 0 || t[k] < t[m])) m = k; }
			if (m >= 0) {
				for (int k = 0; k < nk; k++) if (h[k] && k != m) { if (sp >= 64) abort(); stack[sp++] = kids[k]; }
				id = kids[m];
				continue;
			}
		} else {
			const uint32_t c0 = bvh.nodes[id].first_id, c1 = c0 + 1;
			float ta, tb;
			lc.nodes += 2;
			const bool ha = slab_test(rs, bvh.padded[c0], *tfar, &ta);
			const bool hb = slab_test(rs, bvh.padded[c1], *tfar, &tb);
			if (ha && hb) {
				const bool a_first = ta <= tb;
				if (sp >= 64) abort();
				stack[sp++] = a_first ? c1 : c0;
				id = a_first ? c0 : c1;
				continue;
			}
			if (ha) { id = c0; continue; }
			if (hb) { id = c1; continue; }
		}
		if (sp == 0) return;
		id = stack[--sp];
	}
}
static inline bool traverse_ray_shadow(const BVH& bvh, const std::vector<Sphere>& prims, float px, float py, float pz, float dx, float dy, float dz,
                                       float tfar, LocalCounters& lc) {
	bool fat;
	const RaySlab rs = make_slab(px, py, pz, dx, dy, dz, &fat);
	if (fat) {
		bool occ = false;
		for (size_t p = 0; p < prims.size(); p++) occ |= sphere_occludes(prims[p], px, py, pz, dx, dy, dz, tfar);
		lc.shadow_spheres += prims.size();
		return occ;
	}
	auto leaf = [&](const Node& n) {
		for (uint32_t slot = n.first_id; slot < n.first_id + n.prim_count; slot++) {
			lc.shadow_spheres++;
			if (sphere_occludes(prims[bvh.slot_prim.empty() ? slot : bvh.slot_prim[slot]], px, py, pz, dx, dy, dz, tfar)) return true;
		}
		return false;
	};
	if (bvh.nodes[0].prim_count != 0) {
		float t0; lc.shadow_nodes += bvh.wide ? 1 : 2;
		return slab_test(rs, bvh.padded[0], tfar, &t0) && leaf(bvh.nodes[0]);
	}
	uint32_t stack[64]; size_t sp = 0;
	uint32_t id = 0;
	for (;;) {
		// the nearer hit child first, leaf or not (the order of node_step in csrc/kernels.hpp; any order gives the same answer).  Boxes
		// per shadow ray, nearer-first vs storage order, measured with leaves tested inside the node step: S(1000) 40.4 vs 39.9,
		// S(10000) 51.5 vs 54.5, S(100000) 61.1 vs 68.0 (the NEE rays of these scenes cross the sphere field towards one of a few
		// lights and ~80 % are occluded somewhere along the way: the order matters more the deeper the tree).
		if (bvh.nodes[id].prim_count != 0) { if (leaf(bvh.nodes[id])) return true; }
		else if (bvh.wide) {
			uint32_t kids[4]; int nk = 0;
			for (uint32_t c = bvh.nodes[id].first_id; c <= bvh.nodes[id].first_id + 1; c++) {
				if (bvh.nodes[c].prim_count == 0) { kids[nk++] = bvh.nodes[c].first_id; kids[nk++] = bvh.nodes[c].first_id + 1; }
				else kids[nk++] = c;
			}
			lc.shadow_nodes += static_cast<uint64_t>(nk);
			float t[4]; bool h[4]; int m = -1;
			for (int k = 0; k < nk; k++) { h[k] = slab_test(rs, bvh.padded[kids[k]], tfar, &t[k]); if (h[k] && (m < 0 || t[k] < t[m])) m = k; }
			if (m >= 0) {
				for (int k = 0; k < nk; k++) if (h[k] && k != m) { if (sp >= 64) abort(); stack[sp++] = kids[k]; }
				id = kids[m];
				continue;
			}
		} else {
			const uint32_t c0 = bvh.nodes[id].first_id, c1 = c0 + 1;
			float ta, tb;
			lc.shadow_nodes += 2;
			const bool ha = slab_test(rs, bvh.padded[c0], tfar, &ta);
			const bool hb = slab_test(rs, bvh.padded[c1], tfar, &tb);
			if (ha && hb) { const bool a_first = ta <= tb; if (sp >= 64) abort(); stack[sp++] = a_first ? c1 : c0; id = a_first ? c0 : c1; continue; }
			if (ha) { id = c0; continue; }
			if (hb) { id = c1; continue; }
		}
		if (sp == 0) return false;
		id = stack[--sp];
	}
}

// diagnostic (orc_wide_stats): what the same walk would cost on the tree collapsed to 4-wide (or 8-wide) nodes — every
// inner node absorbs its inner children (and theirs), the hit children of a wide node are visited nearest first, leaves are stack items as above.  Counts
// wide-node visits (= dependent record fetches per ray) and box tests; results are discarded.
static std::atomic<uint64_t> g_wide[6];           // closest: rays, visits, boxes; shadow: rays, visits, boxes
static bool g_wide_on = false;
static int g_wide_variant = 0;
static void wide_walk(const BVH& bvh, const std::vector<Sphere>& prims, float px, float py, float pz, float dx, float dy, float dz, float tfar_in, bool anyhit) {
	bool fat;
	const RaySlab rs = make_slab(px, py, pz, dx, dy, dz, &fat);
	if (fat || bvh.nodes.empty() || bvh.nodes[0].prim_count != 0) return;
	float tfar = tfar_in; int32_t primID = -1;
	uint64_t visits = 0, boxes = 0;
	uint32_t stack[256]; size_t sp = 0;
	uint32_t id = 0;
	for (;;) {
		const Node& n = bvh.nodes[id];
		if (n.prim_count != 0) {
			const uint32_t p = bvh.slot_prim.empty() ? n.first_id : bvh.slot_prim[n.first_id];
			if (anyhit) { if (sphere_occludes(prims[p], px, py, pz, dx, dy, dz, tfar)) break; }
			else sphere_closest_tie(prims[p], static_cast<int32_t>(p), px, py, pz, dx, dy, dz, &tfar, &primID);
		} else {
			uint32_t kids[8]; int nk = 0;
			kids[nk++] = n.first_id; kids[nk++] = n.first_id + 1;
			for (int level = 0; level < (g_wide_variant == 2 ? 2 : 1); level++) {         // absorb the inner kids once (4-wide) or twice (8-wide)
				uint32_t next[8]; int nn = 0;
				for (int k = 0; k < nk; k++) {
					if (bvh.nodes[kids[k]].prim_count == 0) { next[nn++] = bvh.nodes[kids[k]].first_id; next[nn++] = bvh.nodes[kids[k]].first_id + 1; }
					else next[nn++] = kids[k];
				}
				nk = nn; for (int k = 0; k < nk; k++) kids[k] = next[k];
			}
			visits++; boxes += static_cast<uint64_t>(nk);
			float t[8]; uint32_t hit[8]; int nh = 0;
			for (int k = 0; k < nk; k++) { float tn; if (slab_test(rs, bvh.padded[kids[k]], tfar, &tn)) { t[nh] = tn; hit[nh] = kids[k]; nh++; } }
			if (g_wide_variant != 1) { for (int a = 1; a < nh; a++) for (int b = a; b > 0 && t[b] < t[b - 1]; b--) { std::swap(t[b], t[b - 1]); std::swap(hit[b], hit[b - 1]); } }
			else { int m = 0; for (int a = 1; a < nh; a++) if (t[a] < t[m]) m = a; if (nh) { std::swap(t[0], t[m]); std::swap(hit[0], hit[m]); } }     // nearest first, the rest as stored
			for (int k = nh - 1; k >= 1; k--) if (sp < 256) stack[sp++] = hit[k];
			if (nh) { id = hit[0]; continue; }
		}
		if (sp == 0) break;
		id = stack[--sp];
	}
	const int o = anyhit ? 3 : 0;
	g_wide[o]++; g_wide[o + 1] += visits; g_wide[o + 2] += boxes;
}

// ---------------------------------------------------------------------------------
// Oracle context
// ---------------------------------------------------------------------------------
struct Oracle {
	std::vector<Sphere> geometry;
	std::vector<Material> material;
	std::vector<int32_t> lights;          // Scene.hpp:9-17
	Camera camera;
	Sky sky;
	BVH bvh;                              // the reference's tree (BVH.hpp:90-206): modes 0 and 1, and the prim order of every mode
	BVH accel;                            // mode 2: the tree the HIP kernels traverse (internal SAH tree, or a copy of `bvh`)
	bool accel_internal = true, accel_half = false, accel_wide = false;
	uint32_t width = 0, height = 0, h_tiles = 0, v_tiles = 0;
	uint32_t accumulations = 0;
	uint32_t max_bounces = 16;            // Renderer.hpp:24
	uint32_t buckets = 5;                 // Renderer.hpp:41
	int mis = 1;                          // Renderer.hpp:71
	int trav_mode = 0;
	int threads = 0;
	int brdf = 0;                         // Renderer.hpp:70 `#define BRDF`: 0 Closure<LambertianDiffuse>, 1 Closure<GGX>
	std::vector<float> gloss_decay;       // gloss_decay_table by bounce (named at Renderer.hpp:212, never declared); entries beyond its length are 0
	uint32_t light_ris = 0;               // orc_set_light_ris: 0 = the reference's one light sample; 1..32 = candidates of the project's RIS (below)
	float lens_aperture = 0.0f, lens_focus_depth = 0.0f;   // orc_set_lens: aperture 0 = the reference's pinhole camera
	std::vector<float> accumulator;       // [tile][bucket][channel][256]  (Renderer.hpp:43-46)
	std::vector<uint32_t> tile_list;      // orc_set_tile_list: only these LaunchIndices are rendered (full-size spot checks); slab j = tile_list[j]
	Counters counters;
};

// diagnostic (DESIGN.md "Traversal semantics"): histogram of |D|^2 - 1 over all rays handed to traverse() (orc_len_hist)
static std::atomic<uint64_t> g_len_hist[16];
static bool g_len_hist_on = false;
static void traverse(const Oracle& o, const Buffer& in, Hit& out, size_t size, LocalCounters& lc) {
	if (g_len_hist_on) for (size_t i = 0; i < size; i++) {
		const float L2 = (in.dir.x[i] * in.dir.x[i] + in.dir.y[i] * in.dir.y[i]) + in.dir.z[i] * in.dir.z[i];
		const float e = fabsf(L2 - 1.0f);
		int b = 0; float th = 1e-7f; while (b < 15 && e > th) { th *= 3.1622776f; b++; }
		g_len_hist[b * 1 + 0]++;
	}         // BVH.hpp:309-360
	lc.rays += size;
	if (o.trav_mode == 0) {
		intersect_prims(o.bvh, in, out, 0, size, 0, o.bvh.prims.size(), lc);
	} else if (o.trav_mode == 1) {
		if (!o.bvh.nodes.empty()) traverse_stream(o.bvh, in, out, size, lc);
	} else {
		if (!o.accel.nodes.empty())
			for (size_t i = 0; i < size; i++) {
				if (g_wide_on) wide_walk(o.accel, o.bvh.prims, in.p.x[i], in.p.y[i], in.p.z[i], in.dir.x[i], in.dir.y[i], in.dir.z[i], out.tfar[i], false);
				traverse_ray(o.accel, o.bvh.prims, in.p.x[i], in.p.y[i], in.p.z[i], in.dir.x[i], in.dir.y[i], in.dir.z[i], &out.tfar[i], &out.primID[i], lc);
			}
	}
	for (size_t i = 0; i < size; i++)                                                                          // :313-317 / :350-354
		if (int32_t primID = out.primID[i]; primID >= 0) out.matID[i] = o.bvh.prims[primID].material_ID;
}
static void traverse_shadow(const Oracle& o, ShadowStream& in, size_t size, LocalCounters& lc) {             // BVH.hpp:362-404
	lc.shadow_rays += size;
	if (o.trav_mode == 0) {
		intersect_prims_shadow(o.bvh, in, 0, size, 0, o.bvh.prims.size(), lc);
	} else if (o.trav_mode == 1) {
		if (!o.bvh.nodes.empty()) traverse_stream_shadow(o.bvh, in, size, lc);
	} else {
		if (!o.accel.nodes.empty())
			for (size_t i = 0; i < size; i++) {
				if (g_wide_on) wide_walk(o.accel, o.bvh.prims, in.p.x[i], in.p.y[i], in.p.z[i], in.dir.x[i], in.dir.y[i], in.dir.z[i], in.tfar[i], true);
				if (traverse_ray_shadow(o.accel, o.bvh.prims, in.p.x[i], in.p.y[i], in.p.z[i], in.dir.x[i], in.dir.y[i], in.dir.z[i], in.tfar[i], lc))
					in.occluded.set(i);
			}
	}
}

// DataStreams.hpp:221-253
static size_t sort_rayID(uint32_t k, uint32_t count, uint32_t* out, const int32_t* key, uint16_t* sort_buffer) {
	for (uint32_t i = 0; i < count; i++) ++sort_buffer[key[i] + 1];           // histogram(key, sort_buffer + 1, count)
	size_t ret = sort_buffer[0];
	for (uint32_t i = 1; i < k + 1; i++) sort_buffer[i] += sort_buffer[i - 1]; // prefix_sum(sort_buffer, k + 1)
	for (int32_t i = static_cast<int32_t>(count) - 1; i >= 0; i--) out[--sort_buffer[key[i] + 1]] = static_cast<uint32_t>(i);
	return ret;
}

// Debug hook (orc_debug_path): records, for one pixel of one tile, the ray and its hit at every bounce.
// With light RIS it also records every candidate of that pixel: bounce, candidate, the reservoir draw r, the weight w (0: left early).
struct PathDebug { bool on = false; uint32_t px = 0; int n = 0; float rec[64][8]; int n_cand = 0; float cand[256][4]; };
static thread_local PathDebug g_dbg;

// THE PROJECT'S OWN DEFINITION, not a restatement of the reference (Camera.hpp:80-88 ignores its lens fields): the thin-lens
// ray of csrc/device_math.hpp lens_ray, derived from the pinhole direction d of generate_ray_dir.  Binary32, one rounding per operation
// (-ffp-contract=off), spelled as tests/lens_twin.py's docstring spells it:
//   rng = hash_2d(acc, seed + 2 * max_bounces);  u0, u1 = rand_unit_float twice;  (lx, ly) = disk(u0, u1)
//   t = focus_depth / dot3(d, fwd);  P = pos + d * t;  ax = A * lx;  ay = A * ly;  O = pos + (right * ax + up * ay);  D = normalize3(P - O)
// right / up / fwd = the camera's +x, +y, -z under quat_rotate, the same formula generate_ray_dir rotates with.
static inline void lens_ray(const Oracle& o, v3 d, uint32_t accumulations, uint32_t seed, v3* O, v3* D) {
	const v3 right = quat_rotate(o.camera.orient, v3{ 1.0f, 0.0f, 0.0f }), up = quat_rotate(o.camera.orient, v3{ 0.0f, 1.0f, 0.0f });
	const v3 fwd = quat_rotate(o.camera.orient, v3{ 0.0f, 0.0f, -1.0f });
	uint32_t rng = hash_2d(accumulations, seed + 2u * o.max_bounces);
	const float u0 = rand_unit_float(&rng);
	const float u1 = rand_unit_float(&rng);
	float lx, ly; disk(u0, u1, &lx, &ly);
	const float t = o.lens_focus_depth / dot3(d, fwd);
	const v3 pos = o.camera.pos;
	const v3 P{ pos.x + d.x * t, pos.y + d.y * t, pos.z + d.z * t };
	const float ax = o.lens_aperture * lx, ay = o.lens_aperture * ly;
	*O = v3{ pos.x + (right.x * ax + up.x * ay), pos.y + (right.y * ax + up.y * ay), pos.z + (right.z * ax + up.z * ay) };
	*D = normalize3(v3{ P.x - O->x, P.y - O->y, P.z - O->z });
}

// Renderer.hpp:83-432 — one tile, one Accumulate() call, with the closure the reference selects at compile time (Renderer.hpp:70)
template <bool GGX>
static void accumulate_tile_closure(const Oracle& o, uint32_t LaunchIndex, size_t slab, uint32_t accumulations, float* accumulator, LocalCounters& lc) {
	const uint32_t light_count = static_cast<uint32_t>(o.lights.size());
	const float light_selection_pdf = 1.0f / static_cast<float>(o.lights.size());
	const bool has_ambient = std_max(o.sky.ambient[0], std_max(o.sky.ambient[1], o.sky.ambient[2])) > 0.0f;
	const uint32_t bucket_index = accumulations % o.buckets;
	// Q12 guard: no lights => NEE is skipped and the non-MIS emissive branch is taken (reference behaviour is UB there).
	const bool MIS = o.mis && light_count > 0;

	float* out_r = accumulator + (slab * o.buckets + bucket_index) * 3 * TileSize;     // slab == LaunchIndex unless a tile list is set
	float* out_g = out_r + TileSize;
	float* out_b = out_g + TileSize;
	const int32_t tile_x = static_cast<int32_t>(TileRoot * (LaunchIndex % o.h_tiles));
	const int32_t tile_y = static_cast<int32_t>(TileRoot * (LaunchIndex / o.h_tiles));

	static thread_local RayStream ray_stream;
	static thread_local ShaderData sd;
	uint16_t sort_buffer[MaxMaterialID + 2];
	Buffer* in = &ray_stream.buffers[0];
	Buffer* outb = &ray_stream.buffers[1];

	for (size_t i = 0; i < N; i++) {                                            // :97-109
		in->radiance.r[i] = in->radiance.g[i] = in->radiance.b[i] = 0.0f;
		in->throughput.r[i] = in->throughput.g[i] = in->throughput.b[i] = 1.0f;
		in->pixelID[i] = static_cast<uint32_t>(i);
		ray_stream.seed[i] = static_cast<uint32_t>(static_cast<int32_t>((LaunchIndex * TileSize + i) * (o.max_bounces * 2 + 1)));
	}
	for (size_t ID = 0; ID < TileSize; ID++) {                                  // :113-127
		int32_t x = tile_x + static_cast<int32_t>(ID) % static_cast<int32_t>(TileRoot);
		int32_t y = tile_y + static_cast<int32_t>(ID) / static_cast<int32_t>(TileRoot);
		uint32_t rng_state = hash_2d(accumulations, ray_stream.seed[ID]);
		float cs[2]; cs[0] = rand_unit_float(&rng_state); cs[1] = rand_unit_float(&rng_state);
		v3 dir = generate_ray_dir(o.camera, x, y, cs);
		v3 origin = o.camera.pos;
		if (o.lens_aperture > 0.0f) lens_ray(o, dir, accumulations, ray_stream.seed[ID], &origin, &dir);   // the project's lens; 0 = the line above alone
		in->dir.x[ID] = dir.x; in->dir.y[ID] = dir.y; in->dir.z[ID] = dir.z;
		in->p.x[ID] = origin.x; in->p.y[ID] = origin.y; in->p.z[ID] = origin.z;
	}
	size_t active_rays = N;
	for (size_t bounce = 0; bounce < o.max_bounces && active_rays > 0; bounce++, std::swap(in, outb)) {   // :131
		ray_stream.termination.zero(); ray_stream.has_shadowray.zero();         // :135-140
		ray_stream.shadow_rays.occluded.zero(); sd.is_emissive.zero();
		memset(sort_buffer, 0, sizeof sort_buffer);                             // :141-149
		for (size_t i = 0; i < ((active_rays + 7) / 8) * 8; i++) {              // :150-158
			ray_stream.hit.tfar[i] = FLT_MAX; ray_stream.hit.matID[i] = -1; ray_stream.hit.primID[i] = -1;
		}
		traverse(o, *in, ray_stream.hit, active_rays, lc);                      // :165
		if (g_dbg.on) for (size_t ID = 0; ID < active_rays; ID++) if (in->pixelID[ID] == g_dbg.px && g_dbg.n < 64) {
			float* r = g_dbg.rec[g_dbg.n++];
			r[0] = in->p.x[ID]; r[1] = in->p.y[ID]; r[2] = in->p.z[ID]; r[3] = in->dir.x[ID]; r[4] = in->dir.y[ID]; r[5] = in->dir.z[ID];
			r[6] = ray_stream.hit.tfar[ID]; r[7] = static_cast<float>(ray_stream.hit.primID[ID]);
		}
		const float decay = bounce < o.gloss_decay.size() ? o.gloss_decay[bounce] : 0.0f;

		for (size_t ID = 0; ID < active_rays; ID++) {                           // :169-214 closest-hit shader
			const int32_t mat_ID = ray_stream.hit.matID[ID];
			if (mat_ID == -1) continue;
			const int32_t prim_ID = ray_stream.hit.primID[ID];
			const float depth = ray_stream.hit.tfar[ID];
			const v3 D{ in->dir.x[ID], in->dir.y[ID], in->dir.z[ID] };
			v3 hit_point{ in->p.x[ID] + D.x * depth, in->p.y[ID] + D.y * depth, in->p.z[ID] + D.z * depth };
			const Sphere& hp = o.bvh.prims[prim_ID];
			v3 Nn{ hit_point.x - hp.px, hit_point.y - hp.py, hit_point.z - hp.pz };
			Nn = normalize3(Nn);
			if (dot3(Nn, D) >= 0.0f) Nn = v3{ -Nn.x, -Nn.y, -Nn.z };
			q4 T = tangent_space(Nn);
			v3 Vlocal = to_local(T, v3{ -D.x, -D.y, -D.z });
			sd.P.x[ID] = hit_point.x + Nn.x * 1e-4f;
			sd.P.y[ID] = hit_point.y + Nn.y * 1e-4f;
			sd.P.z[ID] = hit_point.z + Nn.z * 1e-4f;
			sd.V.x[ID] = Vlocal.x; sd.V.y[ID] = Vlocal.y; sd.V.z[ID] = Vlocal.z;
			sd.T.x[ID] = T.x; sd.T.y[ID] = T.y; sd.T.z[ID] = T.z; sd.T.w[ID] = T.w;
			const Material& m = o.material[mat_ID];
			if (std_max(m.emission[0], std_max(m.emission[1], m.emission[2])) > FLT_EPSILON) sd.is_emissive.set(ID);
			if (GGX) {                                                           // :209-212
				sd.F0[ID][0] = m.F0[0]; sd.F0[ID][1] = m.F0[1]; sd.F0[ID][2] = m.F0[2];
				float alpha = m.roughness; alpha *= alpha;
				sd.alpha[ID] = alpha + (1.0f - alpha) * decay;
			} else {                                                             // :207-208
				sd.albedo[ID][0] = m.albedo[0]; sd.albedo[ID][1] = m.albedo[1]; sd.albedo[ID][2] = m.albedo[2];
			}
		}
		const size_t miss_count = sort_rayID(static_cast<uint32_t>(o.material.size()), static_cast<uint32_t>(active_rays),
		                                     ray_stream.RayID, ray_stream.hit.matID, sort_buffer);   // :235-241
		const size_t hit_count = active_rays - miss_count;

		// Twin mode only: hits of the LAST bounce are never accumulated (Q5: Renderer.hpp:358,424-425 drops them), so the product
		// emits no NEE rays for them; the reference (modes 0, 1) still traces those shadow rays.  Skipping them changes no result,
		// only the shadow-ray / box / sphere counters, which in mode 2 mirror the HIP kernels'.
		const bool skip_dropped_nee = o.trav_mode == 2 && !(bounce < o.max_bounces - 1);
		if (MIS && !skip_dropped_nee) {                                          // :247-315
			size_t shadow_index = 0;
			ShadowStream& sh = ray_stream.shadow_rays;
			// The light sample of one hit, Renderer.hpp:261-296: ONE text for the plain draw and for every RIS candidate (as csrc/nee_sample_body.inc
			// is on the device).  false: the sample left early and weighs nothing; true: direction, distance and MIS-weighted radiance of its shadow ray.
			auto light_sample = [&](int32_t ID, int32_t selected_light, float u0, float u1, v3& L, float& light_distance, v3& radiance) -> bool {
				int32_t light_primID = o.lights[selected_light];
				const Sphere& light_prim = o.geometry[light_primID];
				if (light_primID == ray_stream.hit.primID[ID]) return false;          // Q11: geometry-order vs BVH-order index
				v3 Wc{ light_prim.px - sd.P.x[ID], light_prim.py - sd.P.y[ID], light_prim.pz - sd.P.z[ID] };
				float center_dist2 = dot3(Wc, Wc);
				if (center_dist2 <= light_prim.radius_sq) return false;
				float center_dist = sqrtf(center_dist2);
				{ float inv = 1.0f / center_dist; Wc.x *= inv; Wc.y *= inv; Wc.z *= inv; }
				float sinThetaMax2 = light_prim.radius_sq / center_dist2;
				{
					float NdotW = (2.0f * sd.T.w[ID]) * (Wc.z * sd.T.w[ID] + Wc.x * sd.T.y[ID] - sd.T.x[ID] * Wc.y) - Wc.z;
					if (NdotW < 0.0f && sinThetaMax2 < NdotW * NdotW) return false;
				}
				float light_pdf;
				L = sample_direction_to_sphere(Wc, sinThetaMax2, center_dist, light_prim.radius_sq, u0, u1, &light_distance, &light_pdf);
				q4 T{ sd.T.x[ID], sd.T.y[ID], sd.T.z[ID], sd.T.w[ID] };
				v3 Llocal = to_local(T, L);
				if (Llocal.z < 0.0f) return false;
				const Material& lm = o.material[light_prim.material_ID];
				radiance = v3{ lm.emission[0] * in->throughput.r[ID], lm.emission[1] * in->throughput.g[ID], lm.emission[2] * in->throughput.b[ID] };
				float brdf_pdf;
				if (GGX) {                                                       // Closure<GGX>::eval / pdf, DataStreams.hpp:189-198
					const v3 f = ggx_eval(v3{ sd.F0[ID][0], sd.F0[ID][1], sd.F0[ID][2] }, sd.alpha[ID], Llocal, v3{ sd.V.x[ID], sd.V.y[ID], sd.V.z[ID] });
					radiance.x *= f.x; radiance.y *= f.y; radiance.z *= f.z;
					brdf_pdf = 0.0f;                                             // "TODO" in the reference
				} else {                                                         // Closure<Lambertian>::eval / pdf, DataStreams.hpp:169-176
					float NdotL = std_max(0.0f, Llocal.z);
					float f = kOneOverPi * NdotL;
					radiance.x *= sd.albedo[ID][0] * f; radiance.y *= sd.albedo[ID][1] * f; radiance.z *= sd.albedo[ID][2] * f;
					brdf_pdf = kOneOverPi * std_max(0.0f, Llocal.z);
				}
				light_pdf *= light_selection_pdf;
				float w = powerHeuristic_over_f(light_pdf, brdf_pdf);
				radiance.x *= w; radiance.y *= w; radiance.z *= w;
				if (std_max(std_max(radiance.x, radiance.y), radiance.z) <= 0.0f) return false;
				return true;
			};
			for (size_t i = 0; i < hit_count; i++) {
				const int32_t ID = static_cast<int32_t>(ray_stream.RayID[miss_count + i]);
				uint32_t rng_state = hash_2d(accumulations, ray_stream.seed[in->pixelID[ID]] + static_cast<uint32_t>(bounce) * 2);
				v3 L{ 0.0f, 0.0f, 0.0f }, radiance{ 0.0f, 0.0f, 0.0f }; float light_distance = 0.0f;
				if (o.light_ris == 0) {
					float ls[2]; ls[0] = rand_unit_float(&rng_state); ls[1] = rand_unit_float(&rng_state);
					int32_t selected_light = static_cast<int32_t>(rand_bounded_int(&rng_state, light_count));
					if (!light_sample(ID, selected_light, ls[0], ls[1], L, light_distance, radiance)) continue;
				} else {
					// THE PROJECT'S OWN DEFINITION, not a line-cited restatement of the reference:
					// DESIGN.md "NEE light by resampled importance sampling", Estimator and Anchor; the device text is csrc/shade_hit_body.inc.
					// M candidates continue the plain draw's generator; each draws u0, u1, the light and the reservoir's r, in that order, whether or
					// not it survives.  Binary32 weighted reservoir: w = max(rad.rgb); weight_sum += w; take it when weight_sum == w (the first
					// positive one, whatever r: rand_unit_float reaches 1.0f) or r < w / weight_sum; the kept radiance is scaled by
					// weight_sum / (float(M) * w_sel).  Nothing kept: no shadow ray.
					float weight_sum = 0.0f, w_sel = 0.0f;
					for (uint32_t cand = 0; cand < o.light_ris; cand++) {
						const float u0 = rand_unit_float(&rng_state);
						const float u1 = rand_unit_float(&rng_state);
						const int32_t selected_light = static_cast<int32_t>(rand_bounded_int(&rng_state, light_count));
						const float r = rand_unit_float(&rng_state);
						v3 Lc{ 0.0f, 0.0f, 0.0f }, rc{ 0.0f, 0.0f, 0.0f }; float dc = 0.0f, w = 0.0f;
						if (light_sample(ID, selected_light, u0, u1, Lc, dc, rc)) {
							w = std_max(std_max(rc.x, rc.y), rc.z);
							weight_sum += w;
							if (weight_sum == w || r < w / weight_sum) { w_sel = w; L = Lc; light_distance = dc; radiance = rc; }
						}
						if (g_dbg.on && in->pixelID[ID] == g_dbg.px && g_dbg.n_cand < 256) {
							float* c = g_dbg.cand[g_dbg.n_cand++];
							c[0] = static_cast<float>(bounce); c[1] = static_cast<float>(cand); c[2] = r; c[3] = w;
						}
					}
					if (!(w_sel > 0.0f)) continue;
					const float k = weight_sum / (static_cast<float>(o.light_ris) * w_sel);
					radiance = v3{ radiance.x * k, radiance.y * k, radiance.z * k };
				}
				sh.dir.x[shadow_index] = L.x; sh.dir.y[shadow_index] = L.y; sh.dir.z[shadow_index] = L.z;
				sh.p.x[shadow_index] = sd.P.x[ID]; sh.p.y[shadow_index] = sd.P.y[ID]; sh.p.z[shadow_index] = sd.P.z[ID];
				sh.tfar[shadow_index] = light_distance;
				sh.radiance.r[shadow_index] = radiance.x; sh.radiance.g[shadow_index] = radiance.y; sh.radiance.b[shadow_index] = radiance.z;
				ray_stream.has_shadowray.set(ID);
				++shadow_index;
			}
			traverse_shadow(o, sh, shadow_index, lc);                            // :302
			for (size_t i = miss_count, shadow_ID = 0; i < active_rays; i++) {   // :304-314
				const int32_t ID = static_cast<int32_t>(ray_stream.RayID[i]);
				if (ray_stream.has_shadowray.test(ID)) {
					if (!sh.occluded.test(shadow_ID)) {
						in->radiance.r[ID] += sh.radiance.r[shadow_ID];
						in->radiance.g[ID] += sh.radiance.g[shadow_ID];
						in->radiance.b[ID] += sh.radiance.b[shadow_ID];
					}
					++shadow_ID;
				}
			}
		}
		if (MIS && bounce > 0) {                                                 // :319-343 (in->pdf: the previous bounce's closure pdf)
			for (size_t ID = 0; ID < active_rays; ID++) {
				if (!sd.is_emissive.test(ID)) continue;
				v3 throughput{ in->throughput.r[ID], in->throughput.g[ID], in->throughput.b[ID] };
				const Sphere& light_prim = o.bvh.prims[ray_stream.hit.primID[ID]];
				const float radius2 = light_prim.radius_sq;
				const float depth = ray_stream.hit.tfar[ID];
				const float NdotV = sd.V.z[ID];
				float center_dist2 = depth * (depth + NdotV * (2.0f * sqrtf(radius2))) + radius2;
				float weight = powerHeuristic(in->pdf[ID], light_selection_pdf * spherePdf(radius2, center_dist2));
				throughput.x *= weight; throughput.y *= weight; throughput.z *= weight;
				const float* em = o.material[ray_stream.hit.matID[ID]].emission;
				in->radiance.r[ID] += throughput.x * em[0];
				in->radiance.g[ID] += throughput.y * em[1];
				in->radiance.b[ID] += throughput.z * em[2];
			}
		} else {                                                                 // :344-353 (Q9: no throughput)
			for (size_t ID = 0; ID < active_rays; ID++) {
				if (!sd.is_emissive.test(ID)) continue;
				const float* em = o.material[ray_stream.hit.matID[ID]].emission;
				in->radiance.r[ID] += em[0]; in->radiance.g[ID] += em[1]; in->radiance.b[ID] += em[2];
			}
		}
		size_t output_index = 0;                                                 // :357-404
		if (bounce < o.max_bounces - 1) {
			for (size_t i = 0; i < hit_count; i++) {
				const int32_t ID = static_cast<int32_t>(ray_stream.RayID[miss_count + i]);
				uint32_t rng_state = hash_2d(accumulations, ray_stream.seed[in->pixelID[ID]] + static_cast<uint32_t>(bounce) * 2 + 1);
				float bs[2]; bs[0] = rand_unit_float(&rng_state); bs[1] = rand_unit_float(&rng_state);
				v3 sdir, estimator;
				if (GGX) {                                                       // Closure<GGX>::sample, DataStreams.hpp:200-218
					ggx_sample(v3{ sd.F0[ID][0], sd.F0[ID][1], sd.F0[ID][2] }, sd.alpha[ID], v3{ sd.V.x[ID], sd.V.y[ID], sd.V.z[ID] }, bs[0], bs[1], &sdir, &estimator);
				} else {                                                         // DataStreams.hpp:177-181
					sdir = hemisphere(bs[0], bs[1]);
					estimator = v3{ sd.albedo[ID][0], sd.albedo[ID][1], sd.albedo[ID][2] };
				}
				v3 throughput{ in->throughput.r[ID] * estimator.x, in->throughput.g[ID] * estimator.y, in->throughput.b[ID] * estimator.z };
				{
					float q = 1.0f - std_max(throughput.x, std_max(throughput.y, throughput.z));
					if (rand_unit_float(&rng_state) < q) { ray_stream.termination.set(ID); continue; }
					float inv = 1.0f / std_max(FLT_EPSILON, 1.0f - q);
					throughput.x *= inv; throughput.y *= inv; throughput.z *= inv;
				}
				q4 T{ sd.T.x[ID], sd.T.y[ID], sd.T.z[ID], sd.T.w[ID] };
				sdir = to_world(T, sdir);
				outb->p.x[output_index] = sd.P.x[ID]; outb->p.y[output_index] = sd.P.y[ID]; outb->p.z[output_index] = sd.P.z[ID];
				outb->dir.x[output_index] = sdir.x; outb->dir.y[output_index] = sdir.y; outb->dir.z[output_index] = sdir.z;
				outb->throughput.r[output_index] = throughput.x; outb->throughput.g[output_index] = throughput.y; outb->throughput.b[output_index] = throughput.z;
				outb->radiance.r[output_index] = in->radiance.r[ID]; outb->radiance.g[output_index] = in->radiance.g[ID]; outb->radiance.b[output_index] = in->radiance.b[ID];
				outb->pixelID[output_index] = in->pixelID[ID];
				// :401 — Closure<GGX>::pdf = 0 ("TODO", DataStreams.hpp:196-198); Lambertian: Q8, pdf of the WORLD-space dir
				outb->pdf[output_index] = GGX ? 0.0f : kOneOverPi * std_max(0.0f, sdir.z);
				output_index++;
			}
		}
		for (size_t i = 0; i < miss_count; i++) ray_stream.termination.set(ray_stream.RayID[i]);   // :408-410
		if (has_ambient) {                                                       // :411-420 (Q10: throughput.r for all channels)
			for (size_t i = 0; i < miss_count; i++) {
				const int32_t ID = static_cast<int32_t>(ray_stream.RayID[i]);
				v3 sky_value = sky_eval(o.sky, in->dir.x[ID], in->dir.y[ID], in->dir.z[ID]);
				in->radiance.r[ID] += in->throughput.r[ID] * sky_value.x;
				in->radiance.g[ID] += in->throughput.r[ID] * sky_value.y;
				in->radiance.b[ID] += in->throughput.r[ID] * sky_value.z;
			}
		}
		for (size_t ID = 0; ID < active_rays; ID++) {                            // :424-430
			if (!ray_stream.termination.test(ID)) continue;
			const uint32_t px = in->pixelID[ID];
			out_r[px] += in->radiance.r[ID];
			out_g[px] += in->radiance.g[ID];
			out_b[px] += in->radiance.b[ID];
			lc.terminated++;
		}
		active_rays = output_index;                                              // :431
	}
}

// The reference's `#define BRDF` as oracle state: accumulate() and orc_debug_path both come through here.
static void accumulate_tile(const Oracle& o, uint32_t LaunchIndex, size_t slab, uint32_t accumulations, float* accumulator, LocalCounters& lc) {
	if (o.brdf == 1) accumulate_tile_closure<true>(o, LaunchIndex, slab, accumulations, accumulator, lc);
	else accumulate_tile_closure<false>(o, LaunchIndex, slab, accumulations, accumulator, lc);
}

static void flush(Counters& c, const LocalCounters& lc) {
	c.rays += lc.rays; c.shadow_rays += lc.shadow_rays; c.nodes += lc.nodes; c.spheres += lc.spheres;
	c.shadow_nodes += lc.shadow_nodes; c.shadow_spheres += lc.shadow_spheres; c.terminated += lc.terminated;
}

static void accumulate(Oracle& o) {                                               // Renderer.hpp:73-75,433
	++o.accumulations;
	const uint32_t tiles = o.tile_list.empty() ? o.h_tiles * o.v_tiles : static_cast<uint32_t>(o.tile_list.size());
	int nthreads = o.threads > 0 ? o.threads : static_cast<int>(std::thread::hardware_concurrency());
	if (nthreads < 1) nthreads = 1;
	if (static_cast<uint32_t>(nthreads) > tiles) nthreads = static_cast<int>(tiles ? tiles : 1);
	std::atomic<uint32_t> next{0};
	auto worker = [&]() {
		LocalCounters lc;
		for (;;) {
			uint32_t t = next.fetch_add(1);
			if (t >= tiles) break;
			accumulate_tile(o, o.tile_list.empty() ? t : o.tile_list[t], t, o.accumulations, o.accumulator.data(), lc);
		}
		flush(o.counters, lc);
	};
	if (nthreads == 1) { worker(); return; }
	std::vector<std::thread> pool;
	for (int i = 0; i < nthreads; i++) pool.emplace_back(worker);
	for (auto& t : pool) t.join();
}

// Renderer.hpp:436-478.  k==5 is the reference; other k is this project's generalisation (Q19):
// odd k -> middle order statistic, even k -> mean of the two middle ones.
static float median_k(float* v, uint32_t k) {
	if (k == 5) return median5(v[0], v[1], v[2], v[3], v[4]);
	std::sort(v, v + k);
	if (k & 1) return v[k / 2];
	return (v[k / 2 - 1] + v[k / 2]) * 0.5f;
}
static int render(const Oracle& o, float* rgba) {
	if (!o.tile_list.empty()) return -1;                                          // a tile subset has no frame
	if (o.accumulations % o.buckets) return 1;                                    // :437
	const float scale = o.camera.exposure / static_cast<float>(o.accumulations / o.buckets);   // :439
	const uint32_t tiles = o.h_tiles * o.v_tiles;
	for (uint32_t t = 0; t < tiles; t++) {
		const float* src = o.accumulator.data() + static_cast<size_t>(t) * o.buckets * 3 * TileSize;
		for (uint32_t px = 0; px < TileSize; px++) {
			float ch[3];
			for (uint32_t c = 0; c < 3; c++) {
				float v[64];
				for (uint32_t b = 0; b < o.buckets; b++) v[b] = src[(static_cast<size_t>(b) * 3 + c) * TileSize + px];
				ch[c] = scale * median_k(v, o.buckets);                              // :453-455
			}
			tonemapping(ch[0], ch[1], ch[2]);                                        // :461
			const uint32_t x = TileRoot * (t % o.h_tiles) + px % TileRoot;
			const uint32_t y = TileRoot * (t / o.h_tiles) + px / TileRoot;
			float* dst = rgba + 4 * (static_cast<size_t>(y) * o.width + x);           // :447
			dst[0] = ch[0]; dst[1] = ch[1]; dst[2] = ch[2]; dst[3] = 1.0f;             // :465
		}
	}
	return 0;
}

} // namespace

// ---------------------------------------------------------------------------------
// C interface for ctypes (tests / smoke / bench cpu_baseline only)
// ---------------------------------------------------------------------------------
// Mode-2 traversal tree = what csrc/mirt_capi.hip lays out for the GPU: by default an internal SAH tree (true half-area
// cost) over the reference tree's prims, or the reference tree itself; boxes padded, optionally rounded outward to binary16.
static void build_accel(Oracle& o) {
	o.accel = BVH{};
	if (o.accel_internal) {
		g_true_half_area = true;
		BVH tmp; std::vector<uint32_t> order;
		bvh_build(o.bvh.prims, tmp, &order);
		g_true_half_area = false;
		o.accel.nodes = tmp.nodes; o.accel.slot_prim = order;
	} else {
		o.accel.nodes = o.bvh.nodes;
	}
	bvh_pad(o.accel, o.bvh.prims, 0x1p-18f);
	if (o.accel_half) bvh_quantize_half(o.accel);
	o.accel.wide = o.accel_wide;
}

extern "C" {

void* orc_create() { return new Oracle(); }
void orc_destroy(void* h) { delete static_cast<Oracle*>(h); }

// Application.cpp:230-234 — takes the authored scene, builds BVH (BVH.hpp:90-206) and light list (Scene.hpp:12-16).
int orc_set_scene(void* h, const void* geometry, int n, const void* materials, int n_mat,
                  const float* ambient, const float* hdri_rgba, int hdri_w, int hdri_h) {
	Oracle& o = *static_cast<Oracle*>(h);
	o.geometry.resize(n); if (n) memcpy(o.geometry.data(), geometry, sizeof(Sphere) * n);
	o.material.resize(n_mat); if (n_mat) memcpy(o.material.data(), materials, sizeof(Material) * n_mat);
	for (int i = 0; i < n; i++) if (o.geometry[i].material_ID < 0 || o.geometry[i].material_ID >= n_mat) return -1;
	memcpy(o.sky.ambient, ambient, 12);
	o.sky.w = hdri_w; o.sky.h = hdri_h;
	o.sky.hdri.assign(hdri_rgba, hdri_rgba + static_cast<size_t>(hdri_w) * hdri_h * 4);
	o.sky.fw = static_cast<float>(hdri_w - 1); o.sky.fh = static_cast<float>(hdri_h - 1);   // Application.cpp:230-231
	bvh_build(o.geometry, o.bvh);
	build_accel(o);
	o.lights.clear();
	for (int32_t i = 0; i < n; i++) {
		const float* em = o.material[o.geometry[i].material_ID].emission;
		if (dot3(v3{em[0], em[1], em[2]}, v3{em[0], em[1], em[2]}) > 0.0f) o.lights.push_back(i);
	}
	return 0;
}
// on = 1: 4-wide, hit kids sorted; 2: 4-wide, nearest first, the rest as stored; 3: 8-wide, sorted
void orc_wide_stats(int on, uint64_t* out) { g_wide_on = on != 0; g_wide_variant = on > 1 ? on - 1 : 0; if (out) for (int i = 0; i < 6; i++) out[i] = g_wide[i]; }
void orc_len_hist(int on, uint64_t* out) { g_len_hist_on = on != 0; if (out) for (int i = 0; i < 16; i++) out[i] = g_len_hist[i]; }
void orc_set_cone_fuzz(float f) { g_cone_fuzz = f; }
void orc_set_padding(void* h, float pad_rel) { Oracle& o = *static_cast<Oracle*>(h); bvh_pad(o.accel, o.bvh.prims, pad_rel); if (o.accel_half) bvh_quantize_half(o.accel); }
// internal_tree: 1 = internal SAH tree (product default), 0 = the reference tree; half: binary16 boxes (product's 32-B records)
void orc_set_mode2_tree(void* h, int internal_tree, int half, int wide) { Oracle& o = *static_cast<Oracle*>(h); o.accel_internal = internal_tree != 0; o.accel_half = half != 0; o.accel_wide = wide != 0; build_accel(o); }
int orc_node_count(void* h) { return static_cast<int>(static_cast<Oracle*>(h)->bvh.nodes.size()); }
int orc_light_count(void* h) { return static_cast<int>(static_cast<Oracle*>(h)->lights.size()); }
void orc_get_bvh(void* h, void* nodes, void* prims) {
	Oracle& o = *static_cast<Oracle*>(h);
	if (nodes) memcpy(nodes, o.bvh.nodes.data(), o.bvh.nodes.size() * sizeof(Node));
	if (prims) memcpy(prims, o.bvh.prims.data(), o.bvh.prims.size() * sizeof(Sphere));
}
void orc_get_lights(void* h, int32_t* lights) { Oracle& o = *static_cast<Oracle*>(h); memcpy(lights, o.lights.data(), o.lights.size() * 4); }

void orc_set_camera(void* h, const float* pos, const float* orient_xyzw, float half_w, float half_h, float z, float exposure) {
	Oracle& o = *static_cast<Oracle*>(h);
	o.camera.pos = { pos[0], pos[1], pos[2] };
	o.camera.orient = { orient_xyzw[0], orient_xyzw[1], orient_xyzw[2], orient_xyzw[3] };
	o.camera.half_width = half_w; o.camera.half_height = half_h; o.camera.z = z; o.camera.exposure = exposure;
}
// Renderer::Resize (Renderer.hpp:53-63) + policy knobs
int orc_config(void* h, uint32_t width, uint32_t height, uint32_t max_bounces, uint32_t buckets, int mis, int trav_mode, int threads) {
	Oracle& o = *static_cast<Oracle*>(h);
	if (buckets < 1 || buckets > 64 || max_bounces < 1) return -1;
	o.width = width; o.height = height;
	o.h_tiles = width / TileRoot; o.v_tiles = height / TileRoot;
	o.max_bounces = max_bounces; o.buckets = buckets; o.mis = mis; o.trav_mode = trav_mode; o.threads = threads;
	o.tile_list.clear();
	o.accumulator.assign(static_cast<size_t>(o.h_tiles) * o.v_tiles * buckets * 3 * TileSize, 0.0f);
	o.accumulations = 0;
	return 0;
}
// Like orc_config, but only the listed LaunchIndices are rendered; the accumulator then holds n slabs in list order.
int orc_config_tiles(void* h, uint32_t width, uint32_t height, uint32_t max_bounces, uint32_t buckets, int mis, int trav_mode, int threads,
                     const uint32_t* tiles, uint32_t n) {
	Oracle& o = *static_cast<Oracle*>(h);
	if (buckets < 1 || buckets > 64 || max_bounces < 1 || !tiles || n == 0) return -1;
	o.width = width; o.height = height;
	o.h_tiles = width / TileRoot; o.v_tiles = height / TileRoot;
	for (uint32_t i = 0; i < n; i++) if (tiles[i] >= o.h_tiles * o.v_tiles) return -1;
	o.max_bounces = max_bounces; o.buckets = buckets; o.mis = mis; o.trav_mode = trav_mode; o.threads = threads;
	o.tile_list.assign(tiles, tiles + n);
	o.accumulator.assign(static_cast<size_t>(n) * buckets * 3 * TileSize, 0.0f);
	o.accumulations = 0;
	return 0;
}
void orc_set_exact_tail(int on) { g_exact_tail = on != 0; }
void orc_reset(void* h) {                                                          // Renderer.hpp:64-67
	Oracle& o = *static_cast<Oracle*>(h);
	o.accumulations = 0;
	std::fill(o.accumulator.begin(), o.accumulator.end(), 0.0f);
	o.counters.rays = 0; o.counters.shadow_rays = 0; o.counters.nodes = 0; o.counters.spheres = 0;
	o.counters.shadow_nodes = 0; o.counters.shadow_spheres = 0; o.counters.terminated = 0;
}
// The closure of every later Accumulate() (0 Lambertian, 1 GGX) and its gloss decay table decay[0..n); the accumulator is left alone.
int orc_set_brdf(void* h, int brdf, const float* decay, uint32_t n) {
	if (brdf != 0 && brdf != 1) return -1;
	Oracle& o = *static_cast<Oracle*>(h);
	o.brdf = brdf;
	if (decay && n) o.gloss_decay.assign(decay, decay + n); else o.gloss_decay.clear();
	return 0;
}
// Candidates of the NEE light's resampled importance sampling in every later Accumulate(): 0 = the reference's one light sample (the old code path),
// 1..32 as mirt_set_light_ris.  The accumulator is left alone.
int orc_set_light_ris(void* h, uint32_t candidates) {
	if (!h || candidates > 32u) return -1;
	static_cast<Oracle*>(h)->light_ris = candidates;
	return 0;
}
// Thin lens of every later Accumulate() and orc_raygen, refused as mirt_set_lens refuses: aperture 0 = the pinhole camera (focus_depth then unused).
int orc_set_lens(void* h, float aperture, float focus_depth) {
	if (!h || !std::isfinite(aperture) || !std::isfinite(focus_depth) || aperture < 0.0f) return -1;
	if (aperture > 0.0f && !(focus_depth > 0.0f)) return -1;
	Oracle& o = *static_cast<Oracle*>(h);
	o.lens_aperture = aperture; o.lens_focus_depth = focus_depth;
	return 0;
}
// Companion of mirt_load_accumulator: overwrite the slab and continue from `accumulations` (the next Accumulate() is number accumulations + 1).
int orc_load_accumulator(void* h, const float* src, uint32_t accumulations) {
	if (!h || !src) return -1;
	Oracle& o = *static_cast<Oracle*>(h);
	memcpy(o.accumulator.data(), src, o.accumulator.size() * 4);
	o.accumulations = accumulations;
	return 0;
}
void orc_accumulate(void* h, uint32_t n_calls) { Oracle& o = *static_cast<Oracle*>(h); for (uint32_t i = 0; i < n_calls; i++) accumulate(o); }
uint32_t orc_accumulations(void* h) { return static_cast<Oracle*>(h)->accumulations; }
size_t orc_accumulator_floats(void* h) { return static_cast<Oracle*>(h)->accumulator.size(); }
void orc_read_accumulator(void* h, float* dst) { Oracle& o = *static_cast<Oracle*>(h); memcpy(dst, o.accumulator.data(), o.accumulator.size() * 4); }
int orc_render(void* h, float* rgba) { return render(*static_cast<Oracle*>(h), rgba); }
// out[0..6] = rays, shadow_rays, nodes, spheres, shadow_nodes, shadow_spheres, terminated
void orc_counters(void* h, uint64_t* out) {
	Oracle& o = *static_cast<Oracle*>(h);
	out[0] = o.counters.rays; out[1] = o.counters.shadow_rays; out[2] = o.counters.nodes; out[3] = o.counters.spheres;
	out[4] = o.counters.shadow_nodes; out[5] = o.counters.shadow_spheres; out[6] = o.counters.terminated;
}

// ---- stage-level entry points for kernel parity tests --------------------------------
// Camera rays of Accumulate() number `accumulations` for every pixel, tile-major order (tile*256 + ID).
void orc_raygen(void* h, uint32_t accumulations, float* p_xyz /*3 planes*/, float* dir_xyz /*3 planes*/) {
	Oracle& o = *static_cast<Oracle*>(h);
	const size_t n = static_cast<size_t>(o.h_tiles) * o.v_tiles * TileSize;
	for (uint32_t t = 0; t < o.h_tiles * o.v_tiles; t++) for (uint32_t ID = 0; ID < TileSize; ID++) {
		const size_t g = static_cast<size_t>(t) * TileSize + ID;
		int32_t x = static_cast<int32_t>(TileRoot * (t % o.h_tiles) + ID % TileRoot);
		int32_t y = static_cast<int32_t>(TileRoot * (t / o.h_tiles) + ID / TileRoot);
		uint32_t seed = static_cast<uint32_t>(static_cast<int32_t>(g * (o.max_bounces * 2 + 1)));
		uint32_t rng = hash_2d(accumulations, seed);
		float cs[2]; cs[0] = rand_unit_float(&rng); cs[1] = rand_unit_float(&rng);
		v3 d = generate_ray_dir(o.camera, x, y, cs);
		v3 origin = o.camera.pos;
		if (o.lens_aperture > 0.0f) lens_ray(o, d, accumulations, seed, &origin, &d);
		p_xyz[g] = origin.x; p_xyz[n + g] = origin.y; p_xyz[2 * n + g] = origin.z;
		dir_xyz[g] = d.x; dir_xyz[n + g] = d.y; dir_xyz[2 * n + g] = d.z;
	}
}
// Closest hit for n independent rays (SoA planes), trav_mode 0 (brute) or 2 (per-ray BVH).
void orc_trace_closest(void* h, int trav_mode, size_t n, const float* p_xyz, const float* dir_xyz, float* tfar, int32_t* primID) {
	Oracle& o = *static_cast<Oracle*>(h);
	LocalCounters lc;
	for (size_t i = 0; i < n; i++) {
		float t = FLT_MAX; int32_t id = -1;
		const float px = p_xyz[i], py = p_xyz[n + i], pz = p_xyz[2 * n + i];
		const float dx = dir_xyz[i], dy = dir_xyz[n + i], dz = dir_xyz[2 * n + i];
		if (trav_mode == 0) { for (size_t p = 0; p < o.bvh.prims.size(); p++) sphere_closest(o.bvh.prims[p], static_cast<int32_t>(p), px, py, pz, dx, dy, dz, &t, &id); }
		else if (!o.accel.nodes.empty()) traverse_ray(o.accel, o.bvh.prims, px, py, pz, dx, dy, dz, &t, &id, lc);
		tfar[i] = t; primID[i] = id;
	}
	o.counters.rays += n; o.counters.nodes += lc.nodes; o.counters.spheres += lc.spheres;
}
void orc_trace_shadow(void* h, int trav_mode, size_t n, const float* p_xyz, const float* dir_xyz, const float* tfar, uint8_t* occluded) {
	Oracle& o = *static_cast<Oracle*>(h);
	LocalCounters lc;
	for (size_t i = 0; i < n; i++) {
		const float px = p_xyz[i], py = p_xyz[n + i], pz = p_xyz[2 * n + i];
		const float dx = dir_xyz[i], dy = dir_xyz[n + i], dz = dir_xyz[2 * n + i];
		bool occ = false;
		if (trav_mode == 0) { for (size_t p = 0; p < o.bvh.prims.size() && !occ; p++) occ = sphere_occludes(o.bvh.prims[p], px, py, pz, dx, dy, dz, tfar[i]); }
		else if (!o.accel.nodes.empty()) occ = traverse_ray_shadow(o.accel, o.bvh.prims, px, py, pz, dx, dy, dz, tfar[i], lc);
		occluded[i] = occ ? 1 : 0;
	}
	o.counters.shadow_rays += n; o.counters.shadow_nodes += lc.shadow_nodes; o.counters.shadow_spheres += lc.shadow_spheres;
}

// Path of one pixel (tile LaunchIndex, pixel px) in Accumulate() number `accumulations`: out[b*8..] = p, dir, tfar, primID per bounce.
int orc_debug_path(void* h, uint32_t LaunchIndex, uint32_t px, uint32_t accumulations, float* out) {
	Oracle& o = *static_cast<Oracle*>(h);
	std::vector<float> scratch(o.accumulator.size(), 0.0f);
	LocalCounters lc;
	g_dbg.on = true; g_dbg.px = px; g_dbg.n = 0; g_dbg.n_cand = 0;
	accumulate_tile(o, LaunchIndex, LaunchIndex, accumulations, scratch.data(), lc);
	g_dbg.on = false;
	memcpy(out, g_dbg.rec, sizeof(float) * 8 * g_dbg.n);
	return g_dbg.n;
}

// The RIS candidates of the same pixel and call (orc_set_light_ris above 0): out[i*4..] = bounce, candidate, reservoir draw r, weight w (0: it left early).
int orc_debug_candidates(void* h, uint32_t LaunchIndex, uint32_t px, uint32_t accumulations, float* out, int max_records) {
	float path[64 * 8];
	orc_debug_path(h, LaunchIndex, px, accumulations, path);
	const int n = g_dbg.n_cand < max_records ? g_dbg.n_cand : max_records;
	memcpy(out, g_dbg.cand, sizeof(float) * 4 * n);
	return n;
}

// ---- unit functions (KATs / per-function fixtures) -------------------------------------
void orc_ggx_eval(const float* F0, float alpha, const float* L, const float* V, float* out) {
	const v3 r = ggx_eval(v3{F0[0], F0[1], F0[2]}, alpha, v3{L[0], L[1], L[2]}, v3{V[0], V[1], V[2]}); out[0] = r.x; out[1] = r.y; out[2] = r.z;
}
void orc_ggx_sample(const float* F0, float alpha, const float* V, float u0, float u1, float* dir_out, float* estimator_out) {
	v3 d, e; ggx_sample(v3{F0[0], F0[1], F0[2]}, alpha, v3{V[0], V[1], V[2]}, u0, u1, &d, &e);
	dir_out[0] = d.x; dir_out[1] = d.y; dir_out[2] = d.z; estimator_out[0] = e.x; estimator_out[1] = e.y; estimator_out[2] = e.z;
}
uint32_t orc_hash_u32(uint32_t i) { return hash_u32(i); }
uint32_t orc_hash_2d(uint32_t x, uint32_t y) { return hash_2d(x, y); }
uint32_t orc_pcg_generate(uint32_t* s) { return pcg_generate(s); }
float orc_make_unit_float(uint32_t x) { return make_unit_float(x); }
uint32_t orc_rand_bounded_int(uint32_t* s, uint32_t range) { return rand_bounded_int(s, range); }
void orc_fast_sincos(float x, float* s, float* c) { fast_sincos(x, s, c); }
float orc_fast_atan2(float y, float x) { return fast_atan2(y, x); }
float orc_fast_asin(float x) { return fast_asin(x); }
void orc_tangent_space(const float* n, float* q_xyzw) { q4 q = tangent_space(v3{n[0], n[1], n[2]}); q_xyzw[0] = q.x; q_xyzw[1] = q.y; q_xyzw[2] = q.z; q_xyzw[3] = q.w; }
void orc_to_local(const float* q, const float* v, float* out) { v3 r = to_local(q4{q[0], q[1], q[2], q[3]}, v3{v[0], v[1], v[2]}); out[0] = r.x; out[1] = r.y; out[2] = r.z; }
void orc_to_world(const float* q, const float* v, float* out) { v3 r = to_world(q4{q[0], q[1], q[2], q[3]}, v3{v[0], v[1], v[2]}); out[0] = r.x; out[1] = r.y; out[2] = r.z; }
void orc_hemisphere(float t, float s, float* out) { v3 r = hemisphere(t, s); out[0] = r.x; out[1] = r.y; out[2] = r.z; }
void orc_sample_direction_to_sphere(const float* wc, float sin2, float dist, float r2, float t, float s, float* out5) {
	float d, pdf; v3 L = sample_direction_to_sphere(v3{wc[0], wc[1], wc[2]}, sin2, dist, r2, t, s, &d, &pdf);
	out5[0] = L.x; out5[1] = L.y; out5[2] = L.z; out5[3] = d; out5[4] = pdf;
}
float orc_median5(float a, float b, float c, float d, float e) { return median5(a, b, c, d, e); }
void orc_tonemap(float* rgb) { tonemapping(rgb[0], rgb[1], rgb[2]); }
int orc_has_avx2() {
#if defined(__AVX2__) && defined(__FMA__)
	return 1;
#else
	return 0;
#endif
}

} // extern "C"
