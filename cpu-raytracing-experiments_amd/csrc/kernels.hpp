// kernels.hpp — HIP kernels of the wavefront path tracer (gfx950 / CDNA4, wave64).
//
// One Renderer::Accumulate() call of the reference (Renderer.hpp:73-434) runs a 256-ray stream per
// 16x16 tile through raygen -> [intersect -> closest-hit shade -> sort -> NEE -> shadow trace ->
// emissive -> BRDF sample/RR/compaction -> miss -> accumulate] on one CPU thread.  Here the same
// path state is a set of SoA ray streams in HBM spanning every pixel this GPU owns times the
// accumulations in flight, and one bounce is two kernels (plus a few-microsecond k_trace_fat for the rare stretched rays):
//
//   k_trace           Traverse (BVH.hpp:309-360) for the rays of bounce b: reads p,dir, writes tfar,primID — and, in the
//                     same launch, Traverse_shadow (BVH.hpp:362-404) for the NEE rays of bounce b-1, each followed by
//                     Renderer.hpp:304-314 and the deferred adds ((R + unoccluded NEE) + emissive, the reference's order) into
//                     the path's word of the batch's contribution buffer, where its radiance R lives from bounce 0 on
//   k_shade           Renderer.hpp:169-431 except the shadow-dependent adds; compacts survivors into the next stream and
//                     NEE candidates into the shadow stream (wave64 ballot + mbcnt prefix sums, one atomic per workgroup)
//   k_primary_cand /  bounce 0 only (RAY GENERATION + the first Traverse, Renderer.hpp:113-127,165): the camera rays have no stream — a
//   k_primary_hits    ray is a function of its index — and the jittered samples of a pixel (one per accumulation of the batch, up to 256) share ONE cone traversal that lists
//                     the spheres they can hit; each sample then tests only its pixel's list (kCollect below)
//
// Per-path results do not depend on stream slot or scheduling: every random draw is re-derived from
// (accumulations, seed[pixel], bounce) (Renderer.hpp:107,117,255,362), which is what lets the
// wavefront reorder rays freely and still reproduce the reference bit for bit — up to the one thing that does depend on the slot, the
// scalar tail of intersect_prims (Q14): k_tile_stream below ("EXACT STREAM ORDER", mirt_set_stream_order) replays slots and tail.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_math.hpp"
#include "hits_wave_map.hpp"
#include "tile_map.hpp"
#include "kernel_types.hpp"

namespace mirt {

// kPrimaryList launches have no ray stream: the words at `a` are the list of pixels instead (k_primary_cand's, or the active tiles' part of it).
MIRT_DI const uint32_t* stream_pixel_list(const StreamBuf& in) { return reinterpret_cast<const uint32_t*>(in.a); }

// ------------------------------------------------------------------------------------------------
// wave64 helpers
// ------------------------------------------------------------------------------------------------
MIRT_DI uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
MIRT_DI uint32_t mask_rank(unsigned long long m) {            // set bits of m below this lane
	return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
}
MIRT_DI void wave_sum(uint32_t v, unsigned long long* counter) {
	for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
	if (lane_id() == 0 && v) atomicAdd(counter, static_cast<unsigned long long>(v));
}
MIRT_DI void wave_sum(unsigned long long v, unsigned long long* counter) {     // k_tile_stream: a lane's count over a whole bounce loop can pass 2^32
	for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
	if (lane_id() == 0 && v) atomicAdd(counter, v);
}

// ---- ray queues -----------------------------------------------------------------------------------------------
// A ray queue (the rays of one bounce, or its NEE shadow rays) is kSegs dense SEGMENTS of the stream planes at fixed offsets:
// segment k holds slots [k * seg_cap, k * seg_cap + n[k]).  Producers (k_shade's compaction) append block-iteration t to
// segment t % kSegs, so the one returning atomicAdd per workgroup and 512 rays is spread over kSegs counters, each on a
// cache line of its own: same-address returning atomics serialise at ~11 ns each (MI355X_MICROARCH.md "dequeue": one word
// saturates at ~88 per microsecond), and with a single counter that alone was 1.9 ms of the 3.3 ms primary-ray k_shade launch
// of a 4096x4096 batch (164 k appends).  A segment receives at most ceil(T / kSegs) iterations of <= 512 rays, T =
// ceil(input rays / 512), hence seg_cap = ceil(ceil(capacity / 512) / kSegs) * 512 never overflows.  Consumers number the
// rays 0 .. total-1 across the segments in order (queue_view / queue_slot); per-path results do not depend on slot order.
struct QueueView { uint32_t pre[kSegs + 1]; uint32_t seg_cap; };     // pre[k] = rays before segment k, pre[kSegs] = total
MIRT_DI QueueView queue_view(const Queue& q) {
	QueueView v; v.seg_cap = q.seg_cap; v.pre[0] = 0;
	for (uint32_t k = 0; k < kSegs; k++) v.pre[k + 1] = v.pre[k] + q.n[k * kSegPitch];     // wave-uniform: scalar loads
	return v;
}
MIRT_DI QueueView queue_identity(uint32_t total) {     // bounce 0: ray i is slot i (the rays are generated from their index)
	QueueView v; v.seg_cap = 0; v.pre[0] = 0;
	for (uint32_t k = 1; k <= kSegs; k++) v.pre[k] = total;
	return v;
}
// The piece [first, end) of the numbering that lies in first's segment, and the offset that turns its numbers into slots.
struct QueuePiece { uint32_t end, offset; };
MIRT_DI QueuePiece queue_piece(const QueueView& v, uint32_t first) {
	uint32_t seg = 0, lo = 0, hi = v.pre[1];
	for (uint32_t k = 1; k < kSegs; k++) { const bool ge = first >= v.pre[k]; seg = ge ? k : seg; lo = ge ? v.pre[k] : lo; hi = ge ? v.pre[k + 1] : hi; }
	return QueuePiece{ hi, seg * v.seg_cap - lo };
}
// The same straight from the counters in memory (k_trace calls it once per reserved chunk of rays and keeps no view in registers:
// the kernel sits at its 64-VGPR budget).  q.n == nullptr: the identity numbering of bounce 0, `total` rays.
MIRT_DI QueuePiece queue_piece(const Queue& q, uint32_t total, uint32_t first) {
	if (q.n == nullptr) return QueuePiece{ total, 0u };
	uint32_t lo = 0, seg = 0, end = 0;
	for (uint32_t k = 0; k < kSegs; k++) {
		const uint32_t cnt = q.n[k * kSegPitch];
		if (first >= lo + cnt && k + 1 < kSegs) { lo += cnt; continue; }
		seg = k; end = lo + cnt; break;
	}
	return QueuePiece{ end, seg * q.seg_cap - lo };
}
MIRT_DI uint32_t queue_total(const Queue& q) { uint32_t t = 0; for (uint32_t k = 0; k < kSegs; k++) t += q.n[k * kSegPitch]; return t; }
MIRT_DI uint32_t queue_slot(const QueueView& v, uint32_t i) { return i + queue_piece(v, i).offset; }     // per-lane form
// The same for consecutive numbers starting at the wave-uniform `first`: scalar segment search, per-lane work only for the
// lanes (if any) that fall into a later segment.
MIRT_DI uint32_t queue_slot(const QueueView& v, uint32_t first, uint32_t i) {
	const QueuePiece p = queue_piece(v, first);
	return i < p.end ? i + p.offset : queue_slot(v, i);
}

// Two-queue compaction for a whole workgroup: wave64 ballots give per-wave counts, one lane per queue adds the workgroup
// total to the counter of segment `seg` (ONE global atomic per queue per `blockDim.x` rays), and every lane gets
// segment start + base + (counts of earlier waves) + (rank inside its wave).  Must be called by all threads of the block,
// converged.  `scratch` = 2*2*16+2*2 words of LDS, double-buffered on `parity` so consecutive calls need no third barrier.
MIRT_DI void block_append2(bool flag_a, bool flag_b, const Queue& qa, const Queue& qb, uint32_t seg, uint32_t* scratch, uint32_t parity,
                           uint32_t& slot_a, uint32_t& slot_b) {
	const unsigned long long ma = __ballot(flag_a), mb = __ballot(flag_b);
	const uint32_t wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6, lane = lane_id();
	uint32_t* cnt_a = scratch + parity * 36u;       // [16] a, [16] b, base a, base b, pad
	uint32_t* cnt_b = cnt_a + 16u;
	uint32_t* base = cnt_a + 32u;
	if (lane == 0) { cnt_a[wave] = static_cast<uint32_t>(__popcll(ma)); cnt_b[wave] = static_cast<uint32_t>(__popcll(mb)); }
	__syncthreads();
	if (threadIdx.x < 2) {
		const uint32_t* cnt = threadIdx.x ? cnt_b : cnt_a;
		uint32_t total = 0;
		for (uint32_t w = 0; w < n_waves; w++) total += cnt[w];
		base[threadIdx.x] = total ? atomicAdd((threadIdx.x ? qb.n : qa.n) + seg * kSegPitch, total) : 0u;
	}
	__syncthreads();
	uint32_t pa = base[0] + seg * qa.seg_cap, pb = base[1] + seg * qb.seg_cap;
	for (uint32_t w = 0; w < wave; w++) { pa += cnt_a[w]; pb += cnt_b[w]; }
	slot_a = pa + mask_rank(ma);
	slot_b = pb + mask_rank(mb);
}

// ------------------------------------------------------------------------------------------------
// Intersection arithmetic
// ------------------------------------------------------------------------------------------------
// 8-ray x 1-sphere AVX2 body of intersect_prims, BVH.hpp:251-267, one lane per ray: the FMA chain as written
// there; accept iff dist < tfar, sign(dist) clear, sign(sqrt(disc)) clear (= disc not negative / -0).
MIRT_DI void sphere_closest(float4 s, int32_t prim, float px, float py, float pz, float dx, float dy, float dz,
                            float& tfar, int32_t& primID) {
	float tx = s.x - px;
	float b = dx * tx;
	float disc = __builtin_fmaf(-tx, tx, s.w);
	float ty = s.y - py;
	b = __builtin_fmaf(dy, ty, b);
	disc = __builtin_fmaf(-ty, ty, disc);
	float tz = s.z - pz;
	b = __builtin_fmaf(dz, tz, b);
	disc = __builtin_fmaf(-tz, tz, disc);
	disc = __builtin_fmaf(b, b, disc);
	if (__float_as_uint(disc) & 0x80000000u) return;
	float sq = __builtin_sqrtf(disc);
	float dist = b - sq;
	if (__float_as_uint(dist) & 0x80000000u) dist = b + sq;
	if ((dist < tfar) && !(__float_as_uint(dist) & 0x80000000u)) { tfar = dist; primID = prim; }
}
// intersect_prims_shadow, BVH.hpp:294-300 (scalar, unfused)
MIRT_DI bool sphere_occludes(float4 s, float px, float py, float pz, float dx, float dy, float dz, float tfar) {
	f3 P{ s.x - px, s.y - py, s.z - pz };
	float b = dot3(f3{ dx, dy, dz }, P);
	float disc = b * b - dot3(P, P) + s.w;
	if (disc < 0.0f) return false;
	disc = __builtin_sqrtf(disc);
	float dist = (b >= disc ? b - disc : b + disc);
	if (dist < 0.0f || dist >= tfar) return false;
	return true;
}
// ---- BVH traversal -----------------------------------------------------------------------------
// Semantics (DESIGN.md "Traversal semantics"): the BVH is a pure acceleration of the reference's shipped
// brute-force loops (BVH.hpp:312 / :365).  Boxes are conservative (bvh_layout.hpp), the ray interval is
// [0, tfar], and the closest hit is the lexicographic minimum of (dist, BVH-order prim index) — which is
// what the ascending strict-'<' scan of intersect_prims returns — so visiting order, pruning and the slab
// arithmetic cannot change the result.  oracle/oracle.cpp mode 2 is the CPU twin of this routine.
// Conservative "cone" slab test.  The reference's sphere tests assume a unit direction (disc = b^2 - |oc|^2 + r^2,
// BVH.hpp:251-260,295-296), but its tangent frame is ill-conditioned near N.z = -1 (Sampling.hpp:150-159) and to_world can
// return a stretched direction (|D| = 1.125 seen in cfg2); for such a ray a sphere it geometrically misses can still pass
// the reference's test, by a margin that grows with distance — no fixed box padding covers that.  Algebra: with d the
// reported hit parameter, |p + d*D - c|^2 = r^2 + d^2 (|D|^2 - 1) (+ rounding of the f32 sphere arithmetic, <= 2^-19 d^2),
// so the reported hit point lies within alpha*d of the sphere, alpha^2 = max(|D|^2-1, 0) + 2^-19.  The boxes are therefore
// tested against the ray inflated by alpha*t (L-inf) at parameter t:
//     lo_i - alpha t <= p_i + t d_i <= hi_i + alpha t   <=>   t (d_i+alpha) >= lo_i - p_i   and   t (d_i-alpha) <= hi_i - p_i
// i.e. the usual slab test with reciprocal 1/(d_i+alpha) for the lo plane and 1/(d_i-alpha) for the hi plane (still one FMA
// per plane).  An axis with |d_i| < alpha has d_i+alpha > 0 > d_i-alpha: BOTH planes give lower bounds on t and there is no
// upper bound (the cone widens faster than the ray drifts).  Such axes cannot simply be dropped: every camera ray near the
// image's centre row/column is nearly axis-parallel, and without its lateral bounds it visits every box in front of it
// (64 438 boxes for one ray of S(100000), a 20 ms tail per launch).  Per axis a constant c = -inf (ordinary) / +inf (both
// lower bounds) turns the two cases into the same two instructions:
//     enter_i = med3(l, h, c)   (min(l,h) | max(l,h))        leave_i = max3(l, h, c)   (max(l,h) | +inf)
// |d_i| == alpha exactly: the axis gives no bound (l = -inf, h = +inf).  For unit directions alpha = 1.4e-3: +4 % box tests on S(1000).
struct RaySlab { float iax, iay, iaz, nax, nay, naz, ibx, iby, ibz, nbx, nby, nbz, cx, cy, cz; };
MIRT_DI void slab_axis(float p, float d, float alpha, float& ia, float& na, float& ib, float& nb, float& c) {
	const float prod = (d - alpha) * (d + alpha);               // one division per axis: 1/(d+a) = (d-a)/(d^2-a^2), 1/(d-a) = (d+a)/(d^2-a^2)
	const bool keep = prod != 0.0f;
	const float r = 1.0f / prod;
	const float ra = (d - alpha) * r, rb = (d + alpha) * r;
	ia = keep ? ra : 0.0f; ib = keep ? rb : 0.0f;
	na = keep ? -(p * ra) : -__builtin_inff();
	nb = keep ? -(p * rb) : __builtin_inff();
	c = (prod < 0.0f) ? __builtin_inff() : -__builtin_inff();
}
MIRT_DI RaySlab make_slab(float px, float py, float pz, float dx, float dy, float dz, float& alpha_out, float alpha_extra = 0.0f) {
	const float L2 = (dx * dx + dy * dy) + dz * dz;
	const float a2 = __builtin_fmaxf(L2 - 1.0f, 0.0f) * 1.0009765625f + 0x1p-19f;
	const float alpha = __builtin_sqrtf(a2) * 1.0009765625f + alpha_extra;     // alpha_extra: a BUNDLE of rays around this axis (k_primary_cand)
	alpha_out = alpha;
	RaySlab s;
	slab_axis(px, dx, alpha, s.iax, s.nax, s.ibx, s.nbx, s.cx);
	slab_axis(py, dy, alpha, s.iay, s.nay, s.iby, s.nby, s.cy);
	slab_axis(pz, dz, alpha, s.iaz, s.naz, s.ibz, s.nbz, s.cz);
	return s;
}
// v_med3_f32 / v_max3_f32 / v_min3_f32; no NaN can reach them (finite boxes, finite or zeroed reciprocals).
MIRT_DI bool slab_hit(const RaySlab& rs, float lx, float hx, float ly, float hy, float lz, float hz, float tfar, float& tnear) {
	const float ex = __builtin_amdgcn_fmed3f(lx, hx, rs.cx), ey = __builtin_amdgcn_fmed3f(ly, hy, rs.cy), ez = __builtin_amdgcn_fmed3f(lz, hz, rs.cz);
	const float ox = __builtin_fmaxf(__builtin_fmaxf(lx, hx), rs.cx), oy = __builtin_fmaxf(__builtin_fmaxf(ly, hy), rs.cy), oz = __builtin_fmaxf(__builtin_fmaxf(lz, hz), rs.cz);
	const float tmin = __builtin_fmaxf(__builtin_fmaxf(ex, ey), __builtin_fmaxf(ez, 0.0f));
	float oz_far;                                                             // min(oz, tfar) as the bare instruction: __builtin_fminf first canonicalises tfar (a v_max_f32 x, x per step) in case it were a signalling NaN
	asm("v_min_f32 %0, %1, %2" : "=v"(oz_far) : "v"(oz), "v"(tfar));
	const float tmax = __builtin_fminf(__builtin_fminf(ox, oy), oz_far);
	tnear = tmin;
	return tmin <= tmax;
}
// intersect_prims acceptance made order-independent: candidate against an open tfar, then (dist, index) order.
MIRT_DI void sphere_closest_tie(float4 s, int32_t prim, float px, float py, float pz, float dx, float dy, float dz,
                                float& tfar, int32_t& primID) {
	float t = MIRT_FLT_MAX; int32_t id = -1;
	sphere_closest(s, prim, px, py, pz, dx, dy, dz, t, id);
	if (id < 0) return;
	if (t < tfar || (t == tfar && (primID < 0 || prim < primID))) { tfar = t; primID = prim; }
}

// LDS views are typed with address_space(3) so every access is a ds_read/ds_write.  (With generic pointers hipcc merged
// the "staged record" and "record in HBM" paths into one pointer select + flat_load_dwordx4, which is several times
// slower than ds_read_b128 and waits on both vmcnt and lgkmcnt.)
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4f lds_v4f;
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) uint16_t lds_u16;
// Select-only forms of the two sphere tests for the traversal loop (same arithmetic and acceptance as sphere_closest /
// sphere_occludes above; a divergent branch costs several scalar exec-mask instructions, and the CU's single scalar unit
// was issuing as many instructions as its four SIMDs).
// sqrt of the two tests below: correctly rounded, bit for bit __builtin_sqrtf (hipcc's expansion around v_sqrt_f32: one fix-up step
// towards each neighbour, decided by an FMA residual) WITHOUT that expansion's seven instructions of denormal scaling and 0 / inf
// pass-through.  Only inputs in [+0, 2^-100) need the scaling (their residuals would be denormal); a wave that holds such a
// discriminant (none in practice) takes the library path as a whole — one unsigned compare on the bits, which negative inputs
// pass.  +inf and the large values fall out right (NaN residuals select nothing); negative and NaN inputs give NaN-or-garbage that
// both callers mask.  Checked against __builtin_sqrtf for EVERY f32 bit pattern >= 0 by profiles/experiments/sqrt_check.hip, and
// by tests (mirt_debug_math fn 10).
MIRT_DI float sqrt_trav(float x) {
	if (__ballot(__float_as_uint(x) < 0x0d800000u) != 0ull) return __builtin_sqrtf(x);     // 0x0d800000 = 2^-100
	const float s = __builtin_amdgcn_sqrtf(x);                                // within 1 ulp
	const float s_dn = __uint_as_float(__float_as_uint(s) - 1u), s_up = __uint_as_float(__float_as_uint(s) + 1u);
	const float r_dn = __builtin_fmaf(-s_dn, s, x), r_up = __builtin_fmaf(-s_up, s, x);
	float r = (r_dn <= 0.0f) ? s_dn : s;
	r = (r_up > 0.0f) ? s_up : r;
	return r;
}
MIRT_DI void sphere_closest_sel(bool lane_on, float4 s, int32_t prim, const float px, const float py, const float pz, const float dx, const float dy,
                                const float dz, float& tfar, int32_t& primID) {
	const float tx = s.x - px;
	float b = dx * tx;
	float disc = __builtin_fmaf(-tx, tx, s.w);
	const float ty = s.y - py;
	b = __builtin_fmaf(dy, ty, b);
	disc = __builtin_fmaf(-ty, ty, disc);
	const float tz = s.z - pz;
	b = __builtin_fmaf(dz, tz, b);
	disc = __builtin_fmaf(-tz, tz, disc);
	disc = __builtin_fmaf(b, b, disc);
	const bool disc_ok = !(__float_as_uint(disc) & 0x80000000u);
	const float sq = sqrt_trav(disc);                             // NaN for a negative discriminant: masked by disc_ok
	float dist = b - sq;
	dist = (__float_as_uint(dist) & 0x80000000u) ? b + sq : dist;
	// bitwise &,| on purpose: short-circuit &&,|| come back as nested exec-mask branches
	const bool cand = lane_on & disc_ok & (dist < MIRT_FLT_MAX) & !(__float_as_uint(dist) & 0x80000000u);
	const bool better = cand & ((dist < tfar) | ((dist == tfar) & ((primID < 0) | (prim < primID))));
	tfar = better ? dist : tfar;
	primID = better ? prim : primID;
}
MIRT_DI bool sphere_occludes_sel(float4 s, const float px, const float py, const float pz, const float dx, const float dy, const float dz, const float tfar) {
	const f3 P{ s.x - px, s.y - py, s.z - pz };
	const float b = dot3(f3{ dx, dy, dz }, P);
	const float disc = b * b - dot3(P, P) + s.w;
	const float sq = sqrt_trav(disc);
	const float dist = (b >= sq ? b - sq : b + sq);
	return !(disc < 0.0f) & !((dist < 0.0f) | (dist >= tfar));
}

struct TraceLds { const lds_v4f* recs; const lds_v4f* spheres; lds_u32* stack; };   // stack: [kLdsStack][blockDim.x] entries (u32, or u16 with half records)
MIRT_DI float half_lo(uint32_t w) { return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<unsigned short>(w & 0xffffu))); }
MIRT_DI float half_hi(uint32_t w) { return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<unsigned short>(w >> 16))); }
MIRT_DI float4 to_float4(v4f v) { return make_float4(v.x, v.y, v.z, v.w); }

// One lane's traversal state.  A lane keeps it in registers across refills of OTHER lanes (persistent waves below).
struct Trav {
	float px, py, pz, dx, dy, dz;
	RaySlab rs;
	float tfar;
	int32_t prim;
	uint32_t cur, sp;
};
// Stack entries beyond the LDS-resident ones.  Kept OUTSIDE Trav: a dynamically indexed member would pin the whole struct
// in scratch memory (every step would then reload the ray through VMEM); alone, only this rarely-touched array lives there.
struct TravSpill { uint32_t e[kStack - kLdsStackWide]; };
// Rays whose cone half-width exceeds kAlphaFat per unit of ray parameter (|D|^2 - 1 > ~1e-3: a few per million, produced
// by the reference's ill-conditioned tangent frame) are not traversed: the inflated ray would touch most of the tree and one
// lane would walk it serially (measured: 20-57 ms per launch on a 100k-sphere scene).  They go to a "fat ray" list and
// k_trace_fat intersects them with every sphere, a whole workgroup per ray — literally the reference's brute-force loop.
// (|D|^2 - 1 over the rays of S(100000), CPU twin, per million: 38 in (1e-4, 3e-4], 16 in (3e-4, 1e-3], 6 above.  With the limit
// at 0.01 the detour took the 60 per million and 1.6 % of the cfg4 step; at 0.03 it takes the 6.)
constexpr float kAlphaFat = 0.03f;
MIRT_DI bool trav_begin(Trav& t, float px, float py, float pz, float dx, float dy, float dz, float tfar, float alpha_extra = 0.0f) {     // true = fat ray
	t.px = px; t.py = py; t.pz = pz; t.dx = dx; t.dy = dy; t.dz = dz;
	float alpha;
	t.rs = make_slab(px, py, pz, dx, dy, dz, alpha, alpha_extra);
	t.tfar = tfar; t.prim = -1; t.cur = 0; t.sp = 0;
	return alpha > kAlphaFat;
}
// One step = one 64-B record: slab-test both children against the current tfar, intersect hit leaf children at once,
// re-check inner children against the shrunken tfar, enter the nearer, push the other (or pop).  Returns true when this
// ray is finished (stack empty, or ANYHIT occluder found -> occluded = true).
// MODE: kClosest (Traverse), kAnyHit (Traverse_shadow), kCollect (candidate spheres of a pixel's bundle of camera rays, below).
constexpr int kClosest = 0, kAnyHit = 1, kCollect = 2;
// kCollect — what the samples of ONE PIXEL can hit.  Within a batch a pixel is sampled once per accumulation (up to 256 times) with sub-pixel jitter
// (Renderer.hpp:117-118); all those camera rays leave cam.pos inside a cone of half-angle rho around the ray through the pixel
// centre.  Traversing that cone once (the same conservative slab test, widened by rho) and listing the spheres it can touch turns
// the primary traversal of every sample into a few exact sphere tests (k_primary_hits).  The list is complete for the closest hit:
//   * a sphere some sample reports a hit on at parameter d has its reported hit point within alpha_s d of the sphere and within
//     rho d of the axis point at d, so its box inflated by (alpha_s + rho) d meets the axis — the cone test with alpha + rho;
//   * the search is cut at F once a sphere is found that EVERY sample must hit: centre within the silhouette by a margin that
//     covers the cone's reach and the reference's f32 discriminant error, origin outside.  F bounds every sample's first-hit
//     distance on it from above, hence every sample's closest-hit distance: a sphere whose box starts beyond F cannot be a closest hit.
// A pixel whose list would exceed kCandMax entries (silhouettes of many small spheres) is marked and its samples are traced normally.
// (15 entries until round 3: 9 % of the cfg4 pixels overflowed; with 31 it is 3.8 % and the step 1 % faster — a sample of k_primary_hits reads its
//  list from registers and L1 —; 63 entries buy nothing more.)
constexpr uint32_t kCandMax = 31, kCandStride = 32, kCandOverflow = 0xffffffffu;
struct Collect { uint32_t* cand; float rho; uint32_t n_pix; };      // cand[k * n_pix + pixel]: k = 0 the count, k = 1.. up to kCandMax BVH-order prim indices (plane-major: neighbouring pixels, neighbouring words)
MIRT_DI void collect_leaf(bool on, float4 s, uint32_t prim, uint32_t pix, const Collect& col, Trav& t) {
	uint32_t cnt = static_cast<uint32_t>(t.prim);
	if (on & (cnt < kCandMax)) col.cand[static_cast<size_t>(1u + cnt) * col.n_pix + pix] = prim;
	cnt += on ? 1u : 0u;
	t.prim = static_cast<int32_t>(cnt);
	// full cover -> every sample hits this sphere no later than F
	const f3 oc{ s.x - t.px, s.y - t.py, s.z - t.pz };
	const float oc2 = dot3(oc, oc), b = dot3(f3{ t.dx, t.dy, t.dz }, oc);
	const float len = __builtin_sqrtf(oc2);
	const float reach = __builtin_sqrtf(__builtin_fmaxf(oc2 - b * b, 0.0f)) + col.rho * len;       // farthest a sample ray can pass from the centre
	// The discriminant every sample is left with after the worst rounding of the reference's f32 evaluation of b^2 - |oc|^2 + r^2
	// (15 roundings of magnitude 2^-24 |oc|^2, directions that are unit only to 1e-7, and this function's own cancellation in
	// oc2 - b*b: together < 2^-19.5 |oc|^2; 2^-17 leaves a factor 5).  Positive: the reference reports a hit for every sample, at a
	// parameter no larger than (b + rho |oc|) - sqrt(slack).
	const float slack = (s.w - reach * reach) - (0x1p-17f * oc2 + 1e-6f * s.w);
	const bool cover = on & (b > 0.0f) & (oc2 > s.w * 1.002f) & (slack > 0.0f);
	const float F = ((b + col.rho * len) - __builtin_sqrtf(__builtin_fmaxf(slack, 0.0f))) * 1.001f + 1e-4f;
	t.tfar = (cover & (F < t.tfar)) ? F : t.tfar;
}
// Per-lane stack: the first kLdsStack entries live in LDS, entry-major ([entry][thread]: a wave's accesses to one depth are
// consecutive, conflict-free); deeper entries (rare) use the scratch array.  An entry is a child reference: a record index, or
// kLeafBit | prim.  ST16 packs it into 16 bits (index < 2^15, the leaf flag moved to bit 15; read back sign-extended).
typedef __attribute__((address_space(3))) int16_t lds_i16;
template <bool HALF, bool ST16>
MIRT_DI void stack_put(const TraceLds lds, TravSpill& spill, uint32_t sp, uint32_t ref) {
	constexpr uint32_t lds_entries = (HALF && !ST16) ? kLdsStackWide : kLdsStack;
	constexpr uint32_t lstride = kTraceBlock;     // every trace launch uses kTraceBlock threads (a runtime blockDim.x costs a quarter-rate v_mul_lo_u32 per push and per pop)
	if (sp < lds_entries) { if (ST16) ((lds_u16*)lds.stack)[sp * lstride + threadIdx.x] = static_cast<uint16_t>(ref | (ref >> 16)); else lds.stack[sp * lstride + threadIdx.x] = ref; }
	else if (sp < kStack) spill.e[sp - lds_entries] = ref;       // depth < kStack is validated on the host
}
template <bool HALF, bool ST16>
MIRT_DI uint32_t stack_get(const TraceLds lds, const TravSpill& spill, uint32_t sp) {
	constexpr uint32_t lds_entries = (HALF && !ST16) ? kLdsStackWide : kLdsStack;
	constexpr uint32_t lstride = kTraceBlock;
	if (sp < lds_entries) {
		if (ST16) return static_cast<uint32_t>(static_cast<int32_t>(((lds_i16*)lds.stack)[sp * lstride + threadIdx.x])) & 0x80007fffu;
		return lds.stack[sp * lstride + threadIdx.x];
	}
	return spill.e[sp - lds_entries];
}
// A ray's traversal is a depth-first walk in which LEAVES ARE STACK ITEMS like inner nodes: t.cur is either a record (node_step:
// slab-test both children against the current tfar, enter the nearer hit child — leaf or not —, push the other, or pop) or a leaf
// (leaf_step: intersect its sphere, then pop).  The two kinds of step are separate so that a wave can run them as separate,
// DENSE passes (trace_persistent): with the sphere test inlined in the node step, as it was, ~58 % of the loop's VALU
// instructions were sphere tests executed for the whole wave on behalf of the ~13 % of lanes that had a hit leaf in that step.
// Both leave t.cur = kHalt when this ray is finished (stack empty, or ANYHIT occluder found -> occluded = true, or a full kCollect list).
constexpr uint32_t kHalt = 0x7fffffffu;         // Trav::cur of a lane that is not walking: no ray, or a finished one whose result waits for the next refill
template <int MODE, bool COUNT, bool ALL_LDS, bool HALF, bool ST16>
MIRT_DI void node_step(const SceneDev& sc, const TraceLds lds, Trav& t, TravSpill& spill, uint32_t& n_nodes) {
	const uint32_t cur = t.cur;
	// child boxes: (lo, hi) per axis for child 0 (a) and child 1 (b)
	float ax0, ax1, ay0, ay1, az0, az1, bx0, bx1, by0, by1, bz0, bz1;
	uint32_t c0, c1;
	if (HALF) {
		v4f q0, q1;                           // 32-B record: 12 binary16 planes + 2 child references
		// Only the top of a large tree is staged.  The choice is made per WAVE: a step whose lanes are all in the staged block reads LDS,
		// any other step reads every lane's record from memory (the top records are the hottest lines of L1 / L2) — one path per step
		// instead of two exec-masked halves.
		if (ALL_LDS || cur < sc.lds_recs) { const lds_v4f* r = lds.recs + cur; q0 = r[0]; q1 = r[sc.lds_recs]; }     // plane-major in LDS
		else { const v4f* r = reinterpret_cast<const v4f*>(reinterpret_cast<const char*>(sc.recs) + (cur << 5)); q0 = r[0]; q1 = r[1]; }   // 32-bit byte offset from a uniform base (n_recs < 2^27, checked on the host)
		const uint32_t w0 = __float_as_uint(q0.x), w1 = __float_as_uint(q0.y), w2 = __float_as_uint(q0.z), w3 = __float_as_uint(q0.w);
		const uint32_t w4 = __float_as_uint(q1.x), w5 = __float_as_uint(q1.y);
		ax0 = half_lo(w0); bx0 = half_hi(w0); ax1 = half_lo(w1); bx1 = half_hi(w1);
		ay0 = half_lo(w2); by0 = half_hi(w2); ay1 = half_lo(w3); by1 = half_hi(w3);
		az0 = half_lo(w4); bz0 = half_hi(w4); az1 = half_lo(w5); bz1 = half_hi(w5);
		c0 = __float_as_uint(q1.z); c1 = __float_as_uint(q1.w);
	} else {
		v4f q0, q1, q2, q3;
		if (ALL_LDS || __ballot(cur >= sc.lds_recs) == 0ull) {     // staged records are stored plane-major (q0[], q1[], q2[], q3[]): 16-B stride between lanes' addresses
			const lds_v4f* r = lds.recs + cur; const uint32_t ns = sc.lds_recs;
			q0 = r[0]; q1 = r[ns]; q2 = r[2u * ns]; q3 = r[3u * ns];
		}
		else { const v4f* r = reinterpret_cast<const v4f*>(sc.recs) + 4ull * cur; q0 = r[0]; q1 = r[1]; q2 = r[2]; q3 = r[3]; }
		ax0 = q0.x; bx0 = q0.y; ax1 = q0.z; bx1 = q0.w;
		ay0 = q1.x; by0 = q1.y; ay1 = q1.z; by1 = q1.w;
		az0 = q2.x; bz0 = q2.y; az1 = q2.z; bz1 = q2.w;
		c0 = __float_as_uint(q3.x); c1 = __float_as_uint(q3.y);
	}
	if (COUNT) n_nodes += 2;
	const RaySlab& rs = t.rs;
	float ta, tb;
	const bool ha = slab_hit(rs, __builtin_fmaf(ax0, rs.iax, rs.nax), __builtin_fmaf(ax1, rs.ibx, rs.nbx),
	                         __builtin_fmaf(ay0, rs.iay, rs.nay), __builtin_fmaf(ay1, rs.iby, rs.nby),
	                         __builtin_fmaf(az0, rs.iaz, rs.naz), __builtin_fmaf(az1, rs.ibz, rs.nbz), t.tfar, ta);
	const bool hb = slab_hit(rs, __builtin_fmaf(bx0, rs.iax, rs.nax), __builtin_fmaf(bx1, rs.ibx, rs.nbx),
	                         __builtin_fmaf(by0, rs.iay, rs.nay), __builtin_fmaf(by1, rs.iby, rs.nby),
	                         __builtin_fmaf(bz0, rs.iaz, rs.naz), __builtin_fmaf(bz1, rs.ibz, rs.nbz), t.tfar, tb);
	// ---- next item: selects, plus one exec region each for the conditional stack write and read ----
	const bool both = ha && hb, none = !ha && !hb;
	const bool a_first = ta <= tb;                                            // any-hit rays too: an occluder is most likely close to the origin (the result does not depend on the order)
	const uint32_t near = (ha && (a_first || !hb)) ? c0 : c1;                 // the child entered when at least one child is hit
	const uint32_t far = a_first ? c1 : c0;
	uint32_t sp = t.sp;
	if (both) { stack_put<HALF, ST16>(lds, spill, sp, far); sp += 1u; }
	uint32_t next = none ? kHalt : near;                                     // nothing hit and nothing stacked: finished
	if (none & (sp != 0u)) { --sp; next = stack_get<HALF, ST16>(lds, spill, sp); }
	t.sp = sp;
	t.cur = next;
}
// The node pass over 4-wide binary16 records (bvh_layout.hpp build_wide_half_records): one 64-B fetch, four slab tests, the nearest
// hit child next (the lowest slot on ties), the other hit children pushed in slot order — sorting them by distance as well buys 2 %
// fewer visits on S(100000) for three times the selection code (oracle twin, orc_wide_stats 1 vs 2).  Unused slots never hit.
template <int MODE, bool COUNT, bool ALL_LDS, bool ST16>
MIRT_DI void node_step_wide(const SceneDev& sc, const TraceLds lds, Trav& t, TravSpill& spill, uint32_t& n_nodes) {
	const uint32_t cur = t.cur;
	v4f q0, q1, q2, q3;
	if (ALL_LDS || cur < sc.lds_recs) { const lds_v4f* r = lds.recs + cur; const uint32_t ns = sc.lds_recs; q0 = r[0]; q1 = r[ns]; q2 = r[2u * ns]; q3 = r[3u * ns]; }
	else { const v4f* r = reinterpret_cast<const v4f*>(reinterpret_cast<const char*>(sc.recs) + (cur << 6)); q0 = r[0]; q1 = r[1]; q2 = r[2]; q3 = r[3]; }
	const uint32_t x0 = __float_as_uint(q0.x), x1 = __float_as_uint(q0.y), x2 = __float_as_uint(q0.z), x3 = __float_as_uint(q0.w);
	const uint32_t y0 = __float_as_uint(q1.x), y1 = __float_as_uint(q1.y), y2 = __float_as_uint(q1.z), y3 = __float_as_uint(q1.w);
	const uint32_t z0 = __float_as_uint(q2.x), z1 = __float_as_uint(q2.y), z2 = __float_as_uint(q2.z), z3 = __float_as_uint(q2.w);
	const uint32_t r0 = __float_as_uint(q3.x), r1 = __float_as_uint(q3.y), r2 = __float_as_uint(q3.z), r3 = __float_as_uint(q3.w);
	if (COUNT) {                                                              // boxes tested = the slots in use (an unused slot's lo.x is +inf)
		n_nodes += ((x0 & 0x7fffu) != 0x7c00u) + (((x0 >> 16) & 0x7fffu) != 0x7c00u) + ((x1 & 0x7fffu) != 0x7c00u) + (((x1 >> 16) & 0x7fffu) != 0x7c00u);
	}
	const RaySlab& rs = t.rs;
	float ta, tb, tc, td;
	const bool ha = slab_hit(rs, __builtin_fmaf(half_lo(x0), rs.iax, rs.nax), __builtin_fmaf(half_lo(x2), rs.ibx, rs.nbx),
	                         __builtin_fmaf(half_lo(y0), rs.iay, rs.nay), __builtin_fmaf(half_lo(y2), rs.iby, rs.nby),
	                         __builtin_fmaf(half_lo(z0), rs.iaz, rs.naz), __builtin_fmaf(half_lo(z2), rs.ibz, rs.nbz), t.tfar, ta);
	const bool hb = slab_hit(rs, __builtin_fmaf(half_hi(x0), rs.iax, rs.nax), __builtin_fmaf(half_hi(x2), rs.ibx, rs.nbx),
	                         __builtin_fmaf(half_hi(y0), rs.iay, rs.nay), __builtin_fmaf(half_hi(y2), rs.iby, rs.nby),
	                         __builtin_fmaf(half_hi(z0), rs.iaz, rs.naz), __builtin_fmaf(half_hi(z2), rs.ibz, rs.nbz), t.tfar, tb);
	const bool hc = slab_hit(rs, __builtin_fmaf(half_lo(x1), rs.iax, rs.nax), __builtin_fmaf(half_lo(x3), rs.ibx, rs.nbx),
	                         __builtin_fmaf(half_lo(y1), rs.iay, rs.nay), __builtin_fmaf(half_lo(y3), rs.iby, rs.nby),
	                         __builtin_fmaf(half_lo(z1), rs.iaz, rs.naz), __builtin_fmaf(half_lo(z3), rs.ibz, rs.nbz), t.tfar, tc);
	const bool hd = slab_hit(rs, __builtin_fmaf(half_hi(x1), rs.iax, rs.nax), __builtin_fmaf(half_hi(x3), rs.ibx, rs.nbx),
	                         __builtin_fmaf(half_hi(y1), rs.iay, rs.nay), __builtin_fmaf(half_hi(y3), rs.iby, rs.nby),
	                         __builtin_fmaf(half_hi(z1), rs.iaz, rs.naz), __builtin_fmaf(half_hi(z3), rs.ibz, rs.nbz), t.tfar, td);
	// ---- the nearest hit child (lowest slot on ties) is next; the other hit children are pushed in slot order ----
	const float inf = __builtin_inff();
	ta = ha ? ta : inf; tb = hb ? tb : inf; tc = hc ? tc : inf; td = hd ? td : inf;
	const bool b_ab = tb < ta, d_cd = td < tc;                                // within each pair the later slot wins only when strictly nearer
	const float tab = b_ab ? tb : ta, tcd = d_cd ? td : tc;
	const uint32_t rab = b_ab ? r1 : r0, rcd = d_cd ? r3 : r2;
	const bool cd = tcd < tab;
	const uint32_t near = cd ? rcd : rab;
	const bool any = ha || hb || hc || hd;
	uint32_t sp = t.sp;
	constexpr uint32_t lds_entries = ST16 ? kLdsStack : kLdsStackWide;
	if (__ballot(sp + 3u > lds_entries) == 0ull) {
		// the usual case, decided for the wave: whatever a lane pushes stays within its LDS entries — four plain conditional writes
		// instead of four times the LDS / scratch / overflow nest of stack_put
		constexpr uint32_t lstride = kTraceBlock;
		if (ha && (cd || b_ab)) { if (ST16) ((lds_u16*)lds.stack)[sp * lstride + threadIdx.x] = static_cast<uint16_t>(r0 | (r0 >> 16)); else lds.stack[sp * lstride + threadIdx.x] = r0; sp += 1u; }
		if (hb && (cd || !b_ab)) { if (ST16) ((lds_u16*)lds.stack)[sp * lstride + threadIdx.x] = static_cast<uint16_t>(r1 | (r1 >> 16)); else lds.stack[sp * lstride + threadIdx.x] = r1; sp += 1u; }
		if (hc && (!cd || d_cd)) { if (ST16) ((lds_u16*)lds.stack)[sp * lstride + threadIdx.x] = static_cast<uint16_t>(r2 | (r2 >> 16)); else lds.stack[sp * lstride + threadIdx.x] = r2; sp += 1u; }
		if (hd && (!cd || !d_cd)) { if (ST16) ((lds_u16*)lds.stack)[sp * lstride + threadIdx.x] = static_cast<uint16_t>(r3 | (r3 >> 16)); else lds.stack[sp * lstride + threadIdx.x] = r3; sp += 1u; }
	} else {
		if (ha && (cd || b_ab)) { stack_put<true, ST16>(lds, spill, sp, r0); sp += 1u; }
		if (hb && (cd || !b_ab)) { stack_put<true, ST16>(lds, spill, sp, r1); sp += 1u; }
		if (hc && (!cd || d_cd)) { stack_put<true, ST16>(lds, spill, sp, r2); sp += 1u; }
		if (hd && (!cd || !d_cd)) { stack_put<true, ST16>(lds, spill, sp, r3); sp += 1u; }
	}
	uint32_t next = any ? near : kHalt;                                       // nothing hit and nothing stacked: finished
	if (!any & (sp != 0u)) { --sp; next = stack_get<true, ST16>(lds, spill, sp); }
	t.sp = sp;
	t.cur = next;
}
template <int MODE, bool COUNT, bool ALL_LDS, bool HALF, bool ST16>
MIRT_DI void leaf_step(const SceneDev& sc, const TraceLds lds, Trav& t, TravSpill& spill, bool& occluded, uint32_t& n_spheres, uint32_t pix, const Collect& col) {
	const uint32_t first = t.cur & ~kLeafBit;
	// (Requesting the sphere when the lane ARRIVES at the leaf, into four registers kept until the pass, was measured: 22 VGPR
	// spills and k_trace 253 -> 283 ms per cfg4 step.  The other seven waves of the SIMD cover this load.)
	float4 s;
	if (ALL_LDS) s = to_float4(lds.spheres[first]); else s = sc.spheres[first];     // spheres are staged all (ALL_LDS) or none
	if (COUNT) n_spheres += 1u;
	bool fin = false;
	if (MODE == kAnyHit) { occluded = sphere_occludes_sel(s, t.px, t.py, t.pz, t.dx, t.dy, t.dz, t.tfar); fin = occluded; }
	else if (MODE == kCollect) { collect_leaf(true, s, first, pix, col, t); fin = static_cast<uint32_t>(t.prim) > kCandMax; }   // a full list: the pixel falls back to tracing
	else sphere_closest_sel(true, s, static_cast<int32_t>(first), t.px, t.py, t.pz, t.dx, t.dy, t.dz, t.tfar, t.prim);
	uint32_t sp = t.sp;
	t.cur = kHalt;
	if (!fin & (sp != 0u)) { --sp; t.cur = stack_get<HALF, ST16>(lds, spill, sp); }
	t.sp = sp;
}

// ---- persistent waves with in-kernel lane refill ------------------------------------------------------------
// Secondary and shadow rays have a heavy-tailed traversal length: with one fixed ray per lane, PMC showed 10-24 % VALU
// lane utilisation (one long ray keeps 63 finished lanes waiting).  Instead every wave keeps a window of ray indices
// [wbeg, wend) that it reserves from a per-launch work counter (one atomic per kChunk rays); whenever at least
// kRefillIdle lanes are idle they are given the next rays of the window — slot = wbeg + rank among idle lanes, from a
// wave64 ballot + mbcnt prefix sum — and the wave goes back to stepping all lanes together.
constexpr uint32_t kNone = 0xffffffffu;
// [beg, end): ray numbers the wave still has to hand out, all in one queue segment (slot = number + offset); [end, chunk_end):
// the rest of the reserved chunk, in later segments.
struct WaveWindow { uint32_t beg, end, chunk_end, offset, chunk; bool more; };
// Rays per reservation: large enough that the work counter sees one atomic per a few thousand rays, small enough that
// every wave of the grid gets a few chunks even on the thin late-bounce streams.
MIRT_DI uint32_t pick_chunk(uint32_t n, uint32_t chunk_max) {
	const uint32_t waves = gridDim.x * (blockDim.x >> 6);
	uint32_t c = n / (waves * 4u);
	c = (c + 63u) & ~63u;
	return c < 64u ? 64u : (c > chunk_max ? chunk_max : c);
}
// Gives the lanes with `want` the slots of the next rays of the wave's window (number = beg + rank among wanting lanes, from a
// wave64 ballot + mbcnt prefix sum), reserving a new chunk from the launch's work counter when the window is empty.
MIRT_DI uint32_t wave_take(bool want, WaveWindow& w, const Queue& q, uint32_t n, uint32_t* work_next) {
	const unsigned long long m = __ballot(want);
	const uint32_t n_want = static_cast<uint32_t>(__popcll(m));
	if (n_want == 0u) return kNone;
	if (w.beg == w.end) {
		if (w.end == w.chunk_end && w.more) {
			uint32_t base = 0;
			if (lane_id() == 0) base = atomicAdd(work_next, w.chunk);
			base = __builtin_amdgcn_readfirstlane(base);
			if (base >= n) { w.more = false; w.beg = w.end = w.chunk_end = 0; }
			else { w.beg = w.end = base; w.chunk_end = min(base + w.chunk, n); }
		}
		if (w.end != w.chunk_end) {                                  // next piece of the chunk: the part that lies in one segment
			const QueuePiece p = queue_piece(q, n, w.beg);
			w.end = min(w.chunk_end, p.end); w.offset = p.offset;
		}
	}
	const uint32_t take = min(n_want, w.end - w.beg);
	uint32_t got = kNone;
	if (want) { const uint32_t r = mask_rank(m); if (r < take) got = w.beg + r + w.offset; }
	w.beg += take;
	return got;
}

// Persistent wave loop shared by the closest-hit and the any-hit kernels.
//   * a lane is WALKING (t.cur is a record or a leaf), DONE (ri != kNone, t.cur == kHalt: result waiting to be flushed) or EMPTY (ri == kNone);
//   * a refill event (>= kRefillIdle lanes not running) flushes the finished lanes' results, hands the idle lanes the next
//     ray indices of the window and loads + sets up their rays — all as batched, mostly coalesced accesses.  (An earlier
//     version also kept one prefetched ray per lane in registers; with the cone slab constants that pushed the kernel past
//     64 VGPRs, i.e. from two 16-wave workgroups per CU to one, which cost far more than the prefetch saved.)
template <int MODE, bool COUNT, bool ALL_LDS, bool HALF, bool ST16, bool WIDE, class LoadRay, class StoreResult>
MIRT_DI void trace_persistent(const SceneDev& sc, const TraceLds tl, const Queue& q, uint32_t n, uint32_t* work_next, FatList fat, uint32_t& c_nodes, uint32_t& c_spheres,
                              LoadRay load_ray, StoreResult store_result, const Collect col = Collect{ nullptr, 0.0f, 0u }) {
	WaveWindow w{ 0, 0, 0, 0, pick_chunk(n, sc.chunk_max), true };
	Trav t;
	TravSpill spill;
	uint32_t ri = kNone;
	bool occluded = false;
	t.cur = kHalt;
	for (;;) {
		// ---- refill event: flush results, hand the idle lanes the next ray indices of the window, load and set up their rays ----
		if ((ri != kNone) & (t.cur == kHalt)) { store_result(ri, t, occluded); ri = kNone; }
		{
			const uint32_t got = wave_take(ri == kNone, w, q, n, work_next);   // a slot of the stream planes
			if (got != kNone) {
				float px, py, pz, dx, dy, dz, tf;
				load_ray(got, px, py, pz, dx, dy, dz, tf);
				ri = got; occluded = false;
				if (MODE == kCollect) {
					if (trav_begin(t, px, py, pz, dx, dy, dz, tf, col.rho)) { t.prim = static_cast<int32_t>(kCandMax + 1u); t.cur = kHalt; }   // a bundle too wide for the tree: the pixel is traced normally
					else t.prim = 0;                                           // candidates listed so far
				} else if (trav_begin(t, px, py, pz, dx, dy, dz, tf)) {
					const uint32_t k = atomicAdd(fat.count, 1u);               // rare: a few rays per million
					if (k < fat.capacity) { fat.rays[k] = got; ri = kNone; t.cur = kHalt; }   // list full -> traverse it after all (correct, only slow)
				}
			}
		}
		const bool work_left = w.more || w.beg != w.chunk_end;
		if (__ballot(ri != kNone) == 0ull) { if (!work_left) break; continue; }
		const bool can_refill = work_left;
		// ---- step every walking lane until enough lanes have finished to make the next refill worthwhile ----
		// A lane's state is its t.cur: a record index (at a node), kLeafBit | prim (at a leaf) or kHalt.  One pass per iteration, chosen
		// for the whole wave: a LEAF pass (the lanes standing at a leaf intersect their sphere) once at least sc.leaf_batch lanes wait
		// for one or no lane stands at a record, a NODE pass otherwise.  A waiting lane loses the node passes it sits out; the sphere
		// test (~50 VALU instructions with its correctly rounded sqrt) runs at several times the lane density it had inside the node step.
		// (Measured and dropped: REQUESTING THE NEXT RECORD EARLY — as soon as a lane knows its next node, into two register quads
		// live across the passes: 51 VGPR spills around the loop and k_trace 249 -> 276 ms per cfg4 step; the other seven waves of
		// the SIMD already cover the load at the head of each pass.)
		// (Measured and dropped: the same request as an LDS-DMA load — global_load_lds_dwordx4 into one 16-B LDS slot per lane when the
		// lane ARRIVES at a leaf, read by the leaf pass after s_waitcnt vmcnt(0); no registers, but 16 KB less of staged records:
		// k_trace 226 -> 242 ms per cfg4 step.  Halving the resident waves costs 1.43x (227 -> 325 ms), so the loop is neither purely
		// latency-bound nor purely issue-bound.)
		// (Measured and dropped: SPECULATION — a lane parks the leaf it meets in a register and walks on until the wave's next leaf pass,
		// so that node passes keep ~0.68 instead of ~0.61 of their lanes and leaf passes fill up.  The box tests made against the stale
		// tfar cost more than that gains: 46 instead of 41 VALU wave-instructions per ray, k_trace 267 instead of 248 ms per cfg4 step.)
		for (;;) {
			const bool at_leaf = static_cast<int32_t>(t.cur) < 0, at_node = t.cur < kHalt;      // kLeafBit is the sign bit
			const unsigned long long leaf_m = __ballot(at_leaf), node_m = __ballot(at_node);
			const unsigned long long walking = leaf_m | node_m;
			if (walking == 0ull) break;
			if (can_refill && 64u - static_cast<uint32_t>(__popcll(walking)) >= sc.refill_idle) break;
			if (node_m == 0ull || static_cast<uint32_t>(__popcll(leaf_m)) >= sc.leaf_batch) {
				if (at_leaf) leaf_step<MODE, COUNT, ALL_LDS, HALF, ST16>(sc, tl, t, spill, occluded, c_spheres, ri, col);
			} else {
				if (at_node) { if (WIDE) node_step_wide<MODE, COUNT, ALL_LDS, ST16>(sc, tl, t, spill, c_nodes); else node_step<MODE, COUNT, ALL_LDS, HALF, ST16>(sc, tl, t, spill, c_nodes); }
			}
		}
	}
}

// Brute force over all prims (the reference as shipped, BVH.hpp:312 / :365), sphere packets staged
// through LDS one chunk at a time by the whole workgroup.
template <bool ANYHIT, bool COUNT>
MIRT_DI bool traverse_brute(const SceneDev& sc, float4* lds, bool active, float px, float py, float pz, float dx, float dy, float dz,
                            float& tfar, int32_t& primID, uint32_t& n_spheres) {
	bool occluded = false;
	for (uint32_t base = 0; base < sc.n_spheres; base += kBruteChunk) {
		const uint32_t cnt = min(kBruteChunk, sc.n_spheres - base);
		__syncthreads();
		for (uint32_t j = threadIdx.x; j < cnt; j += blockDim.x) lds[j] = sc.spheres[base + j];
		__syncthreads();
		if (active && !(ANYHIT && occluded)) {
			for (uint32_t j = 0; j < cnt; j++) {
				if (COUNT) n_spheres++;
				const float4 s = lds[j];
				if (ANYHIT) { if (sphere_occludes(s, px, py, pz, dx, dy, dz, tfar)) { occluded = true; break; } }
				else sphere_closest(s, static_cast<int32_t>(base + j), px, py, pz, dx, dy, dz, tfar, primID);
			}
		}
	}
	return occluded;
}

// Dynamic LDS of the trace kernels: [records 0..lds_recs) | spheres 0..lds_spheres) | stack kLdsStack x blockDim] for
// the BVH path, or one kBruteChunk sphere buffer for the brute-force path.
MIRT_DI TraceLds stage_bvh(const SceneDev& sc, float4* lds_generic) {
	lds_v4f* lds = (lds_v4f*)lds_generic;
	const v4f* recs = reinterpret_cast<const v4f*>(sc.recs);
	const v4f* sph = reinterpret_cast<const v4f*>(sc.spheres);
	const uint32_t planes = (sc.half_boxes && !sc.wide) ? 2u : 4u;   // float4 per record
	const uint32_t nq = sc.lds_recs * planes;
	if (planes == 2u) { for (uint32_t j = threadIdx.x; j < nq; j += blockDim.x) lds[(j & 1u) * sc.lds_recs + (j >> 1)] = recs[j]; }
	else { for (uint32_t j = threadIdx.x; j < nq; j += blockDim.x) lds[(j & 3u) * sc.lds_recs + (j >> 2)] = recs[j]; }   // AoS in HBM -> plane-major in LDS
	for (uint32_t j = threadIdx.x; j < sc.lds_spheres; j += blockDim.x) lds[nq + j] = sph[j];
	__syncthreads();
	return TraceLds{ lds, lds + nq, (lds_u32*)(lds + nq + sc.lds_spheres) };
}
MIRT_DI bool bvh_all_in_lds(const SceneDev& sc) { return sc.lds_recs == sc.n_recs && sc.lds_spheres == sc.n_spheres; }

// ------------------------------------------------------------------------------------------------
// RAY GENERATION — Renderer.hpp:97-127 (stream init is implicit: radiance 0 / throughput 1 are
// supplied by k_shade<FIRST>, so only p, dir and the path id are written)
// ------------------------------------------------------------------------------------------------
// n / d for n < 2^31 and quotients below 2^20 (slots, tile rows, tile columns) with a precomputed 1/d: the float quotient is
// within one of the truth, one correction step either way makes it exact (hipcc's u32 division is ~40 instructions).
MIRT_DI uint32_t udiv_f(uint32_t n, uint32_t d, float inv_d, uint32_t& rem) {
	uint32_t q = static_cast<uint32_t>(static_cast<float>(n) * inv_d);
	int32_t r = static_cast<int32_t>(n - q * d);
	if (r < 0) { q -= 1u; r += static_cast<int32_t>(d); }
	else if (r >= static_cast<int32_t>(d)) { q += 1u; r -= static_cast<int32_t>(d); }
	rem = static_cast<uint32_t>(r);
	return q;
}
// Global LaunchIndex (Renderer.hpp:75,84-88) of this context's local tile: TileMap::global_tile (tile_map.hpp) without its integer division.
MIRT_DI uint32_t global_tile(const FrameParams& fp, uint32_t local_tile) {
	if (fp.stride_tiles == 0u) return fp.first_tile + local_tile;             // wave-uniform branch
	uint32_t in_run;
	const uint32_t run = udiv_f(local_tile, fp.run_tiles, fp.inv_run_tiles, in_run);
	return fp.first_tile + run * fp.stride_tiles + in_run;
}
MIRT_DI uint32_t tile_seed(const FrameParams& fp, uint32_t tile, uint32_t ID) {      // seed[ID], Renderer.hpp:107 (wraps like the int32 cast): global tile, lane of the tile
	return (tile * kTileSize + ID) * (fp.max_bounces * 2u + 1u);
}
MIRT_DI uint32_t path_seed(const FrameParams& fp, uint32_t pix) {      // mirrors tile_seed(fp, global_tile(fp, pix >> 8), pix & 255)
	return (global_tile(fp, pix >> 8) * kTileSize + (pix & 255u)) * (fp.max_bounces * 2u + 1u);
}
// The camera sample of RAY GENERATION, Renderer.hpp:113-127: accumulation `acc` (= ++accumulations, Renderer.hpp:74) of the pixel (x, y) whose
// seed[ID] is `seed` -> the pinhole direction.
MIRT_DI f3 camera_sample(const CameraParams& cam, int32_t x, int32_t y, uint32_t acc, uint32_t seed) {
	uint32_t rng = hash_2d(acc, seed);                                      // Renderer.hpp:117
	const float s0 = rand_unit_float(rng);
	const float s1 = rand_unit_float(rng);
	return camera_ray_dir(cam, x, y, s0, s1);
}
// The same with the thin lens on top where LENS (device_math.hpp lens_ray): O is written by LENS code only.
template <bool LENS>
MIRT_DI void camera_ray(const FrameParams& fp, const LensParams& lens, int32_t x, int32_t y, uint32_t acc, uint32_t seed, f3& O, f3& D) {
	D = camera_sample(fp.cam, x, y, acc, seed);
	if (LENS) lens_ray(fp.cam, lens, D, acc, seed, fp.max_bounces, O, D);
}
// RAY GENERATION, Renderer.hpp:97-127, for stream index i = slot * n_pix + pix of a batch: path id and direction (the origin
// is cam.pos).  Bounce 0 has no ray stream in HBM: k_trace<PRIMARY> and k_shade<FIRST> both derive the ray from its index
// (~90 VALU instructions each, against 28 B written + 52 B read per primary ray).
MIRT_DI void pixel_xy(const FrameParams& fp, uint32_t pix, uint32_t& tile, int32_t& x, int32_t& y) {     // Renderer.hpp:84-88,115-116
	tile = global_tile(fp, pix >> 8);
	const uint32_t ID = pix & 255u;
	uint32_t col;
	const uint32_t row = udiv_f(tile, fp.h_tiles, fp.inv_h_tiles, col);
	x = static_cast<int32_t>(kTileRoot * col + (ID & 15u));
	y = static_cast<int32_t>(kTileRoot * row + (ID >> 4));
}
MIRT_DI void primary_ray(const FrameParams& fp, uint32_t i, uint32_t& path, float& dx, float& dy, float& dz) {
	uint32_t pix, tile;
	const uint32_t slot = udiv_f(i, fp.n_pix, fp.inv_n_pix, pix);
	int32_t x, y;
	pixel_xy(fp, pix, tile, x, y);
	const uint32_t ID = pix & 255u;
	const uint32_t acc = fp.acc_base + slot + 1u;                           // ++accumulations, Renderer.hpp:74
	const f3 d = camera_sample(fp.cam, x, y, acc, tile_seed(fp, tile, ID));
	path = (slot << fp.pix_bits) | pix;
	dx = d.x; dy = d.y; dz = d.z;
}
// The camera ray of stream index i under a lens (mirt_set_lens with a radius above 0; template parameter LENS of the bounce-0 kernels): the
// thin-lens ray derived from the pinhole direction (device_math.hpp lens_ray) — the one case in which camera rays do not share an origin, so
// every bounce-0 consumer takes origin and direction from here.  `lens` is the trailing argument of those kernels and is read by LENS code only;
// the pinhole branches beside each call are the statements the kernels have always had.
MIRT_DI void lens_camera_ray(const FrameParams& fp, const LensParams& lens, uint32_t i, uint32_t& path, float& px, float& py, float& pz, float& dx, float& dy, float& dz) {
	f3 O, D;
	primary_ray(fp, i, path, D.x, D.y, D.z);
	lens_ray(fp.cam, lens, D, fp.acc_base + (path >> fp.pix_bits) + 1u, path_seed(fp, path & fp.pix_mask), fp.max_bounces, O, D);
	px = O.x; py = O.y; pz = O.z; dx = D.x; dy = D.y; dz = D.z;
}
// The same rays written out as a stream (mirt_debug_raygen only).
template <bool LENS = false>
__global__ __launch_bounds__(kBlock) void k_raygen(FrameParams fp, StreamBuf out, uint32_t* stream_count, LensParams lens) {
	const uint32_t total = fp.n_pix * fp.batch_n;
	if (blockIdx.x == 0 && threadIdx.x == 0) stream_count[0] = total;
	for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < total; i += gridDim.x * kBlock) {
		uint32_t path; float px, py, pz, dx, dy, dz;
		if (LENS) lens_camera_ray(fp, lens, i, path, px, py, pz, dx, dy, dz);
		else { primary_ray(fp, i, path, dx, dy, dz); px = fp.cam.pos[0]; py = fp.cam.pos[1]; pz = fp.cam.pos[2]; }
		out.a[i] = make_float4(px, py, pz, __uint_as_float(path));
		out.b[i] = make_float4(dx, dy, dz, 1.0f);
	}
}

// ------------------------------------------------------------------------------------------------
// INTERSECTION — Traverse, BVH.hpp:309-360
// ------------------------------------------------------------------------------------------------
// Drain one ray queue with the persistent-wave loop (dispatch on the staged-BVH variant).
template <int MODE, bool COUNT, class LoadRay, class StoreResult>
MIRT_DI void trace_queue(const SceneDev& sc, const TraceLds tl, const Queue& q, uint32_t n, uint32_t* work_next, FatList fat, uint32_t& c_nodes, uint32_t& c_spheres,
                         LoadRay load_ray, StoreResult store_result, const Collect col = Collect{ nullptr, 0.0f, 0u }) {
	if (n == 0) return;
	const bool all = bvh_all_in_lds(sc);
	if (sc.half_boxes && sc.wide) {
		if (!sc.stack16) trace_persistent<MODE, COUNT, false, true, false, true>(sc, tl, q, n, work_next, fat, c_nodes, c_spheres, load_ray, store_result, col);   // > 32768 records or spheres: never all in LDS
		else if (all) trace_persistent<MODE, COUNT, true, true, true, true>(sc, tl, q, n, work_next, fat, c_nodes, c_spheres, load_ray, store_result, col);
		else trace_persistent<MODE, COUNT, false, true, true, true>(sc, tl, q, n, work_next, fat, c_nodes, c_spheres, load_ray, store_result, col);
	} else if (sc.half_boxes) {                                              // binary 32-B records: trees too deep for the wide layout
		if (!sc.stack16) trace_persistent<MODE, COUNT, false, true, false, false>(sc, tl, q, n, work_next, fat, c_nodes, c_spheres, load_ray, store_result, col);
		else if (all) trace_persistent<MODE, COUNT, true, true, true, false>(sc, tl, q, n, work_next, fat, c_nodes, c_spheres, load_ray, store_result, col);
		else trace_persistent<MODE, COUNT, false, true, true, false>(sc, tl, q, n, work_next, fat, c_nodes, c_spheres, load_ray, store_result, col);
	} else {
		if (all) trace_persistent<MODE, COUNT, true, false, false, false>(sc, tl, q, n, work_next, fat, c_nodes, c_spheres, load_ray, store_result, col);
		else trace_persistent<MODE, COUNT, false, false, false, false>(sc, tl, q, n, work_next, fat, c_nodes, c_spheres, load_ray, store_result, col);
	}
}

// ------------------------------------------------------------------------------------------------
// Contribution words + the deferred shadow-ray adds
// ------------------------------------------------------------------------------------------------
// Contribution buffer of a batch: [tile][slot][256][rgb] (slot = accumulation index inside the batch), so that a path's three words
// share a sector.  A path's word IS its radiance R (Renderer.hpp:98) for the whole batch: k_shade<FIRST> stores it for every path
// (+0, then what bounce 0 adds at once) — so the buffer is never cleared: k_merge_contrib reads every word — and every later
// `R += ...` of the reference is a read-modify-write of the word, in the reference's order: shadow_finish adds the NEE term of an
// unoccluded shadow ray (and the emissive term that had to wait for it), k_shade the emissive term of a hit without a pending
// light record and the sky term of a miss.  The launches of a batch are stream-ordered and a path has one ray per launch, so the
// word needs no atomics.  A path that ends touches nothing — the word already holds its result —, except the paths still alive
// after the last bounce, which are dropped (Q5): their word is overwritten with +0.
// (The sum starts at +0 and can therefore never be -0: x + 0.0f and 0.0f + x are exact identities on it.)
MIRT_DI size_t contrib_index(uint32_t batch_n, uint32_t pix_bits, uint32_t path) {      // path: below 2^30 (no flag bits)
	const uint32_t slot = path >> pix_bits;
	const uint32_t pix = path & ((1u << pix_bits) - 1u);
	return ((static_cast<size_t>(pix >> 8) * batch_n + slot) * kTileSize + (pix & 255u)) * 3u;
}
// Where a finished shadow ray's radiance goes.  The adds that had to wait for the occlusion test — (R + unoccluded NEE) +
// emissive, the reference's order (Renderer.hpp:307-311, then 339-341 / 348-350) — are made by the lane that traced the
// ray, straight into the path's contribution word: k_trace is VALU-bound, so the few memory instructions per shadow ray ride
// along for free, where a separate pass over the shadow stream cost 4.8 ms per cfg2 step.
//   * light record (the common case: the hit was not emissive): an occluded ray (most of them) touches nothing and an
//     unoccluded one adds its NEE radiance: R + S;
//   * kDestFull record (emissive hit): E travels in the record and (R + S) + E, or R + E behind an occluder, is formed here.
// The record carries the path id in every case, so nothing here is found through another stream.
// occ != nullptr (mirt_debug_trace_shadow): only the occlusion flag is stored.
constexpr uint32_t kDestFull = 0x40000000u;
constexpr uint32_t kDestPath = 0x3fffffffu;     // path ids use bits 0-29 (batch slot << pix_bits | pixel; capacity check in mirt_launch.hip)
constexpr uint32_t kSampledGGX = 0x40000000u;   // k_shade<MIXED>, in a STREAM's path word only (kDestFull, the same bit, lives in shadow records only): the ray's direction was sampled by Closure<GGX>
constexpr uint32_t kViaInterface = 0x80000000u; // k_shade<GLASS>, in a STREAM's path word (StreamBuf::a, never a shadow record's): the ray's direction was sampled by a dielectric interface
struct ShadowSink {
	float* contrib;             // the batch's contribution buffer
	uint32_t batch_n, pix_bits;
	uint32_t* occ;
};
// A shadow ray of the queue: two independent 16-B loads.
MIRT_DI void shadow_ray(const ShadowBuf& sh, uint32_t i, float& px, float& py, float& pz, float& dx, float& dy, float& dz, float& tfar) {
	const float4 a = sh.a[i], b = sh.b[i];
	px = a.x; py = a.y; pz = a.z; tfar = a.w; dx = b.x; dy = b.y; dz = b.z;
}
// (`dest` is read again here rather than kept from the refill: k_trace has no register to hold it across the walk.)
MIRT_DI void shadow_finish(const ShadowBuf& sh, const ShadowSink& sink, uint32_t i, bool occluded, uint32_t& c_term) {
	if (sink.occ) { sink.occ[i] = occluded ? 1u : 0u; return; }
	const uint32_t dw = __float_as_uint(sh.b[i].w);
	if (dw & kDestAccum) c_term++;
	const bool full = (dw & kDestFull) != 0u;
	if (occluded & !full) return;
	float* w = sink.contrib + contrib_index(sink.batch_n, sink.pix_bits, dw & kDestPath);
	f3 R{ w[0], w[1], w[2] };
	if (!occluded) { const float4 S = sh.c[i]; R.x += S.x; R.y += S.y; R.z += S.z; }
	if (full) { const float4 E = sh.d[i]; R.x += E.x; R.y += E.y; R.z += E.z; }
	w[0] = R.x; w[1] = R.y; w[2] = R.z;
}

// INTERSECTION + SHADOW RAY TRACING in one launch: Traverse (BVH.hpp:309-360) for the rays of bounce b and
// Traverse_shadow (BVH.hpp:362-404) for the NEE rays emitted at bounce b-1 — the two queues are independent, and every
// launch ends with a tail while its longest rays finish (~180 us at 16k+ rays, measured), so draining both in one
// persistent kernel halves the number of tails: a wave that runs out of closest-hit rays moves on to the shadow queue.
// Either count pointer may refer to a zero word (first bounce: no shadow rays yet; after the last extension: shadow only).
// 8 waves/SIMD (= two 16-wave workgroups per CU, the LDS plan of the binary16 layout) caps the kernel at 64 VGPRs.
// PRIMARY != 0 = bounce 0: the rays are generated from their index (primary_ray), nothing is read; no shadow rays are pending.
//   kPrimaryAll: every ray i of the batch, numbered 0 .. n_pix * batch_n - 1;  kPrimaryList: every sample of the pixels k_primary_cand
//   listed at in.a (stream_pixel_list: pixels without a candidate list; closest_queue.n[0] = how many); results are stored under the ray's index.
//   kPrimaryActive: the camera rays that walk the tree (policy.trace_primary_rays, a lens, a batch below 3, no tree at all) once a tile is frozen
//   (mirt_freeze_tiles): every sample of the local pixels of the tiles still active, which the host lists when the mask changes and hands over
//   as kPrimaryList's are (in.a, closest_queue.n[0]), in kPrimaryList's numbering.  It has what kPrimaryList leaves out: the brute-force loop of
//   a context without a tree, the thin-lens ray, and ctr->rays (n_active x batch_n; no k_primary_hits runs beside it).  Hit records go to
//   slot * n_pix + pixel as ever; those of frozen pixels are neither written nor read.  Its fat rays are k_trace_fat<., kPrimaryList, LENS>'s.
constexpr int kPrimaryNone = 0, kPrimaryAll = 1, kPrimaryList = 2, kPrimaryActive = 3;
constexpr bool primary_listed(int primary) { return primary == kPrimaryList || primary == kPrimaryActive; }
// kPrimaryList numbering: ray j of n_ov * batch_n is sample slot j / n_ov of the j % n_ov-th listed pixel (slot-major: the lanes of a wave
// take neighbouring pixels of one accumulation, like everywhere else); returns its index in the batch, slot * n_pix + pixel.
MIRT_DI uint32_t primary_list_ray(const FrameParams& fp, const uint32_t* __restrict__ ov_pix, uint32_t n_ov, float inv_n_ov, uint32_t j) {
	uint32_t k;
	const uint32_t slot = udiv_f(j, n_ov, inv_n_ov, k);
	return slot * fp.n_pix + ov_pix[k];
}
// Ray i of a trace launch, origin and direction: at bounce 0 the camera ray of index i in the batch (slot * n_pix + pixel; a listed launch maps
// its ray number through primary_list_ray first) — the thin-lens ray or the pinhole ray from cam.pos —, later the two 16-byte loads of stream slot i.
template <int PRIMARY, bool LENS>
MIRT_DI void trace_ray(const FrameParams& fp, const LensParams& lens, const StreamBuf& in, uint32_t i, float& px, float& py, float& pz, float& dx, float& dy, float& dz) {
	if (PRIMARY && LENS) { uint32_t path; lens_camera_ray(fp, lens, i, path, px, py, pz, dx, dy, dz); }
	else if (PRIMARY) { uint32_t path; primary_ray(fp, i, path, dx, dy, dz); px = fp.cam.pos[0]; py = fp.cam.pos[1]; pz = fp.cam.pos[2]; }
	else { const float4 a = in.a[i], b = in.b[i]; px = a.x; py = a.y; pz = a.z; dx = b.x; dy = b.y; dz = b.z; }
}
// LENS (k_trace: with kPrimaryAll and kPrimaryActive): the camera rays are thin-lens rays (lens_camera_ray); candidate lists are neither built nor read under a lens.
template <bool COUNT, int PRIMARY, bool LENS = false>
__global__ __launch_bounds__(kTraceBlock, 8) void k_trace(SceneDev sc, FrameParams fp,
                                                       StreamBuf in, HitRec* __restrict__ hit_out,
                                                       Queue closest_queue, uint32_t* closest_work,
                                                       ShadowBuf sh, ShadowSink sink,
                                                       Queue shadow_queue, uint32_t* shadow_work, FatList fat_closest, FatList fat_shadow,
                                                       DevCounters* ctr, LensParams lens) {
	static_assert(!LENS || PRIMARY == kPrimaryAll || PRIMARY == kPrimaryActive, "the lens concerns bounce 0 only, and candidate lists are not read under it");
	extern __shared__ float4 lds[];
	const uint32_t n_ov = primary_listed(PRIMARY) ? closest_queue.n[0] : 0u;     // listed pixels (k_primary_cand; the active tiles')
	const float inv_n_ov = 1.0f / static_cast<float>(n_ov ? n_ov : 1u);
	if (PRIMARY) closest_queue.n = nullptr;                                    // identity numbering: ray j is slot j
	const uint32_t nc = PRIMARY == kPrimaryAll ? fp.n_pix * fp.batch_n : primary_listed(PRIMARY) ? n_ov * fp.batch_n : queue_total(closest_queue), ns = PRIMARY ? 0u : queue_total(shadow_queue);
	if (nc + ns == 0) return;
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		if (nc && PRIMARY != kPrimaryList) atomicAdd(&ctr->rays, static_cast<unsigned long long>(nc));     // (k_primary_hits has counted the whole batch)
		if (ns) atomicAdd(&ctr->shadow_rays, static_cast<unsigned long long>(ns));
	}
	uint32_t c_nodes = 0, c_spheres = 0, s_nodes = 0, s_spheres = 0, c_term = 0;
	if (sc.use_bvh && sc.n_recs != 0) {
		if (static_cast<uint64_t>(blockIdx.x) * 64u >= static_cast<uint64_t>(nc) + ns) return;   // more workgroups than minimum-size chunks: skip the staging too
		const TraceLds tl = stage_bvh(sc, lds);
		{
			auto load_ray = [&](uint32_t i, float& px, float& py, float& pz, float& dx, float& dy, float& dz, float& tf) {
				trace_ray<PRIMARY, LENS>(fp, lens, in, primary_listed(PRIMARY) ? primary_list_ray(fp, stream_pixel_list(in), n_ov, inv_n_ov, i) : i, px, py, pz, dx, dy, dz);
				tf = MIRT_FLT_MAX;                                                // hit reset, Renderer.hpp:150-158
			};
			auto store_result = [&](uint32_t i, const Trav& t, bool) { const uint32_t o = primary_listed(PRIMARY) ? primary_list_ray(fp, stream_pixel_list(in), n_ov, inv_n_ov, i) : i; hit_out[o] = HitRec{ t.tfar, t.prim }; };
			trace_queue<kClosest, COUNT>(sc, tl, closest_queue, nc, closest_work, fat_closest, c_nodes, c_spheres, load_ray, store_result);
		}
		if (!PRIMARY) {
			auto load_ray = [&](uint32_t i, float& px, float& py, float& pz, float& dx, float& dy, float& dz, float& tf) {
				shadow_ray(sh, i, px, py, pz, dx, dy, dz, tf);
			};
			auto store_result = [&](uint32_t i, const Trav&, bool occluded) { shadow_finish(sh, sink, i, occluded, c_term); };
			trace_queue<kAnyHit, COUNT>(sc, tl, shadow_queue, ns, shadow_work, fat_shadow, s_nodes, s_spheres, load_ray, store_result);
		}
	} else {
		// brute force over all prims (the reference as shipped); also the no-spheres case
		const QueueView qc = PRIMARY ? queue_identity(nc) : queue_view(closest_queue);      // (kPrimaryList is never launched without a tree)
		const QueueView qs = PRIMARY ? queue_identity(0u) : queue_view(shadow_queue);
		for (uint32_t base = blockIdx.x * kTraceBlock; base < nc; base += gridDim.x * kTraceBlock) {
			const bool active = base + threadIdx.x < nc;
			const uint32_t i = !active ? 0u : PRIMARY == kPrimaryActive ? primary_list_ray(fp, stream_pixel_list(in), n_ov, inv_n_ov, base + threadIdx.x) : queue_slot(qc, base, base + threadIdx.x);
			float px = 0, py = 0, pz = 0, dx = 1, dy = 1, dz = 1;
			if (active) {                          // mirrors trace_ray<PRIMARY, LENS> (spelled out: through the call hipcc assigns other registers here)
				if (PRIMARY && LENS) { uint32_t path; lens_camera_ray(fp, lens, i, path, px, py, pz, dx, dy, dz); }
				else if (PRIMARY) { uint32_t path; primary_ray(fp, i, path, dx, dy, dz); px = fp.cam.pos[0]; py = fp.cam.pos[1]; pz = fp.cam.pos[2]; }
				else { const float4 a = in.a[i], b = in.b[i]; px = a.x; py = a.y; pz = a.z; dx = b.x; dy = b.y; dz = b.z; }
			}
			float tfar = MIRT_FLT_MAX;             // hit reset, Renderer.hpp:150-158
			int32_t prim = -1;
			if (sc.use_bvh == 0) traverse_brute<false, COUNT>(sc, lds, active, px, py, pz, dx, dy, dz, tfar, prim, c_spheres);
			if (active) hit_out[i] = HitRec{ tfar, prim };
		}
		for (uint32_t base = blockIdx.x * kTraceBlock; base < ns; base += gridDim.x * kTraceBlock) {
			const bool active = base + threadIdx.x < ns;
			const uint32_t i = active ? queue_slot(qs, base, base + threadIdx.x) : 0u;
			float px = 0, py = 0, pz = 0, dx = 1, dy = 1, dz = 1, tfar = 0;
			if (active) shadow_ray(sh, i, px, py, pz, dx, dy, dz, tfar);
			bool occluded = false;
			int32_t dummy = -1;
			if (sc.use_bvh == 0) occluded = traverse_brute<true, COUNT>(sc, lds, active, px, py, pz, dx, dy, dz, tfar, dummy, s_spheres);
			if (active) shadow_finish(sh, sink, i, occluded, c_term);
		}
	}
	wave_sum(c_term, &ctr->terminated);
	if (COUNT) { wave_sum(c_nodes, &ctr->nodes); wave_sum(c_spheres, &ctr->spheres); wave_sum(s_nodes, &ctr->shadow_nodes); wave_sum(s_spheres, &ctr->shadow_spheres); }
}

// Fat rays (see trav_begin): one workgroup per ray runs the reference's brute-force loops over ALL prims —
// intersect_prims (BVH.hpp:236-288; closest = lexicographic minimum of (dist, prim index), i.e. the ascending strict-'<' scan)
// for the closest-hit list, intersect_prims_shadow (BVH.hpp:290-305) for the shadow list.
template <bool COUNT, int PRIMARY, bool LENS = false>
__global__ __launch_bounds__(1024) void k_trace_fat(SceneDev sc, FrameParams fp, StreamBuf in, HitRec* __restrict__ hit_out, FatList fat_closest,
                                                    ShadowBuf sh, ShadowSink sink, FatList fat_shadow, DevCounters* ctr, const uint32_t* ov_count, LensParams lens) {
	__shared__ float s_t[16];
	__shared__ int32_t s_p[16];
	const uint32_t nc = min(*fat_closest.count, fat_closest.capacity), ns = min(*fat_shadow.count, fat_shadow.capacity);
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
	const uint32_t n_ov = PRIMARY == kPrimaryList ? *ov_count : 0u;
	const float inv_n_ov = 1.0f / static_cast<float>(n_ov ? n_ov : 1u);
	for (uint32_t k = blockIdx.x; k < nc; k += gridDim.x) {
		const uint32_t i = PRIMARY == kPrimaryList ? primary_list_ray(fp, stream_pixel_list(in), n_ov, inv_n_ov, fat_closest.rays[k]) : fat_closest.rays[k];
		float px, py, pz, dx, dy, dz;
		trace_ray<PRIMARY, LENS>(fp, lens, in, i, px, py, pz, dx, dy, dz);
		float tfar = MIRT_FLT_MAX; int32_t prim = -1;
		for (uint32_t p = threadIdx.x; p < sc.n_spheres; p += blockDim.x) sphere_closest(sc.spheres[p], static_cast<int32_t>(p), px, py, pz, dx, dy, dz, tfar, prim);
		// lexicographic (dist, prim) minimum across the workgroup; prim -1 = no hit, always loses (its tfar is FLT_MAX and every hit is < FLT_MAX)
		for (int off = 32; off > 0; off >>= 1) {
			const float ot = __shfl_down(tfar, off, 64); const int32_t op = __shfl_down(prim, off, 64);
			const bool take = (op >= 0) & ((prim < 0) | (ot < tfar) | ((ot == tfar) & (op < prim)));
			tfar = take ? ot : tfar; prim = take ? op : prim;
		}
		__syncthreads();
		if (lane == 0) { s_t[wave] = tfar; s_p[wave] = prim; }
		__syncthreads();
		if (threadIdx.x == 0) {
			for (uint32_t w = 1; w < n_waves; w++) {
				const float ot = s_t[w]; const int32_t op = s_p[w];
				const bool take = (op >= 0) && ((prim < 0) || (ot < tfar) || ((ot == tfar) && (op < prim)));
				if (take) { tfar = ot; prim = op; }
			}
			hit_out[i] = HitRec{ tfar, prim };
			if (COUNT) atomicAdd(&ctr->spheres, static_cast<unsigned long long>(sc.n_spheres));
		}
	}
	for (uint32_t k = blockIdx.x; k < ns; k += gridDim.x) {
		const uint32_t i = fat_shadow.rays[k];
		float px, py, pz, dx, dy, dz, tfar;
		shadow_ray(sh, i, px, py, pz, dx, dy, dz, tfar);
		bool occ = false;
		for (uint32_t p = threadIdx.x; p < sc.n_spheres && !occ; p += blockDim.x) occ = sphere_occludes(sc.spheres[p], px, py, pz, dx, dy, dz, tfar);
		const int any = __syncthreads_or(occ ? 1 : 0);
		if (threadIdx.x == 0) {
			uint32_t c_term = 0;
			shadow_finish(sh, sink, i, any != 0, c_term);
			if (c_term) atomicAdd(&ctr->terminated, 1ull);
			if (COUNT) atomicAdd(&ctr->shadow_spheres, static_cast<unsigned long long>(sc.n_spheres));
		}
	}
}

// ------------------------------------------------------------------------------------------------
// PRIMARY RAYS THROUGH PER-PIXEL CANDIDATE LISTS (see kCollect above)
// ------------------------------------------------------------------------------------------------
// One cone per local pixel: axis = Camera::generate_ray (Camera.hpp:80-88) through the pixel centre, half-angle rho (host:
// 0.7072 / |projection.z| + margins — the jitter moves a sample by at most half a pixel per axis in the image plane, whose
// points are at least |z| from the eye).  Same persistent-wave traversal as k_trace; the result is the pixel's candidate list.
template <bool COUNT>
__global__ __launch_bounds__(kTraceBlock, 8) void k_primary_cand(SceneDev sc, FrameParams fp, uint32_t* __restrict__ cand, float rho, uint32_t* work, FatList unused, DevCounters* ctr,
                                                                uint32_t* __restrict__ ov_pix, uint32_t* __restrict__ ov_count) {
	extern __shared__ float4 lds[];
	const uint32_t n = fp.n_pix;
	if (n == 0 || static_cast<uint64_t>(blockIdx.x) * 64u >= n) return;
	const TraceLds tl = stage_bvh(sc, lds);
	uint32_t c_nodes = 0, c_spheres = 0;
	auto load_ray = [&](uint32_t pix, float& px, float& py, float& pz, float& dx, float& dy, float& dz, float& tf) {
		uint32_t tile; int32_t x, y;
		pixel_xy(fp, pix, tile, x, y);
		const f3 d = camera_ray_dir(fp.cam, x, y, 0.5f, 0.5f);
		px = fp.cam.pos[0]; py = fp.cam.pos[1]; pz = fp.cam.pos[2]; dx = d.x; dy = d.y; dz = d.z; tf = MIRT_FLT_MAX;
	};
	auto store_result = [&](uint32_t pix, const Trav& t, bool) {
		const bool over = static_cast<uint32_t>(t.prim) > kCandMax;
		cand[pix] = over ? kCandOverflow : static_cast<uint32_t>(t.prim);
		// pixels without a list: every sample is traced by k_trace<kPrimaryList>.  One atomic per wave and flush for the lanes that report one.
		const unsigned long long m = __ballot(over);
		if (over) {
			const uint32_t leader = static_cast<uint32_t>(__ffsll(static_cast<long long>(m))) - 1u;
			uint32_t first = 0;
			if (lane_id() == leader) first = atomicAdd(ov_count, static_cast<uint32_t>(__popcll(m)));
			first = __builtin_amdgcn_readlane(first, leader);
			if (ov_pix) ov_pix[first + mask_rank(m)] = pix;
		}
	};
	trace_queue<kCollect, COUNT>(sc, tl, Queue{ nullptr, 0u }, n, work, unused, c_nodes, c_spheres, load_ray, store_result, Collect{ cand, rho, n });
	if (COUNT) { wave_sum(c_nodes, &ctr->nodes); wave_sum(c_spheres, &ctr->spheres); }
}
// cand_listed ∩ active (mirt_freeze_tiles): the listed pixels — those without a candidate list, whose samples k_trace<., kPrimaryList> traces — that
// lie in a tile still active, compacted into `out` in any order (wave64 ballot + mbcnt prefix, one returning atomic per wave and 64 pixels).
// Built when the mask or the lists change; k_trace<., kPrimaryList> then reads `out` / `out_count` in place of the list and its count, so no
// camera ray of a frozen tile is traced.  `out` holds at least n_pix words, *out_count is zero at launch.
__global__ __launch_bounds__(kBlock) void k_listed_active(const uint32_t* __restrict__ listed, const uint32_t* __restrict__ n_listed, const uint32_t* __restrict__ tile_frozen,
                                                          uint32_t* __restrict__ out, uint32_t* __restrict__ out_count) {
	const uint32_t n = *n_listed;
	for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {     // block-uniform bounds: every lane reaches the ballot
		const uint32_t i = base + threadIdx.x;
		uint32_t pix = 0u;
		bool keep = false;
		if (i < n) { pix = listed[i]; keep = tile_frozen[pix >> 8] == 0u; }
		const unsigned long long m = __ballot(keep);
		if (keep) {
			const uint32_t leader = static_cast<uint32_t>(__ffsll(static_cast<long long>(m))) - 1u;
			uint32_t first = 0;
			if (lane_id() == leader) first = atomicAdd(out_count, static_cast<uint32_t>(__popcll(m)));
			first = __builtin_amdgcn_readlane(first, leader);
			out[first + mask_rank(m)] = pix;
		}
	}
}
// Traverse (BVH.hpp:309-360) for the camera rays of a batch, given the lists: one lane per PIXEL runs the batch's accumulations over it.  What
// depends on the pixel alone — tile, x, y, seed[ID], the list and its first kCandRegs spheres — is set up once, so a sample costs its ray
// (hash_2d, two PCG draws, the quaternion rotation and normalisation of Camera::generate_ray, Camera.hpp:80-88) + the exact sphere tests on
// registers (sphere_closest_tie: the reference's arithmetic; the (dist, prim index) minimum does not depend on the order of the list) + one 8-B
// hit record, written for 64 neighbouring pixels at a time.  (Round 2 ran one lane per SAMPLE: every ray paid the pixel's set-up and walked the
// list through three dependent loads — 7.3 ms per cfg4 batch of 537 M rays.)  Pixels without a list are skipped: k_trace<kPrimaryList> traces
// all their samples.
constexpr uint32_t kCandRegs = 3;
// SPARSE (a template argument of every bounce-0 kernel below and of the merge; launched once a tile is frozen — mirt_freeze_tiles):
// tile_frozen[local tile] != 0 marks a tile that takes no more samples.  Its pixels are skipped — no ray, no hit
// record, no store of any kind — and ctr->rays counts active_pix = 256 x the active tiles instead of n_pix.  The owned pixel space, path ids and
// every buffer's indexing stay what they are; after bounce 0 the streams are compact queues that never held a frozen pixel.
// The arguments that only SPARSE (tile_frozen, active_pix) or RIS (ris_m) code reads are always present, last, and the other instantiations never
// load them.  Every instantiation's device code was held to that of the kernel it replaces, listing by listing (profiles/one_kernel_per_stage.txt).
template <bool COUNT, bool SPARSE = false>
__global__ __launch_bounds__(kBlock) void k_primary_hits(SceneDev sc, FrameParams fp, const uint32_t* __restrict__ cand, HitRec* __restrict__ hit_out, DevCounters* ctr,
                                                         const uint32_t* __restrict__ tile_frozen, uint32_t active_pix) {
	if (blockIdx.x == 0 && threadIdx.x == 0 && fp.n_pix) atomicAdd(&ctr->rays, static_cast<unsigned long long>(SPARSE ? active_pix : fp.n_pix) * fp.batch_n);     // Renderer.hpp:165: every camera ray of the batch
	uint32_t c_spheres = 0;
	const float ox = fp.cam.pos[0], oy = fp.cam.pos[1], oz = fp.cam.pos[2];
	for (uint32_t pix = blockIdx.x * kBlock + threadIdx.x; pix < fp.n_pix; pix += gridDim.x * kBlock) {
		if (SPARSE && tile_frozen[pix >> 8] != 0u) continue;
		const uint32_t cnt = cand[pix];
		if (cnt == kCandOverflow) continue;
		uint32_t tile; int32_t x, y;
		pixel_xy(fp, pix, tile, x, y);
		const uint32_t seed = tile_seed(fp, tile, pix & 255u);
		float4 s[kCandRegs]; int32_t id[kCandRegs];
		for (uint32_t k = 0; k < kCandRegs; k++) {
			id[k] = k < cnt ? static_cast<int32_t>(cand[static_cast<size_t>(k + 1u) * fp.n_pix + pix]) : -1;
			s[k] = sc.spheres[id[k] < 0 ? 0 : id[k]];
		}
		for (uint32_t slot = 0; slot < fp.batch_n; slot++) {
			const f3 d = camera_sample(fp.cam, x, y, fp.acc_base + slot + 1u, seed);
			float tfar = MIRT_FLT_MAX; int32_t prim = -1;                          // hit reset, Renderer.hpp:150-158
			for (uint32_t k = 0; k < kCandRegs; k++) if (id[k] >= 0) sphere_closest_tie(s[k], id[k], ox, oy, oz, d.x, d.y, d.z, tfar, prim);
			for (uint32_t k = kCandRegs; k < kCandMax; k++) {                      // the rest of a long list, from L1
				if (__ballot(k < cnt) == 0ull) break;
				if (k < cnt) {
					const uint32_t j = cand[static_cast<size_t>(k + 1u) * fp.n_pix + pix];
					sphere_closest_tie(sc.spheres[j], static_cast<int32_t>(j), ox, oy, oz, d.x, d.y, d.z, tfar, prim);
				}
			}
			if (COUNT) c_spheres += cnt;
			const size_t i = static_cast<size_t>(slot) * fp.n_pix + pix;
			hit_out[i] = HitRec{ tfar, prim };
		}
	}
	if (COUNT) wave_sum(c_spheres, &ctr->spheres);
}
// The same, turned round for a batch that fills a wave: one wave per PIXEL, one lane per accumulation of the batch.  What the lanes of
// k_primary_hits wait for — the longest list among 64 pixels, and a list word + a sphere gathered again by every sample — is wave-uniform here:
// a wave takes a run of kWaveHitsRun consecutive local pixels (one row of a tile), lane k fetches entry k of the pixel's list and that sphere
// ONCE (the fetches of the next pixel are issued before the tests of this one), and the test loop hands them round with v_readlane, so every
// lane runs exactly `cnt` sphere tests on scalar operands.  The per-sample arithmetic is k_primary_hits', in list order; the records are
// bit-identical.  Accumulations beyond 64 go in further groups of 64 lanes (cfg4: one group of 63; 192: three).
// hit_out stays [slot][pixel] (k_shade<FIRST>, k_first_hit_aov and k_trace<kPrimaryList> read that): a lane storing its own slot's plane would
// issue 8-B stores n_pix * 8 B apart, so the run's 16 x 64 records are staged in LDS — private to the wave: no workgroup barrier — and leave
// with the lanes remapped to (slot, pixel of the run): 16 lanes = one slot's 16 records = one 128-B segment.  Column ^ pixel in the staging
// rows keeps both the writes (64 slots of a pixel) and the reads (16 pixels of a slot) off each other's banks.
// 8 KB of LDS per wave: 20 waves per CU (5 per SIMD) whatever the workgroup size; the registers would allow 8 — the kernel is bound by VALU
// issue, which five waves keep busy.
// (hits_wave_map.hpp: kWaveHitsMinBatch, the batch size from which this kernel runs, kWaveHitsRun and the staging indices.)
constexpr uint32_t kWaveHitsWaves = kBlock / 64u;
static_assert(kCandMax < 64u && kTileSize % kWaveHitsRun == 0u && kWaveHitsRun == kTileRoot, "lane k holds list entry k; a run is one row of a tile");
// SPARSE: a run is one row of ONE tile, so the test of its tile is wave-uniform (a scalar load and branch).
template <bool COUNT, bool SPARSE = false>
__global__ __launch_bounds__(kBlock) void k_primary_hits_wave(SceneDev sc, FrameParams fp, const uint32_t* __restrict__ cand, HitRec* __restrict__ hit_out, DevCounters* ctr,
                                                              const uint32_t* __restrict__ tile_frozen, uint32_t active_pix) {
	__shared__ HitRec stage[kWaveHitsWaves][kWaveHitsStage];
	const uint32_t lane = lane_id();
	const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
	const uint32_t n_runs = fp.n_pix / kWaveHitsRun, n_groups = hits_wave_groups(fp.batch_n);
	const uint32_t out_p = hits_wave_out_pixel(lane);                              // write-out: this lane's pixel of the run
	uint32_t c_spheres = 0;
	const float ox = fp.cam.pos[0], oy = fp.cam.pos[1], oz = fp.cam.pos[2];
	for (uint32_t run = blockIdx.x * kWaveHitsWaves + wave; run < n_runs; run += gridDim.x * kWaveHitsWaves) {
		const uint32_t base = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(run * kWaveHitsRun)));     // first local pixel of the run: wave-uniform
		if (SPARSE && tile_frozen[base >> 8] != 0u) continue;
		const uint32_t cnt_v = cand[base + out_p];                                   // lane p (and p + 16, ...): the count of pixel p of the run
		const uint32_t skip = static_cast<uint32_t>(__ballot(cnt_v == kCandOverflow)) & 0xffffu;      // pixels without a list: k_trace<kPrimaryList> writes their records
		if (skip == 0xffffu) continue;
		uint32_t tile; int32_t x0, y;
		pixel_xy(fp, base, tile, x0, y);                                             // the run's pixels: (x0 + p, y), ID = (base & 255) + p
		const uint32_t seed0 = tile * kTileSize + (base & 255u), seed_mul = fp.max_bounces * 2u + 1u;
		auto count_of = [&](uint32_t p) { return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(cnt_v), static_cast<int>(p))) + 1u; };   // entries + 1; 0 without a list
		// Lane k's entry of pixel p's list, and that sphere.  Every lane loads, whatever the list's length — the lanes beyond it read the last entry
		// again (the count word of an empty list) and sphere 0, and nobody reads what they hold: with loads that some lanes or some passes skip, the
		// in-order load counter would have to be waited down to zero before the tests, with the next pixel's loads just issued.
		auto load_ids = [&](uint32_t p) { const uint32_t c1 = count_of(p); return cand[static_cast<size_t>(min(lane + 1u, c1 ? c1 - 1u : 0u)) * fp.n_pix + base + p]; };
		auto load_sphere = [&](uint32_t p, uint32_t j) { return sc.spheres[lane + 1u < count_of(p) ? j : 0u]; };
		for (uint32_t g = 0; g < n_groups; g++) {
			const uint32_t slot = g * 64u + lane;                                     // lanes beyond batch_n compute a ray nobody stores
			uint32_t id_cur = load_ids(0), id_next = load_ids(1);
			float4 s_cur = load_sphere(0, id_cur);
			for (uint32_t p = 0; p < kWaveHitsRun; p++) {
				// the sphere of pixel p + 1 and the list entry of pixel p + 2 (the run's last pixel again beyond it): in flight during the tests of pixel p
				const float4 s_next = load_sphere(min(p + 1u, kWaveHitsRun - 1u), id_next);
				const uint32_t id_next2 = load_ids(min(p + 2u, kWaveHitsRun - 1u));
				const uint32_t cnt1 = count_of(p);
				if (cnt1 != 0u) {
					const uint32_t cnt = cnt1 - 1u;
					uint32_t rng = hash_2d(fp.acc_base + slot + 1u, (seed0 + p) * seed_mul);      // mirrors camera_sample(.., tile_seed(fp, tile, (base & 255) + p)), Renderer.hpp:74,107,117
					const float s0 = rand_unit_float(rng);
					const float s1 = rand_unit_float(rng);
					const f3 d = camera_ray_dir(fp.cam, x0 + static_cast<int32_t>(p), y, s0, s1);
					float tfar = MIRT_FLT_MAX; int32_t prim = -1;                          // hit reset, Renderer.hpp:150-158
					for (uint32_t k = 0; k < cnt; k++) {
						const int32_t j = __builtin_amdgcn_readlane(static_cast<int>(id_cur), static_cast<int>(k));
						const float4 s{ __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s_cur.x), static_cast<int>(k))), __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s_cur.y), static_cast<int>(k))),
						                __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s_cur.z), static_cast<int>(k))), __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s_cur.w), static_cast<int>(k))) };
						sphere_closest_tie(s, j, ox, oy, oz, d.x, d.y, d.z, tfar, prim);
					}
					if (COUNT && slot < fp.batch_n) c_spheres += cnt;
					stage[wave][hits_wave_stage_index(p, lane)] = HitRec{ tfar, prim };
				}
				id_cur = id_next; id_next = id_next2; s_cur = s_next;
			}
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
			const uint32_t n_slots = hits_wave_group_slots(fp.batch_n, g);
			if (!((skip >> out_p) & 1u)) {
				for (uint32_t pass = 0; pass < kWaveHitsPasses; pass++) {
					const uint32_t s = hits_wave_out_slot(lane, pass);
					if (s >= n_slots) break;
					hit_out[static_cast<size_t>(g * 64u + s) * fp.n_pix + base + out_p] = stage[wave][hits_wave_stage_index(out_p, s)];
				}
			}
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
		}
	}
	if (COUNT) wave_sum(c_spheres, &ctr->spheres);
	if (blockIdx.x == 0 && threadIdx.x == 0 && fp.n_pix) atomicAdd(&ctr->rays, static_cast<unsigned long long>(SPARSE ? active_pix : fp.n_pix) * fp.batch_n);     // Renderer.hpp:165: every camera ray of the batch
}

// ------------------------------------------------------------------------------------------------
// FIRST BOUNCE OUTPUTS — Renderer.hpp:216-231 (written down in the reference, compiled out there): per pixel, the running sums of the
// camera ray's hit distance (1e4 on a miss), its world-space shading normal and the colour its closure is set up with (:208-210).
// Slab [local tile][plane 0..6][256] f32 (AccumulationTile with seven planes instead of buckets x 3; not bucketed): plane 0 depth,
// 1-3 N.xyz, 4-6 albedo (policy.brdf = 0) or F0 (policy.brdf = 1) — `mat_colour` is that table.
// One lane per local pixel, as in k_primary_hits: tile, x, y and seed[ID] are set up once, the seven sums live in registers over the
// batch's accumulations — added in accumulation order, which is part of the result — and are stored once.  A sample costs its ray
// (regenerated as k_shade<FIRST> does) + its 8-B hit record, read for 64 neighbouring pixels at a time; the sphere and colour of a hit
// are fetched again only when the prim differs from the previous sample's (the samples of a pixel mostly hit the same sphere).
// The hit arithmetic is the closest-hit shader's of k_shade, operation for operation.  Counts nothing into DevCounters.
// ------------------------------------------------------------------------------------------------
// LENS: the sample's thin-lens ray (lens_ray) instead of the pinhole ray — origin and direction both differ per sample.
// SPARSE: the sums of a frozen tile stop with its accumulator (its hit records are not written either).
template <bool LENS, bool SPARSE = false>
__global__ __launch_bounds__(kBlock) void k_first_hit_aov(SceneDev sc, FrameParams fp, const HitRec* __restrict__ hit_in, const float4* __restrict__ mat_colour, float* __restrict__ aov, LensParams lens,
                                                          const uint32_t* __restrict__ tile_frozen) {
	f3 O{ fp.cam.pos[0], fp.cam.pos[1], fp.cam.pos[2] };
	for (uint32_t pix = blockIdx.x * kBlock + threadIdx.x; pix < fp.n_pix; pix += gridDim.x * kBlock) {
		if (SPARSE && tile_frozen[pix >> 8] != 0u) continue;
		uint32_t tile; int32_t x, y;
		pixel_xy(fp, pix, tile, x, y);
		const uint32_t seed = tile_seed(fp, tile, pix & 255u);
		float* w = aov + static_cast<size_t>(pix >> 8) * (kAovPlanes * kTileSize) + (pix & 255u);
		float sum[kAovPlanes];
		for (uint32_t k = 0; k < kAovPlanes; k++) sum[k] = w[k * kTileSize];
		int32_t cached = -1;
		float4 hs = make_float4(0.0f, 0.0f, 0.0f, 0.0f), colour = hs;
		for (uint32_t slot = 0; slot < fp.batch_n; slot++) {
			f3 D;
			camera_ray<LENS>(fp, lens, x, y, fp.acc_base + slot + 1u, seed, O, D);
			const HitRec h = hit_in[static_cast<size_t>(slot) * fp.n_pix + pix];
			if (h.prim < 0) { sum[0] += kAovMissDepth; continue; }
			if (h.prim != cached) { hs = sc.spheres[h.prim]; colour = mat_colour[sc.prim_mat[h.prim]]; cached = h.prim; }
			const float depth = h.tfar;
			const f3 hit{ O.x + D.x * depth, O.y + D.y * depth, O.z + D.z * depth };      // mirrors shade_hit_body.inc's hit and N, Renderer.hpp:169-214
			f3 N = normalize3(f3{ hit.x - hs.x, hit.y - hs.y, hit.z - hs.z });
			if (dot3(N, D) >= 0.0f) N = f3{ -N.x, -N.y, -N.z };
			sum[0] += depth;
			sum[1] += N.x; sum[2] += N.y; sum[3] += N.z;
			sum[4] += colour.x; sum[5] += colour.y; sum[6] += colour.z;
		}
		for (uint32_t k = 0; k < kAovPlanes; k++) w[k * kTileSize] = sum[k];
	}
}
// ------------------------------------------------------------------------------------------------
// Accumulator addressing — AccumulationTile<k>, Renderer.hpp:43-46,84: [tile][bucket][r,g,b][256]
// ------------------------------------------------------------------------------------------------
// Sky::operator(), Primitives.hpp:35-46
MIRT_DI f3 sky_eval(const SceneDev& sc, float x, float y, float z) {
	const float ex = sc.hdri_fw * (0.5f + MIRT_INV_TWO_PI * fast_atan2(z, x));
	const float ey = sc.hdri_fh * (0.5f - MIRT_INV_PI * fast_asin(y));
	const float4 t = sc.hdri[static_cast<int32_t>(ey) * sc.hdri_w + static_cast<int32_t>(ex)];
	return { t.x * sc.ambient[0], t.y * sc.ambient[1], t.z * sc.ambient[2] };
}

// ------------------------------------------------------------------------------------------------
// The environment map as a light (mirt_set_sky_sampling; the definition is in mirt.h, "sampling the environment map")
// ------------------------------------------------------------------------------------------------
// sky_eval truncates ex = hdri_fw * u and ey = hdri_fh * v, so the image is seen through cols = max(w - 1, 1) by rows = max(h - 1, 1) CELLS: cell
// (r, c) is ex in [c, c + 1), ey in [r, r + 1) and shows texel (r, c).  The table is one allocation of floats:
//   marg[rows]        running sums of the row sums: marg[r] = rowsum[0] + ... + rowsum[r]; marg[rows - 1] is the total
//   rowsum[rows]      the row sums themselves (= the last running sum of each row)
//   tn[rows + 1]      1 - sin el(k), k = 0 .. rows, el(k) = pi (0.5 - k / rows): the cell edges in latitude, as the distance from y = +1 ...
//   ts[rows + 1]      1 + sin el(k): ... and from y = -1 (each rounded from float64: near a pole sin el itself would lose the cell to cancellation)
//   cond[rows * cols] running sums of the importances within each row
//   dens[rows * cols] p(cell) = I / (Omega * total), in 1 / sr

// Running sums of n values by one 256-thread workgroup in a FIXED order: thread t owns the K = ceil(n / 256) consecutive values [t K, t K + K) and
// sums them left to right from +0 (l_j); thread 0 then sums the 256 chunk sums left to right (pre_t = the sum of the chunks before t); the running
// sum at value t K + j is pre_t + l_j.  The last running sum is therefore pre_255 + chunk sum 255 = the value thread 0's loop ends with: what is
// returned as the total to every thread.  A value takes at most K - 1 + 255 + 1 additions; no atomics, and the order does not depend on the launch.
// `in` and `out` may be the same array (a thread reads its own chunk before it writes it).  s_pre = 257 floats of LDS.  All threads, converged.
constexpr uint32_t kSkyBlock = 256;
MIRT_DI float sky_block_scan(const float* in, float* out, uint32_t n, float* s_pre) {
	const uint32_t K = (n + kSkyBlock - 1u) / kSkyBlock;
	const uint32_t first = threadIdx.x * K;
	float l = 0.0f;
	for (uint32_t j = first; j < first + K && j < n; j++) l += in[j];
	__syncthreads();                                                       // (s_pre may still be read from an earlier scan)
	s_pre[threadIdx.x + 1u] = l;
	__syncthreads();
	if (threadIdx.x == 0) { float run = 0.0f; s_pre[0] = 0.0f; for (uint32_t t = 1; t <= kSkyBlock; t++) { run += s_pre[t]; s_pre[t] = run; } }
	__syncthreads();
	if (out) {
		const float pre = s_pre[threadIdx.x];
		l = 0.0f;
		for (uint32_t j = first; j < first + K && j < n; j++) { l += in[j]; out[j] = pre + l; }
	}
	return s_pre[kSkyBlock];
}
// Pass 1, one workgroup per row of cells: the cell importances I = max(t.r amb.r, t.g amb.g, t.b amb.b) * Omega(r) (RIS's weight rule times the
// cell's solid angle), left in dens[] for pass 2, and the row's sum.  Omega(r) = (2 pi / cols) (sin el(r) - sin el(r + 1)) and the edge tables come
// from float64 (the difference of two binary32 sines would lose half the digits at the equator of a 2048-row map), each rounded to binary32 once.
__global__ __launch_bounds__(kSkyBlock) void k_sky_importance(const float4* __restrict__ hdri, int32_t hdri_w, float amb_r, float amb_g, float amb_b, uint32_t rows, uint32_t cols, float* __restrict__ table) {
	__shared__ float s_pre[kSkyBlock + 1];
	const SkyTable sky{ table, rows, cols };
	const uint32_t r = blockIdx.x;
	const double half = 0.5 * (3.14159265358979323846 / static_cast<double>(rows));
	const float omega = static_cast<float>((6.28318530717958647692 / static_cast<double>(cols)) * (2.0 * sin((2.0 * r + 1.0) * half) * sin(half)));
	if (threadIdx.x == 0) {
		for (uint32_t k = r; k <= (r + 1u == rows ? rows : r); k++) {         // edge r, and the last row also writes edge `rows`
			const double sn = sin(k * half), ss = sin((rows - k) * half);
			table[2u * rows + k] = static_cast<float>(2.0 * sn * sn);
			table[3u * rows + 1u + k] = static_cast<float>(2.0 * ss * ss);
		}
	}
	float* I = table + (sky.dens() - sky.t) + static_cast<size_t>(r) * cols;
	const float4* texel = hdri + static_cast<size_t>(r) * static_cast<size_t>(hdri_w);
	for (uint32_t c = threadIdx.x; c < cols; c += kSkyBlock) {
		const float4 t = texel[c];
		I[c] = max_sel(max_sel(t.x * amb_r, t.y * amb_g), t.z * amb_b) * omega;
	}
	__syncthreads();
	const float sum = sky_block_scan(I, nullptr, cols, s_pre);
	if (threadIdx.x == 0) table[rows + r] = sum;
}
// Pass 2, one workgroup per row: every workgroup sums the row sums to the same total (the same order, hence the same word); workgroup 0 also
// stores their running sums; then the row's own running sums and, from I still in dens[], the densities I / (Omega * total).
__global__ __launch_bounds__(kSkyBlock) void k_sky_scan(uint32_t rows, uint32_t cols, float* __restrict__ table) {
	__shared__ float s_pre[kSkyBlock + 1];
	const SkyTable sky{ table, rows, cols };
	const uint32_t r = blockIdx.x;
	const float total = sky_block_scan(sky.rowsum(), r == 0 ? table : nullptr, rows, s_pre);
	float* I = table + (sky.dens() - sky.t) + static_cast<size_t>(r) * cols;
	(void)sky_block_scan(I, table + (sky.cond() - sky.t) + static_cast<size_t>(r) * cols, cols, s_pre);
	const double half = 0.5 * (3.14159265358979323846 / static_cast<double>(rows));
	const float omega = static_cast<float>((6.28318530717958647692 / static_cast<double>(cols)) * (2.0 * sin((2.0 * r + 1.0) * half) * sin(half)));
	const float norm = omega * total;
	__syncthreads();                                                       // the scan's second loop has read every I
	for (uint32_t c = threadIdx.x; c < cols; c += kSkyBlock) I[c] = I[c] / norm;
}

// Smallest i in [0, n) with cdf[i] > x; the caller has x < cdf[n - 1].  ~log2(n) dependent loads.
MIRT_DI uint32_t sky_upper(const float* cdf, uint32_t n, float x) {
	uint32_t lo = 0u, hi = n - 1u;
	while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (cdf[mid] > x) hi = mid; else lo = mid + 1u; }
	return lo;
}
MIRT_DI float sky_below(float v) { return __uint_as_float(__float_as_uint(v) - 1u); }     // the binary32 below a positive v
// sky_sample: (u0, u1) -> a direction and the density q (1 / sr) it was drawn with.  Operation order, one binary32 rounding each:
//   x = min(u0 * total, below(total));  row = the first r with marg[r] > x;  lo = marg[r - 1] (0 for r = 0)
//   du = min((x' - lo') / (hi' - lo'), 1 - 2^-24) for the column, from u1, the row's sum and its running sums
//   the row's remainder is measured from the edge NEARER A POLE, where cos(elevation) = sqrt(t (2 - t)) is ill-conditioned in anything else:
//     a cell above the equator (the straddling row: the half of it x falls in): dv = min((x - lo) / (hi - lo), 1 - 2^-24) from the upper edge,
//       t = ta + dv * (tb - ta) over tn (the distance from y = +1), y = 1 - t
//     a cell below it: dw = (hi - x) / (hi - lo) from the lower edge (> 0: x < hi), t = tb + dw * (ta - tb) over ts (the distance from y = -1), y = t - 1
//   — either way uniform in sin(elevation)
//   cos_el = sqrt(t * (2 - t));  phi = ((col - cols / 2) + du) * (2 pi / cols): uniform in azimuth;  dir = (cos_el cos phi, y, cos_el sin phi)
// — the inverse of the latitude-longitude map of sky_eval (u = 1/2 + atan2(z, x) / 2 pi, v = 1/2 - asin(y) / pi) with exact arc functions.
// A row or cell whose running sum does not rise is never picked, so q > 0.
MIRT_DI f3 sky_sample(const SkyTable& sky, float u0, float u1, float& q, uint32_t& row, uint32_t& col) {
	const float* marg = sky.marg();
	const float total = marg[sky.rows - 1u];
	const float x = min_sel(u0 * total, sky_below(total));
	row = sky_upper(marg, sky.rows, x);
	const float lo = row ? marg[row - 1u] : 0.0f;
	const float hi = marg[row];
	const float* cond = sky.cond() + static_cast<size_t>(row) * sky.cols;
	const float rowsum = cond[sky.cols - 1u];
	const float y_ = min_sel(u1 * rowsum, sky_below(rowsum));
	col = sky_upper(cond, sky.cols, y_);
	const float lo2 = col ? cond[col - 1u] : 0.0f;
	const float du = min_sel((y_ - lo2) / (cond[col] - lo2), 0x1.fffffep-1f);
	q = sky.dens()[static_cast<size_t>(row) * sky.cols + col];
	const bool north = 2u * row + 1u == sky.rows ? (x - lo) <= (hi - x) : 2u * row + 1u < sky.rows;
	const float* edge = north ? sky.tn() : sky.ts();
	const float ta = edge[row], tb = edge[row + 1u];
	const float t = north ? ta + min_sel((x - lo) / (hi - lo), 0x1.fffffep-1f) * (tb - ta) : tb + ((hi - x) / (hi - lo)) * (ta - tb);
	const float y = north ? 1.0f - t : t - 1.0f;
	const float cos_el = __builtin_sqrtf(max_sel(0.0f, t * (2.0f - t)));
	// (phi through float64 and rounded once: in binary32 the scale 2 pi / cols and the product would each cost up to pi 2^-24 near the meridian)
	const double dcols = static_cast<double>(sky.cols);
	const float phi = static_cast<float>(((static_cast<double>(col) - 0.5 * dcols) + static_cast<double>(du)) * (6.28318530717958647692 / dcols));
	float sn, cs; sincosf(phi, &sn, &cs);
	return { cos_el * cs, y, cos_el * sn };
}
// sky_pdf: the density of the cell that sky_eval's own arithmetic (fast_atan2 / fast_asin) names for the direction — a function of the direction alone, what
// both MIS weights are formed from.  Texel column w - 1 and row h - 1 (ex = hdri_fw, ey = hdri_fh exactly: measure zero) count as the last cell.
MIRT_DI float sky_pdf(const SceneDev& sc, const SkyTable& sky, float x, float y, float z, uint32_t& row, uint32_t& col) {
	const float ex = sc.hdri_fw * (0.5f + MIRT_INV_TWO_PI * fast_atan2(z, x));
	const float ey = sc.hdri_fh * (0.5f - MIRT_INV_PI * fast_asin(y));
	const uint32_t c = static_cast<uint32_t>(static_cast<int32_t>(ex)), r = static_cast<uint32_t>(static_cast<int32_t>(ey));
	col = c < sky.cols ? c : sky.cols - 1u;
	row = r < sky.rows ? r : sky.rows - 1u;
	return sky.dens()[static_cast<size_t>(row) * sky.cols + col];
}

// ------------------------------------------------------------------------------------------------
// SHADE — closest-hit shader, NEE, emissive, BRDF sample + Russian roulette + compaction, miss, accumulate
// (Renderer.hpp:169-431).  FIRST = bounce 0: throughput 1 (Renderer.hpp:98-101) without reading it, and the path's contribution
// word — its radiance for the rest of the batch (contrib_index) — is stored here for every path: +0 and what bounce 0 adds at once.
// ------------------------------------------------------------------------------------------------
// Dense list of the rays for which `flag` is set, in LDS: list[rank] = value; returns the number of entries.  All threads
// of the block, converged.  scratch = 17 words.  (Two barriers; the list may be read after return.)
MIRT_DI uint32_t block_compact(bool flag, uint32_t value, uint32_t* scratch, uint32_t* list) {
	const unsigned long long m = __ballot(flag);
	const uint32_t wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
	if (lane_id() == 0) scratch[wave] = static_cast<uint32_t>(__popcll(m));
	__syncthreads();
	uint32_t before = 0, total = 0;
	for (uint32_t w = 0; w < n_waves; w++) { const uint32_t c = scratch[w]; before += (w < wave) ? c : 0u; total += c; }
	if (flag) list[before + mask_rank(m)] = value;
	__syncthreads();
	return total;
}

// Block-iterations.  A later bounce reads a stream: iteration t covers its ray numbers [512 t, 512 t + 512), t = blockIdx.x, + gridDim.x, ...
// Bounce 0 (FIRST) has no stream — ray i = slot * n_pix + pixel is a function of its index — and runs PIXEL-MAJOR: a workgroup takes chunks of
// 512 local pixels (two tiles) and runs all the batch's accumulations over each, so what depends on the pixel alone (tile, x, y, seed[ID],
// seed[ID]) is set up once per chunk.  Its hit records come from k_primary_hits (pixels with a candidate list) or k_trace.
// (Measured and dropped twice: the candidate tests inside this kernel instead of k_primary_hits — ray-major in round 2, pixel-major in
// round 3: at 6 waves per SIMD and 80 VGPRs the list's dependent loads cost k_shade<FIRST> 5 ms per cfg4 batch, as much as the kernel saved.)
// Phase 2 (closest-hit shader, NEE, emissive MIS, closure sample, roulette) is shade_hit_body.inc, the text k_tile_stream shades its hits with too.
// GGX = #define BRDF 1 (Renderer.hpp:70): every closure is Closure<GGX> (DataStreams.hpp:184-219) with F0 = material.F0 and
// alpha = r^2 + (1 - r^2) * gloss_decay (Renderer.hpp:210-212; `gloss_decay` = the host's table at this bounce, one launch per
// bounce), read from mat_ggx = {F0.xyz, roughness}.  Its pdf() is 0: NEE weighs 1 / light_pdf and emitters hit by an extension
// ray weigh powerHeuristic(0, .) = 0.  GGX = false does not read mat_ggx and gloss_decay.
// LENS (with FIRST only): bounce 0 re-derives the thin-lens ray (lens_ray) — its origin is the sample's lens point, not cam.pos.  Same launch
// bounds as the pinhole variants; `lens` is read by LENS code only.
// SPARSE (with FIRST only): the lanes whose pixel lies in a frozen tile behave as the lanes beyond n_pix do — they take part in the barriers and
// in the compaction, but read no hit record, emit nothing and store nothing, their path's contribution word included.
// RIS (mirt_set_light_ris): next event estimation picks its light among ris_m candidates by resampled importance sampling (shade_hit_body.inc) —
// ris_m is 1 .. MIRT_MAX_LIGHT_RIS, the same for every lane.  The same text, the same launch bounds.
// GLASS (mirt_set_transmission, launched only while the scene has a transmissive material): such a material can take the dielectric interface of
// shade_hit_body.inc, read from s_glass = sc.mat_glass.  pdf_in is recomputed from D (Q8), so "D was sampled by an interface" — an emitter it reaches
// weighs 1 — travels as kViaInterface in the stream's path word: set where the survivor is stored, taken off where the word is read (phase 2) or
// turned into a contribution index (phase 1).  GLASS = false reads neither, and is the text as it was.  The same launch bounds.
// SKY (mirt_set_sky_sampling, launched only while the table's total is above 0, the scene has ambient light and MIS is on): the environment map is
// light number n_lights of next event estimation, drawn from `sky` (sky_sample) with one shadow ray of tfar = FLT_MAX, and the miss shader weighs
// thr.r x sky by the MIS weight phase 2 stored for the ray in StreamBuf::w (bounce 0: 1).  SKY = false names neither `sky` nor the plane.
// MIXED (mirt_set_material_closures, launched only while the scene's materials do not all take one closure; GGX = false): a hit is shaded by the
// closure of its material — bit `mat` of closure_mask (MIRT_MAX_MATERIALS is 63), a kernel argument, so it stays in a scalar register pair — in one
// wave without sorting: a wave with hits of both kinds runs both branches.  Both tables are staged: s_albedo = sc.mat_albedo, s_ggx = mat_ggx.
// Q8's pdf_in belongs to the closure that SAMPLED the ray, so "sampled by Closure<GGX>" travels as kSampledGGX in the stream's path word, as
// kViaInterface does.  MIXED = false names neither the mask nor s_ggx, and is the text as it was.  The same launch bounds.
// PDF (mirt_set_ggx_pdf, launched only while some material of the scene ends up GGX: with GGX or MIXED, never the all-Lambertian form): Closure<GGX>::pdf
// is ggx_pdf instead of 0 in the three MIS weights that read it — next event estimation's, the emitter hit's and (SKY) the miss shader's.  The
// emitter hit's is p~ of the hit that SAMPLED the ray, so it travels in a plane beside the stream (pdf_plane_out, indexed as `out` is; pdf_plane_in
// as `in` is; nullptr without the switch): written with the survivor, read back as pdf_in in phase 2
// (a Lambertian-sampled ray stores Q8's word there, the bits it would otherwise recompute).  The closure sample, its estimator and the roulette
// read nothing new.  PDF = false names neither ggx_pdf nor the plane, and is the text as it was.  The same launch bounds.
//
// ShadeForm: k_shade's nine template arguments as one value, in their order — what the host decides per launch (mirt_launch.hip shade_form) and
// looks up in its table of instantiations (shade_kernel).  valid() is the one statement of which combinations exist: 5 bounce forms (later
// bounce; bounce 0, with the lens, with frozen tiles, with both) x 8 of (RIS, GLASS, SKY) x 5 of closure and pdf (Lambertian, GGX, MIXED, GGX + PDF,
// MIXED + PDF).  A new switch is one more member, one more bit and, if it cannot stand alone, one more term of valid().
struct ShadeForm {
	bool first, ggx, lens, sparse, ris, glass, sky, mixed, pdf;
	static constexpr uint32_t kBits = 9u;
	constexpr uint32_t bits() const {
		return uint32_t(first) | uint32_t(ggx) << 1 | uint32_t(lens) << 2 | uint32_t(sparse) << 3 | uint32_t(ris) << 4 | uint32_t(glass) << 5 | uint32_t(sky) << 6 | uint32_t(mixed) << 7 | uint32_t(pdf) << 8;
	}
	static constexpr ShadeForm from_bits(uint32_t b) {
		return ShadeForm{ (b & 1u) != 0, (b >> 1 & 1u) != 0, (b >> 2 & 1u) != 0, (b >> 3 & 1u) != 0, (b >> 4 & 1u) != 0, (b >> 5 & 1u) != 0, (b >> 6 & 1u) != 0, (b >> 7 & 1u) != 0, (b >> 8 & 1u) != 0 };
	}
	constexpr bool valid() const { return (!(lens || sparse) || first) && !(mixed && ggx) && (!pdf || ggx || mixed); }
};
constexpr uint32_t shade_forms_valid() {
	uint32_t n = 0;
	for (uint32_t b = 0; b < (1u << ShadeForm::kBits); b++) n += ShadeForm::from_bits(b).valid() && ShadeForm::from_bits(b).bits() == b;
	return n;
}
static_assert(shade_forms_valid() == 200u, "k_shade has 5 bounce forms x 8 of (RIS, GLASS, SKY) x 5 of closure and pdf = 200 instantiations");
// Waves per SIMD a form is compiled for, and with it the workgroups of 512 a CU holds (waves / 2: launch_batch sizes the grid by it).  The later
// bounces wait on memory three quarters of their time, so the two forms whose text fits 64 VGPRs with no more scratch than it had at 80 — the
// Lambertian and the GGX one without a further switch — run as k_shade<ShadeWaves8, ...>: 8 waves, four workgroups.  They fit only without the packed
// FP32 instructions (v_pk_mul_f32 and kin want even-aligned register pairs, and their loop-invariant constant pairs were what spilled): the same IEEE
// operations in the same order, one lane-wide instruction each — target("no-packed-fp32-ops").  A kernel whose target features differ from its
// callees' gets none of them inlined unless they are always_inline: MIRT_DI functions are, the HIP headers' __float_as_uint, make_float4,
// __syncthreads ... are not and became real calls (s_swappc_b64, each waiting for every load in flight), hence `flatten`, which inlines every call
// the kernel's own text makes.  The listing of these two kernels must hold no s_swappc (profiles/shade_occupancy.txt; Makefile, mirt_launch.o).
// Bounce 0 is bound by VALU issue and keeps its packed instructions; the other later-bounce forms were not measured: they stay k_shade, as they were.
constexpr uint32_t shade_waves(ShadeForm f) { return (f.first || f.lens || f.sparse || f.ris || f.glass || f.sky || f.mixed || f.pdf) ? 6u : 8u; }
#if defined(__HIP_DEVICE_COMPILE__)
#define MIRT_NO_PACKED_F32 __attribute__((target("no-packed-fp32-ops"), flatten))
#else
#define MIRT_NO_PACKED_F32
#endif
#define MIRT_SHADE_PARAMS SceneDev sc, FrameParams fp, StreamBuf in, const HitRec* __restrict__ hit_in, StreamBuf out, ShadowBuf sh, uint32_t bounce, \
                          Queue in_queue, Queue next_queue, Queue shadow_queue, float* __restrict__ contrib, DevCounters* ctr, \
                          const float4* __restrict__ mat_ggx, float gloss_decay, LensParams lens, uint32_t ris_m, const uint32_t* __restrict__ tile_frozen, SkyTable sky, \
                          unsigned long long closure_mask, const float* __restrict__ pdf_plane_in, float* __restrict__ pdf_plane_out
// One text, two kernels: shade_kernel_body.inc is the body of both (included as statements, as shade_hit_body.inc is: a shared function moved the
// register assignment of the forms that stay k_shade).
template <bool FIRST, bool GGX, bool LENS = false, bool SPARSE = false, bool RIS = false, bool GLASS = false, bool SKY = false, bool MIXED = false, bool PDF = false>
__global__ __launch_bounds__(kShadeBlock, 6) void k_shade(MIRT_SHADE_PARAMS) {
	static_assert(ShadeForm{ FIRST, GGX, LENS, SPARSE, RIS, GLASS, SKY, MIXED, PDF }.valid(),
	              "the lens and the frozen tiles concern bounce 0 only; "
	              "MIXED takes the closure from the material: it is instantiated with GGX = false; "
	              "the GGX pdf concerns hits that Closure<GGX> shades: the all-Lambertian form has no PDF instantiation");
#include "shade_kernel_body.inc"
}
// (The 8-wave kernel is an overload of the same name told apart by a leading tag, k_shade<ShadeWaves8, false, GGX>: what reads kernel names
// — bench.py's roll-up of a counter pass, the scripts under profiles/ — keeps finding every shading launch under `k_shade<`.)
struct ShadeWaves8 {};
template <typename WAVES8, bool FIRST, bool GGX, bool LENS = false, bool SPARSE = false, bool RIS = false, bool GLASS = false, bool SKY = false, bool MIXED = false, bool PDF = false>
__global__ __launch_bounds__(kShadeBlock, 8) MIRT_NO_PACKED_F32 void k_shade(MIRT_SHADE_PARAMS) {
	static_assert(ShadeForm{ FIRST, GGX, LENS, SPARSE, RIS, GLASS, SKY, MIXED, PDF }.valid() && shade_waves(ShadeForm{ FIRST, GGX, LENS, SPARSE, RIS, GLASS, SKY, MIXED, PDF }) == 8u,
	              "only the forms shade_waves names fit 64 VGPRs");
#include "shade_kernel_body.inc"
}
#undef MIRT_SHADE_PARAMS

// ------------------------------------------------------------------------------------------------
// EXACT STREAM ORDER (mirt_set_stream_order) — Renderer.hpp:83-432 with the reference's stream slots
// ------------------------------------------------------------------------------------------------
// The one thing the wavefront kernels above normalise (Q14): intersect_prims runs the stream eight rays at a time through the FMA
// body (BVH.hpp:250-268) and the last `active_rays % 8` rays through an unfused scalar tail (BVH.hpp:270-286).  Which rays those are
// depends on the slot a path holds after the per-bounce counting sort by material (DataStreams.hpp:221-253) and the in-order
// compaction of the survivors (Renderer.hpp:357-404), so this mode keeps the reference's unit of work: one 256-thread workgroup is
// one tile's stream of one accumulation, lane ID is stream slot ID, and the whole bounce loop runs inside the kernel.
//   * the ray of slot ID lives in lane ID's registers; the survivors are written to their new slots in one LDS copy of the stream
//     (13 dword planes: p, dir, throughput, radiance, pixelID) and read back by the lane of that slot;
//   * traversal is the reference's as shipped (USEBVH false): every sphere in ascending BVH-order index, packets staged through a
//     kBruteChunk LDS buffer — for every ray of the mode, since the tree's conservative boxes were argued for the FMA form only;
//   * a survivor's new slot = survivors with a smaller key (material; a miss never survives) + survivors with the same key in a lower
//     slot — what the stable counting sort followed by the in-order compaction gives —, from a (key, wave) table of ballot
//     popcounts and a 256-entry prefix sum; no atomics, no serial lane;
//   * a path's radiance is stored once, into its word of the batch's contribution buffer, at the bounce where it ends (+0 for a path
//     dropped after the last bounce, Q5), so every word of the (tile, slot) is written and k_merge_contrib applies the slots as usual.
// The shading of a hit is k_shade's: one text, shade_hit_body.inc, included by both (stream_shade_hit).
// Scalar tail of intersect_prims, BVH.hpp:270-286: separate multiply and add, dimension by dimension (built with -ffp-contract=off).
MIRT_DI void sphere_closest_scalar_tail(float4 s, int32_t prim, float px, float py, float pz, float dx, float dy, float dz,
                                        float& tfar, int32_t& primID) {
	float b = 0.0f;
	float disc = s.w;
	float temp = s.x - px;
	b += dx * temp;
	disc -= temp * temp;
	temp = s.y - py;
	b += dy * temp;
	disc -= temp * temp;
	temp = s.z - pz;
	b += dz * temp;
	disc -= temp * temp;
	disc += b * b;
	if (disc < 0.0f) return;
	disc = __builtin_sqrtf(disc);
	const float dist = (b >= disc ? b - disc : b + disc);
	if (dist < 0.0f || dist >= tfar) return;
	tfar = dist; primID = prim;
}
// What one hit leaves behind: shade_hit_body.inc for the ray (O, D, thr) of a stream slot that hit `prim` at `stream_depth`.
struct StreamHit {
	bool survive, has_shadow, has_E;
	f3 P, ndir, L, srad, E, thr;
	float light_distance;
};
template <bool GGX>
MIRT_DI void stream_shade_hit(const SceneDev& sc, const FrameParams& fp, const float4* s_albedo, const float4* s_emission, uint32_t bounce, float gloss_decay,
                              uint32_t stream_acc, uint32_t stream_seed, f3 stream_O, f3 D, f3 thr, float stream_depth, int32_t prim, StreamHit& h) {
	const float light_selection_pdf = 1.0f / static_cast<float>(fp.n_lights);  // Renderer.hpp:78
	const float pdf_in = (GGX || bounce == 0u) ? 0.0f : MIRT_INV_PI * max_sel(0.0f, D.z);      // out->pdf of the bounce that sampled D (Q8); Closure<GGX>::pdf = 0
	const HitRec hrec{ stream_depth, prim };
	bool& survive = h.survive; bool& has_shadow = h.has_shadow; bool& has_E = h.has_E;
	f3& P = h.P; f3& ndir = h.ndir; f3& L = h.L; f3& srad = h.srad; f3& E = h.E;
	float& light_distance = h.light_distance;
	bool terminated = false;                                                   // here: a shaded hit that does not survive
	constexpr bool RIS = false; constexpr uint32_t ris_m = 0u;                 // exact stream order replays the reference: one uniform draw
	constexpr bool GLASS = false, after_interface = false;                     // ... and no closure of the reference reads transmission (mirt_set_transmission excludes this mode)
	const float4* const s_glass = nullptr; bool via_interface = false;         // named by the GLASS text only: never evaluated here
	constexpr bool MIXED = false; constexpr unsigned long long closure_mask = 0ull;   // ... and takes every closure from policy.brdf (mirt_set_material_closures excludes this mode)
	const float4* const s_ggx = nullptr; bool sampled_ggx = false;             // named by the MIXED text only: never evaluated here
	constexpr bool SKY = false; const SkyTable sky{}; float miss_w = 1.0f;     // ... and draws its NEE light among the sphere lights only (mirt_set_sky_sampling excludes this mode)
	constexpr bool PDF = false; float pdf_out = 0.0f;                          // ... and Closure<GGX>::pdf is the reference's 0 (mirt_set_ggx_pdf excludes this mode)
#define SHADE_HIT_ORIGIN stream_O
#define SHADE_HIT_ACC stream_acc
#define SHADE_HIT_SEED stream_seed
#include "shade_hit_body.inc"
	(void)via_interface; (void)miss_w; (void)sky; (void)sampled_ggx; (void)s_ggx; (void)pdf_out;
	if (!terminated) h.thr = thr;                                            // the survivor's throughput
}
constexpr uint32_t kStreamPlanes = 13;          // p, dir, throughput, radiance, pixelID
constexpr uint32_t kStreamKeys = 64;            // material keys 0 .. MIRT_MAX_MATERIALS - 1 (Renderer.hpp:23,92)
// gloss_decay: the host's table by bounce (n_decay entries, the rest 0), GGX only.  count: policy.count_traffic.
template <bool GGX>
__global__ __launch_bounds__(kTileSize, 4) void k_tile_stream(SceneDev sc, FrameParams fp, float* __restrict__ contrib, DevCounters* ctr,
                                                              const float4* __restrict__ mat_ggx, const float* __restrict__ gloss_decay, uint32_t n_decay, uint32_t count) {
	__shared__ float4 s_chunk[kBruteChunk];
	__shared__ float s_stream[kStreamPlanes][kTileSize];
	__shared__ uint32_t s_rank[kStreamKeys * 4u];                              // [key][wave]: survivors of that key in that wave, then their first new slot
	__shared__ uint32_t s_wave_total[4];
	__shared__ float4 s_albedo[MIRT_MAX_MATERIALS + 1], s_emission[MIRT_MAX_MATERIALS + 1];      // GGX: s_albedo = {F0, roughness}
	const uint32_t ID = threadIdx.x, wave = ID >> 6, lane = ID & 63u;
	const uint32_t tile_local = blockIdx.x / fp.batch_n, slot = blockIdx.x - tile_local * fp.batch_n;      // one workgroup per (local tile, batch slot)
	float* out = contrib + static_cast<size_t>(blockIdx.x) * (kTileSize * 3u);    // [tile][slot][256][rgb]
	for (uint32_t m = ID; m < sc.n_mat; m += kTileSize) { s_albedo[m] = GGX ? mat_ggx[m] : sc.mat_albedo[m]; s_emission[m] = sc.mat_emission[m]; }

	// stream init + RAY GENERATION, Renderer.hpp:97-127: slot ID of bounce 0 is pixel ID
	const uint32_t tile = global_tile(fp, tile_local);
	const uint32_t tile_row = tile / fp.h_tiles, tile_col = tile - tile_row * fp.h_tiles;
	const uint32_t seed_stride = fp.max_bounces * 2u + 1u;
	const uint32_t acc = fp.acc_base + slot + 1u;                                // ++accumulations, Renderer.hpp:74
	uint32_t pixelID = ID;
	f3 O{ fp.cam.pos[0], fp.cam.pos[1], fp.cam.pos[2] }, D, thr{ 1.0f, 1.0f, 1.0f }, R{ 0.0f, 0.0f, 0.0f };
	D = camera_sample(fp.cam, static_cast<int32_t>(kTileRoot * tile_col + (ID & 15u)), static_cast<int32_t>(kTileRoot * tile_row + (ID >> 4)), acc, tile_seed(fp, tile, ID));
	uint32_t c_term = 0, c_drop = 0, c_shadow = 0;
	unsigned long long c_shadow_spheres = 0;                                     // sphere tests of this lane's shadow rays (reported with count_traffic)
	unsigned long long c_rays = 0;                                               // sum of active_rays over the bounces (uniform)
	uint32_t active_rays = kTileSize;
	for (uint32_t bounce = 0; bounce < fp.max_bounces && active_rays > 0u; bounce++) {     // Renderer.hpp:131
		const bool active = ID < active_rays;
		const bool tail = ID >= (active_rays & ~7u);                             // BVH.hpp:270: the rays the 8-wide body leaves over
		const bool last_bounce = !(bounce < fp.max_bounces - 1u);                // Renderer.hpp:358
		c_rays += active_rays;
		// INTERSECTION: intersect_prims over all prims, BVH.hpp:236-288,312
		float tfar = MIRT_FLT_MAX;                                                // hit reset, Renderer.hpp:150-158
		int32_t prim = -1;
		for (uint32_t base = 0; base < sc.n_spheres; base += kBruteChunk) {
			const uint32_t cnt = min(kBruteChunk, sc.n_spheres - base);
			__syncthreads();
			for (uint32_t j = ID; j < cnt; j += kTileSize) s_chunk[j] = sc.spheres[base + j];
			__syncthreads();
			if (active) {
				if (tail) { for (uint32_t j = 0; j < cnt; j++) sphere_closest_scalar_tail(s_chunk[j], static_cast<int32_t>(base + j), O.x, O.y, O.z, D.x, D.y, D.z, tfar, prim); }
				else { for (uint32_t j = 0; j < cnt; j++) sphere_closest(s_chunk[j], static_cast<int32_t>(base + j), O.x, O.y, O.z, D.x, D.y, D.z, tfar, prim); }
			}
		}
		// closest-hit shader .. BRDF sample for the hits; the miss shader; Q5 for what is alive after the last bounce
		StreamHit h;
		h.survive = false; h.has_shadow = false; h.has_E = false;
		bool ended = false;                                                       // this path's radiance is final at this bounce
		int32_t key = -1;                                                         // matID, DataStreams.hpp:221-253 (-1 = miss)
		if (active) {
			if (prim < 0) {
				if (sc.has_ambient) {                                                // MISS SHADER, Renderer.hpp:408-420 (Q10: throughput.r scales all three channels)
					const f3 sky = sky_eval(sc, D.x, D.y, D.z);
					R.x += thr.x * sky.x; R.y += thr.x * sky.y; R.z += thr.x * sky.z;
				}
				ended = true; c_term++;
			} else if (last_bounce) {
				R = { 0.0f, 0.0f, 0.0f };                                            // Q5: never accumulated
				ended = true; c_drop++;
			} else {
				key = sc.prim_mat[prim];
				const float decay = (GGX && bounce < n_decay) ? gloss_decay[bounce] : 0.0f;
				stream_shade_hit<GGX>(sc, fp, s_albedo, s_emission, bounce, decay, acc, (tile * kTileSize + pixelID) * seed_stride, O, D, thr, tfar, prim, h);      // the seed mirrors tile_seed(fp, tile, pixelID)
			}
		}
		// SHADOW RAY TRACING: intersect_prims_shadow over all prims, BVH.hpp:290-305,365 (wave-uniform skip when no lane of the tile has one)
		if (__syncthreads_or(h.has_shadow ? 1 : 0)) {
			int32_t unused = -1;
			uint32_t tested = 0;                                                     // at most n_spheres per ray
			const bool occluded = traverse_brute<true, true>(sc, s_chunk, h.has_shadow, h.P.x, h.P.y, h.P.z, h.L.x, h.L.y, h.L.z, h.light_distance, unused, tested);
			c_shadow_spheres += tested;
			if (h.has_shadow) {
				c_shadow++;
				if (!occluded) { R.x += h.srad.x; R.y += h.srad.y; R.z += h.srad.z; } // Renderer.hpp:304-314
			}
		}
		if (h.has_E) { R.x += h.E.x; R.y += h.E.y; R.z += h.E.z; }                    // Renderer.hpp:339-341 / 348-350, after the NEE add
		if (active && key >= 0 && !h.survive) { ended = true; c_term++; }            // Russian roulette ended it
		if (ended) { float* w = out + pixelID * 3u; w[0] = R.x; w[1] = R.y; w[2] = R.z; }   // ACCUMULATION, Renderer.hpp:424-430 (the add itself: k_merge_contrib)

		// the survivors' slots in the next stream: (key, old slot) order
		const uint32_t k = static_cast<uint32_t>(key) & (kStreamKeys - 1u);
		s_rank[ID] = 0u;
		__syncthreads();
		uint32_t rank_in_wave = 0u;
		for (unsigned long long rem = __ballot(h.survive); rem != 0ull;) {
			const uint32_t leader = static_cast<uint32_t>(__ffsll(static_cast<long long>(rem))) - 1u;
			const uint32_t k_now = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int32_t>(k), static_cast<int32_t>(leader)));
			const bool mine = h.survive & (k == k_now);
			const unsigned long long m = __ballot(mine);
			if (mine) rank_in_wave = mask_rank(m);
			if (lane == leader) s_rank[k_now * 4u + wave] = static_cast<uint32_t>(__popcll(m));
			rem &= ~m;
		}
		__syncthreads();
		const uint32_t mine_cnt = s_rank[ID];                                      // entry ID = (key ID / 4, wave ID % 4): index order is (key, wave) order
		uint32_t incl = mine_cnt;
		for (uint32_t off = 1u; off < 64u; off <<= 1) { const uint32_t t = __shfl_up(incl, off, 64); if (lane >= off) incl += t; }
		if (lane == 63u) s_wave_total[wave] = incl;
		__syncthreads();
		uint32_t before = 0u, total = 0u;
		for (uint32_t w = 0; w < 4u; w++) { const uint32_t c = s_wave_total[w]; before += (w < wave) ? c : 0u; total += c; }
		s_rank[ID] = before + incl - mine_cnt;
		__syncthreads();
		if (h.survive) {
			const uint32_t ns = s_rank[k * 4u + wave] + rank_in_wave;
			s_stream[0][ns] = h.P.x; s_stream[1][ns] = h.P.y; s_stream[2][ns] = h.P.z;
			s_stream[3][ns] = h.ndir.x; s_stream[4][ns] = h.ndir.y; s_stream[5][ns] = h.ndir.z;
			s_stream[6][ns] = h.thr.x; s_stream[7][ns] = h.thr.y; s_stream[8][ns] = h.thr.z;
			s_stream[9][ns] = R.x; s_stream[10][ns] = R.y; s_stream[11][ns] = R.z;
			s_stream[12][ns] = __uint_as_float(pixelID);
		}
		__syncthreads();
		active_rays = total;                                                       // Renderer.hpp:431
		if (ID < active_rays) {
			O = { s_stream[0][ID], s_stream[1][ID], s_stream[2][ID] };
			D = { s_stream[3][ID], s_stream[4][ID], s_stream[5][ID] };
			thr = { s_stream[6][ID], s_stream[7][ID], s_stream[8][ID] };
			R = { s_stream[9][ID], s_stream[10][ID], s_stream[11][ID] };
			pixelID = __float_as_uint(s_stream[12][ID]);
		}
		// (the next write of the stream copy lies behind the barriers of the next bounce's shadow vote and slot table)
	}
	if (ID == 0u) {
		atomicAdd(&ctr->rays, c_rays);
		if (count) atomicAdd(&ctr->spheres, c_rays * sc.n_spheres);             // every ray meets every sphere, as the brute-force reference counts them
	}
	wave_sum(c_term, &ctr->terminated);
	wave_sum(c_drop, &ctr->dropped);
	wave_sum(c_shadow, &ctr->shadow_rays);
	if (count) wave_sum(c_shadow_spheres, &ctr->shadow_spheres);
}

// In-order merge of one batch's contribution buffer ([tile][slot][256][rgb], slot = accumulation index inside the batch; see
// contrib_index) into the accumulator ([tile][bucket][rgb][256]; see launch_batch in mirt_launch.hip): exactly the
// `output_color[px] += radiance` of Renderer.hpp:427-429, one add per (pixel, bucket) per Accumulate() call.  Accumulation
// acc_base+k+1 lands in bucket (acc_base+k+1) % buckets (Renderer.hpp:82); each accumulator word is owned by one thread, which
// applies that bucket's contributions in ascending k, i.e. in accumulation order.  A thread owns 4 pixels of a tile: per slot it
// reads their 12 interleaved words (three float4) and adds them to the 4-pixel float4 of each channel plane.
// SPARSE: a frozen tile is neither read nor written — its words of the contribution buffer are stale (the buffer is never cleared).
template <bool SPARSE = false>
__global__ __launch_bounds__(kBlock) void k_merge_contrib(float4* __restrict__ accum, const float4* __restrict__ contrib, uint32_t n_tiles, uint32_t buckets,
                                                          uint32_t batch_n, uint32_t acc_base, const uint32_t* __restrict__ tile_frozen) {
	constexpr uint32_t kQuads = kTileSize / 4u;                                 // 4-pixel groups per tile
	const size_t n_items = static_cast<size_t>(n_tiles) * kQuads;
	const uint32_t first = min(buckets, batch_n);
	for (size_t item = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; item < n_items; item += static_cast<size_t>(gridDim.x) * kBlock) {
		const size_t tile = item / kQuads; const uint32_t q = static_cast<uint32_t>(item % kQuads);
		if (SPARSE && tile_frozen[tile] != 0u) continue;
		for (uint32_t k0 = 0; k0 < first; k0++) {
			const uint32_t bucket = (acc_base + k0 + 1u) % buckets;
			float4* dst = accum + (tile * buckets + bucket) * 3u * kQuads + q;  // channel c of the 4 pixels: dst[c * kQuads]
			float4 r = dst[0], g = dst[kQuads], b = dst[2u * kQuads];
			for (uint32_t k = k0; k < batch_n; k += buckets) {
				const float4* src = contrib + ((tile * batch_n + k) * kQuads + q) * 3u;
				const float4 c0 = src[0], c1 = src[1], c2 = src[2];                // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
				r.x += c0.x; g.x += c0.y; b.x += c0.z;
				r.y += c0.w; g.y += c1.x; b.y += c1.y;
				r.z += c1.z; g.z += c1.w; b.z += c2.x;
				r.w += c2.y; g.w += c2.z; b.w += c2.w;
			}
			dst[0] = r; dst[kQuads] = g; dst[2u * kQuads] = b;
		}
	}
}

// ------------------------------------------------------------------------------------------------
// Stage-level debug kernels (mirt_debug_*)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_debug_math(int fn, uint32_t n, const float* in, float* out) {
	for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
		switch (fn) {
		case 0: { float s, c; fast_sincos(in[i], s, c); out[i] = s; out[n + i] = c; } break;
		case 1: out[i] = fast_atan2(in[i], in[n + i]); break;
		case 2: out[i] = fast_asin(in[i]); break;
		case 3: out[i] = 1.0f / in[i]; out[n + i] = __builtin_sqrtf(fabs_bits(in[i])); out[2 * n + i] = in[i] / in[n + i]; break;
		case 4: { f3 h = hemisphere(in[i], in[n + i]); out[i] = h.x; out[n + i] = h.y; out[2 * n + i] = h.z; } break;
		case 5: {
			f3 N{ in[i], in[n + i], in[2 * n + i] }, v{ in[3 * n + i], in[4 * n + i], in[5 * n + i] };
			quat T = tangent_space(N); f3 l = to_local(T, v); f3 w = to_world(T, v);
			out[i] = T.x; out[n + i] = T.y; out[2 * n + i] = T.z; out[3 * n + i] = T.w;
			out[4 * n + i] = l.x; out[5 * n + i] = l.y; out[6 * n + i] = l.z;
			out[7 * n + i] = w.x; out[8 * n + i] = w.y; out[9 * n + i] = w.z;
		} break;
		case 6: {
			f3 Wc{ in[i], in[n + i], in[2 * n + i] };
			float dist, pdf;
			f3 Ld = sample_direction_to_sphere(Wc, in[3 * n + i], in[4 * n + i], in[5 * n + i], in[6 * n + i], in[7 * n + i], dist, pdf);
			out[i] = Ld.x; out[n + i] = Ld.y; out[2 * n + i] = Ld.z; out[3 * n + i] = dist; out[4 * n + i] = pdf;
		} break;
		case 7: {
			uint32_t s = hash_2d(__float_as_uint(in[i]), __float_as_uint(in[n + i]));
			out[i] = __uint_as_float(s);
			out[n + i] = rand_unit_float(s); out[2 * n + i] = rand_unit_float(s);
			uint32_t s2 = s;
			out[3 * n + i] = rand_unit_float(s);
			out[4 * n + i] = __uint_as_float(rand_bounded_int(s2, __float_as_uint(in[2 * n + i])));
		} break;
		case 10: out[i] = sqrt_trav(in[i]); break;
		case 11: {  // dielectric_interface: in Vl(3), n, entering (!= 0), s1 -> out dir(3), F, reflected, tir
			f3 d; float F; bool reflected, tir;
			dielectric_interface(f3{ -in[i], -in[n + i], -in[2 * n + i] }, f3{ 0.0f, 0.0f, 1.0f }, in[3 * n + i], in[4 * n + i] != 0.0f, in[5 * n + i], d, F, reflected, tir);
			out[i] = d.x; out[n + i] = d.y; out[2 * n + i] = d.z; out[3 * n + i] = F; out[4 * n + i] = reflected ? 1.0f : 0.0f; out[5 * n + i] = tir ? 1.0f : 0.0f;
		} break;
		case 8: {   // Closure<GGX>::eval: in F0(3), alpha, L(3), V(3) -> out 3
			const f3 r = ggx_eval(f3{ in[i], in[n + i], in[2 * n + i] }, in[3 * n + i], f3{ in[4 * n + i], in[5 * n + i], in[6 * n + i] }, f3{ in[7 * n + i], in[8 * n + i], in[9 * n + i] });
			out[i] = r.x; out[n + i] = r.y; out[2 * n + i] = r.z;
		} break;
		case 9: {   // Closure<GGX>::sample: in F0(3), alpha, V(3), u0, u1 -> out dir(3), estimator(3)
			f3 d, e;
			ggx_sample(f3{ in[i], in[n + i], in[2 * n + i] }, in[3 * n + i], f3{ in[4 * n + i], in[5 * n + i], in[6 * n + i] }, in[7 * n + i], in[8 * n + i], d, e);
			out[i] = d.x; out[n + i] = d.y; out[2 * n + i] = d.z; out[3 * n + i] = e.x; out[4 * n + i] = e.y; out[5 * n + i] = e.z;
		} break;
		default: break;
		}
	}
}
// mirt_debug_math fn 12 and 13: the two functions of the context's sky table (mirt_set_sky_sampling), which k_debug_math has no argument for.
//   12  sky_sample: in u0, u1 -> out dir(3), q, row, column (the last two as floats: exact below 2^24)
//   13  sky_pdf:    in dir(3) -> out p~, row, column
__global__ __launch_bounds__(kBlock) void k_debug_sky(int fn, uint32_t n, const float* in, float* out, SceneDev sc, SkyTable sky) {
	for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
		uint32_t row, col;
		if (fn == 12) {
			float q;
			const f3 d = sky_sample(sky, in[i], in[n + i], q, row, col);
			out[i] = d.x; out[n + i] = d.y; out[2 * n + i] = d.z; out[3 * n + i] = q; out[4 * n + i] = static_cast<float>(row); out[5 * n + i] = static_cast<float>(col);
		} else {
			out[i] = sky_pdf(sc, sky, in[i], in[n + i], in[2 * n + i], row, col);
			out[n + i] = static_cast<float>(row); out[2 * n + i] = static_cast<float>(col);
		}
	}
}
// mirt_debug_math fn 14: ggx_pdf (mirt_set_ggx_pdf).  in: alpha, L(3), V(3) -> out p~.  A kernel of its own, so that k_debug_math stays the code it was.
__global__ __launch_bounds__(kBlock) void k_debug_ggx_pdf(uint32_t n, const float* in, float* out) {
	for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock)
		out[i] = ggx_pdf(in[i], f3{ in[n + i], in[2 * n + i], in[3 * n + i] }, f3{ in[4 * n + i], in[5 * n + i], in[6 * n + i] });
}

} // namespace mirt
