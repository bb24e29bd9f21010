"""The HIP kernels against the float64 definitions of tests/definitions.py: the checks, inputs and bounds of test_definitions_cpu.py, run on
the device through debug_math, debug_raygen, debug_trace_closest, debug_trace_shadow, Accumulate, Render and render_aov.  The bounds are the
CPU file's constants: the two sides are bit-identical, so what the oracle meets the kernels must meet.  A failure here that the CPU file does
not show cannot come from the definitions - it is a kernel bug."""
import numpy as np
import pytest

import definitions as df
import test_definitions_cpu as cpu
from test_definitions_cpu import f32, f64, TRACE_SCENES

pytestmark = pytest.mark.gpu


class GpuBackend:
    name = "gpu"
    variants = (("brute", dict(use_bvh=False)), ("bvh", dict(use_bvh=True)), ("gpu_built_bvh", dict(use_bvh=True, gpu_build=True)))

    def __init__(self, mirt):
        self.mirt = mirt
        self.r = mirt.Renderer(mirt.scene.default9(), device=0)

    def close(self):
        self.r.close()

    @staticmethod
    def _rows(*parts):
        return np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=f32).reshape(len(p), -1).T for p in parts]), dtype=f32)

    def hemisphere(self, t, s):
        return self.r.debug_math(4, np.stack([t, s]), 3).T.copy()

    def frame(self, N, v):
        out = self.r.debug_math(5, self._rows(N, v), 10)
        return out[0:4].T.copy(), out[4:7].T.copy(), out[7:10].T.copy()

    def sample_sphere(self, Wc, sin2, dist, r2, t, s):
        return self.r.debug_math(6, self._rows(Wc, sin2, dist, r2, t, s), 5).T.copy()

    def ggx_eval(self, F0, alpha, L, V):
        return self.r.debug_math(8, self._rows(F0, alpha, L, V), 3).T.copy()

    def ggx_sample(self, F0, alpha, V, u0, u1):
        out = self.r.debug_math(9, self._rows(F0, alpha, V, u0, u1), 6)
        return out[:3].T.copy(), out[3:].T.copy()

    def raygen(self, sc, w, h, acc, max_bounces=16):
        r = self.mirt.Renderer(sc, max_bounces=max_bounces); r.Resize(w, h)
        p, d = r.debug_raygen(acc); r.close()
        return p, d

    def tracers(self, sc, with_gpu_build=False):
        for label, kw in self.variants[: 3 if with_gpu_build else 2]:
            r = self.mirt.Renderer(sc, **kw)
            yield label, r.debug_trace_closest, r.debug_trace_shadow
            r.close()

    def render(self, sc, w, h, n_acc, max_bounces, buckets=5, mis=True, variant=0, brdf=0, gloss_decay=None, exact_stream_order=False, trace_primary_rays=False):
        r = self.mirt.Renderer(sc, max_bounces=max_bounces, buckets=buckets, mis=mis, brdf=brdf, gloss_decay=gloss_decay, exact_stream_order=exact_stream_order,
                               trace_primary_rays=trace_primary_rays, **self.variants[variant][1])
        r.Resize(w, h); r.Accumulate(n_acc)
        frame = r.GetFrame().copy() if (n_acc % buckets == 0 and r.Render()) else None
        out = dict(acc=r.accumulator(), frame=frame, counters=r.counters())
        r.close()
        return out


@pytest.fixture(scope="module")
def be(mirt):
    b = GpuBackend(mirt)
    yield b
    b.close()


# ---- A ----
@pytest.mark.parametrize("scene_name", list(TRACE_SCENES))
def test_intersection(be, mirt, scene_name):
    """k_trace / k_trace_fat, brute force and BVH, and on S1000a the tree built on the device as well."""
    if scene_name == "S1000a":
        plain = be.tracers
        be.tracers = lambda sc: plain(sc, with_gpu_build=True)
        try:
            cpu.check_intersection(be, mirt, scene_name)
        finally:
            del be.tracers
    else:
        cpu.check_intersection(be, mirt, scene_name)


# ---- B ----
def test_hemisphere(be, mirt):
    cpu.check_hemisphere(be, mirt)


def test_sample_direction_to_sphere(be, mirt):
    cpu.check_sample_sphere(be, mirt)


def test_tangent_frame(be, mirt):
    cpu.check_frame(be, mirt)


# ---- C ----
def test_ggx_eval(be, mirt):
    cpu.check_ggx_eval(be, mirt)


def test_ggx_sample(be, mirt):
    cpu.check_ggx_sample(be, mirt)


def test_ggx_energy(be, mirt):
    cpu.check_ggx_energy(be, mirt)


def test_ggx_sample_distribution(be, mirt):
    """D7 on the device: debug_math fn 9, nine (alpha, V) pairs of 20 000 samples each against the definition's cell probabilities."""
    cpu.check_ggx_sample_distribution(be, mirt)


# ---- D ----
def test_raygen(be, mirt):
    cpu.check_raygen(be, mirt)


def test_sky_lookup(be, mirt):
    cpu.check_sky(be, mirt, variants=(0, 1))


def test_resolve(be, mirt):
    cpu.check_resolve(be, mirt, variants=(0, 1))


def test_first_hit_depth(be, mirt):
    cpu.check_first_hit_depth(be, mirt)


def test_aov_depth_and_normal(be, mirt):
    """render_aov on the one-sphere scene (eye (0, 0, 6), 32 x 32, 12 accumulations), per pixel.  Depth: the mean over the jitter lies between
    the float64 ray-sphere distances at the footprint's nearest and farthest points, +- the largest part-A bound of the pixel's own rays and
    4e-6 for the binary32 sum (12 additions of at most half an ulp of 64 each, over 12) and its division; a
    footprint wholly off the sphere gives the miss depth 1e4 exactly; one that straddles the silhouette lies between its nearest hit and 1e4.
    Normal: the normalised sum of unit normals from a patch of the sphere lies in the patch's spherical hull, so its angle to the normal at the
    footprint's centre is at most the largest such angle over the footprint's border (float64, 8 points a side, x 1.05 for the border sampling)
    + 1e-6; it faces the eye."""
    sc = cpu.one_sphere(mirt, eye_z=6.0, focal=50.0)
    w = h = 32; n_acc = 12
    for kw in (dict(use_bvh=False), dict(use_bvh=True)):
        r = mirt.Renderer(sc, max_bounces=4, aov=True, **kw); r.Resize(w, h); r.Accumulate(n_acc)
        depth = r.render_aov(mirt.AOV_DEPTH).astype(f64); normal = r.render_aov(mirt.AOV_NORMAL).astype(f64)
        r.close()
        lo, hi = cpu.footprint_depth_bounds(w, h, 50.0, 6.0)
        tol = cpu.footprint_root_error(be, sc, w, h, range(1, n_acc + 1), max_bounces=4)[0] + 4e-6
        inside, outside = np.isfinite(hi), np.isinf(lo)
        assert inside.sum() > 20 and outside.sum() > 100 and (~inside & ~outside).sum() > 10
        assert (depth[inside] >= (lo - tol)[inside]).all() and (depth[inside] <= (hi + tol)[inside]).all()
        assert (depth[outside] == 1e4).all() and not normal[outside].any()
        edge = ~inside & ~outside
        assert (depth[edge] >= (lo - tol)[edge]).all() and (depth[edge] <= 1e4).all()
        z = df.lens_z(h, 50.0)
        ys, xs = np.nonzero(inside)
        centre = df.sphere_depth_normal(xs + 0.5, ys + 0.5, w / 2.0, h / 2.0, z, 6.0)[1]
        s = np.linspace(0.0, 1.0, 9)
        bx = np.concatenate([s, s, np.zeros(9), np.ones(9)]); by = np.concatenate([np.zeros(9), np.ones(9), s, s])
        border = df.sphere_depth_normal(xs[:, None] + bx[None, :], ys[:, None] + by[None, :], w / 2.0, h / 2.0, z, 6.0)[1]
        spread = np.arccos(np.clip((border * centre[:, None, :]).sum(axis=-1), -1, 1)).max(axis=1)
        got = normal[ys, xs]
        assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() <= 8 * df.u
        angle = np.arccos(np.clip((got * centre).sum(axis=1), -1, 1))
        assert (angle <= 1.05 * spread + 1e-6).all(), float((angle / spread).max())
        assert (got[:, 2] > 0).all()
        cpu.report(f"gpu/aov/{kw}", worst_angle_over_spread=float((angle / spread).max()), pixels=int(inside.sum()))


# ---- E ----
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("w,h,n_acc", [(64, 64, 50), (256, 256, 20)])
def test_filling_sphere(be, mirt, w, h, n_acc, variant):
    cpu.check_filling_sphere(be, mirt, w, h, n_acc, variant=variant)


@pytest.mark.parametrize("variant", [0, 1])
def test_two_tone_sky(be, mirt, variant):
    cpu.check_two_tone_sky(be, mirt, variant=variant)


@pytest.mark.parametrize("variant", [0, 1])
def test_emissive_sphere(be, mirt, variant):
    cpu.check_emissive_sphere(be, mirt, variant=variant)


# ---- F ----
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", cpu.F_LAMBERT)
def test_direct_lighting(be, mirt, name, variant):
    cpu.check_direct(be, mirt, name, variant=variant)


@pytest.mark.parametrize("name", ["F1_high", "F1_low", "F1_sunk"])
def test_direct_lighting_exact_stream_order(be, mirt, name):
    """The second user of the per-hit shading text: k_tile_stream."""
    cpu.check_direct(be, mirt, name, variant=0, exact_stream_order=True)


@pytest.mark.parametrize("name", ["F1_high", "F1_low", "F1_below"])
def test_direct_lighting_traced_primary_rays(be, mirt, name):
    cpu.check_direct(be, mirt, name, variant=1, trace_primary_rays=True)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("max_bounces", [4, 16])
def test_several_bounces(be, mirt, max_bounces, variant):
    cpu.check_several_bounces(be, mirt, max_bounces, variant=variant)


# ---- G ----
@pytest.mark.parametrize("variant", [0, 1])
def test_ggx_direct(be, mirt, variant):
    cpu.check_ggx_direct(be, mirt, variant=variant)


def test_ggx_direct_exact_stream_order(be, mirt):
    """The second user of the per-hit shading text under GGX: k_tile_stream."""
    cpu.check_ggx_direct(be, mirt, variant=0, exact_stream_order=True)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("max_bounces", [4, 16])
def test_ggx_bounces(be, mirt, max_bounces, variant):
    cpu.check_ggx_bounces(be, mirt, max_bounces, variant=variant)


@pytest.mark.parametrize("variant", [0, 1])
def test_ggx_grazing(be, mirt, variant):
    cpu.check_ggx_grazing(be, mirt, variant=variant)
