"""The float64 side of the dielectric interface (mirt_set_transmission): tests/glass_definitions.py against itself and against the textbook limits,
the grid that tests/test_glass_gpu.py sends through mirt_debug_math fn 11, and the C interface as far as it goes without a device."""
import ctypes as C

import numpy as np

import glass_definitions as gd

INDICES = (1.0001, 1.44, 1.5, 1.762, 11.0)


def test_fresnel_is_symmetric_between_the_two_sides():
    """Reversibility (Stokes): a ray arriving under theta_i from the r side and one arriving under theta_t from the other side see the same
    reflectance: F(r, c) = F(1 / r, c_t)."""
    c = np.linspace(1e-3, 1.0, 2001)          # (at c = 0 the other side stands at its critical angle, where float64's own c_t carries sqrt(2^-53))
    for n in INDICES:
        r = 1.0 / n                                                                 # entering: never total internal reflection
        _, c_t = gd.snell(r, c)
        # from the dense side F has slope ~ 4 n / c_t' against the cosine, c_t' >= 1e-3 / n here: float64's 1e-16 on c_t grows to < 1e-9
        assert np.allclose(gd.fresnel(r, c), gd.fresnel(1.0 / r, c_t), rtol=0, atol=1e-9), n


def test_normal_incidence():
    for n in INDICES:
        want = ((n - 1.0) / (n + 1.0)) ** 2
        for r in (n, 1.0 / n):
            assert abs(gd.fresnel(np.array([r]), np.array([1.0]))[0] - want) < 1e-15, (n, r)
    assert gd.fresnel(np.array([1.0 / 1.5]), np.array([0.0]))[0] == 1.0             # grazing incidence reflects everything


def test_total_internal_reflection_exactly_where_sin2_t_reaches_one():
    c = np.linspace(0.0, 1.0, 4001)
    for n in INDICES:
        sin2_t, c_t = gd.snell(n, c)
        Vl = np.stack([np.sqrt(1 - c * c), np.zeros_like(c), c], axis=1)
        _, F, reflected, tir = gd.interface(Vl, np.full_like(c, n), np.zeros(len(c), dtype=bool), np.full_like(c, 0.999999))
        assert np.array_equal(tir, sin2_t >= 1.0) and np.array_equal(np.isnan(c_t), sin2_t > 1.0)
        assert (F[tir] == 1.0).all() and reflected[tir].all() and (F[~tir] < 1.0).all()
        # the critical angle: sin(theta_c) = 1 / n
        c_crit = np.sqrt(1.0 - 1.0 / (n * n))
        assert tir[c < c_crit - 1e-9].all() and not tir[c > c_crit + 1e-9].any()
        # entering never reflects totally
        assert (gd.snell(1.0 / n, c)[0] < 1.0).all()


def test_a_ray_that_entered_a_sphere_never_meets_total_internal_reflection():
    """The chord of a sphere meets the surface under the angle it was refracted to: cos = c_t, and sin2 of the way out is n^2 (1 - c_t^2) =
    1 - c^2 < 1 for every c > 0.  Checked through the tree: nothing is dropped by an endless chain when the depth allows the way out, and
    the in-sphere angle of incidence is the refraction angle."""
    for n in INDICES:
        c = np.linspace(1e-6, 1.0, 1001)
        _, c_t = gd.snell(1.0 / n, c)
        assert (gd.snell(n, c_t)[0] < 1.0).all(), n
    O, D, _ = gd.camera_rays(48, 32, 35.0, 4.0, sub=2)
    rad, dropped, _ = gd.glass_ball_radiance(O, D, 1.5, (1, 1, 1), 64, ((np.ones(3),) * 2,) * 2)
    assert np.allclose(rad + dropped[:, None], 1.0, atol=1e-12) and dropped.max() < 1e-9   # a furnace: every branch reaches the sky


def test_interface_directions():
    rng = np.random.default_rng(5)
    c = rng.uniform(0.05, 1.0, 500)
    phi = rng.uniform(0, 2 * np.pi, 500)
    Vl = np.stack([np.sqrt(1 - c * c) * np.cos(phi), np.sqrt(1 - c * c) * np.sin(phi), c], axis=1)
    for n in INDICES:
        for entering in (True, False):
            t, F, reflected, tir = gd.interface(Vl, np.full(500, n), np.full(500, entering), np.ones(500))      # s1 = 1: refract wherever that is possible
            assert np.array_equal(reflected, tir)
            ok = ~tir
            r = 1.0 / n if entering else n
            assert np.allclose(np.linalg.norm(t[ok], axis=1), 1.0, atol=1e-12)
            # Snell: the tangential part scales by r and keeps its direction; the ray goes on to the other side
            assert np.allclose(t[ok, :2], -r * Vl[ok, :2], atol=1e-12) and (t[ok, 2] < 0).all()
    m, F, reflected, _ = gd.interface(Vl, np.full(500, 1.5), np.ones(500, dtype=bool), np.zeros(500))
    assert reflected.all() and np.allclose(m, Vl * [-1, -1, 1])                     # s1 = 0 < F: the mirror direction
    m, F, reflected, tir = gd.interface(Vl, np.ones(500), np.ones(500, dtype=bool), np.zeros(500))
    assert not reflected.any() and not tir.any() and (F == 0).all() and np.array_equal(m, -Vl)     # index-matched: straight on


def test_the_fn11_grid_excludes_at_most_one_percent():
    """The condition tests/test_glass_gpu.py::test_fn11 puts on its inputs, checked here where no device is needed; and the error model holds a
    binary32 restatement of device_math.hpp's operation order."""
    Vl, n, entering, s1 = gd.fn11_grid()
    assert 3500 <= len(Vl) <= 4500 and Vl.dtype == np.float32
    _, F, reflected, tir = gd.interface(Vl, n, entering, s1)
    model = gd.interface_error_model(Vl, n, entering)
    ties = gd.interface_ties(model, F, s1)
    assert ties.mean() <= 0.01, ties.mean()
    assert tir.any() and (~tir & ~entering).any() and model["tie_tir"].any()        # the critical angle is straddled, ties included
    f = np.float32
    r = np.where(entering, f(1) / n, n).astype(f)
    c = Vl[:, 2]
    sin2_t = ((r * r) * (f(1) - c * c)).astype(f)
    c_t = np.sqrt(np.maximum(f(1) - sin2_t, f(0))).astype(f)
    with np.errstate(all="ignore"):
        rs, rp = (r * c - c_t) / (r * c + c_t), (c - r * c_t) / (c + r * c_t)
        F32 = np.where(n == 1, f(0), np.where(sin2_t >= 1, f(1), f(0.5) * (rs * rs + rp * rp)))
    tir32 = (sin2_t >= 1) & (n != 1)
    assert np.array_equal(tir32[~model["tie_tir"]], tir[~model["tie_tir"]])
    same = tir32 == tir
    assert (np.abs(F32.astype(np.float64) - F)[same] <= model["E_F"][same]).all()


def test_symbols(mirt):
    lib = mirt.load_library()
    for name in ("mirt_set_transmission", "mirt_get_transmission", "mirt_group_set_transmission"):
        assert name in lib._declared and getattr(lib, name)
    for method in ("set_transmission", "transmission"):
        assert callable(getattr(mirt.Renderer, method)) and callable(getattr(mirt.GroupRenderer, method))


def test_null_arguments(mirt):
    """The checks that come before any context is touched: MIRT_ERR_ARG = -1.  (The other refusals need a context: test_glass_gpu.py.)"""
    lib = mirt.load_library()
    v = C.c_uint32(7)
    assert lib.mirt_set_transmission(None, 1) == -1
    assert lib.mirt_get_transmission(None, C.byref(v)) == -1 and v.value == 7
    assert lib.mirt_group_set_transmission(None, 1) == -1
