"""The float64 side of sky sampling (mirt_set_sky_sampling): tests/sky_definitions.py held to itself, and the C interface as far as it goes
without a device.  The kernels are held to the twin by tests/test_sky_sampling_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import definitions as df
import sky_definitions as sd

MAPS = ((1, 1), (2, 2), (2, 1), (1, 2), (9, 5), (65, 33), (4096, 2048))


def random_map(w, h, seed=3):
    rng = np.random.default_rng(seed)
    m = rng.uniform(0.0, 2.0, (h, w, 4)).astype(np.float32)
    m[rng.uniform(size=(h, w)) < 0.2] = 0.0                                       # black texels: cells that must never be drawn
    m[0, 0, :3] = 1.0                                                             # (a 1 x 1 map keeps a total)
    return m


def test_solid_angles_cover_the_sphere():
    for w, h in MAPS:
        rows, cols = sd.cells(w, h)
        om = sd.solid_angle(rows, cols)
        assert (om > 0).all() and abs(om.sum() * cols - 4 * np.pi) < 1e-12 * 4 * np.pi, (w, h)
        el = sd.elevation(np.arange(rows + 1), rows)
        assert np.allclose(om, (2 * np.pi / cols) * (np.sin(el[:-1]) - np.sin(el[1:])), rtol=1e-9, atol=0)     # the issue's form
    assert sd.solid_angle(1, 7)[0] == 2 * 2 * np.pi / 7                            # one row: 2 x 2 pi / cols


def test_densities_integrate_to_one():
    for w, h in MAPS[:-1]:
        tab = sd.table(random_map(w, h), (1.0, 0.5, 0.25))
        om = sd.solid_angle(tab["rows"], tab["cols"])
        assert abs((tab["dens"] * om[:, None]).sum() - 1.0) < 1e-12, (w, h)
        assert np.allclose(tab["dens"] * om[:, None], tab["prob"], rtol=1e-12, atol=0)
        assert abs(tab["marg"][-1] - tab["total"]) <= 1e-12 * tab["total"] and np.allclose(tab["cond"][:, -1], tab["rowsum"], rtol=1e-12)


def test_sampler_chi_square_and_placement():
    """2^18 stratified-free uniform draws through the twin's sampler: cell counts against the cell probabilities, black cells never drawn, and
    every direction lies in the cell it was drawn for by the textbook map."""
    rng = np.random.default_rng(11)
    n = 1 << 18
    for w, h in ((9, 5), (65, 33)):
        m = random_map(w, h) if (w, h) == (9, 5) else sd.sun_map()
        tab = sd.table(m, (1.0, 1.0, 1.0))
        u0, u1 = rng.uniform(size=n), rng.uniform(size=n)
        d, row, col, dv, du = sd.sample(tab, u0, u1)
        assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-12)
        r2, c2 = sd.cell_of(d, w, h)
        inside = (dv > 1e-9) & (dv < 1 - 1e-9) & (du > 1e-9) & (du < 1 - 1e-9)
        assert np.array_equal(r2[inside], row[inside]) and np.array_equal(c2[inside], col[inside])
        p = tab["prob"].reshape(-1)
        counts = np.bincount(row * tab["cols"] + col, minlength=p.size).astype(np.float64)
        assert (counts[p == 0] == 0).all()
        live = p > 0
        chi2 = ((counts[live] - n * p[live]) ** 2 / (n * p[live])).sum()
        assert chi2 < df.chi2_upper(int(live.sum()) - 1, 1e-6), (w, h, chi2)
        # uniform in sin(elevation) and in azimuth: the fractions are uniform, so the density over the cell is constant
        for frac in (dv, du):
            hist = np.bincount(np.minimum((frac * 16).astype(int), 15), minlength=16)
            assert ((hist - n / 16) ** 2 / (n / 16)).sum() < df.chi2_upper(15, 1e-6)


def test_mis_weights_partition_unity():
    rng = np.random.default_rng(2)
    tab = sd.table(sd.sun_map(), (1.0, 1.0, 1.0))
    d = rng.normal(size=(20000, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = sd.pdf(tab, d, 65, 33)
    for n_lights in (0, 1, 7):
        sel = 1.0 / (n_lights + 1)
        f = sd.lambert_pdf(d[:, 2])                                               # any local frame: here z is the normal
        g = sel * p
        w = sd.nee_weight(sel, p, f) + sd.miss_weight(sel, p, f)
        above = f * f + g * g >= 1e-6
        assert above.any() and np.allclose(w[above], 1.0, rtol=0, atol=1e-12)
        assert (w[~above] <= 1.0 + 1e-12).all()                                   # under the reference's floor energy is lost, never made
    # GGX (pdf 0): everything to next event estimation; after an interface the miss shader keeps everything
    assert (sd.nee_weight(0.5, p[p > 0], 0.0) == 1.0).all() and (sd.miss_weight(0.5, p, 0.0) == 0.0).all()


def test_floor_loss_is_what_the_documents_state():
    """Where both pdfs are below the heuristic's 1e-6 floor (f^2 + g^2 < 1e-6) the two weights add to less than one.  With g = 0 that is the
    cosine lobe below f = (1/pi) cos < 1e-3: a share (pi 1e-3)^2 of the cosine-weighted energy, the figure mirt.h and DESIGN.md quote."""
    c = (np.arange(200000) + 0.5) / 200000                                        # cos(theta), midpoints: the cosine-weighted measure is 2 c dc
    f = c / np.pi
    lost = (2 * c * (1.0 - sd.miss_weight(1.0, 0.0, f) - sd.nee_weight(1.0, 0.0, f))).sum() / 200000
    assert 0 < lost <= (np.pi * 1e-3) ** 2, lost                                 # (exactly half of it: the weight rises as (c / c0)^2 below c0 = pi 1e-3)


def test_band_share_of_the_sun_map():
    """What test_sky_sampling_gpu.py caps the set-aside share of fn 13 with, for the 65 x 33 sun map: the bands' probability under the table's
    own sampling, with the edge-band widths of definitions' row D."""
    tab = sd.table(sd.sun_map(), (1.0, 1.0, 1.0))
    share = sd.band_share(tab, 2e-3 + 1e-4 * 2 * np.pi / 64, 1e-3 + 1e-4 * np.pi / 32)
    assert 0.03 < share < 0.12, share
    assert tab["prob"][10, 20] > 0.5                                              # one texel of sun carries most of the power


def test_symbols(mirt):
    lib = mirt.load_library()
    for name in ("mirt_set_sky_sampling", "mirt_get_sky_sampling", "mirt_group_set_sky_sampling", "mirt_debug_sky_table"):
        assert name in lib._declared and getattr(lib, name)
    for method in ("set_sky_sampling", "sky_sampling"):
        assert callable(getattr(mirt.Renderer, method)) and callable(getattr(mirt.GroupRenderer, method))
    assert callable(mirt.Renderer.debug_sky_table)


def test_null_arguments(mirt):
    """The checks that come before any context is touched: MIRT_ERR_ARG = -1.  (The other refusals need a context: test_sky_sampling_gpu.py.)"""
    lib = mirt.load_library()
    v = C.c_uint32(7)
    info = (C.c_uint32 * 4)()
    assert lib.mirt_set_sky_sampling(None, 1) == -1
    assert lib.mirt_get_sky_sampling(None, C.byref(v)) == -1 and v.value == 7
    assert lib.mirt_group_set_sky_sampling(None, 1) == -1
    assert lib.mirt_debug_sky_table(None, None, 0, info) == -1


def test_headless_help_names_the_flag(mirt):
    exe = os.path.join(mirt.CSRC, "mirt_headless")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", mirt.CSRC, "mirt_headless"], check=True)
    out = subprocess.run([exe, "--help"], check=True, capture_output=True, text=True).stdout
    assert "--sky-sampling" in out and "mirt_set_sky_sampling" in out
