"""k_shade's composed forms against ONE float64 path sampler (composed_definitions.composed_sampler): closures {lambert, ggx, mixed} x light RIS x
transmission x sky sampling x GGX pdf x lens, 80 cases of 32 x 32 x N_ACC, each held to the twin's expectation per first-hit region and channel
within SIGMA standard errors - not bit for bit - and its counters to the twin's.  The twin's side is the fixture tests/golden/composed_forms.npz,
recorded from the oracle's camera rays (the 80 twin runs take minutes: test_composed_cpu.py says how it is written and recomputes four forms);
test_rays_are_the_fixtures holds this device's own camera rays to it.  What makes the comparison a test - the reductions, the oracle, the twelve
mutations - is test_composed_cpu.py's.  Three exact checks follow: SPARSE under the all-on form, the exact no-ops across forms, every form reached."""
import numpy as np
import pytest

import composed_definitions as cd
from oracle_binding import bits
from test_composed_cpu import N_ACC, BUCKETS, check_form, load_fixture

pytestmark = pytest.mark.gpu
f32 = np.float32
ALL_ON = dict(closures="mixed", ris=4, glass=True, sky=True, pdf=True, lens=True)


def same_words(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, what
    bad = int((got != want).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} words differ"


def renderer(mirt, form, sc=None):
    """A context for one form (a status other than MIRT_OK raises: MIRT_ERR_ARG would mean a missing form)."""
    sc = sc if sc is not None else cd.composed_scene(mirt)
    r = mirt.Renderer(sc, max_bounces=cd.MAX_BOUNCES, buckets=BUCKETS, use_bvh=True, gloss_decay=list(cd.DECAY), light_ris=form["ris"], transmission=form["glass"],
                      sky_sampling=form["sky"], material_closures=cd.CLOSURES[form["closures"]], ggx_pdf=form["pdf"])
    r.Resize(cd.W, cd.H)
    if form["lens"]:
        r.set_lens(cd.LENS_APERTURE, cd.focus_depth(sc))
    return r


def render(mirt, form, n_acc, sc=None):
    r = renderer(mirt, form, sc)
    r.Accumulate(n_acc)
    out = dict(acc=r.accumulator(), counters=r.counters())
    r.close()
    assert out["counters"]["terminated"] + out["counters"]["dropped"] == cd.W * cd.H * n_acc, cd.form_name(form)   # every batch launched, every path ended
    return out


@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "lens"])
def test_rays_are_the_fixtures(mirt, lens):
    """The regions of the fixture are those of this device's camera rays: float64 first hits of every accumulation's rays from debug_raygen."""
    r = renderer(mirt, dict(ALL_ON, lens=lens))
    rays = [tuple(a.T.copy() for a in r.debug_raygen(acc)) for acc in range(1, N_ACC + 1)]
    sc = r.scene
    assert np.array_equal(r.prims["position"], r.geometry["position"])              # tree order = authoring order: Q11 cannot bite
    r.close()
    assert np.array_equal(cd.regions_of(sc, rays), load_fixture()["labels"][int(lens)])


@pytest.mark.parametrize("form", cd.composed_forms(), ids=cd.form_name)
def test_composed_form(mirt, form):
    """Per region and channel the accumulator's mean within SIGMA of the twin's expectation (standard error: the twin's per-path variance at N_ACC and
    the twin's own error); rays, terminated and dropped within SIGMA of the twin's per-path means, shadow_rays too (exactly where the twin holds it
    deterministic)."""
    check_form(render(mirt, form, N_ACC), form, load_fixture(), "composed/gpu")


def test_sparse_under_the_all_on_form(mirt):
    """Freeze one tile after a batch and accumulate again: the three other tiles are word-identical to the run with nothing frozen, the frozen tile
    keeps its words (test_adaptive_gpu holds this for the default form only)."""
    accs = {}
    for freeze in (False, True):
        r = renderer(mirt, ALL_ON)
        r.Accumulate(BUCKETS)
        first = r.accumulator()
        if freeze:
            r.freeze_tiles([0, 1, 0, 0])
        r.Accumulate(BUCKETS)
        accs[freeze] = (first, r.accumulator(), r.counters())
        r.close()
    same_words(accs[True][0], accs[False][0], "the first batch")
    same_words(accs[True][1][[0, 2, 3]], accs[False][1][[0, 2, 3]], "the tiles that were not frozen")
    same_words(accs[True][1][1], accs[True][0][1], "the frozen tile")
    assert (bits(accs[False][1][1]) != bits(accs[False][0][1])).any()
    n = cd.W * cd.H * BUCKETS
    assert accs[True][2]["terminated"] + accs[True][2]["dropped"] == 2 * n - 256 * BUCKETS


def test_exact_no_ops_across_forms(mirt):
    """Three switches that must leave the accumulator and the counters word-identical, each with the other switches on: ggx_pdf on an all-Lambertian
    table, transmission on a scene without a transmissive material, sky_sampling with ambient = 0."""
    opaque = cd.composed_scene(mirt)
    opaque.material["transmission"] = 0.0
    dark = cd.composed_scene(mirt)
    dark.ambient = np.zeros(3, dtype=f32)
    cases = {"ggx_pdf, all Lambertian": ("pdf", dict(ALL_ON, closures="lambert"), None),
             "transmission, no transmissive material": ("glass", dict(ALL_ON), opaque),
             "sky_sampling, ambient 0": ("sky", dict(ALL_ON), dark)}
    for label, (switch, form, sc) in cases.items():
        on, off = render(mirt, dict(form, **{switch: True}), 2 * BUCKETS, sc), render(mirt, dict(form, **{switch: False}), 2 * BUCKETS, sc)
        same_words(on["acc"], off["acc"], label)
        assert on["counters"] == off["counters"] and on["acc"].any(), label


def test_all_forms_reached(mirt):
    """One batch of every form (the frozen-tile form is test_sparse_under_the_all_on_form's): no status but MIRT_OK (a missing form would be
    MIRT_ERR_ARG) and every path of every batch accounted for by the counters."""
    for form in cd.composed_forms():
        assert np.isfinite(render(mirt, form, BUCKETS)["acc"]).all(), cd.form_name(form)
    assert len(cd.composed_forms()) == 80
