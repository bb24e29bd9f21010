"""The lifetime of what a context owns (csrc/ctx.hpp): every device buffer, stream and event is a member with a destructor, grouped by lifetime, and
mirt_destroy deletes the context.  Ordinary use that reaches every owner — the switches' planes and tables on and off, the temporal history and
its id planes, the noise scratch, the freeze lists, slots created and dropped (streams 3 -> 1 -> 3), two resizes, a scene handed over again —
must leave a renderer that computes what a fresh one computes, word for word, and closing it must leave the process able to do it all again.

default9, max_bounces = 4, buckets = 2, four accumulations at 32 x 32 (two tile rows: one for each member of the group): seconds."""
import numpy as np
import pytest

from oracle_binding import bits

pytestmark = pytest.mark.gpu

SIZE, ACC = (32, 32), 4
POLICY = {"max_bounces": 4, "buckets": 2, "use_bvh": True}


def words(r):
    """(accumulator, resolved frame) of ACC accumulations at SIZE, as raw words."""
    r.Resize(*SIZE)
    r.Accumulate(ACC)
    assert r.Render()
    return bits(r.accumulator()).copy(), bits(r.GetFrame()).copy()


def assert_same(got, want, what):
    for g, w, part in zip(got, want, ("accumulator", "frame")):
        assert g.shape == w.shape, f"{what}, {part}: shape {g.shape} vs {w.shape}"
        assert np.array_equal(g, w), f"{what}, {part}: {int((g != w).sum())} of {g.size} words differ"


@pytest.fixture(scope="module")
def fresh_words(mirt):
    r = mirt.Renderer(mirt.scene.default9(), device=0, streams=3, **POLICY)
    want = words(r)
    r.close()
    return want


def churn(r):
    """Every owner of the context allocated, used and let go; leaves r with its switches off and nothing accumulated that the caller does not reset."""
    r.Resize(*SIZE)
    r.set_aov(True)
    r.set_sky_sampling(True)
    r.set_ggx_pdf(True)
    r.set_light_ris(4)
    r.set_material_closures([1])
    r.set_history_motion(True)
    r.Accumulate(2)
    assert r.render_temporal(iterations=2) is not None                     # the history, its id planes and the sphere snapshot
    assert r.history_info()["valid"]
    assert r.noise() is not None                                           # the noise scratch
    mask = np.zeros(r._tiles(), dtype=np.uint8)
    mask[0] = 1
    r.freeze_tiles(mask)                                                   # the freeze mask and the active list ...
    r.Accumulate(2)                                                        # ... and the sparse launches that read them
    r.ResetAccumulator()
    for streams in (3, 1, 3):                                              # slots dropped and built again
        r.set_policy(streams=streams)
        r.Accumulate(2)
    r.Resize(48, 32)
    info = r.history_info()
    assert not info["valid"] and info["bytes"] == 0, info                  # another image: the history went with the resize
    r.Accumulate(2)
    r.Resize(*SIZE)
    r.set_material_closures(None)
    r.set_light_ris(0)
    r.set_ggx_pdf(False)
    r.set_sky_sampling(False)
    r.set_history_motion(False)
    r.set_aov(False)
    r.UpdateScene()


def test_churned_context_computes_what_a_fresh_one_does(mirt, fresh_words):
    r = mirt.Renderer(mirt.scene.default9(), device=0, streams=3, **POLICY)
    churn(r)
    assert_same(words(r), fresh_words, "after the churn")
    r.close()
    # the process goes on: a second context, built and closed, gives the same words
    again = mirt.Renderer(mirt.scene.default9(), device=0, streams=3, **POLICY)
    assert_same(words(again), fresh_words, "a second context after the first was closed")
    again.close()


def test_group_rehearsal_closes_and_matches(mirt, fresh_words):
    g = mirt.GroupRenderer(mirt.scene.default9(), devices=(0, 0), streams=3, **POLICY)
    g.Resize(*SIZE)
    g.Accumulate(ACC)
    g.Gather()
    got = bits(g.accumulator()).copy()
    assert g.Render()
    assert_same((got, bits(g.GetFrame()).copy()), fresh_words, "a group of two members on device 0")
    g.close()
