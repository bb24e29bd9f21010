"""The tile map (csrc/tile_map.hpp): which tiles a context owns and where their pixels lie in the image.

On the host, without a GPU: tests/native/tile_map_check.cpp, a stand-alone program built under sanitizers, runs the header's own functions over
every small image, range and interleaving, and prints the row counts, which are compared with mirt.distributed.tile_rows (the Python statement
of the same rule).  On the GPU (-m gpu): contexts whose ranges start and end in the middle of a tile row, in an image whose width and height are
no multiples of 16, paint Render(), render_aov() and the noise map into sentinel-filled images: their own tiles bit for bit as a context that
owns the whole image renders them, and not one other word."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = np.float32(-12345.0)


def test_tile_map_under_sanitizers(mirt, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "tile_map_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "native", "tile_map_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "tile_map ok" in out.stdout
    rows = [tuple(int(v) for v in line.split()[1:]) for line in out.stdout.splitlines() if line.startswith("rows ")]
    assert len(rows) >= 8 * 15 and {r[2] for r in rows} == {1, 2, 3, 4, 5} and {r[0] for r in rows} == set(range(8))
    assert any(first >= v for v, first, _, _ in rows) and any(n > 1 for *_, n in rows)
    for v_tiles, first_row, stride, n_rows in rows:
        assert mirt.distributed.tile_rows(v_tiles, first_row, stride) == (first_row, stride, n_rows), (v_tiles, first_row, stride, n_rows)


def same_words(got, want, what):
    bad = int((np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).sum())
    assert bad == 0, f"{what}: {bad} of {got.size} words differ"


@pytest.mark.gpu
def test_partial_contexts_write_their_tiles_and_nothing_else(mirt):
    """default9 at 72 x 40: 4 x 2 tiles, and 8 columns and 8 rows that belong to no tile.  Tiles 3..5 start mid-row and cross a row end."""
    w, h, h_tiles, v_tiles = 72, 40, 4, 2
    aovs = (mirt.AOV_DEPTH, mirt.AOV_NORMAL, mirt.AOV_ALBEDO)

    def context(setup=None):
        r = mirt.Renderer(mirt.scene.default9(), use_bvh=False, buckets=5, aov=True)
        r.Resize(w, h)
        if setup:
            setup(r)
        r.Accumulate(5)
        return r

    whole = context()
    assert whole.Render()
    want = {"frame": whole.GetFrame().copy(), "noise": whole.noise(want_map=True)["map"], **{k: whole.render_aov(k) for k in aovs}}
    whole.close()
    assert all(np.isfinite(v).all() and (v != SENTINEL).all() for v in want.values())

    cases = [("SetTileRange(3, 3)", lambda r: r.SetTileRange(3, 3), [3, 4, 5]),
             ("SetTileRange(0, 0)", lambda r: r.SetTileRange(0, 0), []),
             ("SetTileRows(1, 2)", lambda r: r.SetTileRows(1, 2), [4, 5, 6, 7])]
    for name, setup, tiles in cases:
        mine = np.zeros((h, w), dtype=bool)
        for t in tiles:
            mine[16 * (t // h_tiles): 16 * (t // h_tiles) + 16, 16 * (t % h_tiles): 16 * (t % h_tiles) + 16] = True
        r = context(setup)
        assert r.accumulator().shape[0] == len(tiles)
        r.framebuffer[:] = SENTINEL
        assert r.Render()
        got = {"frame": r.GetFrame()}
        for k in aovs:
            got[k] = r.render_aov(k, out=np.full_like(want[k], SENTINEL))
        noise = r.noise(map_out=np.full((h, w), SENTINEL, dtype=np.float32))
        assert noise["owned_pixels"] == 256 * len(tiles)
        got["noise"] = noise["map"]
        r.close()
        for k, image in got.items():
            same_words(image[mine], want[k][mine], f"{name}, {k}: pixels of the owned tiles")
            same_words(image[~mine], np.full_like(image[~mine], SENTINEL), f"{name}, {k}: pixels of no owned tile")
