// Stand-alone check of the tile map (csrc/tile_map.hpp), meant to be compiled under -fsanitize=address,undefined (tests/test_tile_map.py).
// For images of 1..5 x 0..7 tiles, 16 * h_tiles wide and 8 wider, every contiguous range that fits and every interleaving of the tile rows
// by 1..5: the local tiles ascend strictly and stay inside the image, the members of an interleaving partition it, and copy_owned_tiles,
// run on exactly-sized heap buffers, writes every pixel of an owned tile and no other float, for 1, 3 and 4 channels.  Prints
// "rows <v_tiles> <first_row> <row_stride> <n_rows>" for every interleaving: the test compares them with mirt.distributed.tile_rows.
#include "../../cpu-raytracing-experiments_amd/csrc/tile_map.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

using namespace mirt;

static int fail(const char* what, const TileMap& m, uint32_t a, uint32_t b) {
	std::printf("FAIL %s (%u, %u): first %u run %u stride %u h_tiles %u width %u\n", what, a, b, m.first_tile, m.run_tiles, m.stride_tiles, m.h_tiles, m.width);
	return 1;
}

// The n_tiles local tiles of m in an image of h_tiles x v_tiles tiles; owners[T]++ for every tile T they name.
static int check_map(const TileMap& m, uint32_t n_tiles, uint32_t v_tiles, std::vector<uint32_t>& owners) {
	const uint32_t all = m.h_tiles * v_tiles;
	for (uint32_t local = 0; local < n_tiles; local++) {
		const uint32_t t = m.global_tile(local);
		if (t >= all) return fail("tile outside the image", m, local, t);
		if (local && t <= m.global_tile(local - 1)) return fail("tiles do not ascend", m, local, t);
		owners[t]++;
		if (m.pixel_offset(local, 0u, 1u) != static_cast<size_t>(16u * (t / m.h_tiles)) * m.width + 16u * (t % m.h_tiles)) return fail("origin of the tile", m, local, t);
		if (m.pixel_offset(local, 255u, 4u) != (m.pixel_offset(local, 0u, 1u) + 15u * m.width + 15u) * 4u) return fail("last pixel of the tile", m, local, t);
	}
	return 0;
}

static int check_copy(const TileMap& m, uint32_t n_tiles, uint32_t v_tiles, const std::vector<uint32_t>& owned) {
	const uint32_t height = 16u * v_tiles;
	const float sentinel = -7.0f;
	for (uint32_t ch : { 1u, 3u, 4u }) {
		const size_t n = static_cast<size_t>(m.width) * height * ch;
		float* from = new float[n];                      // exactly sized: a write or read past either end is the sanitizer's
		float* to = new float[n];
		for (size_t i = 0; i < n; i++) { from[i] = static_cast<float>(i + 1); to[i] = sentinel; }
		copy_owned_tiles(m, n_tiles, ch, from, to);
		int bad = 0;
		for (uint32_t y = 0; y < height && !bad; y++)
			for (uint32_t x = 0; x < m.width && !bad; x++) {
				const bool mine = x < 16u * m.h_tiles && owned[(y / 16u) * m.h_tiles + x / 16u] != 0u;
				for (uint32_t k = 0; k < ch; k++) {
					const size_t i = (static_cast<size_t>(y) * m.width + x) * ch + k;
					if (to[i] != (mine ? from[i] : sentinel)) bad = fail(mine ? "owned pixel not copied" : "pixel of another tile written", m, x, y);
				}
			}
		delete[] from;
		delete[] to;
		if (bad) return 1;
	}
	return 0;
}

// An image of width x height pixels that is no whole number of tiles (70 x 40: 4 x 2 tiles, 6 columns and 8 rows that no tile owns): pixel_offset
// of every pixel of every tile against a plain double loop over the image, and copy_owned_tiles into an exactly-sized width x height buffer, for the
// whole image and for every interleaving of the tile rows by 1..3: every pixel of an owned tile is copied, the remainder and the others' tiles are not.
static int check_ragged(uint32_t width, uint32_t height) {
	const uint32_t h_tiles = width / 16u, v_tiles = height / 16u;
	int bad = 0;
	for (uint32_t stride = 1; stride <= 3; stride++)
		for (uint32_t first_row = 0; first_row < stride; first_row++) {
			const TileMap m = TileMap::of_rows(first_row, stride, h_tiles, width);
			const uint32_t n_tiles = TileMap::tile_rows_owned(v_tiles, first_row, stride) * h_tiles;
			std::vector<uint32_t> local_of(static_cast<size_t>(width) * height, UINT32_MAX);     // the double loop: which local tile owns pixel (x, y)
			uint32_t local = 0;
			for (uint32_t ty = first_row; ty < v_tiles; ty += stride)
				for (uint32_t tx = 0; tx < h_tiles; tx++, local++)
					for (uint32_t y = 16u * ty; y < 16u * ty + 16u; y++)
						for (uint32_t x = 16u * tx; x < 16u * tx + 16u; x++) {
							local_of[static_cast<size_t>(y) * width + x] = local;
							const uint32_t ID = (y - 16u * ty) * 16u + (x - 16u * tx);
							for (uint32_t ch : { 1u, 3u, 4u })
								if (m.pixel_offset(local, ID, ch) != (static_cast<size_t>(y) * width + x) * ch) bad += fail("ragged pixel_offset", m, x, y);
						}
			if (local != n_tiles) bad += fail("ragged tile count", m, local, n_tiles);
			for (uint32_t ch : { 1u, 3u, 4u }) {
				const size_t n = static_cast<size_t>(width) * height * ch;
				float* from = new float[n];
				float* to = new float[n];
				for (size_t i = 0; i < n; i++) { from[i] = static_cast<float>(i + 1); to[i] = -7.0f; }
				copy_owned_tiles(m, n_tiles, ch, from, to);
				for (size_t i = 0; i < n && !bad; i++)
					if (to[i] != (local_of[i / ch] != UINT32_MAX ? from[i] : -7.0f)) bad += fail("ragged copy_owned_tiles", m, static_cast<uint32_t>((i / ch) % width), static_cast<uint32_t>((i / ch) / width));
				delete[] from;
				delete[] to;
			}
		}
	if (!bad) std::printf("ragged %u %u ok\n", width, height);
	return bad;
}

int main() {
	int bad = 0;
	size_t cases = 0;
	for (const auto& size : { std::pair<uint32_t, uint32_t>{ 70u, 40u }, { 40u, 70u }, { 17u, 16u }, { 16u, 31u }, { 79u, 33u } }) { bad += check_ragged(size.first, size.second); cases++; }
	for (uint32_t h_tiles = 1; h_tiles <= 5; h_tiles++)
		for (uint32_t v_tiles = 0; v_tiles <= 7; v_tiles++)
			for (uint32_t width : { 16u * h_tiles, 16u * h_tiles + 8u }) {
				const uint32_t all = h_tiles * v_tiles;
				for (uint32_t first = 0; first <= all; first++)
					for (uint32_t n = 0; first + n <= all; n++, cases++) {
						const TileMap m = TileMap::of_range(first, h_tiles, width);
						std::vector<uint32_t> owned(all, 0u);
						if (check_map(m, n, v_tiles, owned)) { bad++; continue; }
						for (uint32_t t = 0; t < all; t++) if (owned[t] != (t >= first && t < first + n ? 1u : 0u)) bad += fail("range ownership", m, t, owned[t]);
						bad += check_copy(m, n, v_tiles, owned);
					}
				for (uint32_t stride = 1; stride <= 5; stride++) {
					std::vector<uint32_t> owners(all, 0u);
					for (uint32_t first_row = 0; first_row < stride || first_row <= v_tiles + 1u; first_row++, cases++) {
						const TileMap m = TileMap::of_rows(first_row, stride, h_tiles, width);
						const uint32_t n_rows = TileMap::tile_rows_owned(v_tiles, first_row, stride);      // (no function of h_tiles or width: printed once)
						if (width == 16u && h_tiles == 1) std::printf("rows %u %u %u %u\n", v_tiles, first_row, stride, n_rows);
						uint32_t expect_rows = 0;
						for (uint32_t r = first_row; r < v_tiles; r += stride) expect_rows++;
						if (n_rows != expect_rows || (first_row >= v_tiles && n_rows != 0u)) bad += fail("tile_rows_owned", m, first_row, n_rows);
						std::vector<uint32_t> owned(all, 0u);
						if (check_map(m, n_rows * h_tiles, v_tiles, owned)) { bad++; continue; }
						uint32_t count = 0;
						for (uint32_t t = 0; t < all; t++) {
							const uint32_t row = t / h_tiles;
							const bool mine = row >= first_row && (row - first_row) % stride == 0u;
							if (owned[t] != (mine ? 1u : 0u)) bad += fail("row ownership", m, t, owned[t]);
							count += owned[t];
							if (first_row < stride) owners[t] += owned[t];
						}
						if (count != n_rows * h_tiles) bad += fail("owned count", m, count, n_rows * h_tiles);
						bad += check_copy(m, n_rows * h_tiles, v_tiles, owned);
					}
					for (uint32_t t = 0; t < all; t++) if (owners[t] != 1u) { std::printf("FAIL members 0..%u do not partition %u x %u tiles: tile %u has %u owners\n", stride - 1u, h_tiles, v_tiles, t, owners[t]); bad++; }
				}
			}
	if (bad) std::printf("tile_map: %d failures in %zu cases\n", bad, cases);
	else std::printf("tile_map ok (%zu cases)\n", cases);
	return bad ? 1 : 0;
}
