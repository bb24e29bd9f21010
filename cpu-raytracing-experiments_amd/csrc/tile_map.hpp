// Which tiles of the image a context owns, and where their pixels lie in it — the one statement of the rule, for host and device.
// A context owns runs of run_tiles consecutive LaunchIndices (Renderer.hpp:75,84-88), stride_tiles apart, starting at first_tile; its local
// tile t is the t-th of them in ascending order; a tile is 16 x 16 pixels, tile T at x = 16 (T % h_tiles), y = 16 (T / h_tiles) of an image
// `width` pixels wide.  Plain constexpr and inline functions, no HIP: k_resolve, k_resolve_aov and k_noise (resolve.hpp), the host layer
// (mirt_capi.hip, mirt_resolve.hip, mirt_group.hip) and the host-only check tests/native/tile_map_check.cpp, built under sanitizers, evaluate the same text.
// (The trace and shade kernels keep FrameParams and its global_tile with udiv_f: the hot-path form of the same rule.)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace mirt {

constexpr uint32_t kTileSize = 256;
constexpr uint32_t kTileRoot = 16;

struct TileMap {
	uint32_t first_tile;
	uint32_t run_tiles;         // at least 1
	uint32_t stride_tiles;      // 0: one contiguous range (mirt_set_tile_range)
	uint32_t h_tiles, width;

	// Global LaunchIndex of the context's local tile.
	constexpr uint32_t global_tile(uint32_t local) const {
		if (stride_tiles == 0u) return first_tile + local;
		const uint32_t run = local / run_tiles;
		return first_tile + run * stride_tiles + (local - run * run_tiles);
	}
	// Where pixel ID (0..255, row-major in its tile) of a local tile lies in a row-major image of `channels` words per pixel (row 0 = y 0).
	constexpr size_t pixel_offset(uint32_t local, uint32_t ID, uint32_t channels) const {
		const uint32_t tile = global_tile(local);
		const uint32_t x = kTileRoot * (tile % h_tiles) + (ID & 15u);
		const uint32_t y = kTileRoot * (tile / h_tiles) + (ID >> 4);
		return (static_cast<size_t>(y) * width + x) * channels;
	}
	// Interleaved tile rows (mirt_set_tile_rows): of v_tiles tile rows, the rows first_row, first_row + row_stride, ... — how many they are,
	constexpr static uint32_t tile_rows_owned(uint32_t v_tiles, uint32_t first_row, uint32_t row_stride) {
		return first_row < v_tiles ? (v_tiles - first_row + row_stride - 1u) / row_stride : 0u;
	}
	// ... and their map: runs of one tile row; tile_rows_owned(...) * h_tiles local tiles.
	constexpr static TileMap of_rows(uint32_t first_row, uint32_t row_stride, uint32_t h_tiles, uint32_t width) {
		return TileMap{ first_row * h_tiles, h_tiles ? h_tiles : 1u, row_stride > 1u ? row_stride * h_tiles : 0u, h_tiles, width };
	}
	// One contiguous range of local tiles from first_tile on (mirt_set_tile_range; the whole image: first_tile = 0).
	constexpr static TileMap of_range(uint32_t first_tile, uint32_t h_tiles, uint32_t width) { return TileMap{ first_tile, 1u, 0u, h_tiles, width }; }
};

// Copies the pixels of the map's first n_tiles local tiles, and no others, from one full-image buffer to another of the same layout
// (`channels` floats per pixel): pixels of other contexts' tiles are never written.
inline void copy_owned_tiles(const TileMap& m, uint32_t n_tiles, uint32_t channels, const float* from, float* to) {
	for (uint32_t local = 0; local < n_tiles; local++)
		for (uint32_t row = 0; row < kTileRoot; row++) {
			const size_t off = m.pixel_offset(local, row * kTileRoot, channels);
			memcpy(to + off, from + off, kTileRoot * channels * sizeof(float));
		}
}

}  // namespace mirt
