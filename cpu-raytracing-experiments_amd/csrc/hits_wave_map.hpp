// k_primary_hits_wave (kernels.hpp): which batches it takes, and where a record lies in the wave's staging area on its way from the lane that
// computed it (lane = slot of a group of 64, one pixel of the run after the other) to the lane that stores it (16 lanes = the 16 pixels of
// the run for one slot = one 128-B segment of hit_out[slot][pixel]).  Plain constexpr functions, no HIP: the kernel and the host-only check
// tests/native/hits_wave_map_check.cpp, built under sanitizers, evaluate the same text.
#pragma once
#include <stdint.h>

namespace mirt {

constexpr uint32_t kWaveHitsMinBatch = 32;      // batches below this keep one lane per pixel (a wave per pixel would be mostly empty lanes)
constexpr uint32_t kWaveHitsRun = 16;           // pixels a wave takes at a time = one row of a tile
constexpr uint32_t kWaveHitsPasses = kWaveHitsRun;                 // write-out passes of a group: 64 lanes store 4 slots x 16 pixels each
constexpr uint32_t kWaveHitsStage = kWaveHitsRun * 64u;            // records staged per wave (8 B each)

constexpr uint32_t hits_wave_groups(uint32_t batch_n) { return (batch_n + 63u) >> 6; }
constexpr uint32_t hits_wave_group_slots(uint32_t batch_n, uint32_t g) { return batch_n - g * 64u < 64u ? batch_n - g * 64u : 64u; }   // g < hits_wave_groups(batch_n)
// Row p = the 64 slots of pixel p, column ^ p: the 64 lanes that write a row, and the 16 lanes that read one column of 16 rows, each
// touch 16 different 8-B bank pairs.
constexpr uint32_t hits_wave_stage_index(uint32_t p, uint32_t s) { return p * 64u + (s ^ p); }
constexpr uint32_t hits_wave_out_pixel(uint32_t lane) { return lane & (kWaveHitsRun - 1u); }
constexpr uint32_t hits_wave_out_slot(uint32_t lane, uint32_t pass) { return pass * (64u / kWaveHitsRun) + lane / kWaveHitsRun; }       // slot within the group

}  // namespace mirt
