// Host side of the split-bf16 ("bf16x3") weight tapes that are functions of a packed fp32 blob (csrc/dgt2d_pack.cpp, csrc/cdgs_pack.cpp):
// the conversion of tiled matrices, one implementation for every model that derives its tape this way.
//
// A tiled matrix float [tiles = nb * nk][8 quads][64 lanes][4] is re-read as
//     bf16 [tiles * 4 K16 steps][3 terms: hi, mid, lo][64 lanes][8]
// where element j of lane l in K16 step G of a chunk is the chunk's f32 k-step 8 G + j of the same lane, tile[(8 G + j) / 4][l][(8 G + j) % 4]
// (the relation of csrc/dgt_split.h between the two MFMA forms), so row maps and slot order have no second implementation.  Every term is
// rounded to nearest even, as split8 rounds the activations; hi + mid + lo is the float exactly.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace jd_tape {

constexpr size_t TILE_FLOATS = 2048, TILE_BYTES = 4 * 3072;      // one (output block, K chunk) tile: fp32 packing, split tape

inline uint16_t bf16_rne(float v) {                               // finite inputs (weights); NaN keeps a quiet payload
    uint32_t u;
    std::memcpy(&u, &v, 4);
    if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)((u >> 16) | ((u & 0xffffu) ? 0x40u : 0u));
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float bf16_f32(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}

// `tiles` tiles at src (fp32 packing) -> tiles * TILE_BYTES bytes at dst
inline void split_tiles(const float* src, size_t tiles, uint16_t* dst) {
    for (size_t t = 0; t < tiles; ++t)
        for (int G = 0; G < 4; ++G)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int k = 8 * G + j;
                    const float v = src[t * TILE_FLOATS + ((size_t)(k / 4) * 64 + l) * 4 + k % 4];
                    const uint16_t hi = bf16_rne(v);
                    const float r1 = v - bf16_f32(hi);
                    const uint16_t mid = bf16_rne(r1);
                    const float r2 = r1 - bf16_f32(mid);
                    uint16_t* o = dst + (t * 4 + G) * 1536 + (size_t)l * 8 + j;
                    o[0] = hi; o[512] = mid; o[1024] = bf16_rne(r2);
                }
}

}  // namespace jd_tape
