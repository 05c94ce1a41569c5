// conv_tiles.h -- which tiles of the halo conv kernels are instantiated, and which of them have a
// hi-only (XHI) split instantiation: the one list behind the dispatch ladders of conv3.hip,
// conv3w.hip and conv3w8.hip (which expand it into kernel instantiations) and conv_plan.cpp (which
// takes the small tiles from it and refuses a plan that is not on it).  Plain C++, no HIP.
// The flags a launcher decides itself (split, MX, BST, ASMR, WIDE, dma_end) are expanded there.
#pragma once

namespace opk {

// conv3_kernel<BM, BN, HR, TAPU, MINB, KS, NW>.  The last four (NW = 4) are family conv3s, the
// small tiles of the small-batch mode (logged as conv3s_kernel<...>), per kernel size the smaller
// first; 7x7: a tap row per K unit under halos of 64 + 6 * 53 and 128 + 6 * 53 rows -- a 46-wide
// crop with its 3 + 3 border columns is one strip.  MINB = 1 for all four: the 128 x 64 3x3 tile's
// 76 KB of LDS do fit twice per CU, but MINB = 2 (waves_per_eu 2) moves its accumulators from AGPRs
// into VGPRs, a schedule nobody measured
#define OPK_CONV3_TILES(X)                                                                     \
    X(256, 64, 1024, 1, 1, 7, 8) X(256, 96, 1024, 1, 1, 7, 8) X(256, 128, 1024, 1, 1, 7, 8)    \
    X(256, 256, 256, 1, 1, 1, 16) X(512, 64, 512, 1, 1, 1, 16) X(512, 128, 512, 1, 1, 1, 16)   \
    X(256, 64, 256, 1, 2, 1, 8) X(256, 96, 256, 1, 2, 1, 8) X(256, 128, 256, 1, 2, 1, 8)       \
    X(256, 64, 448, 1, 2, 3, 8) X(512, 64, 768, 3, 1, 3, 8)                                    \
    X(512, 96, 704, 3, 1, 3, 16) X(256, 96, 448, 1, 2, 3, 8) X(256, 96, 512, 3, 1, 3, 8)       \
    X(512, 128, 704, 3, 1, 3, 16) X(256, 128, 448, 1, 2, 3, 8) X(256, 128, 512, 3, 1, 3, 8)    \
    X(64, 32, 256, 9, 1, 3, 4) X(128, 64, 320, 3, 1, 3, 4)                                     \
    X(64, 32, 384, 7, 1, 7, 4) X(128, 64, 448, 7, 1, 7, 4)
// conv3w8_kernel<BN, NB, POOL>
#define OPK_CONV3W8_TILES(X)                                                                   \
    X(128, 4, true) X(128, 2, true) X(64, 1, true) X(128, 1, true)                             \
    X(128, 4, false) X(128, 2, false) X(128, 1, false) X(96, 1, false) X(64, 1, false)
// conv3w_kernel<BN> and conv3p_kernel<BN>
#define OPK_CONV3W_BNS(X) X(96) X(128)

// a conv3_kernel tile (either family) has a hi-only instantiation unless it is a 7x7 tile
constexpr bool conv3_tile_has_xhi(int ks) { return ks != 7; }
// a conv3w8_kernel tile has one if it is a non-pooled 96 / 128-output tile
constexpr bool conv3w8_tile_has_xhi(int bn, bool pool) { return !pool && bn != 64; }

// the lists as data, for the planner
struct Conv3Tile { int bm, bn, hr, tapu, minb, ks, nw; };
struct Conv3w8Tile { int bn, nb; bool pool; };
#define OPK_TILE_ROW(...) {__VA_ARGS__},
#define OPK_TILE_BN(BN_) BN_,
constexpr Conv3Tile kConv3Tiles[] = {OPK_CONV3_TILES(OPK_TILE_ROW)};
constexpr Conv3w8Tile kConv3w8Tiles[] = {OPK_CONV3W8_TILES(OPK_TILE_ROW)};
constexpr int kConv3wBNs[] = {OPK_CONV3W_BNS(OPK_TILE_BN)};
#undef OPK_TILE_BN
#undef OPK_TILE_ROW

}  // namespace opk
