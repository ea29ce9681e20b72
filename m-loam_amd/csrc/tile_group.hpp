// Tile bookkeeping of the host-staged factor tables (odom.hip: mlh_pure_odom_set, calib.hip: mlh_calib_add), host arithmetic only: n factors are grouped by
// an integer key (ascending, stable within a key), every key starts on a 256-factor tile boundary and its last tile is padded. Kept in a header of its own
// so that a stand-alone host program can run it under a sanitizer (tests/host/tile_group_main.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mlh {

constexpr int CALIB_TILE = 256;

// the 256-record tiles of one stored cloud of n records, in order: emit(first record, records). A tile never straddles a cloud. (cloudbuild.hip: the map builder
// over stored clouds; session_host.hpp: the session image's pack)
template <class Emit> inline void segment_tiles(int n, Emit emit)
{
    for (int at = 0; at < n; at += CALIB_TILE) emit(at, n - at < CALIB_TILE ? n - at : CALIB_TILE);
}

struct TileGrouping {
    std::vector<int> slot_of;    // n: factor i -> slot relative to the grouping's first slot
    std::vector<int> perm;       // tiles * 256: slot -> first + i for the factor i it holds, or -1 for padding
    std::vector<int> tile_key;   // tiles: the key every factor of the tile has
    int n_tiles = 0, max_key = -1;
};

// key[i] >= 0 for every i (the caller has checked). mlh_calib_add: key = extrinsic, first = the number of factors the store was given before this append;
// mlh_pure_odom_set: key = frame * (max_ext + 1) + extrinsic, first = 0
inline TileGrouping tile_group(int n, const int32_t *key, int first)
{
    TileGrouping T;
    if (n <= 0) return T;
    for (int i = 0; i < n; ++i) if (key[i] > T.max_key) T.max_key = key[i];
    const size_t nk = size_t(T.max_key) + 1;
    std::vector<int> cnt(nk, 0), tile_start(nk + 1, 0), fill(nk, 0);
    for (int i = 0; i < n; ++i) cnt[size_t(key[i])]++;
    for (size_t g = 0; g < nk; ++g) tile_start[g + 1] = tile_start[g] + (cnt[g] + CALIB_TILE - 1) / CALIB_TILE;
    T.n_tiles = tile_start[nk];
    T.slot_of.assign(size_t(n), 0);
    T.perm.assign(size_t(T.n_tiles) * CALIB_TILE, -1);
    T.tile_key.assign(size_t(T.n_tiles), 0);
    for (int i = 0; i < n; ++i) {
        const size_t g = size_t(key[i]);
        const int slot = tile_start[g] * CALIB_TILE + fill[g]++;
        T.slot_of[size_t(i)] = slot;
        T.perm[size_t(slot)] = first + i;
    }
    for (size_t g = 0; g < nk; ++g) for (int t = tile_start[g]; t < tile_start[g + 1]; ++t) T.tile_key[size_t(t)] = int(g);
    return T;
}

// tiles of every extrinsic in tile order, as the assembly walks them: start (n_ext + 1 entries), tiles (one per tile whose extrinsic is < n_ext)
inline void calib_ext_lists(const std::vector<int> &tile_ext, int n_ext, std::vector<int> &start, std::vector<int> &tiles)
{
    start.assign(size_t(n_ext) + 1, 0);
    for (int e : tile_ext) if (e >= 0 && e < n_ext) start[size_t(e) + 1]++;
    for (int e = 0; e < n_ext; ++e) start[size_t(e) + 1] += start[size_t(e)];
    tiles.assign(size_t(start[size_t(n_ext)]), 0);
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (size_t t = 0; t < tile_ext.size(); ++t) {
        const int e = tile_ext[t];
        if (e >= 0 && e < n_ext) tiles[size_t(fill[size_t(e)]++)] = int(t);
    }
}

// n factor rows point[3] | coeff[6] | sqrt_info (null: 1.0, what the reference constructs these factors with, estimator.cpp:735, 751) into tab at slot
// slot_of[i] (null: i), the factor's type into type_out[type_stride * slot]. false at a type that is neither 0 (plane) nor 1 (edge).
inline bool pack_factor_rows(int n, const int32_t *type, const double *points, const double *coeffs, const double *sqrt_info, const int *slot_of,
                             double *tab, int *type_out, int type_stride)
{
    for (int i = 0; i < n; ++i) {
        if (type[i] != 0 && type[i] != 1) return false;
        const size_t s = slot_of ? size_t(slot_of[i]) : size_t(i);
        double *t = tab + s * 10;
        for (int k = 0; k < 3; ++k) t[k] = points[size_t(i) * 3 + k];
        for (int k = 0; k < 6; ++k) t[3 + k] = coeffs[size_t(i) * 6 + k];
        t[9] = sqrt_info ? sqrt_info[i] : 1.0;
        type_out[s * size_t(type_stride)] = type[i];
    }
    return true;
}

}  // namespace mlh
