// Tile bookkeeping of one mlh_calib_add (calib.hip), host arithmetic only: the n factors of an append are grouped by extrinsic (ascending index, stable
// within a group), every group starts on a 256-factor tile boundary and its last tile is padded. Kept in a header of its own so that a stand-alone host
// program can run it under a sanitizer (tests/host/calib_group_main.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mlh {

constexpr int CALIB_TILE = 256;

struct CalibGrouping {
    std::vector<int> slot_of;    // n: factor i of the append -> slot relative to the append's first slot
    std::vector<int> perm;       // tiles * 256: slot -> first_given + i, or -1 for padding
    std::vector<int> tile_ext;   // tiles: the extrinsic every factor of the tile belongs to
    int n_tiles = 0, max_ext = -1;
};

// ext_idx[i] >= 0 for every i (the caller has checked); first_given: the number of factors the store was given before this append
inline CalibGrouping calib_group(int n, const int32_t *ext_idx, int first_given)
{
    CalibGrouping G;
    if (n <= 0) return G;
    for (int i = 0; i < n; ++i) if (ext_idx[i] > G.max_ext) G.max_ext = ext_idx[i];
    const size_t ne = size_t(G.max_ext) + 1;
    std::vector<int> cnt(ne, 0), tile_start(ne + 1, 0), fill(ne, 0);
    for (int i = 0; i < n; ++i) cnt[size_t(ext_idx[i])]++;
    for (size_t e = 0; e < ne; ++e) tile_start[e + 1] = tile_start[e] + (cnt[e] + CALIB_TILE - 1) / CALIB_TILE;
    G.n_tiles = tile_start[ne];
    G.slot_of.assign(size_t(n), 0);
    G.perm.assign(size_t(G.n_tiles) * CALIB_TILE, -1);
    G.tile_ext.assign(size_t(G.n_tiles), 0);
    for (int i = 0; i < n; ++i) {
        const size_t e = size_t(ext_idx[i]);
        const int slot = tile_start[e] * CALIB_TILE + fill[e]++;
        G.slot_of[size_t(i)] = slot;
        G.perm[size_t(slot)] = first_given + i;
    }
    for (size_t e = 0; e < ne; ++e) for (int t = tile_start[e]; t < tile_start[e + 1]; ++t) G.tile_ext[size_t(t)] = int(e);
    return G;
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

}  // namespace mlh
