// Stand-alone check of the tile bookkeeping of mlh_calib_add and mlh_pure_odom_set (m-loam_amd/csrc/tile_group.hpp), meant to be built with
// -fsanitize=address,undefined: counts 0, 1, 255, 256, 257 per extrinsic, interleaved extrinsics, several appends, the per-extrinsic tile lists of the
// assembly, and the (frame, extrinsic) keying of the window table against the counting sort mlh_pure_odom_set used to carry inline.
// Exit status 0 = pass.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "tile_group.hpp"

using namespace mlh;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static void check_append(const std::vector<int> &counts, unsigned seed, int first_given, std::vector<int> &all_tile_ext)
{
    std::vector<int32_t> ext;
    for (size_t e = 0; e < counts.size(); ++e) for (int k = 0; k < counts[e]; ++k) ext.push_back(int32_t(e));
    std::mt19937 rng(seed);
    for (size_t i = ext.size(); i > 1; --i) std::swap(ext[i - 1], ext[rng() % i]);      // interleaved
    const int n = int(ext.size());
    const TileGrouping G = tile_group(n, ext.data(), first_given);
    int want_tiles = 0, max_ext = -1;
    for (size_t e = 0; e < counts.size(); ++e) { want_tiles += (counts[e] + 255) / 256; if (counts[e] > 0) max_ext = int(e); }
    REQUIRE(G.n_tiles == want_tiles && G.max_key == max_ext);
    REQUIRE(G.perm.size() == size_t(want_tiles) * 256 && G.tile_key.size() == size_t(want_tiles) && G.slot_of.size() == size_t(n));
    std::vector<int> seen(size_t(n), 0);
    int n_pad = 0;
    for (size_t s = 0; s < G.perm.size(); ++s) {
        const int g = G.perm[s];
        if (g < 0) { ++n_pad; continue; }
        const int i = g - first_given;
        REQUIRE(i >= 0 && i < n);
        seen[size_t(i)]++;
        REQUIRE(G.slot_of[size_t(i)] == int(s));
        REQUIRE(G.tile_key[s / 256] == ext[size_t(i)]);                                // every tile belongs to one extrinsic
        if (s % 256 != 0 && G.perm[s - 1] >= 0) REQUIRE(G.perm[s - 1] < g);             // stable within a group
        if (s % 256 != 0) REQUIRE(G.perm[s - 1] >= 0);                                  // padding only at a tile's end
    }
    for (int i = 0; i < n; ++i) REQUIRE(seen[size_t(i)] == 1);
    REQUIRE(n_pad == want_tiles * 256 - n);
    for (size_t t = 1; t < G.tile_key.size(); ++t) REQUIRE(G.tile_key[t - 1] <= G.tile_key[t]);
    all_tile_ext.insert(all_tile_ext.end(), G.tile_key.begin(), G.tile_key.end());
}

// the grouping mlh_pure_odom_set had inline before it moved to tile_group(): a stable counting sort of the factor indices by frame * (max_ext + 1) + ext,
// every group padded to whole 256-factor tiles
static void inline_sort(const std::vector<int32_t> &frame_idx, const std::vector<int32_t> &ext_idx, int mf, int me, std::vector<int> &perm, std::vector<int> &tgrp)
{
    const int n = int(frame_idx.size()), ne = me + 1, ng = (mf + 1) * ne;
    std::vector<int> cnt(size_t(ng) + 1, 0), tile_start(size_t(ng) + 1, 0), fill(size_t(ng), 0);
    for (int i = 0; i < n; ++i) cnt[size_t(frame_idx[size_t(i)]) * ne + ext_idx[size_t(i)] + 1]++;
    for (int g = 0; g < ng; ++g) tile_start[size_t(g) + 1] = tile_start[size_t(g)] + (cnt[size_t(g) + 1] + 255) / 256;
    const int n_tiles = tile_start[size_t(ng)];
    perm.assign(size_t(n_tiles) * 256, -1); tgrp.assign(size_t(n_tiles), 0);
    for (int i = 0; i < n; ++i) {
        const int g = frame_idx[size_t(i)] * ne + ext_idx[size_t(i)];
        perm[size_t(tile_start[size_t(g)]) * 256 + fill[size_t(g)]++] = i;
    }
    for (int g = 0; g < ng; ++g) for (int t = tile_start[size_t(g)]; t < tile_start[size_t(g) + 1]; ++t) tgrp[size_t(t)] = g;
}

// counts[f * n_ext + e] factors on (frame f, extrinsic e), interleaved: the keying of mlh_pure_odom_set (perm[slot] = i) against inline_sort
static void check_window_keying(const std::vector<int> &counts, int n_ext, unsigned seed)
{
    std::vector<int32_t> fi, ei;
    int mf = 0, me = 0;
    for (size_t g = 0; g < counts.size(); ++g)
        for (int k = 0; k < counts[g]; ++k) { fi.push_back(int32_t(g) / n_ext); ei.push_back(int32_t(g) % n_ext); }
    std::mt19937 rng(seed);
    for (size_t i = fi.size(); i > 1; --i) { const size_t j = rng() % i; std::swap(fi[i - 1], fi[j]); std::swap(ei[i - 1], ei[j]); }
    const int n = int(fi.size());
    for (int i = 0; i < n; ++i) { if (fi[size_t(i)] > mf) mf = fi[size_t(i)]; if (ei[size_t(i)] > me) me = ei[size_t(i)]; }
    std::vector<int32_t> key(size_t(n), 0);
    for (int i = 0; i < n; ++i) key[size_t(i)] = fi[size_t(i)] * (me + 1) + ei[size_t(i)];
    const TileGrouping T = tile_group(n, key.data(), 0);
    const std::vector<int> &perm = T.perm;
    std::vector<int> want_perm, want_tgrp;
    inline_sort(fi, ei, mf, me, want_perm, want_tgrp);
    REQUIRE(T.n_tiles == int(want_tgrp.size()) && T.tile_key == want_tgrp && perm == want_perm);
    REQUIRE(T.slot_of.size() == size_t(n));
    for (int i = 0; i < n; ++i) REQUIRE(perm[size_t(T.slot_of[size_t(i)])] == i);
    int max_key = -1;
    for (int k : key) if (k > max_key) max_key = k;
    REQUIRE(T.max_key == max_key);
}

int main()
{
    std::vector<int> tile_ext;
    int given = 0;
    const std::vector<std::vector<int>> appends = {{0, 1, 0, 255}, {0}, {256}, {0, 257, 3, 0, 1}, {0, 2600, 0, 2500}, {1, 1, 1, 1, 1, 1}, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 512}};
    unsigned seed = 1;
    for (const auto &c : appends) {
        check_append(c, seed++, given, tile_ext);
        for (int x : c) given += x;
    }
    // n = 0: nothing
    const TileGrouping none = tile_group(0, nullptr, 5);
    REQUIRE(none.n_tiles == 0 && none.slot_of.empty() && none.perm.empty() && none.tile_key.empty() && none.max_key == -1);
    // the assembly's lists: every tile once, under its extrinsic, in tile order; extrinsics the call does not have are left out
    for (int n_ext : {1, 2, 4, 21, 30}) {
        std::vector<int> start, tiles;
        calib_ext_lists(tile_ext, n_ext, start, tiles);
        REQUIRE(start.size() == size_t(n_ext) + 1 && start[0] == 0 && size_t(start[size_t(n_ext)]) == tiles.size());
        size_t expect = 0;
        for (int e : tile_ext) expect += e < n_ext;
        REQUIRE(tiles.size() == expect);
        for (int e = 0; e < n_ext; ++e)
            for (int k = start[size_t(e)]; k < start[size_t(e) + 1]; ++k) {
                REQUIRE(tiles[size_t(k)] >= 0 && size_t(tiles[size_t(k)]) < tile_ext.size() && tile_ext[size_t(tiles[size_t(k)])] == e);
                if (k > start[size_t(e)]) REQUIRE(tiles[size_t(k) - 1] < tiles[size_t(k)]);
            }
    }
    std::vector<int> start, tiles;
    calib_ext_lists({}, 3, start, tiles);
    REQUIRE(start.size() == 4 && tiles.empty());
    // the window table's (frame, extrinsic) keying: 3 frames x 2 extrinsics with the edge counts, a key with no factor between two that have some, one key alone
    check_window_keying({1, 255, 0, 256, 257, 3}, 2, 11);
    check_window_keying({256, 0, 0, 0, 0, 1}, 2, 12);
    check_window_keying({0, 0, 0, 0, 700, 0}, 2, 13);
    check_window_keying({5}, 1, 14);
    check_window_keying({0, 1, 255, 256, 257, 0, 0, 2, 513}, 3, 15);
    // pack_factor_rows: rows land in their slots, the type beside them at the caller's stride; a type outside {0, 1} is refused
    {
        const int32_t type[3] = {1, 0, 1};
        const int slot_of[3] = {2, 0, 1};
        double points[9], coeffs[18], sq[3] = {0.5, 2.0, 3.0};
        for (int k = 0; k < 9; ++k) points[k] = 10.0 + k;
        for (int k = 0; k < 18; ++k) coeffs[k] = 100.0 + k;
        std::vector<double> tab(30, 0.0);
        std::vector<int> side(9, -7);
        REQUIRE(pack_factor_rows(3, type, points, coeffs, sq, slot_of, tab.data(), side.data(), 3));
        for (int i = 0; i < 3; ++i) {
            const double *t = tab.data() + 10 * slot_of[i];
            for (int k = 0; k < 3; ++k) REQUIRE(t[k] == points[3 * i + k]);
            for (int k = 0; k < 6; ++k) REQUIRE(t[3 + k] == coeffs[6 * i + k]);
            REQUIRE(t[9] == sq[i] && side[size_t(3 * slot_of[i])] == type[i] && side[size_t(3 * slot_of[i] + 1)] == -7);
        }
        std::vector<int> types(3, -7);
        REQUIRE(pack_factor_rows(3, type, points, coeffs, nullptr, nullptr, tab.data(), types.data(), 1));
        REQUIRE(tab[9] == 1.0 && tab[10] == points[3] && types[0] == 1 && types[1] == 0 && types[2] == 1);
        const int32_t bad[3] = {0, 2, 1};
        REQUIRE(!pack_factor_rows(3, bad, points, coeffs, nullptr, nullptr, tab.data(), types.data(), 1));
    }
    std::printf("tile_group: ok (%zu tiles over %d factors)\n", tile_ext.size(), given);
    return 0;
}
