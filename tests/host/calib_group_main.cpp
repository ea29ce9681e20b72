// Stand-alone check of the tile bookkeeping of mlh_calib_add (m-loam_amd/csrc/calib_group.hpp), meant to be built with -fsanitize=address,undefined:
// counts 0, 1, 255, 256, 257 per extrinsic, interleaved extrinsics, several appends, and the per-extrinsic tile lists of the assembly.
// Exit status 0 = pass.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "calib_group.hpp"

using namespace mlh;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static void check_append(const std::vector<int> &counts, unsigned seed, int first_given, std::vector<int> &all_tile_ext)
{
    std::vector<int32_t> ext;
    for (size_t e = 0; e < counts.size(); ++e) for (int k = 0; k < counts[e]; ++k) ext.push_back(int32_t(e));
    std::mt19937 rng(seed);
    for (size_t i = ext.size(); i > 1; --i) std::swap(ext[i - 1], ext[rng() % i]);      // interleaved
    const int n = int(ext.size());
    const CalibGrouping G = calib_group(n, ext.data(), first_given);
    int want_tiles = 0, max_ext = -1;
    for (size_t e = 0; e < counts.size(); ++e) { want_tiles += (counts[e] + 255) / 256; if (counts[e] > 0) max_ext = int(e); }
    REQUIRE(G.n_tiles == want_tiles && G.max_ext == max_ext);
    REQUIRE(G.perm.size() == size_t(want_tiles) * 256 && G.tile_ext.size() == size_t(want_tiles) && G.slot_of.size() == size_t(n));
    std::vector<int> seen(size_t(n), 0);
    int n_pad = 0;
    for (size_t s = 0; s < G.perm.size(); ++s) {
        const int g = G.perm[s];
        if (g < 0) { ++n_pad; continue; }
        const int i = g - first_given;
        REQUIRE(i >= 0 && i < n);
        seen[size_t(i)]++;
        REQUIRE(G.slot_of[size_t(i)] == int(s));
        REQUIRE(G.tile_ext[s / 256] == ext[size_t(i)]);                                // every tile belongs to one extrinsic
        if (s % 256 != 0 && G.perm[s - 1] >= 0) REQUIRE(G.perm[s - 1] < g);             // stable within a group
        if (s % 256 != 0) REQUIRE(G.perm[s - 1] >= 0);                                  // padding only at a tile's end
    }
    for (int i = 0; i < n; ++i) REQUIRE(seen[size_t(i)] == 1);
    REQUIRE(n_pad == want_tiles * 256 - n);
    for (size_t t = 1; t < G.tile_ext.size(); ++t) REQUIRE(G.tile_ext[t - 1] <= G.tile_ext[t]);
    all_tile_ext.insert(all_tile_ext.end(), G.tile_ext.begin(), G.tile_ext.end());
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
    const CalibGrouping none = calib_group(0, nullptr, 5);
    REQUIRE(none.n_tiles == 0 && none.perm.empty() && none.tile_ext.empty() && none.max_ext == -1);
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
    std::printf("calib_group: ok (%zu tiles over %d factors)\n", tile_ext.size(), given);
    return 0;
}
