// The device tail's plan of m-loam_amd/csrc/fgr_host.hpp replayed on the host, in a stand-alone program built with plain g++ and -fsanitize=address,undefined and run
// directly (tests/test_fgr_tail_cases.py): nothing here is loaded into another process.
//   rng                       fgr_rng_at(seed, k) against sequential stepping of FgrRng at k = 0, 1, 2, 63, 64, 65, 3 2^20 + 1 and (seed 1) 3 10^8, for the seeds 1, 7,
//                             2^63 + 5 and 0; prints "R <seed> <k> <state> <draw>" for every pair
//   replay <manifest>         every line of the manifest: <file> <n> <swapped> <scale> <max> <seed>, <file> holding n x 6 f32 (p, q). Per line the count -> scan ->
//                             emit plan exactly as fgr.hip's three kernels run it -- segments of FGR_TT_RUN x FGR_TT_TPB trials, a run per thread, the exclusive
//                             prefix of the segments' counts, ranks in trial order, the cut at the cap -- through the functions the kernels call, held equal to
//                             fgr_tuple_test in corres and n_trials; every write of a segment must fall inside its slice [base, min(base + count, cap)) of corres,
//                             every kept rank must be written exactly once, and no draw may happen with ncorr = 0. Prints "T <tuples> <trials> <segments>" per line.
// Prints "fgr_tail: ok" and returns 0 when every check holds.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "fgr_host.hpp"

using namespace mlh;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static std::vector<FgrPair> read_pairs(const char *path, int n)
{
    std::vector<float> v(size_t(n) * 6);
    if (n > 0) {
        FILE *f = std::fopen(path, "rb");
        if (!f || std::fread(v.data(), sizeof(float), v.size(), f) != v.size()) { std::printf("cannot read %s\n", path); std::exit(2); }
        std::fclose(f);
    }
    std::vector<FgrPair> p(static_cast<size_t>(n));
    for (int e = 0; e < n; ++e) { p[size_t(e)].i = p[size_t(e)].j = e; for (int d = 0; d < 3; ++d) { p[size_t(e)].p[d] = v[size_t(6 * e + d)]; p[size_t(e)].q[d] = v[size_t(6 * e + 3 + d)]; } }
    return p;
}

static void rng_checks()
{
    const uint64_t seeds[4] = {1ull, 7ull, (1ull << 63) + 5ull, 0ull};
    const uint64_t ks[8] = {0, 1, 2, 63, 64, 65, 3ull * (1ull << 20) + 1ull, 300000000ull};
    for (uint64_t seed : seeds) {
        FgrRng step(seed);
        uint64_t at = 0;
        for (uint64_t k : ks) {                      // ascending: one stepped run serves them all; the longest for the first seed alone
            if (k > (1ull << 24) && seed != seeds[0]) continue;
            for (; at < k; ++at) step.next();
            FgrRng jump = fgr_rng_at(seed, k);
            CHECK(jump.s == step.s);
            FgrRng a = jump, b = step;
            const uint32_t da = a.next(), db = b.next();
            CHECK(da == db && a.s == b.s);
            std::printf("R %" PRIu64 " %" PRIu64 " %" PRIu64 " %u\n", seed, k, jump.s, da);
        }
    }
    // the table's first matrix is the update itself
    FgrRng r(12345);
    const uint64_t s0 = r.s;
    r.next();
    CHECK(fgr_gf2_apply(fgr_rng_table(), s0) == r.s);
    CHECK(FGR_TT_RUN <= 32 && FGR_TT_SEGMENT == (long long)FGR_TT_RUN * FGR_TT_TPB && FGR_OPT_REG_MAX == FGR_OPT_TPB * FGR_OPT_QREG);
}

// fgr.hip's three launches for `pairs`, each workgroup and thread in turn
static void replay(const std::vector<FgrPair> &pairs, bool swapped, float scale, int cap, uint64_t seed)
{
    const uint64_t *table = fgr_rng_table();
    const int ncorr = int(pairs.size());
    const long long total_trials = fgr_tt_total_trials(ncorr);
    const int nseg = fgr_tt_segments(ncorr);
    CHECK(total_trials == 100ll * ncorr && (long long)nseg * FGR_TT_SEGMENT >= total_trials);
    CHECK(nseg == 0 ? total_trials == 0 : (long long)(nseg - 1) * FGR_TT_SEGMENT < total_trials);
    const FgrPair *P = ncorr ? pairs.data() : nullptr;       // (ncorr = 0: any access would be a null dereference, any draw a division by zero)
    // count
    std::vector<int> counts(size_t(nseg) + 1, 0), base(size_t(nseg) + 1, 0);
    for (int s = 0; s < nseg + 1; ++s) {                      // (one segment behind the last: the launch is sized for the largest pair count)
        int c = 0;
        for (int t = 0; t < FGR_TT_TPB; ++t) {
            long long b, e;
            fgr_tt_run(total_trials, s, t, &b, &e);
            CHECK(b <= e && e <= total_trials && e - b <= FGR_TT_RUN);
            c += __builtin_popcount(fgr_tt_run_mask(table, P, ncorr, swapped, scale, seed, b, e));
        }
        if (s < nseg) counts[size_t(s)] = c; else CHECK(c == 0);
    }
    // scan
    long long total = 0;
    for (int s = 0; s < nseg; ++s) { base[size_t(s)] = int(total < cap ? total : cap); total += counts[size_t(s)]; }
    const int tuples = fgr_tt_tuples(total, cap);
    long long n_trials = fgr_tt_cap_reached(total, cap) ? -1 : total_trials;
    // emit
    std::vector<int32_t> corres(size_t(3 * tuples));          // exactly the kept tuples: one write past them is the sanitizer's
    std::vector<int> written(size_t(tuples), 0);
    for (int s = 0; s < nseg; ++s) {
        if (!fgr_tt_segment_emits(base[size_t(s)], counts[size_t(s)], cap)) continue;
        const int lo = base[size_t(s)], hi = int(std::min<long long>((long long)lo + counts[size_t(s)], cap));
        int rank = lo;
        for (int t = 0; t < FGR_TT_TPB; ++t) {
            long long b, e;
            fgr_tt_run(total_trials, s, t, &b, &e);
            const uint32_t mask = fgr_tt_run_mask(table, P, ncorr, swapped, scale, seed, b, e);
            if (!mask) continue;
            FgrRng rng = fgr_rng_at(table, seed, uint64_t(b) * 3ull);
            for (long long tr = b; tr < e; ++tr) {
                int r[3];
                fgr_trial_draw(ncorr, rng, r);
                if (!((mask >> int(tr - b)) & 1u)) continue;
                if (fgr_tt_rank_kept(rank, cap)) {
                    CHECK(rank >= lo && rank < hi && rank < tuples);
                    if (rank < tuples) { for (int d = 0; d < 3; ++d) corres[size_t(3 * rank + d)] = r[d]; ++written[size_t(rank)]; }
                }
                if (fgr_tt_rank_is_last(rank, cap)) { CHECK(n_trials == -1); n_trials = tr; }
                ++rank;
            }
        }
        CHECK(rank == lo + counts[size_t(s)]);
    }
    for (int w : written) CHECK(w == 1);
    // the sequential loop
    std::vector<int32_t> want;
    int want_trials = -1;
    const int want_tuples = fgr_tuple_test(pairs, swapped, scale, cap, seed, want, &want_trials);
    CHECK(want_tuples == tuples);
    CHECK(want == corres);
    CHECK((long long)want_trials == n_trials);
    std::printf("T %d %lld %d\n", tuples, n_trials, nseg);
}

int main(int argc, char **argv)
{
    if (argc >= 2 && std::string(argv[1]) == "rng") rng_checks();
    else if (argc >= 3 && std::string(argv[1]) == "replay") {
        FILE *m = std::fopen(argv[2], "r");
        if (!m) { std::printf("cannot read %s\n", argv[2]); return 2; }
        char path[4096];
        int n, swapped, cap;
        float scale;
        unsigned long long seed;
        while (std::fscanf(m, "%4095s %d %d %f %d %llu", path, &n, &swapped, &scale, &cap, &seed) == 6) replay(read_pairs(path, n), swapped != 0, scale, cap, uint64_t(seed));
        std::fclose(m);
    } else { std::printf("usage: fgr_tail_main rng | replay <manifest>\n"); return 2; }
    if (failures) { std::printf("fgr_tail: %d check(s) FAILED\n", failures); return 1; }
    std::printf("fgr_tail: ok\n");
    return 0;
}
