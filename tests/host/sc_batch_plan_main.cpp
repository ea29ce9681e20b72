// The host plan of the batched place-index build (m-loam_amd/csrc/sc_host.hpp: sc_batch_plan, sc_grown_cap) in a program of its own; tests/test_sc_batch_cases.py
// builds it with -fsanitize=address,undefined and runs it. It checks the plan itself -- every point of every entry in exactly one chunk, a chunk inside one entry,
// full chunks a multiple of the pass, at most SC_BATCH_MAX_CHUNKS per entry, no more chunks than sc_batch_chunk_bound gave room for -- and prints it for the
// Python restatement to compare:
//   sc_batch_plan_main plan <target_workgroups> <n_points of entry 0> <of entry 1> ...     ->  "C entry first count" per chunk
//   sc_batch_plan_main cap <n> <cap> <more>                                                  ->  "G capacity"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sc_host.hpp"

using namespace mlh;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

int main(int argc, char **argv)
{
    if (argc >= 5 && !std::strcmp(argv[1], "cap")) {
        std::printf("G %lld\n", sc_grown_cap(std::atoll(argv[2]), std::atoll(argv[3]), std::atoll(argv[4])));
        std::printf("sc_batch_plan: ok\n");
        return 0;
    }
    if (argc < 3 || std::strcmp(argv[1], "plan")) return 2;
    const int target = std::atoi(argv[2]), n_entries = argc - 3;
    std::vector<int> n_points;
    for (int i = 3; i < argc; ++i) n_points.push_back(std::atoi(argv[i]));
    const size_t bound = sc_batch_chunk_bound(n_entries, target);
    std::vector<ScChunk> chunks(bound);                       // exactly the room the library gives it: a chunk too many is an overrun the sanitizer reports
    const size_t n_chunks = sc_batch_plan(n_points.data(), n_entries, target, chunks.data());
    EXPECT(n_chunks <= bound);
    std::vector<long long> next(size_t(n_entries), 0);        // the first point of each entry no chunk has taken yet
    std::vector<int> per_entry(size_t(n_entries), 0);
    int last_entry = -1;
    for (size_t c = 0; c < n_chunks; ++c) {
        const ScChunk &k = chunks[c];
        EXPECT(k.entry >= 0 && k.entry < n_entries);
        if (k.entry < 0 || k.entry >= n_entries) break;
        EXPECT(k.entry >= last_entry);
        last_entry = k.entry;
        EXPECT(k.count > 0 && (long long)k.first == next[size_t(k.entry)]);
        next[size_t(k.entry)] += k.count;
        EXPECT(next[size_t(k.entry)] <= (long long)n_points[size_t(k.entry)]);
        if (next[size_t(k.entry)] < (long long)n_points[size_t(k.entry)]) EXPECT(k.count % SC_BATCH_CHUNK_POINTS == 0);
        per_entry[size_t(k.entry)] += 1;
        std::printf("C %d %d %d\n", k.entry, k.first, k.count);
    }
    for (int e = 0; e < n_entries; ++e) {
        EXPECT(next[size_t(e)] == (long long)(n_points[size_t(e)] > 0 ? n_points[size_t(e)] : 0));
        EXPECT(per_entry[size_t(e)] <= SC_BATCH_MAX_CHUNKS);
    }
    std::printf("sc_batch_plan: %s\n", fails ? "FAILED" : "ok");
    return fails ? 1 : 0;
}
