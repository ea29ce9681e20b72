// m-loam_amd/csrc/session_host.hpp in a program of its own (tests/test_session_cases.py builds it with -fsanitize=address,undefined and runs it):
//   session_host_main write <path>      a small image from fixed formulae (tests/session_cases.py: small_image writes the same bytes in Python)
//   session_host_main fuzz <path>       the validation over the image in <path>: accepted as it is (payload checksums included); EVERY truncation refused;
//                                       the listed corruptions refused -- each in a heap block of exactly the image's size, so a read out of bounds is reported
//   session_host_main tiles src:n ...   the pack's tiles over clouds given in canonical order: "T src dst count word0" per tile
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <vector>
#include "session_host.hpp"

using namespace mlh;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static std::vector<unsigned char> small_image()
{
    const int n[2][3] = {{2, 1, 0}, {0, 1, 2}};
    std::vector<unsigned char> keys(sess_keyframes_bytes(2), 0), pts(16 * 6), pg(sess_pg_bytes(3), 0);
    for (int i = 0; i < 2; ++i) {
        SessKey k;
        std::memset(&k, 0, sizeof(k));
        for (int j = 0; j < 7; ++j) k.pose[j] = 0.5 * j + i;
        for (int j = 0; j < 36; ++j) k.cov[j] = 1e-4 * (j + 1) + i;
        for (int j = 0; j < 3; ++j) { k.pos[j] = float(k.pose[j]); k.n[j] = n[i][j]; }
        k.has_outlier = i;
        std::memcpy(keys.data() + sizeof(k) * size_t(i), &k, sizeof(k));
    }
    for (int j = 0; j < 6; ++j) {
        const float p[4] = {j + 0.25f, -float(j), 0.5f * j, float(j % 2)};
        std::memcpy(pts.data() + 16 * j, p, 16);
    }
    SessScHead sh;
    std::memset(&sh, 0, sizeof(sh));
    sh.opts.lidar_height = 2.0; sh.opts.num_ring = 2; sh.opts.num_sector = 3; sh.opts.max_radius = 80.0; sh.opts.num_exclude_recent = 1; sh.opts.num_candidates = 4;
    sh.opts.search_ratio = 0.1; sh.opts.dist_thres = 0.5; sh.opts.tree_making_period = 3; sh.opts.loop_distance_threshold = 50.0;
    sh.n = 2; sh.book_counter = 5; sh.book_prefix = 1; sh.last_host_decided = 3; sh.last_skipped = 1; sh.points_host_decided = 7; sh.points_skipped = 2;
    const SessScLayout L = sess_sc_layout(2, 3, 2);
    std::vector<unsigned char> sc(L.bytes, 0);
    std::memcpy(sc.data(), &sh, sizeof(sh));
    for (int j = 0; j < 12; ++j) { const float v = 0.5f * j; std::memcpy(sc.data() + L.desc + 4 * j, &v, 4); }
    for (int j = 0; j < 4; ++j) { const float v = 0.25f * j; std::memcpy(sc.data() + L.ring_key + 4 * j, &v, 4); }
    for (int j = 0; j < 6; ++j) {
        const double a = 1.5 * j, c = 2.5 * j, p = j - 1.0;
        std::memcpy(sc.data() + L.sector_key + 8 * j, &a, 8); std::memcpy(sc.data() + L.col_norm + 8 * j, &c, 8); std::memcpy(sc.data() + L.pos + 8 * j, &p, 8);
    }
    sc[L.has_pos] = 1;
    const SessPgHead ph = {3, 0, 128, 0};
    std::memcpy(pg.data(), &ph, sizeof(ph));
    for (int i = 0; i < 3; ++i) {
        SessPgRecord r;
        std::memset(&r, 0, sizeof(r));
        r.pose[0] = i; r.pose[1] = 1.0; r.pose[2] = 2.0; r.pose[6] = 1.0; r.last[6] = 1.0; r.loop_rel[0] = 0.1 * i; r.loop_rel[6] = 1.0;
        r.loop_index = i == 2 ? 0 : -1;
        std::memcpy(pg.data() + sizeof(ph) + sizeof(r) * size_t(i), &r, sizeof(r));
    }
    const std::vector<unsigned char> *part[SESS_SLOTS] = {&keys, &pts, &sc, &pg};
    const uint64_t bytes[SESS_SLOTS] = {keys.size(), pts.size(), sc.size(), pg.size()}, count[SESS_SLOTS] = {2, 6, 2, 3};
    const bool present[SESS_SLOTS] = {true, true, true, true};
    SessHeader H;
    sess_lay_out(H, bytes, count, present);
    std::vector<unsigned char> img(H.total_bytes, 0);
    for (int k = 0; k < SESS_SLOTS; ++k) {
        std::memcpy(img.data() + H.sec[k].offset, part[k]->data(), part[k]->size());
        H.sec[k].checksum = sess_checksum(part[k]->data(), part[k]->size());
    }
    sess_seal(H);
    std::memcpy(img.data(), &H, sizeof(H));
    return img;
}

// validation of exactly `n` bytes in a heap block of that size
static const char *check(const unsigned char *p, size_t n)
{
    unsigned char *blk = static_cast<unsigned char *>(std::malloc(n ? n : 1));
    if (n) std::memcpy(blk, p, n);
    SessHeader H;
    const char *why = sess_validate(n ? blk : nullptr, n, H);
    if (!why) why = sess_verify(blk, H);
    std::free(blk);
    return why;
}

int main(int argc, char **argv)
{
    if (argc >= 3 && !std::strcmp(argv[1], "write")) {
        const std::vector<unsigned char> img = small_image();
        FILE *f = std::fopen(argv[2], "wb");
        if (!f || std::fwrite(img.data(), 1, img.size(), f) != img.size()) return 2;
        std::fclose(f);
        std::printf("session_host: ok\n");
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "tiles")) {
        std::vector<SessTile> tiles;
        long long dst = 0;
        for (int i = 2; i < argc; ++i) {
            long long src = 0;
            int n = 0;
            if (std::sscanf(argv[i], "%lld:%d", &src, &n) != 2) return 2;
            sess_cloud_tiles(tiles, src, dst, 0, n, 0, SESS_POINTS);
            dst += n;
        }
        for (const SessTile &t : tiles) std::printf("T %lld %lld %d %llu\n", t.src, t.dst, t.count, t.word0);
        std::printf("session_host: ok\n");
        return 0;
    }
    if (argc < 3 || std::strcmp(argv[1], "fuzz")) return 2;
    std::vector<unsigned char> img;
    {
        FILE *f = std::fopen(argv[2], "rb");
        if (!f) return 2;
        unsigned char buf[4096];
        size_t got;
        while ((got = std::fread(buf, 1, sizeof(buf), f)) > 0) img.insert(img.end(), buf, buf + got);
        std::fclose(f);
    }
    const char *why = check(img.data(), img.size());
    if (why) std::printf("the valid image is refused: %s\n", why);
    EXPECT(why == nullptr);
    int refused = 0;
    for (size_t n = 0; n < img.size(); ++n) { const char *w = check(img.data(), n); EXPECT(w != nullptr); refused += w != nullptr; }
    std::printf("%d truncations refused\n", refused);

    SessHeader H0;
    std::memcpy(&H0, img.data(), sizeof(H0));
    // a corruption: edits a copy of the image (header included: `H` is written back and, when `reseal`, given a fresh checksum, so that the field's own check
    // is what refuses it and not the header checksum)
    int n_corrupt = 0;
    const auto corrupt = [&](const char *what, bool reseal, const std::function<void(SessHeader &, std::vector<unsigned char> &)> &edit) {
        std::vector<unsigned char> c = img;
        SessHeader H = H0;
        edit(H, c);
        if (reseal) sess_seal(H);
        std::memcpy(c.data(), &H, sizeof(H));
        const char *w = check(c.data(), c.size());
        if (!w) { std::printf("FAILED: accepted with %s%s\n", what, reseal ? " (resealed)" : ""); ++fails; }
        ++n_corrupt;
    };
    // every header field at 0, at its maximum, and one past the valid value; with and without a fresh header checksum
    for (int reseal = 0; reseal < 2; ++reseal) {
        const uint32_t m32 = std::numeric_limits<uint32_t>::max();
        const uint64_t m64 = std::numeric_limits<uint64_t>::max();
        uint32_t SessHeader::*const f32[] = {&SessHeader::magic, &SessHeader::version, &SessHeader::rec_point, &SessHeader::rec_pg, &SessHeader::rec_key, &SessHeader::n_slots};
        for (auto f : f32)
            for (int v = 0; v < 3; ++v) corrupt("a u32 header field", reseal, [&](SessHeader &H, std::vector<unsigned char> &) { H.*f = v == 0 ? 0u : (v == 1 ? m32 : H.*f + 1u); });
        for (int v = 0; v < 3; ++v) corrupt("total_bytes", reseal, [&](SessHeader &H, std::vector<unsigned char> &) { H.total_bytes = v == 0 ? 0 : (v == 1 ? m64 : H.total_bytes + 1); });
        for (int v = 1; v < 3; ++v) corrupt("reserved", reseal, [&](SessHeader &H, std::vector<unsigned char> &) { H.reserved = v == 1 ? m64 : 1; });
        for (int k = 0; k < SESS_SLOTS; ++k) {
            for (int v = 0; v < 3; ++v) {
                corrupt("section kind", reseal, [&](SessHeader &H, std::vector<unsigned char> &) { H.sec[k].kind = v == 0 ? 0u : (v == 1 ? m32 : H.sec[k].kind + 1u); });
                corrupt("section offset", reseal, [&](SessHeader &H, std::vector<unsigned char> &) { H.sec[k].offset = v == 0 ? 0 : (v == 1 ? m64 : H.sec[k].offset + 1); });
                corrupt("section bytes", reseal, [&](SessHeader &H, std::vector<unsigned char> &) { H.sec[k].bytes = v == 0 ? 0 : (v == 1 ? m64 : H.sec[k].bytes + 1); });
                corrupt("section count", reseal, [&](SessHeader &H, std::vector<unsigned char> &) { H.sec[k].count = v == 0 ? 0 : (v == 1 ? m64 : H.sec[k].count + 1); });
                corrupt("section checksum", reseal, [&](SessHeader &H, std::vector<unsigned char> &) { H.sec[k].checksum = v == 0 ? 0 : (v == 1 ? m64 : H.sec[k].checksum + 1); });
            }
            corrupt("section reserved", reseal, [&](SessHeader &H, std::vector<unsigned char> &) { H.sec[k].reserved = 1; });
            corrupt("section bytes + 16 (out of bounds / overlap)", reseal, [&](SessHeader &H, std::vector<unsigned char> &) { H.sec[k].bytes += 16; });
            corrupt("section offset - 16 (overlap)", reseal, [&](SessHeader &H, std::vector<unsigned char> &) { H.sec[k].offset -= 16; });
            corrupt("section offset beyond the image", reseal, [&](SessHeader &H, std::vector<unsigned char> &) { H.sec[k].offset = H.total_bytes; });
        }
        corrupt("header checksum", false, [&](SessHeader &H, std::vector<unsigned char> &) { H.header_checksum ^= 1; });
    }
    // contents, the section's checksum made to fit so that the contents' own check is what refuses them
    const auto in_section = [&](int slot, size_t at, const void *v, size_t n) {
        return [=](SessHeader &H, std::vector<unsigned char> &c) {
            std::memcpy(c.data() + H.sec[slot].offset + at, v, n);
            H.sec[slot].checksum = sess_checksum(c.data() + H.sec[slot].offset, size_t(H.sec[slot].bytes));
        };
    };
    const int32_t minus2 = -2, neg = -1, big = 1 << 20, two = 2, three = 3, zero = 0;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    corrupt("a negative n[]", true, in_section(SESS_KEYFRAMES, offsetof(SessKey, n), &neg, 4));
    corrupt("n[] that disagrees with POINTS", true, in_section(SESS_KEYFRAMES, offsetof(SessKey, n) + 4, &big, 4));
    corrupt("n[] of key 1 that disagrees with POINTS", true, in_section(SESS_KEYFRAMES, sizeof(SessKey) + offsetof(SessKey, n), &two, 4));
    corrupt("a NaN pose", true, in_section(SESS_KEYFRAMES, 8 * 3, &nan, 8));
    corrupt("an infinite pose of key 1", true, in_section(SESS_KEYFRAMES, sizeof(SessKey) + 8, &inf, 8));
    corrupt("outlier points without the flag", true, in_section(SESS_KEYFRAMES, sizeof(SessKey) + offsetof(SessKey, has_outlier), &zero, 4));
    corrupt("SC num_ring 0", true, in_section(SESS_SC, offsetof(mlh_sc_opts, num_ring), &zero, 4));
    corrupt("SC num_ring * num_sector too large", true, in_section(SESS_SC, offsetof(mlh_sc_opts, num_ring), &big, 4));
    corrupt("SC n that disagrees with the length", true, in_section(SESS_SC, offsetof(SessScHead, n), &three, 4));
    corrupt("SC negative n", true, in_section(SESS_SC, offsetof(SessScHead, n), &neg, 4));
    corrupt("SC prefix beyond n", true, in_section(SESS_SC, offsetof(SessScHead, book_prefix), &three, 4));
    corrupt("SC NaN max_radius", true, in_section(SESS_SC, offsetof(mlh_sc_opts, max_radius), &nan, 8));
    corrupt("PG count that disagrees with the length", true, in_section(SESS_PG, 0, &two, 4));
    corrupt("PG max_loops beyond the limit", true, in_section(SESS_PG, 8, &big, 4));
    corrupt("PG max_loops 0", true, in_section(SESS_PG, 8, &zero, 4));
    corrupt("PG loop index >= count", true, in_section(SESS_PG, sizeof(SessPgHead) + 2 * sizeof(SessPgRecord) + offsetof(SessPgRecord, loop_index), &three, 4));
    corrupt("PG loop index = own index", true, in_section(SESS_PG, sizeof(SessPgHead) + 2 * sizeof(SessPgRecord) + offsetof(SessPgRecord, loop_index), &two, 4));
    corrupt("PG loop index -2", true, in_section(SESS_PG, sizeof(SessPgHead) + offsetof(SessPgRecord, loop_index), &minus2, 4));
    corrupt("PG NaN pose", true, in_section(SESS_PG, sizeof(SessPgHead) + sizeof(SessPgRecord), &nan, 8));
    const unsigned char one = 1;
    corrupt("PG record padding not zero", true, in_section(SESS_PG, sizeof(SessPgHead) + offsetof(SessPgRecord, pad), &three, 4));
    corrupt("SC padding behind has_pos not zero", true, in_section(SESS_SC, size_t(sess_sc_layout(2, 3, 2).has_pos) + 5, &one, 1));
    corrupt("SC head padding not zero", true, in_section(SESS_SC, offsetof(SessScHead, pad) + 4, &three, 4));
    corrupt("PG earliest_loop without a loop at or before it", true, in_section(SESS_PG, 4, &two, 4));
    // one flipped payload bit per section, the checksum left as it was
    for (int k = 0; k < SESS_SLOTS; ++k)
        corrupt("a flipped payload bit", true, [&](SessHeader &H, std::vector<unsigned char> &c) { c[H.sec[k].offset + H.sec[k].bytes / 2] ^= 0x10; });
    std::printf("%d corruptions refused\n", n_corrupt);
    // absent sections: KEYFRAMES without POINTS is refused; an image of the PG section alone is accepted
    {
        const uint64_t bytes[SESS_SLOTS] = {0, 0, 0, H0.sec[SESS_PG].bytes}, count[SESS_SLOTS] = {0, 0, 0, H0.sec[SESS_PG].count};
        const bool present[SESS_SLOTS] = {false, false, false, true};
        SessHeader H;
        sess_lay_out(H, bytes, count, present);
        H.sec[SESS_PG].checksum = H0.sec[SESS_PG].checksum;
        sess_seal(H);
        std::vector<unsigned char> c(H.total_bytes);
        std::memcpy(c.data(), &H, sizeof(H));
        std::memcpy(c.data() + H.sec[SESS_PG].offset, img.data() + H0.sec[SESS_PG].offset, size_t(H0.sec[SESS_PG].bytes));
        EXPECT(check(c.data(), c.size()) == nullptr);
    }
    std::printf("session_host: %s\n", fails ? "FAILED" : "ok");
    return fails ? 1 : 0;
}
