// The session image (row f17; session.hip): the format of the byte image mlh_session_export writes of the keyframe store, the Scan Context store and the pose
// graph -- what PoseGraph::savePoseGraph / loadPoseGraph keep over a restart (mloam_loop/src/pose_graph.cpp:655-781) --, its checksum, and the validation an
// image passes on the host before a context is touched. Host arithmetic only, no HIP types: the library, the facade and a stand-alone program under sanitizers
// (tests/host/session_host_main.cpp) share it. The format is this project's own.
//
// Little-endian throughout. [SessHeader: 208 bytes][KEYFRAMES][POINTS][SC][PG]: the stored sections in this order, back to back, each starting and ending on a
// 16-byte boundary (padding: zero bytes, part of the section and of its checksum), the last one ending the image. An absent section has an all-zero table slot.
//   KEYFRAMES  one SessKey per keyframe: pose[7], cov[36], pos[3], n[3] (surf, corner, outlier), has_outlier
//   POINTS     every stored cloud as float4 {x, y, z, lidar} in CANONICAL order -- key 0 surf, key 0 corner, key 0 outlier, key 1 surf, ... --, whatever order the
//              store's arena got them in; the offsets are the prefix sums of n[] and are not stored. KEYFRAMES and POINTS are stored together.
//   SC         SessScHead (the options, n, ScBook's two words, the four statistics counters), then of entries 0..n-1 the descriptors (f32), ring keys (f32),
//              sector keys (f64) and column norms (f64) in the store's own layouts, the positions (3 f64 each) and has_pos (a byte each); every array padded to 16
//   PG         SessPgHead (count, earliest_loop, max_loops), then the 176-byte pose-graph records
// Not in the image: the local-map cache, the local and global map clouds, any scratch.
// Checksum of a section of u32 words w_0 .. w_{m-1}: sum_i (w_i XOR 0x9E3779B9) * (2 i + 1) mod 2^64 -- a sum of integers, so any order of reduction gives the
// same bits (the device's does); the odd factor catches swapped words. The header's own checksum covers the bytes before it.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include "sc_host.hpp"
#include "tile_group.hpp"

namespace mlh {

constexpr uint32_t SESS_MAGIC = 0x53484C4Du;        // "MLHS"
constexpr uint32_t SESS_VERSION = 1;
constexpr uint32_t SESS_REC_POINT = 16, SESS_REC_PG = 176;
constexpr uint32_t SESS_XOR = 0x9E3779B9u;
constexpr int SESS_PG_MIN_LOOPS = 128;              // pg_host.hpp: PG_MAX_LOOPS, the capacity of a context that never called mlh_pg_reserve
enum { SESS_KEYFRAMES = 0, SESS_POINTS = 1, SESS_SC = 2, SESS_PG = 3, SESS_SLOTS = 4 };

struct SessKey { double pose[7], cov[36]; float pos[3]; int32_t n[3]; int32_t has_outlier, pad; };
static_assert(sizeof(SessKey) == 376, "the per-key record: 43 doubles, 3 floats, 5 ints");
struct SessSection { uint32_t kind, reserved; uint64_t offset, bytes, count, checksum; };       // kind = slot + 1; all zero: absent
struct SessHeader {
    uint32_t magic, version, rec_point, rec_pg, rec_key, n_slots;
    uint64_t total_bytes, reserved;
    SessSection sec[SESS_SLOTS];
    uint64_t header_checksum;                       // of the 200 bytes before it
};
static_assert(sizeof(SessHeader) == 208 && offsetof(SessHeader, header_checksum) == 200, "the image's header");
struct SessScHead {
    mlh_sc_opts opts;
    int32_t n, book_counter, book_prefix, last_host_decided, last_skipped, pad[3];
    int64_t points_host_decided, points_skipped;
};
static_assert(sizeof(mlh_sc_opts) == 64 && sizeof(SessScHead) == 112, "the SC section's head");
struct SessPgHead { int32_t count, earliest_loop, max_loops, pad; };
struct SessPgRecord { double pose[7], last[7], loop_rel[7]; int32_t loop_index, pad; };       // ctx.hpp: PgKeyframe (session.hip asserts they agree)
static_assert(sizeof(SessPgRecord) == SESS_REC_PG, "the pose graph's record");

inline uint64_t sess_pad16(uint64_t v) { return (v + 15u) & ~uint64_t(15); }

// the scalar form of the checksum; bytes is a multiple of 4
inline uint64_t sess_checksum(const void *p, size_t bytes)
{
    const unsigned char *b = static_cast<const unsigned char *>(p);
    uint64_t sum = 0;
    for (size_t i = 0; i < bytes / 4; ++i) {
        uint32_t w;
        std::memcpy(&w, b + 4 * i, 4);
        sum += uint64_t(w ^ SESS_XOR) * (2 * uint64_t(i) + 1);
    }
    return sum;
}

// the arrays of the SC section behind its head: byte offsets within the section, and the section's length
struct SessScLayout { uint64_t desc, ring_key, sector_key, col_norm, pos, has_pos, bytes; };
inline SessScLayout sess_sc_layout(int R, int S, int n)
{
    const uint64_t r = uint64_t(R), s = uint64_t(S), e = uint64_t(n);
    SessScLayout L;
    L.desc = sizeof(SessScHead);
    L.ring_key = L.desc + sess_pad16(4 * r * s * e);
    L.sector_key = L.ring_key + sess_pad16(4 * r * e);
    L.col_norm = L.sector_key + sess_pad16(8 * s * e);
    L.pos = L.col_norm + sess_pad16(8 * s * e);
    L.has_pos = L.pos + sess_pad16(24 * e);
    L.bytes = L.has_pos + sess_pad16(e);
    return L;
}
inline uint64_t sess_keyframes_bytes(uint64_t n_keys) { return sess_pad16(sizeof(SessKey) * n_keys); }
inline uint64_t sess_pg_bytes(uint64_t count) { return sizeof(SessPgHead) + SESS_REC_PG * count; }

// The offsets of a header whose sections' bytes (0: absent) and counts are given: kinds, offsets, total_bytes and the record sizes filled in; the checksums are
// the caller's (sess_seal once they are known)
inline void sess_lay_out(SessHeader &H, const uint64_t bytes[SESS_SLOTS], const uint64_t count[SESS_SLOTS], const bool present[SESS_SLOTS])
{
    std::memset(&H, 0, sizeof(H));
    H.magic = SESS_MAGIC; H.version = SESS_VERSION; H.rec_point = SESS_REC_POINT; H.rec_pg = SESS_REC_PG; H.rec_key = uint32_t(sizeof(SessKey)); H.n_slots = SESS_SLOTS;
    uint64_t at = sizeof(SessHeader);
    for (int k = 0; k < SESS_SLOTS; ++k) {
        if (!present[k]) continue;
        H.sec[k].kind = uint32_t(k + 1); H.sec[k].offset = at; H.sec[k].bytes = bytes[k]; H.sec[k].count = count[k];
        at += bytes[k];
    }
    H.total_bytes = at;
}
inline void sess_seal(SessHeader &H) { H.header_checksum = sess_checksum(&H, offsetof(SessHeader, header_checksum)); }

// One 256-record tile of the pack: `count` 16-byte records from record `src` of arena `arena` to record `dst` of the image; arena < 0: the records are already
// in the image at `dst` and only their checksum terms are taken. `word0`: the index of the tile's first u32 word within its section.
struct SessTile { long long src; long long dst; unsigned long long word0; int count, arena, slot, pad; };
// the tiles of one cloud of n records at arena record `src`, going to image record `dst` of section `slot`, whose first record is image record `sec_first`
template <class Out> inline void sess_cloud_tiles(Out &tiles, long long src, long long dst, long long sec_first, int n, int arena, int slot)
{
    segment_tiles(n, [&](int at, int len) { tiles.push_back(SessTile{src + at, dst + at, 4ull * (unsigned long long)(dst + at - sec_first), len, arena, slot, 0}); });
}

inline bool sess_zero(const unsigned char *b, uint64_t from, uint64_t to) { for (uint64_t i = from; i < to; ++i) if (b[i]) return false; return true; }
inline bool sess_finite(const double *v, int n) { for (int i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false; return true; }

// The whole image held to the format before anything else looks at it: nullptr, or what is wrong with it. Reads nothing outside [image, image + bytes). The
// payload checksums are NOT taken here (mlh_session_import takes them on the device, sess_verify on the host). max_pg_loops: MLH_PG_LOOPS_LIMIT.
inline const char *sess_validate(const void *image, size_t bytes, SessHeader &H, int max_pg_loops = MLH_PG_LOOPS_LIMIT)
{
    const unsigned char *b = static_cast<const unsigned char *>(image);
    if (!image || bytes < sizeof(SessHeader)) return "shorter than a header";
    std::memcpy(&H, b, sizeof(H));
    if (H.magic != SESS_MAGIC) return "bad magic";
    if (H.version != SESS_VERSION) return "unknown format version";
    if (H.rec_point != SESS_REC_POINT || H.rec_pg != SESS_REC_PG || H.rec_key != sizeof(SessKey) || H.n_slots != SESS_SLOTS) return "written with other record sizes";
    if (H.reserved != 0) return "reserved header word set";
    if (H.header_checksum != sess_checksum(&H, offsetof(SessHeader, header_checksum))) return "header checksum mismatch";
    if (H.total_bytes != uint64_t(bytes)) return "length differs from the header's (truncated?)";
    uint64_t at = sizeof(SessHeader);
    for (int k = 0; k < SESS_SLOTS; ++k) {
        const SessSection &s = H.sec[k];
        if (s.kind == 0) {
            if (s.reserved || s.offset || s.bytes || s.count || s.checksum) return "absent section with fields set";
            continue;
        }
        if (s.kind != uint32_t(k + 1) || s.reserved != 0) return "section of the wrong kind";
        if (s.offset != at) return "section out of place (overlap or gap)";
        if (s.bytes % 16 != 0 || s.bytes > uint64_t(bytes) - at) return "section out of bounds";
        at += s.bytes;
    }
    if (at != uint64_t(bytes)) return "bytes behind the last section";
    if ((H.sec[SESS_KEYFRAMES].kind != 0) != (H.sec[SESS_POINTS].kind != 0)) return "KEYFRAMES and POINTS go together";
    if (H.sec[SESS_KEYFRAMES].kind) {
        const SessSection &ks = H.sec[SESS_KEYFRAMES], &ps = H.sec[SESS_POINTS];
        if (ks.count > uint64_t(INT32_MAX) || ks.bytes != sess_keyframes_bytes(ks.count)) return "KEYFRAMES: count disagrees with length";
        if (ps.count >= uint64_t(INT32_MAX) || ps.bytes != SESS_REC_POINT * ps.count) return "POINTS: count disagrees with length";
        uint64_t total = 0;
        for (uint64_t i = 0; i < ks.count; ++i) {
            SessKey k;
            std::memcpy(&k, b + ks.offset + sizeof(SessKey) * i, sizeof(k));
            if (!sess_finite(k.pose, 7) || !sess_finite(k.cov, 36)) return "KEYFRAMES: non-finite pose";
            if (!std::isfinite(k.pos[0]) || !std::isfinite(k.pos[1]) || !std::isfinite(k.pos[2])) return "KEYFRAMES: non-finite position";
            if (k.n[0] < 0 || k.n[1] < 0 || k.n[2] < 0) return "KEYFRAMES: negative n[]";
            if ((k.has_outlier != 0 && k.has_outlier != 1) || (!k.has_outlier && k.n[2] != 0) || k.pad != 0) return "KEYFRAMES: bad outlier flag";
            total += uint64_t(k.n[0]) + uint64_t(k.n[1]) + uint64_t(k.n[2]);
        }
        if (total != ps.count) return "KEYFRAMES: n[] disagrees with POINTS' length";
        if (!sess_zero(b, ks.offset + sizeof(SessKey) * ks.count, ks.offset + ks.bytes)) return "KEYFRAMES: padding not zero";
    }
    if (H.sec[SESS_SC].kind) {
        const SessSection &s = H.sec[SESS_SC];
        if (s.bytes < sizeof(SessScHead)) return "SC: shorter than its head";
        SessScHead h;
        std::memcpy(&h, b + s.offset, sizeof(h));
        if (const char *f = sc_opts_fault(h.opts)) { (void)f; return "SC: bad options"; }
        if (h.n < 0 || uint64_t(h.n) != s.count) return "SC: count disagrees with the head's";
        if (s.bytes != sess_sc_layout(h.opts.num_ring, h.opts.num_sector, h.n).bytes) return "SC: count disagrees with length";
        if (h.book_counter < 0 || h.book_prefix < 0 || h.book_prefix > h.n || h.last_host_decided < 0 || h.last_skipped < 0 || h.points_host_decided < 0 ||
            h.points_skipped < 0 || h.pad[0] || h.pad[1] || h.pad[2]) return "SC: bad bookkeeping";
        const SessScLayout L = sess_sc_layout(h.opts.num_ring, h.opts.num_sector, h.n);
        for (int i = 0; i < h.n; ++i) {
            double p[3];
            std::memcpy(p, b + s.offset + L.pos + 24 * uint64_t(i), sizeof(p));
            if (!sess_finite(p, 3) || b[s.offset + L.has_pos + uint64_t(i)] > 1) return "SC: bad position";
        }
        // every array ends where its data does; the rest up to the next array is padding
        const uint64_t r = uint64_t(h.opts.num_ring), c = uint64_t(h.opts.num_sector), e = uint64_t(h.n);
        const uint64_t end[6] = {L.desc + 4 * r * c * e, L.ring_key + 4 * r * e, L.sector_key + 8 * c * e, L.col_norm + 8 * c * e, L.pos + 24 * e, L.has_pos + e};
        const uint64_t next[6] = {L.ring_key, L.sector_key, L.col_norm, L.pos, L.has_pos, L.bytes};
        for (int a = 0; a < 6; ++a) if (!sess_zero(b, s.offset + end[a], s.offset + next[a])) return "SC: padding not zero";
    }
    if (H.sec[SESS_PG].kind) {
        const SessSection &s = H.sec[SESS_PG];
        if (s.bytes < sizeof(SessPgHead)) return "PG: shorter than its head";
        SessPgHead h;
        std::memcpy(&h, b + s.offset, sizeof(h));
        if (h.count < 0 || uint64_t(h.count) != s.count || s.bytes != sess_pg_bytes(s.count)) return "PG: count disagrees with length";
        if (h.max_loops < SESS_PG_MIN_LOOPS || h.max_loops > max_pg_loops || h.pad != 0) return "PG: max_loops out of range";
        int earliest = -1;
        for (int i = 0; i < h.count; ++i) {
            SessPgRecord r;
            std::memcpy(&r, b + s.offset + sizeof(SessPgHead) + sizeof(r) * uint64_t(i), sizeof(r));
            if (!sess_finite(r.pose, 7) || !sess_finite(r.last, 7) || !sess_finite(r.loop_rel, 7)) return "PG: non-finite pose";
            if (r.loop_index < -1 || r.loop_index >= i) return "PG: loop index out of range";
            if (r.pad != 0) return "PG: padding not zero";
            if (r.loop_index >= 0 && (earliest < 0 || r.loop_index < earliest)) earliest = r.loop_index;
        }
        if (earliest < 0 ? h.earliest_loop != -1 : (h.earliest_loop < 0 || h.earliest_loop > earliest)) return "PG: earliest_loop disagrees with the loop indices";
    }
    return nullptr;
}

// the payload checksums on the host (mlh_session_inspect; a caller without a device): nullptr, or the section at fault. The image has passed sess_validate.
inline const char *sess_verify(const void *image, const SessHeader &H)
{
    static const char *const name[SESS_SLOTS] = {"KEYFRAMES: checksum mismatch", "POINTS: checksum mismatch", "SC: checksum mismatch", "PG: checksum mismatch"};
    for (int k = 0; k < SESS_SLOTS; ++k)
        if (H.sec[k].kind && sess_checksum(static_cast<const unsigned char *>(image) + H.sec[k].offset, size_t(H.sec[k].bytes)) != H.sec[k].checksum) return name[k];
    return nullptr;
}

}  // namespace mlh
