// The session image on gfx950 (row f17): the keyframe store, the Scan Context store and the pose graph out of a context and back into one -- what
// PoseGraph::savePoseGraph / loadPoseGraph keep over a restart (mloam_loop/src/pose_graph.cpp:655-781, 225-279, 77-90). session_host.hpp states the format, its
// checksum and the validation; include/mloam_hip.h (f17) what is reproduced, chosen and departed from.
//   session_pack_kernel   one workgroup per 256-record tile (a tile never straddles a stored cloud: tile_group.hpp's cutting, as cloudbuild.hip's). A thread moves
//                         one 16-byte record -- one 16-byte load, one 16-byte store, coalesced -- from the store's arena to its canonical place in the staging
//                         image, or reads it where it already lies there (the SC and PG sections; every section of an import), and adds its four checksum terms;
//                         the workgroup's sum (wg_dev.hpp: block_sum: shuffles, then LDS) goes to the section's word by ONE 64-bit integer atomic add. An integer
//                         sum is the same bits in any order: no float atomics.
// Export: tables, device-to-device copies of the contiguous sections, ONE pack launch, one copy out, ONE host wait. Import: validation on the host, upload into
// the staging image, ONE pack launch (checksums only), copies into NEW buffers, ONE host wait, then -- only if every checksum matches -- the swap.
#include "ctx.hpp"
#include "wg_dev.hpp"
#include "session_host.hpp"
#include "pg_host.hpp"
#include <algorithm>

namespace mlh {

static_assert(sizeof(PgKeyframe) == sizeof(SessPgRecord) && offsetof(PgKeyframe, loop_index) == offsetof(SessPgRecord, loop_index) &&
              offsetof(PgKeyframe, loop_rel) == offsetof(SessPgRecord, loop_rel), "the image's pose-graph record is the store's");
static_assert(SESS_PG_MIN_LOOPS == PG_MAX_LOOPS, "a context's capacity of loop edges before mlh_pg_reserve");

__global__ __launch_bounds__(256) void session_pack_kernel(const SessTile *tiles, const uint4 *arena, uint4 *image, unsigned long long *sums)
{
    __shared__ unsigned long long s_sum[4];
    const SessTile t = tiles[blockIdx.x];
    unsigned long long acc = 0ull;
    if (int(threadIdx.x) < t.count) {
        uint4 v;
        if (t.arena >= 0) { v = arena[t.src + threadIdx.x]; image[t.dst + threadIdx.x] = v; }
        else v = image[t.dst + threadIdx.x];
        const unsigned long long f = 2ull * (t.word0 + 4ull * threadIdx.x) + 1ull;
        acc = (unsigned long long)(v.x ^ SESS_XOR) * f + (unsigned long long)(v.y ^ SESS_XOR) * (f + 2ull) + (unsigned long long)(v.z ^ SESS_XOR) * (f + 4ull) +
              (unsigned long long)(v.w ^ SESS_XOR) * (f + 6ull);
    }
    const unsigned long long sum = block_sum<4>(acc, s_sum);
    if (threadIdx.x == 0) atomicAdd(&sums[t.slot], sum);
}

namespace {

constexpr uint32_t SESS_ALL = MLH_SESSION_KEYFRAMES | MLH_SESSION_SC | MLH_SESSION_PG;

// the staging image, the tile table and the host block of a call are the call's: a context does not keep an image-sized buffer between calls
struct SessScratch {
    SessStore &X;
    ~SessScratch() { X.stage.release(); X.tab.release(); std::vector<unsigned char>().swap(X.himg); }
};

// the header (offsets, counts, no checksums yet) of an export of `sections` as the context stands
int sess_header_of(mlh_ctx *ctx, const char *entry, uint32_t sections, SessHeader &H)
{
    if (sections == 0 || (sections & ~SESS_ALL)) return fail(ctx, MLH_ERR_INVALID, (std::string(entry) + ": sections is an OR of MLH_SESSION_*").c_str());
    if ((sections & MLH_SESSION_SC) && !ctx->sc.configured) return fail(ctx, MLH_ERR_STATE, (std::string(entry) + ": mlh_sc_reset has not been called").c_str());
    uint64_t bytes[SESS_SLOTS] = {0, 0, 0, 0}, count[SESS_SLOTS] = {0, 0, 0, 0};
    bool present[SESS_SLOTS] = {false, false, false, false};
    if (sections & MLH_SESSION_KEYFRAMES) {
        const KfStore &K = ctx->kf;
        uint64_t pts = 0;
        for (const KfStore::Key &k : K.keys) pts += uint64_t(k.n[0]) + uint64_t(k.n[1]) + uint64_t(k.n[2]);
        present[SESS_KEYFRAMES] = present[SESS_POINTS] = true;
        count[SESS_KEYFRAMES] = K.keys.size(); bytes[SESS_KEYFRAMES] = sess_keyframes_bytes(K.keys.size());
        if (pts >= uint64_t(INT32_MAX)) return fail(ctx, MLH_ERR_UNSUPPORTED, (std::string(entry) + ": 2^31 or more stored points (no import would take the image)").c_str());
        count[SESS_POINTS] = pts; bytes[SESS_POINTS] = SESS_REC_POINT * pts;
    }
    if (sections & MLH_SESSION_SC) {
        const ScStore &S = ctx->sc;
        present[SESS_SC] = true; count[SESS_SC] = uint64_t(S.n); bytes[SESS_SC] = sess_sc_layout(S.opts.num_ring, S.opts.num_sector, S.n).bytes;
    }
    if (sections & MLH_SESSION_PG) {
        present[SESS_PG] = true; count[SESS_PG] = uint64_t(ctx->pg.count); bytes[SESS_PG] = sess_pg_bytes(uint64_t(ctx->pg.count));
    }
    sess_lay_out(H, bytes, count, present);
    return MLH_OK;
}

void sess_info_of(const SessHeader &H, uint32_t sections, int launches, int host_waits, mlh_session_info &I)
{
    std::memset(&I, 0, sizeof(I));
    I.version = H.version; I.sections = sections; I.launches = launches; I.host_waits = host_waits; I.total_bytes = int64_t(H.total_bytes);
    for (int k = 0; k < SESS_SLOTS; ++k) { I.count[k] = int64_t(H.sec[k].count); I.bytes[k] = int64_t(H.sec[k].bytes); I.checksum[k] = H.sec[k].checksum; }
}

uint32_t sess_sections_of(const SessHeader &H)
{
    return (H.sec[SESS_KEYFRAMES].kind ? MLH_SESSION_KEYFRAMES : 0u) | (H.sec[SESS_SC].kind ? MLH_SESSION_SC : 0u) | (H.sec[SESS_PG].kind ? MLH_SESSION_PG : 0u);
}

// in-place tiles (checksum only) over a whole section of the staging image
int sess_section_tiles(mlh_ctx *ctx, std::vector<SessTile> &tiles, const SessSection &s, int slot)
{
    const uint64_t recs = s.bytes / 16;
    if (recs > uint64_t(INT32_MAX)) return fail(ctx, MLH_ERR_UNSUPPORTED, "session image: a section of more than 2^31 16-byte records");
    sess_cloud_tiles(tiles, 0, (long long)(s.offset / 16), (long long)(s.offset / 16), int(recs), -1, slot);
    return MLH_OK;
}

// the tile table up, the checksum words cleared, the ONE pack launch, the words on their way to pinned memory
int sess_pack_launch(mlh_ctx *ctx, const std::vector<SessTile> &tiles, const float4 *arena)
{
    SessStore &X = ctx->sess;
    hipStream_t st = ctx->stream;
    MLH_HIP(ctx, X.sums.ensure(sizeof(unsigned long long) * SESS_SLOTS));
    MLH_HIP(ctx, X.h_pin.ensure(sizeof(SessHeader) + 64));
    MLH_HIP(ctx, hipMemsetAsync(X.sums.p, 0, sizeof(unsigned long long) * SESS_SLOTS, st));
    if (!tiles.empty()) {
        MLH_HIP(ctx, X.tab.ensure(sizeof(SessTile) * tiles.size()));
        MLH_HIP(ctx, hipMemcpyAsync(X.tab.p, tiles.data(), sizeof(SessTile) * tiles.size(), hipMemcpyHostToDevice, st));
        MLH_LAUNCH(session_pack_kernel, dim3(unsigned(tiles.size())), dim3(256), 0, st, (const SessTile *)X.tab.as<SessTile>(), reinterpret_cast<const uint4 *>(arena),
                   X.stage.as<uint4>(), X.sums.as<unsigned long long>());
        MLH_HIP(ctx, hipGetLastError());
    }
    MLH_HIP(ctx, hipMemcpyAsync(X.h_pin.p, X.sums.p, sizeof(unsigned long long) * SESS_SLOTS, hipMemcpyDeviceToHost, st));
    return MLH_OK;
}

int session_export_run(mlh_ctx *ctx, uint32_t sections, void *dst, size_t capacity, int mem, size_t *written)
{
    SessHeader H;
    { const int rc = sess_header_of(ctx, "mlh_session_export", sections, H); if (rc) return rc; }
    if (written) *written = size_t(H.total_bytes);
    if (!dst || capacity < H.total_bytes) return fail(ctx, MLH_ERR_INVALID, "mlh_session_export: capacity is smaller than the image (*written has its length)");
    if (mem != MLH_MEM_HOST && mem != MLH_MEM_DEVICE) return fail(ctx, MLH_ERR_INVALID, "mlh_session_export: mem is MLH_MEM_HOST or MLH_MEM_DEVICE");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    SessStore &X = ctx->sess;
    SessScratch scratch{X};
    hipStream_t st = ctx->stream;
    MLH_HIP(ctx, X.stage.ensure(size_t(H.total_bytes)));
    unsigned char *img = X.stage.as<unsigned char>();
    // what the host holds of the image: the KEYFRAMES records, the SC head, positions and flags, the PG head -- built in one block, uploaded section by section;
    // the padding of every section is zeroed with it
    std::vector<unsigned char> &h = X.himg;
    std::vector<SessTile> tiles;
    if (sections & MLH_SESSION_KEYFRAMES) {
        const KfStore &K = ctx->kf;
        const SessSection &ks = H.sec[SESS_KEYFRAMES], &ps = H.sec[SESS_POINTS];
        h.assign(size_t(ks.bytes), 0);
        long long at = (long long)(ps.offset / 16);
        for (size_t i = 0; i < K.keys.size(); ++i) {
            const KfStore::Key &k = K.keys[i];
            SessKey r;
            std::memset(&r, 0, sizeof(r));
            std::memcpy(r.pose, k.pose, sizeof(r.pose)); std::memcpy(r.cov, k.cov, sizeof(r.cov)); std::memcpy(r.pos, k.pos, sizeof(r.pos));
            for (int c = 0; c < 3; ++c) {
                r.n[c] = k.n[c];
                sess_cloud_tiles(tiles, (long long)k.off[c], at, (long long)(ps.offset / 16), k.n[c], 0, SESS_POINTS);
                at += k.n[c];
            }
            r.has_outlier = k.has_outlier ? 1 : 0;
            std::memcpy(h.data() + sizeof(SessKey) * i, &r, sizeof(r));
        }
        if (ks.bytes) MLH_HIP(ctx, hipMemcpyAsync(img + ks.offset, h.data(), size_t(ks.bytes), hipMemcpyHostToDevice, st));
        { const int rc = sess_section_tiles(ctx, tiles, ks, SESS_KEYFRAMES); if (rc) return rc; }
    }
    std::vector<unsigned char> hsc;
    if (sections & MLH_SESSION_SC) {
        const ScStore &S = ctx->sc;
        const SessSection &s = H.sec[SESS_SC];
        const int R = S.opts.num_ring, C = S.opts.num_sector;
        const SessScLayout L = sess_sc_layout(R, C, S.n);
        const size_t n = size_t(S.n);
        MLH_HIP(ctx, hipMemsetAsync(img + s.offset, 0, size_t(s.bytes), st));
        SessScHead head;
        std::memset(&head, 0, sizeof(head));
        head.opts = S.opts; head.n = S.n; head.book_counter = S.book.counter; head.book_prefix = S.book.prefix;
        head.last_host_decided = S.last_host_decided; head.last_skipped = S.last_skipped;
        head.points_host_decided = S.points_host_decided; head.points_skipped = S.points_skipped;
        hsc.assign(sizeof(head) + size_t(L.bytes - L.pos), 0);
        std::memcpy(hsc.data(), &head, sizeof(head));
        if (n) {
            std::memcpy(hsc.data() + sizeof(head), S.pos.data(), 24 * n);
            std::memcpy(hsc.data() + sizeof(head) + size_t(L.has_pos - L.pos), S.has_pos.data(), n);
        }
        MLH_HIP(ctx, hipMemcpyAsync(img + s.offset, hsc.data(), sizeof(head), hipMemcpyHostToDevice, st));
        if (n) {
            MLH_HIP(ctx, hipMemcpyAsync(img + s.offset + L.pos, hsc.data() + sizeof(head), size_t(L.bytes - L.pos), hipMemcpyHostToDevice, st));
            MLH_HIP(ctx, hipMemcpyAsync(img + s.offset + L.desc, S.desc.p, sizeof(float) * size_t(R) * C * n, hipMemcpyDeviceToDevice, st));
            MLH_HIP(ctx, hipMemcpyAsync(img + s.offset + L.ring_key, S.ring_key.p, sizeof(float) * size_t(R) * n, hipMemcpyDeviceToDevice, st));
            MLH_HIP(ctx, hipMemcpyAsync(img + s.offset + L.sector_key, S.sector_key.p, sizeof(double) * size_t(C) * n, hipMemcpyDeviceToDevice, st));
            MLH_HIP(ctx, hipMemcpyAsync(img + s.offset + L.col_norm, S.col_norm.p, sizeof(double) * size_t(C) * n, hipMemcpyDeviceToDevice, st));
        }
        { const int rc = sess_section_tiles(ctx, tiles, s, SESS_SC); if (rc) return rc; }
    }
    SessPgHead pg_head = {0, 0, 0, 0};
    if (sections & MLH_SESSION_PG) {
        const PgStore &G = ctx->pg;
        const SessSection &s = H.sec[SESS_PG];
        pg_head.count = G.count; pg_head.earliest_loop = G.earliest_loop; pg_head.max_loops = G.max_loops;
        MLH_HIP(ctx, hipMemcpyAsync(img + s.offset, &pg_head, sizeof(pg_head), hipMemcpyHostToDevice, st));
        if (G.count) MLH_HIP(ctx, hipMemcpyAsync(img + s.offset + sizeof(pg_head), G.kf.p, sizeof(PgKeyframe) * size_t(G.count), hipMemcpyDeviceToDevice, st));
        { const int rc = sess_section_tiles(ctx, tiles, s, SESS_PG); if (rc) return rc; }
    }
    { const int rc = sess_pack_launch(ctx, tiles, ctx->kf.pts.as<float4>()); if (rc) return rc; }
    unsigned char *out = static_cast<unsigned char *>(dst);
    const size_t body = size_t(H.total_bytes) - sizeof(SessHeader);
    if (body) MLH_HIP(ctx, hipMemcpyAsync(out + sizeof(SessHeader), img + sizeof(SessHeader), body, mem == MLH_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    MLH_HIP(ctx, stream_wait_spin(ctx));
    int waits = 1;
    { const int rc = device_error_check(ctx); if (rc) return rc; }
    // the header last, from the read-back checksums
    const unsigned long long *sums = X.h_pin.as<unsigned long long>();
    for (int k = 0; k < SESS_SLOTS; ++k) if (H.sec[k].kind) H.sec[k].checksum = sums[k];
    sess_seal(H);
    if (mem == MLH_MEM_HOST) {
        std::memcpy(out, &H, sizeof(H));
        // what an import would refuse is refused now, not at restore time (a pose graph whose optimisation left a non-finite pose, say)
        SessHeader again;
        if (const char *why = sess_validate(out, size_t(H.total_bytes), again))
            return fail(ctx, MLH_ERR_STATE, (std::string("mlh_session_export: the stores hold what no import would take: ") + why).c_str());
    } else {
        std::memcpy(X.h_pin.as<unsigned char>() + 64, &H, sizeof(H));
        MLH_HIP(ctx, hipMemcpyAsync(out, X.h_pin.as<unsigned char>() + 64, sizeof(H), hipMemcpyHostToDevice, st));
        MLH_HIP(ctx, stream_wait_spin(ctx));
        ++waits;
    }
    sess_info_of(H, sections, (tiles.empty() ? 0 : 1) + waits, waits, X.last);
    return MLH_OK;
}

void swap_buf(DevBuf &a, DevBuf &b) { std::swap(a.p, b.p); std::swap(a.cap, b.cap); }

int session_import_run(mlh_ctx *ctx, const void *image, size_t bytes, uint32_t sections, mlh_session_info *out)
{
    SessHeader H;
    if (const char *why = sess_validate(image, bytes, H)) return fail(ctx, MLH_ERR_INVALID, (std::string("mlh_session_import: ") + why).c_str());
    if (sections == 0 || (sections & ~SESS_ALL)) return fail(ctx, MLH_ERR_INVALID, "mlh_session_import: sections is an OR of MLH_SESSION_*");
    if (sections & ~sess_sections_of(H)) return fail(ctx, MLH_ERR_INVALID, "mlh_session_import: the image lacks a requested section");
    MLH_HIP(ctx, hipSetDevice(ctx->device));
    SessStore &X = ctx->sess;
    SessScratch scratch{X};
    hipStream_t st = ctx->stream;
    const unsigned char *b = static_cast<const unsigned char *>(image);
    bool want[SESS_SLOTS];
    want[SESS_KEYFRAMES] = want[SESS_POINTS] = (sections & MLH_SESSION_KEYFRAMES) != 0;
    want[SESS_SC] = (sections & MLH_SESSION_SC) != 0; want[SESS_PG] = (sections & MLH_SESSION_PG) != 0;
    // the requested sections into the staging image at the image's own offsets, their checksums taken there
    MLH_HIP(ctx, X.stage.ensure(size_t(H.total_bytes)));
    unsigned char *img = X.stage.as<unsigned char>();
    std::vector<SessTile> tiles;
    for (int k = 0; k < SESS_SLOTS; ++k) {
        if (!want[k] || H.sec[k].bytes == 0) continue;
        MLH_HIP(ctx, hipMemcpyAsync(img + H.sec[k].offset, b + H.sec[k].offset, size_t(H.sec[k].bytes), hipMemcpyHostToDevice, st));
        const int rc = sess_section_tiles(ctx, tiles, H.sec[k], k);
        if (rc) return rc;
    }
    { const int rc = sess_pack_launch(ctx, tiles, nullptr); if (rc) return rc; }
    // ... and from there into NEW buffers, which become the stores' only if the checksums match
    DevBuf pts, desc, ring_key, sector_key, col_norm, pgkf;
    SessScHead sh;
    SessScLayout L = {};
    SessPgHead ph = {0, -1, 0, 0};
    if (want[SESS_KEYFRAMES]) {
        const SessSection &ps = H.sec[SESS_POINTS];
        MLH_HIP(ctx, pts.ensure(sizeof(float4) * (size_t(ps.count) + 1)));
        if (ps.bytes) MLH_HIP(ctx, hipMemcpyAsync(pts.p, img + ps.offset, size_t(ps.bytes), hipMemcpyDeviceToDevice, st));
    }
    if (want[SESS_SC]) {
        const SessSection &s = H.sec[SESS_SC];
        std::memcpy(&sh, b + s.offset, sizeof(sh));
        const size_t R = size_t(sh.opts.num_ring), C = size_t(sh.opts.num_sector), n = size_t(sh.n);
        L = sess_sc_layout(sh.opts.num_ring, sh.opts.num_sector, sh.n);
        if (n) {
            MLH_HIP(ctx, desc.ensure(sizeof(float) * R * C * n)); MLH_HIP(ctx, ring_key.ensure(sizeof(float) * R * n));
            MLH_HIP(ctx, sector_key.ensure(sizeof(double) * C * n)); MLH_HIP(ctx, col_norm.ensure(sizeof(double) * C * n));
            MLH_HIP(ctx, hipMemcpyAsync(desc.p, img + s.offset + L.desc, sizeof(float) * R * C * n, hipMemcpyDeviceToDevice, st));
            MLH_HIP(ctx, hipMemcpyAsync(ring_key.p, img + s.offset + L.ring_key, sizeof(float) * R * n, hipMemcpyDeviceToDevice, st));
            MLH_HIP(ctx, hipMemcpyAsync(sector_key.p, img + s.offset + L.sector_key, sizeof(double) * C * n, hipMemcpyDeviceToDevice, st));
            MLH_HIP(ctx, hipMemcpyAsync(col_norm.p, img + s.offset + L.col_norm, sizeof(double) * C * n, hipMemcpyDeviceToDevice, st));
        }
    }
    if (want[SESS_PG]) {
        const SessSection &s = H.sec[SESS_PG];
        std::memcpy(&ph, b + s.offset, sizeof(ph));
        if (ph.count) {
            MLH_HIP(ctx, pgkf.ensure(sizeof(PgKeyframe) * size_t(ph.count)));
            MLH_HIP(ctx, hipMemcpyAsync(pgkf.p, img + s.offset + sizeof(ph), sizeof(PgKeyframe) * size_t(ph.count), hipMemcpyDeviceToDevice, st));
        }
    }
    MLH_HIP(ctx, stream_wait_spin(ctx));
    { const int rc = device_error_check(ctx); if (rc) return rc; }
    const unsigned long long *sums = X.h_pin.as<unsigned long long>();
    static const char *const name[SESS_SLOTS] = {"KEYFRAMES", "POINTS", "SC", "PG"};
    for (int k = 0; k < SESS_SLOTS; ++k)
        if (want[k] && sums[k] != H.sec[k].checksum)
            return fail(ctx, MLH_ERR_INVALID, (std::string("mlh_session_import: ") + name[k] + ": checksum mismatch (the context is unchanged)").c_str());
    // the swap: the stream is idle, nothing enqueued reads the old buffers. What could still refuse comes first.
    if (want[SESS_PG] && ph.max_loops > ctx->pg.max_loops) { const int rc = mlh_pg_reserve(ctx, ph.max_loops); if (rc) return rc; }
    if (want[SESS_KEYFRAMES]) {
        KfStore &K = ctx->kf;
        keyframes_release(ctx);                              // as mlh_keyframes_reset: cache, slots, local and global map clouds emptied
        swap_buf(K.pts, pts);
        const SessSection &ks = H.sec[SESS_KEYFRAMES];
        K.keys.resize(size_t(ks.count));
        size_t at = 0;
        for (size_t i = 0; i < K.keys.size(); ++i) {
            SessKey r;
            std::memcpy(&r, b + ks.offset + sizeof(SessKey) * i, sizeof(r));
            KfStore::Key &k = K.keys[i];
            std::memcpy(k.pose, r.pose, sizeof(k.pose)); std::memcpy(k.cov, r.cov, sizeof(k.cov)); std::memcpy(k.pos, r.pos, sizeof(k.pos));
            for (int c = 0; c < 3; ++c) { k.off[c] = at; k.n[c] = r.n[c]; at += size_t(r.n[c]); }
            k.has_outlier = r.has_outlier != 0;
        }
        K.pts_used = at;
    }
    if (want[SESS_SC]) {
        ScStore &S = ctx->sc;
        const SessSection &s = H.sec[SESS_SC];
        const size_t n = size_t(sh.n);
        S.unc.release(); S.counters.release(); S.keys.release(); S.work.release(); S.unc_entry.release(); S.batch_tab.release();
        S.desc.release(); S.ring_key.release(); S.sector_key.release(); S.col_norm.release();
        swap_buf(S.desc, desc); swap_buf(S.ring_key, ring_key); swap_buf(S.sector_key, sector_key); swap_buf(S.col_norm, col_norm);
        S.opts = sh.opts; S.configured = true; S.n = sh.n; S.cap = sh.n;
        S.pos.resize(3 * n); S.has_pos.resize(n);
        if (n) { std::memcpy(S.pos.data(), b + s.offset + L.pos, 24 * n); std::memcpy(S.has_pos.data(), b + s.offset + L.has_pos, n); }
        S.book.counter = sh.book_counter; S.book.prefix = sh.book_prefix;
        S.last_host_decided = sh.last_host_decided; S.last_skipped = sh.last_skipped;
        S.points_host_decided = sh.points_host_decided; S.points_skipped = sh.points_skipped;
        S.batch = ScBatchStats();
    }
    if (want[SESS_PG]) {
        PgStore &G = ctx->pg;
        const SessSection &s = H.sec[SESS_PG];
        G.kf.release();
        swap_buf(G.kf, pgkf);
        ++G.allocations;
        G.count = ph.count; G.earliest_loop = ph.earliest_loop;
        G.invalidate_marginals();
        G.loop_index.resize(size_t(ph.count));
        for (int i = 0; i < ph.count; ++i) {
            SessPgRecord r;
            std::memcpy(&r, b + s.offset + sizeof(ph) + sizeof(r) * size_t(i), sizeof(r));
            G.loop_index[size_t(i)] = r.loop_index;
        }
    }
    sess_info_of(H, sections, (tiles.empty() ? 0 : 1) + 1, 1, X.last);
    for (int k = 0; k < SESS_SLOTS; ++k) if (!want[k]) { X.last.count[k] = X.last.bytes[k] = 0; X.last.checksum[k] = 0; }
    if (out) *out = X.last;
    return MLH_OK;
}

}  // namespace

}  // namespace mlh

using namespace mlh;

extern "C" {

int mlh_session_export_size(mlh_ctx *ctx, uint32_t sections, size_t *bytes)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!bytes) return fail(ctx, MLH_ERR_INVALID, "mlh_session_export_size: null output");
    SessHeader H;
    { const int rc = sess_header_of(ctx, "mlh_session_export_size", sections, H); if (rc) return rc; }
    *bytes = size_t(H.total_bytes);
    return MLH_OK;
}

int mlh_session_export(mlh_ctx *ctx, uint32_t sections, void *dst, size_t capacity, int mem, size_t *written)
{
    if (!ctx) return MLH_ERR_INVALID;
    return session_export_run(ctx, sections, dst, capacity, mem, written);
}

int mlh_session_inspect(const void *image, size_t bytes, mlh_session_info *out)
{
    SessHeader H;
    if (!out || sess_validate(image, bytes, H) || sess_verify(image, H)) return MLH_ERR_INVALID;
    sess_info_of(H, sess_sections_of(H), 0, 0, *out);
    return MLH_OK;
}

int mlh_session_import(mlh_ctx *ctx, const void *image, size_t bytes, uint32_t sections, mlh_session_info *out)
{
    if (!ctx) return MLH_ERR_INVALID;
    return session_import_run(ctx, image, bytes, sections, out);
}

int mlh_session_last_info(mlh_ctx *ctx, mlh_session_info *out)
{
    if (!ctx) return MLH_ERR_INVALID;
    if (!out) return fail(ctx, MLH_ERR_INVALID, "mlh_session_last_info: null output");
    *out = ctx->sess.last;
    return MLH_OK;
}

}  // extern "C"
