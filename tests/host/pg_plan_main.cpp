// TEST INFRASTRUCTURE ONLY. The launch plan of the pose-graph optimisation's blocked dense stage (m-loam_amd/csrc/pg_host.hpp: pg_dense_step, pg_dense_sum_tile,
// pg_dense_launches -- the functions the host side of posegraph.hip enqueues from) in a stand-alone program, so that tests/test_pg_many_cases.py can build it with
// -fsanitize=address,undefined and run it directly. It replays the plan for every m = 6 L, L = first .. last (default 129 .. the limit), with, per launch and per
// workgroup, the memory that workgroup READS and WRITES as the kernels of posegraph.hip do (the model is written out in `replay` below; keep it in step with the kernels):
//   C(k, i)   tile (k, i) of the transposed factor P.C            D(k)    the factored diagonal tile k in P.Dg
//   W(t)      the 64 entries of the backward substitution's w (P.zw) of row tile t          Z(t)   those of the solution (P.z)
//   pg_csum_kernel     workgroup of tile (k, i): writes C(k, i) (reads the Gram partials, which no launch of the stage writes)
//   pg_cupdate_kernel  k, workgroup i: reads C(j, k) and C(j, i) for every j < k; reads and writes C(k, i)
//   pg_cpanel_kernel   k, workgroup i: reads C(k, k); i == k: writes D(k); i > k: reads and writes C(k, i)
//   pg_cback_kernel    k, workgroup jt: reads D(k) and w of panel k -- W(k), or in the first of these launches (k = T - 1) the bordering row where the panel solves
//                      left it: column m of tile row k, that is D(k) when m lies inside the last diagonal tile and C(k, m / 64) otherwise; jt == k: writes Z(k);
//                      jt < k: reads C(jt, k) and its own w (W(jt), or C(jt, m / 64) in the first launch), writes W(jt)
// Checked: the plan is the left-looking blocked Cholesky of the bordered matrix and the blocked backward substitution --
//   every tile (k, i), k < T, k <= i < Tb (the lower triangle and the bordering row) is summed once, updated once when k > 0 and then factored (i == k, into D(k)) or
//     solved (i > k) once; every row tile of the backward substitution is solved once, after it has been updated once by each later panel;
//   everything a workgroup reads was last written by an EARLIER launch, or by that workgroup itself, and is final where the algorithm needs it final;
//   inside one launch, nothing that one workgroup writes is read or written by another (kernel boundaries are the only synchronisation);
//   the number of launches is pg_dense_launches(m) = 3 T.
//   (no argument) / <first> <last>   the replay; prints "pg_plan: ok"
//   count <m>                        "N <launches> <T> <Tb>"
#include "pg_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace mlh;

static long failures = 0;
static int m = 0;
static bool quiet = false;
#define CHECK(cond) do { if (!(cond)) { if (failures < 20 && !quiet) std::printf("pg_plan: CHECK FAILED line %d (m = %d): %s\n", __LINE__, m, #cond); ++failures; } } while (0)

// what is known of one piece of memory
struct Res {
    int summed = 0, updated = 0, done = 0;   // a tile's history (done: factored into D, or solved in place)
    int last_write = -1;                     // the launch that wrote it last
    // within the launch `stamp`: the workgroup that writes it (-1: none) and up to two different workgroups that read it
    int stamp = -1, writer = -1, reader_a = -1, reader_b = -1;
};

struct Replay {
    int T, Tb, launch = -1;
    std::vector<Res> res;
    Replay(int T_, int Tb_) : T(T_), Tb(Tb_), res(size_t(T_) * Tb_ + 3 * size_t(T_)) {}
    Res &C(int k, int i) { return res[size_t(k) * Tb + i]; }
    Res &D(int k) { return res[size_t(T) * Tb + k]; }
    Res &W(int t) { return res[size_t(T) * Tb + T + t]; }
    Res &Z(int t) { return res[size_t(T) * Tb + 2 * size_t(T) + t]; }
    void touch(Res &r)
    {
        if (r.stamp != launch) { r.stamp = launch; r.writer = r.reader_a = r.reader_b = -1; }
    }
    void read(Res &r, int wg)
    {
        touch(r);
        CHECK(r.last_write >= 0);                                    // never read before it was written
        CHECK(r.writer == -1 || r.writer == wg);                     // not written by another workgroup of this launch
        if (r.reader_a == -1 || r.reader_a == wg) r.reader_a = wg;
        else if (r.reader_b == -1 || r.reader_b == wg) r.reader_b = wg;
    }
    void write(Res &r, int wg)
    {
        touch(r);
        CHECK(r.writer == -1 || r.writer == wg);                     // one writer per launch
        CHECK((r.reader_a == -1 || r.reader_a == wg) && (r.reader_b == -1 || r.reader_b == wg));       // and no other reader
        r.writer = wg;
    }
    // reads are recorded before writes of OTHER workgroups may follow: run every workgroup's reads and writes, then stamp last_write
    void commit(Res &r) { if (r.stamp == launch && r.writer != -1) r.last_write = launch; }
};

static void replay(int mm)
{
    m = mm;
    const int T = pg_dense_panels(m), Tb = pg_dense_row_tiles(m), tm = m / PG_PANEL;
    CHECK(T >= 1 && T * PG_PANEL >= m && (T - 1) * PG_PANEL < m);
    CHECK(Tb * PG_PANEL >= m + 1 && (Tb - 1) * PG_PANEL < m + 1 && (Tb == T || Tb == T + 1));
    CHECK(tm < Tb && tm >= T - 1);                                   // the bordering row's tile exists: the last diagonal tile (tm == T - 1) or a row tile of its own
    Replay R(T, Tb);
    std::vector<int> row_updates(size_t(T), 0), row_solved(size_t(T), 0);
    const int n = pg_dense_launches(m);
    CHECK(n == 3 * T);
    int back_seen = 0;
    for (int s = 0; s < n; ++s) {
        const PgDenseStep d = pg_dense_step(m, s);
        R.launch = s;
        CHECK(d.hi > d.lo);
        if (d.kind == PG_STEP_SUM) {
            CHECK(s == 0 && d.lo == 0);
            for (int w = d.lo; w < d.hi; ++w) {
                int k = -1, i = -1;
                pg_dense_sum_tile(w, Tb, &k, &i);
                CHECK(k >= 0 && k < T && i >= k && i < Tb);
                if (!(k >= 0 && k < T && i >= k && i < Tb)) continue;
                R.write(R.C(k, i), w);
                ++R.C(k, i).summed;
            }
            for (int k = 0; k < T; ++k)
                for (int i = k; i < Tb; ++i) R.commit(R.C(k, i));
        } else if (d.kind == PG_STEP_UPDATE) {
            const int k = d.k;
            CHECK(k > 0 && k < T && d.lo == k && d.hi == Tb && back_seen == 0);
            if (!(k > 0 && k < T && d.lo >= k && d.hi <= Tb)) continue;
            for (int i = d.lo; i < d.hi; ++i) {
                Res &t = R.C(k, i);
                for (int j = 0; j < k; ++j) {
                    CHECK(R.C(j, k).done == 1 && R.C(j, i).done == 1);
                    R.read(R.C(j, k), i);
                    R.read(R.C(j, i), i);
                }
                CHECK(t.summed == 1 && t.updated == 0 && t.done == 0);
                R.read(t, i);
                R.write(t, i);
                ++t.updated;
            }
            for (int i = d.lo; i < d.hi; ++i) R.commit(R.C(k, i));
        } else if (d.kind == PG_STEP_PANEL) {
            const int k = d.k;
            CHECK(k >= 0 && k < T && d.lo == k && d.hi == Tb && back_seen == 0);
            if (!(k >= 0 && k < T && d.lo >= k && d.hi <= Tb)) continue;
            for (int i = d.lo; i < d.hi; ++i) {
                Res &kk = R.C(k, k), &t = R.C(k, i);
                CHECK(kk.summed == 1 && kk.updated == (k > 0 ? 1 : 0));
                R.read(kk, i);                                       // every workgroup factors the diagonal tile for itself
                CHECK(t.summed == 1 && t.updated == (k > 0 ? 1 : 0) && t.done == 0);
                if (i == k) R.write(R.D(k), i);                      // ... and ONE stores the factor, away from what the others read
                else { R.read(t, i); R.write(t, i); }
                ++t.done;
            }
            R.commit(R.D(k));
            for (int i = d.lo; i < d.hi; ++i) R.commit(R.C(k, i));
        } else {
            CHECK(d.kind == PG_STEP_BACK);
            const int k = d.k;
            const bool first = back_seen == 0;
            CHECK(k == T - 1 - back_seen && d.lo == 0 && d.hi == k + 1);
            ++back_seen;
            if (!(k >= 0 && k < T && d.lo >= 0 && d.hi <= k + 1)) continue;
            for (int jt = d.lo; jt < d.hi; ++jt) {
                CHECK(R.C(k, k).done == 1 && R.D(k).last_write >= 0);
                R.read(R.D(k), jt);
                if (!first) R.read(R.W(k), jt);
                else if (tm == k) R.read(R.D(k), jt);
                else { CHECK(R.C(k, tm).done == 1); R.read(R.C(k, tm), jt); }
                CHECK(row_updates[size_t(k)] == T - 1 - k);          // z_k is solved (by every workgroup for itself) from a finished w_k
                if (jt == k) { R.write(R.Z(k), jt); ++row_solved[size_t(k)]; continue; }
                CHECK(R.C(jt, k).done == 1);
                R.read(R.C(jt, k), jt);
                if (!first) R.read(R.W(jt), jt);
                else { CHECK(R.C(jt, tm).done == 1); R.read(R.C(jt, tm), jt); }
                R.write(R.W(jt), jt);
                CHECK(row_updates[size_t(jt)] == T - 1 - k);
                ++row_updates[size_t(jt)];
            }
            for (int jt = d.lo; jt < d.hi; ++jt) { R.commit(R.W(jt)); R.commit(R.Z(jt)); }
        }
    }
    for (int k = 0; k < T; ++k) {
        for (int i = k; i < Tb; ++i) CHECK(R.C(k, i).summed == 1 && R.C(k, i).updated == (k > 0 ? 1 : 0) && R.C(k, i).done == 1);
        for (int i = 0; i < k; ++i) CHECK(R.C(k, i).summed == 0 && R.C(k, i).last_write == -1 && R.C(k, i).stamp == -1);
        CHECK(R.D(k).last_write >= 0 && R.Z(k).last_write >= 0);
        CHECK(row_solved[size_t(k)] == 1 && row_updates[size_t(k)] == T - 1 - k);
    }
}

// the replay must NOT accept the hazard it is there for: a panel launch whose workgroup k stores the factor over tile (k, k), which the others read
static void self_check()
{
    m = 774;
    Replay R(pg_dense_panels(m), pg_dense_row_tiles(m));
    R.launch = 0;
    R.write(R.C(0, 0), 0);
    R.commit(R.C(0, 0));
    R.launch = 1;
    quiet = true;
    const long before = failures;
    R.read(R.C(0, 0), 0); R.read(R.C(0, 0), 1);
    R.write(R.C(0, 0), 0);
    const bool caught = failures > before;
    failures = before;
    R.launch = 2;
    R.write(R.C(0, 0), 0);
    const long mid = failures;
    R.read(R.C(0, 0), 1);
    const bool caught_late_reader = failures > mid;
    failures = before;
    quiet = false;
    if (!caught || !caught_late_reader) { std::printf("pg_plan: the replay does not see a tile written by one workgroup and read by another\n"); ++failures; }
}

int main(int argc, char **argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "count")) {
        m = std::atoi(argv[2]);
        std::printf("N %d %d %d\npg_plan: ok\n", pg_dense_launches(m), pg_dense_panels(m), pg_dense_row_tiles(m));
        return 0;
    }
    const int first = argc >= 3 ? std::atoi(argv[1]) : PG_MAX_LOOPS + 1, last = argc >= 3 ? std::atoi(argv[2]) : int(MLH_PG_LOOPS_LIMIT);
    CHECK(PG_MAX_LOOPS == 128 && MLH_PG_LOOPS_LIMIT >= PG_MAX_LOOPS && pg_dense_launches(0) == 0);
    self_check();
    for (int L = first; L <= last; ++L) replay(6 * L);
    if (failures) { std::printf("pg_plan: %ld checks failed\n", failures); return 1; }
    std::printf("pg_plan: ok (%d .. %d)\n", first, last);
    return 0;
}
