// The launch planner of the correspondence kernels (m-loam_amd/csrc/match_plan_host.hpp) over its whole domain, stand-alone, under AddressSanitizer and UBSan
// (tests/test_match_plan.py builds and runs it). Every combination of the planner's discrete inputs, lanes of 8, 16 and 32 per kind and feature counts on either
// side of the two thresholds the rules compare them with (one 256-thread workgroup per compute unit; KNN_LATENCY_LIMIT queries) goes through knn_plan(), and for
// every one:
//   (a) the result is a named refusal or a form of the list -- match_launch's "not in the list of forms" is never reached;
//   (b) fused implies wide, a prologue and W / lanes >= 64 for every kind present;
//   (c) a wide form implies !MB && !K10 && !DEVM && (PRE || WARM), on an unsharded launch;
//   (d) four-row records in front give a wide form or a refusal, never a 256-thread kernel;
//   (e) pose blocks with a prologue give PRE == 1 && WARM;
//   (f) the plan equals the ladder of function-like macros match_launch held before the planner existed, RESTATED below as plain if / else (parent_ladder).
// `match_plan_main forms` prints the list of forms, one "W G MB K10 PRE WARM DEVM FIT" per line (tests/test_gn_fit_in_search_isa.py compares it with the symbols
// of the code object).
#include <cstdio>
#include <cstring>
#include "match_plan_host.hpp"

using namespace mlh;

// ---------------------------------------------------------------- RESTATEMENT (not shared with the planner): fill_params + fit_in_search + match_launch as they stood
enum { OLD_WIDE_GRID_WITHOUT_KERNEL = -101, OLD_FUSED_WITHOUT_KERNEL = -102 };   // two of the three "cannot happen" errors (the third is a refusal the planner keeps)
struct Old {
    int err = MLH_OK;
    KnnForm form{};
    int kid = MLH_K_KNN;
    bool fused = false, wg_recorded = false;
    KnnFit fit = KNN_FIT_NONE;
};
static Old old_refuse(int err) { Old o; o.err = err; return o; }

static Old parent_ladder(const KnnPlanIn &in)
{
    Old o;
    const bool mb = in.mb, k10 = in.k10, warm = in.warm;
    const int pre = in.pre_finish;      // (0, 1, 2: PRE_NONE, PRE_ITERATION, PRE_SOLVE -- the kernels' PRE argument)
    // fill_params: P.knn_lanes
    int G;
    if ((in.kind_mask & 3) == 3) G = in.lanes[0] == in.lanes[1] ? in.lanes[0] : 0;
    else G = in.lanes[(in.kind_mask & 1) ? 0 : 1];
    if (G == 32) G = 0;
    // fill_params: wg = knn_width_of(ctx, mask, prologue_or_warm && n_blocks == 1 && kmax == 5 && !gn_blocks && !m_dev) -> knn_wg_threads_for(has_wide_form, tiles256)
    int wg = 256;
    if ((pre != 0 || warm) && !mb && !k10 && !in.gn_blocks && !in.m_dev && !in.sharded) {
        int tiles256 = 0;
        for (int k = 0; k < 2; ++k)
            if ((in.kind_mask & (1 << k)) && in.m[k] > 0) tiles256 += (in.m[k] + 256 / in.lanes[k] - 1) / (256 / in.lanes[k]);
        if (in.wg_pin) wg = in.wg_pin;
        else wg = tiles256 > in.cu_solver ? 1024 : 256;
    }
    // fit_in_search
    bool fused = true;
    if (in.fit_pin == 0 || wg == 256 || pre == 0) fused = false;
    else if (in.tail != TAIL_RECORDS || in.no_fit || in.dense || in.lmc || in.stat || in.sharded || mb || in.gn_blocks || in.m_dev) fused = false;
    else {
        long long queries = 0;
        for (int k = 0; k < 2; ++k) {
            if (!(in.kind_mask & (1 << k))) continue;
            if (in.lanes[k] < 8 || wg / in.lanes[k] < 64) fused = false;
            queries += in.m[k];
        }
        if (fused) fused = in.fit_pin > 0 || queries > 8192;
    }
    // match_launch
    if (in.rows_in == 4 && wg == 256) return old_refuse(MLH_ERR_STATE);
    if (wg != 256 && !((pre != 0 || warm) && !mb && !k10 && !in.gn_blocks && !in.m_dev)) return old_refuse(OLD_WIDE_GRID_WITHOUT_KERNEL);
    if (in.m_dev) {
        if (mb || k10 || in.tail != TAIL_RECORDS || pre != 0 || (in.kind_mask & 3) != 3) return old_refuse(MLH_ERR_UNSUPPORTED);
        if (warm) o.form = KnnForm{256, 0, false, false, 0, true, true, false};
        else o.form = KnnForm{256, 0, false, false, 0, false, true, false};
        if (!in.no_fit) o.fit = KNN_FIT_DEVM;
        return o;
    }
    if ((pre != 0 || warm) && (mb || k10 || in.gn_blocks)) {
        if (!(pre == 1 && warm)) return old_refuse(MLH_ERR_UNSUPPORTED);
        // MLH_KNN_LAUNCH_GN_MB(G)
        if (k10) o.form = KnnForm{256, G, true, true, 1, true, false, false};
        else o.form = KnnForm{256, G, true, false, 1, true, false, false};
        o.kid = MLH_K_KNN_PRE;
    } else if (fused) {
        // MLH_KNN_LAUNCH_GN_FUSED(W, G)
        if (!((wg == 1024 && (G == 0 || G == 16 || G == 8)) || (wg == 512 && G == 8))) return old_refuse(OLD_FUSED_WITHOUT_KERNEL);
        if (pre == 2) { o.form = KnnForm{wg, G, false, false, 2, false, false, true}; o.kid = MLH_K_KNN_FIRST; }
        else if (warm) { o.form = KnnForm{wg, G, false, false, 1, true, false, true}; o.kid = MLH_K_KNN_PRE; }
        else { o.form = KnnForm{wg, G, false, false, 1, false, false, true}; o.kid = MLH_K_KNN_PRE; }
        o.wg_recorded = true;
    } else if (pre != 0 || warm) {
        // MLH_KNN_LAUNCH_GN_W(G): _GN_WIDE(1024, G), _GN_WIDE(512, G) or _GN(G) -- the same four arms each
        if (pre == 2) { o.form = KnnForm{wg, G, false, false, 2, false, false, false}; o.kid = MLH_K_KNN_FIRST; }
        else if (pre != 0 && warm) { o.form = KnnForm{wg, G, false, false, 1, true, false, false}; o.kid = MLH_K_KNN_PRE; }
        else if (pre != 0) { o.form = KnnForm{wg, G, false, false, 1, false, false, false}; o.kid = MLH_K_KNN_PRE; }
        else { o.form = KnnForm{wg, G, false, false, 0, true, false, false}; o.kid = MLH_K_KNN; }
        o.wg_recorded = true;
    } else {
        // MLH_KNN_LAUNCH(G)
        o.form = KnnForm{256, G, mb, k10, 0, false, false, false};
    }
    if (fused) { o.fused = true; return o; }
    if (in.no_fit) {
        if (k10 || mb || in.tail != TAIL_RECORDS || (in.kind_mask & 3) != 3 || in.dense) return old_refuse(MLH_ERR_UNSUPPORTED);
        return o;
    }
    if (in.tail == TAIL_LM_BEGIN) {
        if (k10 || mb) return old_refuse(MLH_ERR_UNSUPPORTED);
        o.fit = KNN_FIT_LM_BEGIN;
    } else if (k10 && in.tail == TAIL_RECORDS) o.fit = KNN_FIT_K10_RECORDS;
    else if (k10) o.fit = KNN_FIT_K10;
    else if (in.tail == TAIL_RECORDS) o.fit = KNN_FIT_RECORDS;
    else o.fit = KNN_FIT_FINISH;
    return o;
}

// ---------------------------------------------------------------- the checks
static long long n_cases = 0, n_refused = 0, n_fused = 0, n_wide = 0;
static int failures = 0;
static bool reached[KNN_FORM_COUNT];       // the list holds nothing the planner never returns

static void fail_case(const char *what, const KnnPlanIn &in, const KnnPlan &p)
{
    if (++failures > 20) return;
    std::printf("FAIL %s: mask %d m %d %d lanes %d %d cu %d wg_pin %d fit_pin %d sharded %d mb %d k10 %d gn_blocks %d m_dev %d pre %d warm %d tail %d no_fit %d dense %d lmc %d stat %d rows_in %d"
                " -> err %d form {%d %d %d %d %d %d %d %d} kid %d fused %d fit %d\n",
                what, in.kind_mask, in.m[0], in.m[1], in.lanes[0], in.lanes[1], in.cu_solver, in.wg_pin, in.fit_pin, in.sharded, in.mb, in.k10, in.gn_blocks, in.m_dev, in.pre_finish,
                in.warm, int(in.tail), in.no_fit, in.dense, in.lmc, in.stat, in.rows_in, p.err, p.form.W, p.form.G, p.form.MB, p.form.K10, p.form.PRE, p.form.WARM, p.form.DEVM,
                p.form.FIT, p.kid, p.fused, int(p.fit));
}

static void check(const KnnPlanIn &in)
{
    ++n_cases;
    const KnnPlan p = knn_plan(in);
    const Old o = parent_ladder(in);
    // (f), refusals included; the old ladder's two unreachable errors are reached by nothing
    if (o.err == OLD_WIDE_GRID_WITHOUT_KERNEL || o.err == OLD_FUSED_WITHOUT_KERNEL) fail_case("the old ladder reaches a cannot-happen error", in, p);
    if (p.err != o.err) fail_case("(f) refusal", in, p);
    if (p.err != MLH_OK) {
        ++n_refused;
        if (!p.why || !p.why[0] || (p.err != MLH_ERR_STATE && p.err != MLH_ERR_UNSUPPORTED)) fail_case("(a) a refusal without a name", in, p);
        return;
    }
    if (!(p.form == o.form) || p.kid != o.kid || p.fused != o.fused || p.fit != o.fit || (p.gn_shape != o.wg_recorded)) fail_case("(f) plan", in, p);
    const KnnForm &f = p.form;
    if (knn_form_index(f) < 0) fail_case("(a) the form is not in the list", in, p);
    else reached[knn_form_index(f)] = true;
    if (p.fused != f.FIT || (p.fused && p.fit != KNN_FIT_NONE)) fail_case("fused, FIT and the fit launch disagree", in, p);
    const bool wide = f.W != 256;
    if (f.W != 256 && f.W != 512 && f.W != 1024) fail_case("width", in, p);
    if (f.W != knn_plan_width(in)) fail_case("the form's width is not the width rule's (tiles_a counts by it)", in, p);
    if (p.fused) {
        ++n_fused;
        bool ok = wide && f.PRE != 0;
        for (int k = 0; k < 2; ++k) if ((in.kind_mask & (1 << k)) && f.W / in.lanes[k] < 64) ok = false;
        if (!ok) fail_case("(b)", in, p);
    }
    if (wide) {
        ++n_wide;
        if (f.MB || f.K10 || f.DEVM || !(f.PRE != 0 || f.WARM) || in.sharded) fail_case("(c)", in, p);
    }
    if (in.rows_in == 4 && !wide) fail_case("(d)", in, p);
    if ((in.mb || in.gn_blocks) && in.pre_finish != 0 && !(f.PRE == 1 && f.WARM)) fail_case("(e)", in, p);
    if (f.PRE != in.pre_finish) fail_case("the form's prologue is not the launch's", in, p);
}

int main(int argc, char **argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "forms")) {
        for (int i = 0; i < KNN_FORM_COUNT; ++i) {
            const KnnForm &f = KNN_FORMS[i];
            std::printf("%d %d %d %d %d %d %d %d\n", f.W, f.G, f.MB, f.K10, f.PRE, f.WARM, f.DEVM, f.FIT);
        }
        return 0;
    }
    // the list itself: no form twice (a second instantiation of one kernel would not link as two table entries, but the index would hide it)
    for (int i = 0; i < KNN_FORM_COUNT; ++i)
        if (knn_form_index(KNN_FORMS[i]) != i) { std::printf("FAIL form %d is in the list twice\n", i); ++failures; }

    const int lanes_v[3] = {8, 16, 32}, cu_v[2] = {256, 64}, wg_pin_v[4] = {0, 256, 512, 1024}, fit_pin_v[3] = {-1, 0, 1};
    for (int mask = 1; mask <= 3; ++mask)
    for (int l0 = 0; l0 < 3; ++l0)
    for (int l1 = 0; l1 < 3; ++l1)
    for (int ci = 0; ci < 2; ++ci) {
        KnnPlanIn in;
        in.kind_mask = mask; in.lanes[0] = lanes_v[l0]; in.lanes[1] = lanes_v[l1]; in.cu_solver = cu_v[ci];
        // feature counts: tiny; a kind without features; 256-thread tiles == compute units and one more (the width rule's threshold, for these lanes and this mask);
        // KNN_LATENCY_LIMIT queries and one more (the fusion rule's); a large frame
        const int q0 = 256 / in.lanes[0], q1 = 256 / in.lanes[1], cu = in.cu_solver;
        int m_v[8][2];
        int n_m = 0;
        auto add = [&](int a, int b) { m_v[n_m][0] = a; m_v[n_m][1] = b; ++n_m; };
        if (ci == 0) { add(300, 300); add(0, 300); add(300, 0); }        // (the second compute-unit count, a CU mask's: the width threshold only)
        if (mask == 3) { add((cu / 2) * q0, (cu / 2) * q1); add((cu / 2) * q0, (cu / 2) * q1 + 1); }
        else { add(cu * q0, cu * q1); add(cu * q0 + 1, cu * q1 + 1); }
        if (ci == 0 && mask == 3) { add(4096, 4096); add(4096, 4097); }
        if (ci == 0 && mask != 3) { add(8192, 8192); add(8193, 8193); }
        if (ci == 0) add(20000, 20000);
        for (int mi = 0; mi < n_m; ++mi)
        for (int wi = 0; wi < 4; ++wi)
        for (int fi = 0; fi < 3; ++fi)
        for (int bits = 0; bits < 1024; ++bits)        // sharded, mb, k10, gn_blocks, m_dev, warm, no_fit, dense, lmc, stat
        for (int pre = 0; pre < 3; ++pre)
        for (int tail = TAIL_RECORDS; tail <= TAIL_LM_STEP; ++tail)
        for (int rows = 1; rows <= (pre ? 4 : 1); rows += 3) {      // (no prologue: no records in front)
            in.m[0] = m_v[mi][0]; in.m[1] = m_v[mi][1];
            in.wg_pin = wg_pin_v[wi]; in.fit_pin = fit_pin_v[fi];
            in.sharded = bits & 1; in.mb = bits & 2; in.k10 = bits & 4; in.gn_blocks = bits & 8; in.m_dev = bits & 16;
            in.warm = bits & 32; in.no_fit = bits & 64; in.dense = bits & 128; in.lmc = bits & 256; in.stat = bits & 512;
            in.pre_finish = PreFinish(pre); in.tail = LaunchTail(tail); in.rows_in = rows;
            check(in);
        }
    }
    for (int i = 0; i < KNN_FORM_COUNT; ++i)
        if (!reached[i]) { std::printf("FAIL form %d of the list is planned by no input\n", i); ++failures; }
    std::printf("match_plan: %lld cases, %lld refused, %lld wide, %lld fused, %d forms, %d failures\n", n_cases, n_refused, n_wide, n_fused, KNN_FORM_COUNT, failures);
    if (failures || n_fused == 0 || n_wide == 0 || n_refused == 0) return 1;
    std::printf("match_plan: ok\n");
    return 0;
}
