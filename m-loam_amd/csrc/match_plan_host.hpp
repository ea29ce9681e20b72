// The launch planner of the correspondence kernels (match.hip), host arithmetic only: which instantiation of knn_features_kernel / knn_features_wide_kernel a
// launch gets, under which profiler id, whether it carries its fit and which fit launch follows it otherwise -- ONE pure function of a small record, with the list of
// instantiated forms behind it. No HIP and no mlh_ctx in here: match.hip fills the record from the context and looks the planned form up in its kernel table; a
// stand-alone host program enumerates the record's whole domain under a sanitizer (tests/host/match_plan_main.cpp).
#pragma once
#include <cstddef>
#include "../../include/mloam_hip.h"
#include "launch_modes.hpp"

namespace mlh {

constexpr int KNN_WG_NARROW = 256;           // (== TPB, knn_dev.hpp: match.hip asserts it)
constexpr int KNN_FUSE_MIN_QUERIES = 8192;   // (== KNN_LATENCY_LIMIT, knn_dev.hpp: match.hip asserts it) the fusion rule's "chip-filling", see knn_fit_in_search

// ---------------------------------------------------------------- the forms
// The template arguments of a correspondence kernel as data. W: threads per workgroup (256: knn_features_kernel<G, MB, K10, PRE, WARM, DEVM>; 512 / 1024:
// knn_features_wide_kernel<W, G, PRE, WARM, FIT>, whose MB, K10 and DEVM are false); the kernels' own comments say what each argument compiles in.
struct KnnForm {
    int W, G;
    bool MB, K10;
    int PRE;
    bool WARM, DEVM, FIT;
};
inline bool operator==(const KnnForm &a, const KnnForm &b)
{
    return a.W == b.W && a.G == b.G && a.MB == b.MB && a.K10 == b.K10 && a.PRE == b.PRE && a.WARM == b.WARM && a.DEVM == b.DEVM && a.FIT == b.FIT;
}

// EVERY instantiation of the two kernels, named here and nowhere else: X(W, G, MB, K10, PRE, WARM, DEVM, FIT). This header expands the list to KNN_FORMS, match.hip
// to its table of {form, kernel}; a form that is not in the list does not exist (32 narrow + 36 wide kernels; a 1 024-thread kernel costs a minute of build time, so
// the list holds what knn_plan() can return and nothing else -- tests/test_gn_fit_in_search_isa.py compares it with the code object's symbols).
//   the schedules of mlh_gn_solve*'s single-block, K = 5 launches: PRE 2, PRE 1 warm, PRE 1 cold (those three also fused) and the bounded search without a prologue
#define MLH_KNN_FORMS_PRE(X, W, G, FIT) X(W, G, 0, 0, 2, 0, 0, FIT) X(W, G, 0, 0, 1, 1, 0, FIT) X(W, G, 0, 0, 1, 0, 0, FIT)
#define MLH_KNN_FORMS_GN(X, W, G) MLH_KNN_FORMS_PRE(X, W, G, 0) X(W, G, 0, 0, 0, 1, 0, 0)
#define MLH_KNN_FORMS_GN_ALL_W(X, G) MLH_KNN_FORMS_GN(X, 1024, G) MLH_KNN_FORMS_GN(X, 512, G) MLH_KNN_FORMS_GN(X, 256, G)
//   pose blocks (or K = 10) with the finish in the consumer: PRE 1 and warm together, K10 or not
#define MLH_KNN_FORMS_BLOCKS(X, G) X(256, G, 1, 1, 1, 1, 0, 0) X(256, G, 1, 0, 1, 1, 0, 0)
//   every other launch: <lanes, pose blocks, any block with K = 10>
#define MLH_KNN_FORMS_PLAIN(X, G) X(256, G, 1, 1, 0, 0, 0, 0) X(256, G, 1, 0, 0, 0, 0, 0) X(256, G, 0, 1, 0, 0, 0, 0) X(256, G, 0, 0, 0, 0, 0, 0)
#define MLH_KNN_FORMS(X)                                                                                                                  \
    X(256, 0, 0, 0, 0, 1, 1, 0) X(256, 0, 0, 0, 0, 0, 1, 0) /* device-side feature counts: per-kind lanes, bounded search or not */      \
    MLH_KNN_FORMS_BLOCKS(X, 0) MLH_KNN_FORMS_BLOCKS(X, 16) MLH_KNN_FORMS_BLOCKS(X, 8)                                                     \
    /* fused: every kind puts 64 queries or more into a workgroup -- 8 or 16 lanes at 1 024 threads, 8 lanes at 512 */                    \
    MLH_KNN_FORMS_PRE(X, 1024, 0, 1) MLH_KNN_FORMS_PRE(X, 1024, 16, 1) MLH_KNN_FORMS_PRE(X, 1024, 8, 1) MLH_KNN_FORMS_PRE(X, 512, 8, 1)  \
    MLH_KNN_FORMS_GN_ALL_W(X, 0) MLH_KNN_FORMS_GN_ALL_W(X, 16) MLH_KNN_FORMS_GN_ALL_W(X, 8)                                               \
    MLH_KNN_FORMS_PLAIN(X, 0) MLH_KNN_FORMS_PLAIN(X, 16) MLH_KNN_FORMS_PLAIN(X, 8)

#define MLH_KNN_FORM_ENTRY(W, G, MB, K10, PRE, WARM, DEVM, FIT) KnnForm{W, G, bool(MB), bool(K10), PRE, bool(WARM), bool(DEVM), bool(FIT)},
constexpr KnnForm KNN_FORMS[] = {MLH_KNN_FORMS(MLH_KNN_FORM_ENTRY)};
#undef MLH_KNN_FORM_ENTRY
constexpr int KNN_FORM_COUNT = int(sizeof(KNN_FORMS) / sizeof(KNN_FORMS[0]));

// the form's place in the list (match.hip's table has the same order), or -1: no such kernel
inline int knn_form_index(const KnnForm &f)
{
    for (int i = 0; i < KNN_FORM_COUNT; ++i) if (KNN_FORMS[i] == f) return i;
    return -1;
}

// ---------------------------------------------------------------- what the decision depends on
enum KnnFit : int {       // the fit launch behind the search: fit_linearize_kernel<KMAX, LM, FIN, DEVM>
    KNN_FIT_NONE = 0,     // none: the search launch carries it (fused), or the loop launch behind this one does (no_fit)
    KNN_FIT_DEVM,         // <5, false, false, true>
    KNN_FIT_LM_BEGIN,     // <5, true>
    KNN_FIT_K10_RECORDS,  // <10, false, false>
    KNN_FIT_K10,          // <10, false>
    KNN_FIT_RECORDS,      // <5, false, false>
    KNN_FIT_FINISH        // <5, false>
};

struct KnnPlanIn {
    int kind_mask = 3;              // bit MLH_SURF, bit MLH_CORNER
    int m[2] = {0, 0};              // feature slots per kind (FeatSet::m)
    int lanes[2] = {16, 16};        // lanes per query per kind, as knn_lanes_for resolved them (rule and MLH_KNN_LANES): 8, 16 or 32
    int cu_solver = 256;            // compute units of the solver's stream
    int wg_pin = 0;                 // MLH_KNN_WG_THREADS: 0 (the rule), 256, 512, 1024
    int fit_pin = -1;               // MLH_GN_FIT_IN_SEARCH: -1 (the rule), 0, 1
    bool sharded = false;           // ownership planes or an ownership modulus (KParams::own_mode != 0)
    bool mb = false, k10 = false;   // more than one pose block; any block with N_NEIGH = 10
    bool gn_blocks = false;         // a solve over pose blocks (even over one): the blocks' pose slots
    bool m_dev = false;             // the feature counts are on the device only
    PreFinish pre_finish = PRE_NONE;
    bool warm = false;
    LaunchTail tail = TAIL_RECORDS;
    bool no_fit = false, dense = false, lmc = false, stat = false;
    int rows_in = 1;                // the layout of the records in front of a prologue: 1 record or 4 wavefront rows per 256-feature tile
};

struct KnnPlan {
    int err = MLH_OK;               // MLH_OK, or the refusal: no such launch exists (why says which rule)
    const char *why = nullptr;
    KnnForm form{};
    int kid = MLH_K_KNN;            // the search launch's profiler id
    bool gn_shape = false;          // one of the launches whose width the rule below decides (wide or not): mlh_ctx::knn_wg_last records it
    bool fused = false;             // == form.FIT: a whole Gauss-Newton iteration in this launch, it leaves wavefront rows
    KnnFit fit = KNN_FIT_NONE;
};

// ---------------------------------------------------------------- the rules
// Threads per workgroup of a correspondence launch. Only the single-block, K = 5 launches of mlh_gn_solve* with a prologue or a bounded search, host-side counts and
// one rank have wide forms (knn_features_wide_kernel) -- THE wide-form rule, written here and nowhere else; every other launch is 256 threads. Every workgroup of
// those launches runs the Gauss-Newton prologue, so what counts is workgroups per compute unit: a launch goes wide when its 256-thread grid (tiles256) would put more
// than one workgroup on a compute unit of the solver's stream (cu_solver: the device's, or the CU mask's), and stays narrow otherwise -- wider workgroups would only
// leave compute units without work. KNN_WG_WIDE is the measured choice (profiles/r08_knn_workgroup_width.txt); MLH_KNN_WG_THREADS in the environment at mlh_create
// pins the width of the launches that have wide forms (tests, A/B runs).
constexpr int KNN_WG_WIDE = 1024;
inline bool knn_gn_shape(const KnnPlanIn &in) { return (in.pre_finish != PRE_NONE || in.warm) && !in.mb && !in.k10 && !in.gn_blocks && !in.m_dev; }
inline int knn_tiles256(const KnnPlanIn &in)
{
    int tiles256 = 0;
    for (int k = 0; k < 2; ++k)
        if ((in.kind_mask & (1 << k)) && in.m[k] > 0) tiles256 += (in.m[k] + KNN_WG_NARROW / in.lanes[k] - 1) / (KNN_WG_NARROW / in.lanes[k]);
    return tiles256;
}
inline int knn_plan_width(const KnnPlanIn &in)
{
    if (!(knn_gn_shape(in) && !in.sharded)) return KNN_WG_NARROW;
    if (in.wg_pin) return in.wg_pin;
    return knn_tiles256(in) > in.cu_solver ? KNN_WG_WIDE : KNN_WG_NARROW;
}

// One Gauss-Newton iteration as ONE launch -- the fit in the tail of its search (knn_features_wide_kernel<.., FIT>) -- or as two. Fused: a launch that goes wide
// anyway, has a prologue in front (PRE 1 / PRE 2), whose fit launch would be fit_linearize_kernel<5, false, false> leaving records (single block, K = 5 and one rank
// come with the wide form; no dense rows, no statistics, no publication from the fit), and whose every kind puts whole wavefront rows -- 64 queries or more -- into
// a workgroup. Everything else keeps two launches.
// Of the launches that can fuse, the rule fuses the chip-filling ones -- more than KNN_LATENCY_LIMIT queries, the throughput regime of knn_lanes_for, where the gain
// was measured (profiles/r09_gn_fit_in_search.txt: one 1 024-thread workgroup per compute unit, half of them idle through the search's last 4 us). A smaller frame that
// goes wide (the 16-ring frame of tests/test_gpu_launch_census.py: 5 451 features, 86 wide workgroups on 256 compute units) keeps its two launches: not measured, and
// recorded that way. MLH_GN_FIT_IN_SEARCH=1 fuses every launch that can, =0 none (tests, A/B runs).
inline bool knn_fit_in_search(const KnnPlanIn &in, int wg)
{
    if (in.fit_pin == 0 || wg == KNN_WG_NARROW || in.pre_finish == PRE_NONE) return false;
    if (in.tail != TAIL_RECORDS || in.no_fit || in.dense || in.lmc || in.stat || in.sharded || in.mb || in.gn_blocks || in.m_dev) return false;
    long long queries = 0;
    for (int k = 0; k < 2; ++k) {
        if (!(in.kind_mask & (1 << k))) continue;
        if (in.lanes[k] < 8 || wg / in.lanes[k] < 64) return false;
        queries += in.m[k];
    }
    return in.fit_pin > 0 || queries > KNN_FUSE_MIN_QUERIES;
}

// lanes per query as a template argument (KParams::knn_lanes): one value for both kinds, or 0 = per kind, KindP::lanes (different lanes; 32 lanes per query exist in
// the per-kind kernels only)
inline int knn_plan_lanes(const KnnPlanIn &in)
{
    const int G = (in.kind_mask & 3) == 3 ? (in.lanes[0] == in.lanes[1] ? in.lanes[0] : 0) : in.lanes[(in.kind_mask & 1) ? 0 : 1];
    return G == 32 ? 0 : G;
}

inline KnnPlan knn_refuse(int err, const char *why) { KnnPlan p; p.err = err; p.why = why; return p; }

// THE decision. A plan, or a refusal; a plan's form is in KNN_FORMS (tests/host/match_plan_main.cpp runs the whole domain through this and checks it).
inline KnnPlan knn_plan(const KnnPlanIn &in)
{
    KnnPlan p;
    const int wg = knn_plan_width(in);
    p.gn_shape = knn_gn_shape(in);
    // the records in front of the prologue: wavefront rows are read by the wide kernels only
    if (in.rows_in == 4 && wg == KNN_WG_NARROW) return knn_refuse(MLH_ERR_STATE, "wavefront rows in front of a launch without a wide kernel");
    const int G = knn_plan_lanes(in);
    const bool pre_or_warm = in.pre_finish != PRE_NONE || in.warm;
    // (a prologue that completes the previous solve starts a solve: nothing bounds its search; without a prologue only the bounded search is one of these launches)
    const bool warm_form = in.pre_finish == PRE_ITERATION ? in.warm : in.pre_finish == PRE_NONE;
    if (in.m_dev) {
        // the feature counts are on the device only (mlh_downsample_scan2map): per-kind lanes, both kinds, one block, K = 5, records only
        if (in.mb || in.k10 || in.tail != TAIL_RECORDS || in.pre_finish != PRE_NONE || (in.kind_mask & 3) != 3)
            return knn_refuse(MLH_ERR_UNSUPPORTED, "device-side feature counts: one block, N_NEIGH 5, both kinds, records only");
        p.form = KnnForm{KNN_WG_NARROW, 0, false, false, 0, in.warm, true, false};
        p.fit = in.no_fit ? KNN_FIT_NONE : KNN_FIT_DEVM;      // (no_fit: the loop launch behind this one fits)
        return p;
    }
    if (pre_or_warm && (in.mb || in.k10 || in.gn_blocks)) {      // (gn_blocks: a blocks solve over ONE block keeps the blocks' pose slots)
        // a solve over pose blocks (or with N_NEIGH = 10): the finish in the consumer and the bounded search come together or not at all
        if (!(in.pre_finish == PRE_ITERATION && in.warm)) return knn_refuse(MLH_ERR_UNSUPPORTED, "pose blocks: the deferred finish and the bounded search are one schedule");
        p.form = KnnForm{KNN_WG_NARROW, G, true, in.k10, 1, true, false, false};
        p.kid = MLH_K_KNN_PRE;
    } else if (pre_or_warm) {
        // the whole iteration in this launch (fused: the search's profiler id, no MLH_K_FIT launch), or its search in 256, 512 or 1 024 threads
        p.fused = knn_fit_in_search(in, wg);
        p.form = KnnForm{wg, G, false, false, int(in.pre_finish), warm_form, false, p.fused};
        p.kid = in.pre_finish == PRE_SOLVE ? MLH_K_KNN_FIRST : in.pre_finish == PRE_ITERATION ? MLH_K_KNN_PRE : MLH_K_KNN;
    } else
        p.form = KnnForm{KNN_WG_NARROW, G, in.mb, in.k10, 0, false, false, false};
    if (p.fused) return p;
    if (in.no_fit) {
        // the fit rides in the loop launch behind this one (lm_consume_launch, fit_in_loop): single block, N_NEIGH 5, both kinds, records only
        if (in.k10 || in.mb || in.tail != TAIL_RECORDS || (in.kind_mask & 3) != 3 || in.dense)
            return knn_refuse(MLH_ERR_UNSUPPORTED, "match_launch without its fit: single block, N_NEIGH 5, both kinds, records only");
        return p;
    }
    if (in.tail == TAIL_LM_BEGIN) {
        if (in.k10 || in.mb) return knn_refuse(MLH_ERR_UNSUPPORTED, "the fused Levenberg-Marquardt begin is single-block, N_NEIGH = 5");
        p.fit = KNN_FIT_LM_BEGIN;
    } else if (in.k10) p.fit = in.tail == TAIL_RECORDS ? KNN_FIT_K10_RECORDS : KNN_FIT_K10;
    else p.fit = in.tail == TAIL_RECORDS ? KNN_FIT_RECORDS : KNN_FIT_FINISH;
    return p;
}

}  // namespace mlh
