// The rest of a solver launch's plan (match.hip), beside the correspondence kernels' (match_plan_host.hpp) and under the same rules -- host arithmetic only, no HIP
// and no mlh_ctx: WHERE the poses of a launch are read and written (pose_plan: the slot rule of a Gauss-Newton solve with the finish in the consumer, written here and
// nowhere else), and WHICH linearise / Levenberg-Marquardt kernel a launch gets, or why it gets none (lm_plan, with the list of instantiations behind it). match.hip
// turns a symbolic slot into a pointer and looks the form up in its kernel table; solve_host.hip and the chain's owner (ctx.hpp: GnChain) ask the two slot helpers;
// a stand-alone host program enumerates both domains under a sanitizer (tests/host/solve_plan_main.cpp).
#pragma once
#include "../../include/mloam_hip.h"
#include "launch_modes.hpp"

namespace mlh {

// ---------------------------------------------------------------- the pose plan
// THE slot rule. Iteration i >= 1 of a solve whose finish runs in the consumer (MatchArgs::gn_iter) turns iteration i - 1's records and pose (x_prev) into pose i
// (x_next) in the prologue of its correspondence launch -- ONE workgroup stores x_next while the others may still be reading x_prev, so the two are never one slot --
// and evaluates there (pose0). A single-block solve keeps pose i in SolverState::xi[base + (i & 1)]; consecutive submitted solves alternate base 0 / 2, because a
// solve's first launch (PRE_SOLVE, MatchArgs::pre_final) still reads its predecessor's LAST slot while it stores this frame's start pose to xi[base]. Iteration 1
// finds pose 0 where iteration 0 found it: the kernel arguments (pre_from_init), the state's x, or xi[base] behind a PRE_SOLVE launch. A solve over pose blocks keeps
// every block's pose of iteration i in SolverState::xib[i & 1]; its iteration 1 updates the poses the state holds (pre_from_state).
enum PoseSlotKind : int { SLOT_NONE = 0, SLOT_STATE_X, SLOT_STATE_CAND, SLOT_STATE_XB, SLOT_XI, SLOT_XIB };
struct PoseSlot {
    PoseSlotKind kind = SLOT_NONE;
    int n = 0;                      // SLOT_XI: the slot, 0..3; SLOT_XIB: the parity, 0 / 1
};
inline bool operator==(const PoseSlot &a, const PoseSlot &b) { return a.kind == b.kind && a.n == b.n; }
inline bool operator!=(const PoseSlot &a, const PoseSlot &b) { return !(a == b); }

struct PosePlanIn {
    int gn_iter = -1;               // MatchArgs::gn_iter: < 0 is the classic form
    bool gn_blocks = false, pre_final = false, init_pose = false;      // (the two pointers of MatchArgs as "present")
    int pose_sel = 0;
    int slot_base = 0;              // this solve's pair of xi slots: 0 or 2
    int pre_slot = 0;               // pre_final: the predecessor's last slot
};
struct PosePlan {
    PreFinish pre_finish = PRE_NONE;
    PoseSlot x_prev, x_next, pose0;                 // (KParams' fields of the same names)
    PoseSlot pose_b0, pose_bn;                      // where the launch's poses are when they are not init_pose: block 0's, the other blocks'
    bool use_init = false, pre_from_init = false, pre_from_state = false;
};

inline PosePlan pose_plan(const PosePlanIn &in)
{
    PosePlan p;
    p.pre_finish = in.gn_iter >= 1 ? PRE_ITERATION : (in.gn_iter == 0 && in.pre_final) ? PRE_SOLVE : PRE_NONE;
    if (p.pre_finish == PRE_NONE) p.use_init = in.init_pose;
    else if (p.pre_finish == PRE_SOLVE) {
        p.x_prev = PoseSlot{SLOT_XI, in.pre_slot};
        p.x_next = PoseSlot{SLOT_XI, in.slot_base};
    } else if (in.gn_blocks) {
        p.pre_from_state = in.gn_iter == 1;
        p.x_prev = PoseSlot{SLOT_XIB, (in.gn_iter - 1) & 1};
        p.x_next = PoseSlot{SLOT_XIB, in.gn_iter & 1};
    } else {
        p.pre_from_init = in.gn_iter == 1 && in.init_pose;
        p.x_prev = (in.gn_iter == 1 && !in.pre_final) ? PoseSlot{SLOT_STATE_X, 0} : PoseSlot{SLOT_XI, in.slot_base + ((in.gn_iter - 1) & 1)};
        p.x_next = PoseSlot{SLOT_XI, in.slot_base + (in.gn_iter & 1)};
    }
    p.pose0 = p.x_next;             // (a launch with a prologue evaluates at the pose the prologue leaves)
    p.pose_b0 = p.pose0.kind != SLOT_NONE ? p.pose0 : PoseSlot{in.pose_sel ? SLOT_STATE_CAND : SLOT_STATE_X, 0};
    p.pose_bn = p.pose0.kind != SLOT_NONE ? p.pose0 : PoseSlot{SLOT_STATE_XB, 0};
    return p;
}
// what the hosts of a solve need of the rule: the slot its last iteration (of n_iters >= 2) leaves the pose in; the base of the solve submitted after it; and whether
// the caller's start pose goes in with iteration `it` (iteration 0 evaluates at it; with the finish in the consumer iteration 1's prologue updates it: pre_from_init)
inline int gn_last_slot(int slot_base, int n_iters) { return slot_base + ((n_iters - 1) & 1); }
inline int gn_next_slot_base(int slot_base) { return slot_base ^ 2; }
inline bool gn_start_pose_goes_in(int it, bool defer) { return it == 0 || (defer && it == 1); }

// ---------------------------------------------------------------- the linearise / LM kernels
// EVERY instantiation of linearize_kernel<LM, COV>, lm_consume_kernel<FIRST, COV> and lm_loop_kernel<DEVM, FIT, COV>, named here and nowhere else:
// X(family, A, B, C), the family's template arguments in order (C is unused by the two-argument families). This header expands the list to LM_FORMS, match.hip to its
// table of kernels; tests/test_gn_fit_in_search_isa.py compares it with the code object's symbols.
enum LmFamily : int { LM_LINEARIZE = 0, LM_CONSUME = 1, LM_LOOP = 2 };
#define MLH_LM_FORMS(X)                                                                                                           \
    X(LM_LINEARIZE, 0, 0, 0) X(LM_LINEARIZE, 1, 0, 0) X(LM_LINEARIZE, 1, 1, 0)                                                    \
    X(LM_CONSUME, 0, 0, 0) X(LM_CONSUME, 0, 1, 0) X(LM_CONSUME, 1, 0, 0) X(LM_CONSUME, 1, 1, 0)                                   \
    X(LM_LOOP, 0, 0, 0) X(LM_LOOP, 0, 0, 1) X(LM_LOOP, 0, 1, 0) X(LM_LOOP, 0, 1, 1) X(LM_LOOP, 1, 0, 0) X(LM_LOOP, 1, 0, 1) X(LM_LOOP, 1, 1, 0) X(LM_LOOP, 1, 1, 1)
struct LmForm {
    LmFamily family;
    bool a, b, c;
};
inline bool operator==(const LmForm &x, const LmForm &y) { return x.family == y.family && x.a == y.a && x.b == y.b && x.c == y.c; }
#define MLH_LM_FORM_ENTRY(F, A, B, C) LmForm{F, bool(A), bool(B), bool(C)},
constexpr LmForm LM_FORMS[] = {MLH_LM_FORMS(MLH_LM_FORM_ENTRY)};
#undef MLH_LM_FORM_ENTRY
constexpr int LM_FORM_COUNT = int(sizeof(LM_FORMS) / sizeof(LM_FORMS[0]));
inline int lm_form_index(const LmForm &f)
{
    for (int i = 0; i < LM_FORM_COUNT; ++i) if (LM_FORMS[i] == f) return i;
    return -1;
}

struct LmPlanIn {
    LmFamily family = LM_LINEARIZE;  // linearize_launch; lm_consume_launch names LM_CONSUME and the decision moves an LMC_LOOP launch to LM_LOOP
    LaunchTail tail = TAIL_RECORDS;
    LmConsumer lmc = LMC_NONE;
    int lmc_j = 0;
    bool cov = false;               // the launch publishes, and MLH_FLAG_POSE_COV asks for the covariance with the publication
    bool m_dev = false, fit_in_loop = false;
    int n_blocks = 1;               // MatchArgs::n_blocks as given
    bool dense = false;
    int kind_mask = 3, matched_mask = 3;      // the launch's kinds; the kinds whose correspondences a match launch left
    int n_ranks = 1;                // ranks the launch's finishing workgroup would exchange with (KParams::p2p)
    int tiles = 0, gate_tiles = 0;  // the launch's 256-feature tiles; as many as the device keeps resident for this loop kernel (mlh_ctx::caps, by cov and m_dev)
    bool tagged = false;            // the loop would exchange tagged records: the switch (read at launch time) and an iteration count the tag's byte holds
};
struct LmPlan {
    int err = MLH_OK;
    const char *why = nullptr;
    LmForm form{};
};
inline LmPlan lm_refuse(int err, const char *why) { LmPlan p; p.err = err; p.why = why; return p; }

// THE decision. A form of the list, or the refusal.
inline LmPlan lm_plan(const LmPlanIn &in)
{
    LmPlan p;
    const bool unmatched = (in.kind_mask & 3 & ~in.matched_mask) != 0;
    if (in.family == LM_LINEARIZE) {
        if (unmatched) return lm_refuse(MLH_ERR_STATE, "linearize needs a previous match of this kind");
        // (the covariance of MLH_FLAG_POSE_COV rides in a publication: launches that publish nothing are the default kernels)
        const bool lm = in.tail == TAIL_LM_BEGIN || in.tail == TAIL_LM_STEP;
        p.form = LmForm{LM_LINEARIZE, lm, lm && in.cov, false};
        return p;
    }
    const char *tagged_only = "the fit rides in the one-launch loop with tagged records only";
    if (unmatched && !in.fit_in_loop) return lm_refuse(MLH_ERR_STATE, "the Levenberg-Marquardt launches need a previous match of this kind");
    if (in.lmc == LMC_NONE || in.lmc_j < 1 || in.n_blocks > 1 || in.dense) return lm_refuse(MLH_ERR_INVALID, "lm_consume_launch: single block, no dense rows");
    if (in.fit_in_loop && (in.lmc != LMC_LOOP || (in.kind_mask & 3) != 3 || !in.tagged || in.n_blocks != 1)) return lm_refuse(MLH_ERR_INVALID, tagged_only);
    if (in.n_ranks > 1) return lm_refuse(MLH_ERR_UNSUPPORTED, "the consumer-side Levenberg-Marquardt schedule is single-GPU");
    if (in.lmc != LMC_LOOP) {
        p.form = LmForm{LM_CONSUME, in.lmc == LMC_BEGIN, in.cov, false};
        return p;
    }
    // every tile's workgroup has to be resident for the loop's barrier: the host's gate (capi.hip: loop_tiles_ok) is what the device admits, asked at mlh_create
    if (in.tiles > in.gate_tiles) return lm_refuse(MLH_ERR_INVALID, "lm_loop_kernel: more tiles than can be resident at once on this device");
    p.form = LmForm{LM_LOOP, in.m_dev, in.fit_in_loop, in.cov};
    return p;
}

}  // namespace mlh
