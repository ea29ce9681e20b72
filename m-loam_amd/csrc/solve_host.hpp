// What the hosts of the solvers share: the arguments of a correspondence / linearise launch (match.hip, select.hip, solve_host.hip) and the helpers around the
// solver state, the publication records and the residency gates that solve_host.hip, track.hip and grid.hip use. Kept out of ctx.hpp: units that do not solve do
// not see them.
#pragma once
#include "ctx.hpp"

namespace mlh {

// match.hip
struct MatchArgs {
    int kind_mask = 3;   // bit MLH_SURF, bit MLH_CORNER: which feature kinds take part in the launch
    uint32_t flags = 0;
    float min_match_sq_dis = 1.f, min_plane_dis = 0.2f;
    double huber_delta = 0.1, cov_measurement_trace = 0.0075;
    bool dense = false;  // also write r / J per feature
    int pose_sel = 0;    // 0: SolverState::x, 1: SolverState::cand
    LaunchTail finish = TAIL_RECORDS;
    int lm_max_it = 30, lm_min_blocks = 0;
    LmExpect lm_expect_done = LM_VERDICT_READ;   // read by the launch that runs an LM begin (TAIL_LM_BEGIN, LMC_BEGIN, LMC_LOOP)
    int stat_slot = -1;
    int n_blocks = 1;    // pose blocks
    int k_neigh[8] = {5, 5, 5, 5, 5, 5, 5, 5};
    double eig_thre[8] = {100, 100, 100, 100, 100, 100, 100, 100};
    int freeze[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const double *init_pose = nullptr;       // host: block 0's pose for this launch comes from the kernel arguments and is written to the state by the finish
    // Gauss-Newton with the finish done by the consumer: this launch pair is iteration `gn_iter` of `gn_iters` (>= 2). The fit kernel of every iteration but the last
    // only leaves its tiles' records; the correspondence kernel of the next iteration -- or of a CHAINED successor's iteration 0, pre_final -- starts by completing it
    // (every workgroup, same order, same bits). gn_iter < 0: the classic form (the fit kernel's last-arriving workgroup finishes). Where each launch's poses are
    // read and written follows from these fields alone: solve_plan_host.hpp, pose_plan.
    int gn_iter = -1, gn_iters = 0;
    int gn_slot_base = 0;     // this solve's pair of SolverState::xi slots (mlh_ctx::GnChain::solve_begins)
    bool gn_blocks = false;   // the solve runs over pose blocks
    bool warm = false;   // the neighbour records of the previous iteration (same features, same map) bound this iteration's search
    // the predecessor's pending record, as gn_solve_submit copied it (mlh_ctx::GnChain::pending) -- where its records are, its last pose slot, threshold, host record
    // and sequence number. Set for EVERY iteration of the completing solve; iteration 0 publishes that solve's pose and chains this frame's start pose from it
    const mlh_ctx::GnPending *pre_final = nullptr;
    const double *chain_prev = nullptr, *chain_cur = nullptr;   // host: the two odometry poses of the chain (7 doubles each)
    LmConsumer lmc = LMC_NONE;
    int lmc_j = 0;       // lm_consume_launch: the launch's number within its loop (1, 2, ...: record buffer (j - 1) & 1 is read, j & 1 written)
    // The fit of an outer iteration inside the loop launch that follows it (lm_loop_kernel<.., FIT>; one launch boundary fewer): match_launch with `no_fit` ends behind
    // the correspondence kernel, lm_consume_launch (LMC_LOOP) with `fit_in_loop` begins with the fit. Only together, and only where loop_fit_fusable() says so (tagged
    // records: the fit's record leaves as the loop's own do); solve_host.hip builds the pair in one place (s2m_loop_args).
    bool no_fit = false, fit_in_loop = false;
    const int *m_dev = nullptr;   // device: the two feature counts (surf, corner) when the host has not read them (mlh_downsample_scan2map); FeatSet::m then holds upper bounds
    HostPublish *publish = nullptr;          // pinned host record the launch writes the pose(s) to: honoured by TAIL_GN, TAIL_LM_STEP and every consumer-side launch
    unsigned long long publish_seq = 0;
};
int match_launch(mlh_ctx *ctx, const MatchArgs &a);
bool gn_first_launch_takes_rows(const mlh_ctx *ctx, int kind_mask);   // the planner's answer: iteration 0 of a deferred solve over these kinds that completes its predecessor can read that solve's wavefront rows
int linearize_launch(mlh_ctx *ctx, const MatchArgs &a);
int lm_consume_launch(mlh_ctx *ctx, const MatchArgs &a);
bool loop_fit_fusable(const MatchArgs &loop_args);   // the loop launch described by these arguments can carry its fit (tagged records, one block, no dense rows)

// solve_host.hip
int ensure_state(mlh_ctx *ctx, int n_stats);
int upload_pose(mlh_ctx *ctx, const double pose[7]);
int solver_begin(mlh_ctx *ctx, int n_stats);
int publish_slot(mlh_ctx *ctx, HostPublish **h, unsigned long long *seq, int which = -1);
int wait_published(mlh_ctx *ctx, unsigned long long seq, HostPublish &out, void *record = nullptr);
int fetch_pose_and_stats(mlh_ctx *ctx, double pose[7], mlh_iter_stat *stats, int n_stats);
int collect_loop_pose(mlh_ctx *ctx, unsigned long long seq, HostPublish *rec, double pose_out[7], bool *given_up, HostPublish *hp_out = nullptr);
inline int tiles_of(int m) { return (m + 255) / 256; }      // (the fit / linearise kernels' tile: 256 features, match.hip and track.hip)

// capi.hip: the residency gates of the one-launch loops (set_loop_gates has the reasoning behind the two bounds)
constexpr int GN_DEFER_MAX_TILES = 160;
constexpr int FUSED_LOOP_MAX_TILES = 512;
void demote_loop_gate(mlh_ctx *c, int which, int tiles);
bool loop_tiles_ok(const mlh_ctx *c, int which, int tiles, bool cov = false);
void note_loop_given_up(mlh_ctx *ctx, int gate, int tiles);

}  // namespace mlh
