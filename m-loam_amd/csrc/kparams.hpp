// The parameter block of the correspondence / fit / linearise kernels (match.hip), in a header of its own so that the launch-cost probe
// (scripts/exp/launch_floor.hip) passes the very block the product's kernels take.
#pragma once
#include "ctx.hpp"
#include "p2p_dev.hpp"

namespace mlh {

constexpr int MAX_BLOCKS = 8;

// One feature kind of a launch, without the pose-block table: what a workgroup reads of its kind. A kernel copies both kinds' records out of the argument
// segment at entry (kernel_args_ready, match.hip) and selects its own, so the order here is the order of that one batch of scalar loads: the pointers and
// counts every kernel needs first (64 bytes: one wide load), then the map grid, which only the correspondence kernel reads.
struct KindL {
    const float4 *feat;      // {x,y,z,intensity}; intensity < 0 marks a padding slot between pose blocks
    const float4 *covd;      // {cxx,cyy,czz,_} or null
    float4 *nbr;             // nbr_stride per feature: {x,y,z, sq-dist} of the k-th neighbour (w = +inf when missing)
    Corr *corr;
    double *r_out;           // nullable
    double *J_out;           // nullable
    int m;                   // feature slots (real + padding)
    int tiles_a;             // correspondence-kernel tiles (TPB / lanes features each)
    int tiles_b;             // fit / linearise tiles (256 features each)
    int nbr_stride;          // max K over the blocks
    int lanes;               // lanes per query of the correspondence kernel for this kind (8 or 16)
    int pad_;
    GridDev grid;
};

struct KindP : KindL {
    int blk_start[MAX_BLOCKS + 1];   // first slot of every pose block (multiples of 256), blk_start[n_blocks] = m
};

struct KParams {
    KindP k[2];              // [MLH_SURF], [MLH_CORNER]; m = 0 when a kind is not part of the launch
    double *partials;        // tiles_b(surf) + tiles_b(corner) records
    // the poses of this launch when they are not init_pose, resolved on the host (fill_params): block 0's at pose_b0, block b >= 1's at pose_bn + 7 b -- an
    // iteration slot of a deferred-finish solve (pose0), or the state's x / cand and xb. No kernel of the Gauss-Newton path goes through `state` for a pose.
    const double *pose_b0, *pose_bn;
    // the words every workgroup branches on, side by side (one load):
    uint32_t flags;
    int own_mode;            // "is this launch sharded, and how" (owns): bit 0 / 1: the lo / hi ownership half-space is set (mlh_shard_set), bit 2: own_mod > 1.
                             // 0 on one rank: nothing else of the ownership fields is read
    int n_blocks;            // pose blocks (BASELINE config 4: block 0 = body pose, block n = extrinsic of LiDAR n; 1 block otherwise)
    int use_init;            // block 0's pose is init_pose (first iteration of a solve: no separate upload launch)
    float min_match_sq_dis, min_plane_dis;
    double huber_delta, cov_measurement_trace;
    double init_pose[7];
    SolverState *state;
    int pose_sel;
    int own_mod, own_rem;    // ownership by feature index: slot f belongs to this rank iff f % own_mod == own_rem (mlh_shard_set_features)
    float lo[4], hi[4];      // the ownership half-spaces
    int kb[MAX_BLOCKS];      // N_NEIGH per block (5 or 10)
    double thre_b[MAX_BLOCKS];   // eigen threshold per block
    int freeze_b[MAX_BLOCKS];    // 0: project the degenerate directions out (evalDegenracy); 1: do not update the block at all
    // fused Gauss-Newton finish: the last workgroup to arrive sums the partials, solves and updates the pose(s)
    HostPublish *publish;    // the finish of the last iteration hands the result to the host through pinned memory
    unsigned long long publish_seq;
    int knn_lanes;           // lanes per query of the correspondence kernel: 8 or 16 for every kind of the launch, 0 = per kind (KindP::lanes)
    LaunchTail finish;
    int lm_max_it, lm_min_blocks;
    LmExpect lm_expect_done;
    unsigned *ticket;
    IterStatDev *stat;       // n_blocks consecutive records, or null
    // sharded over several ranks with the mailbox communicator: the finishing workgroup exchanges each block's summed record with the peers (one hop, inside
    // this launch) before it solves -- a sharded Gauss-Newton iteration is the same two launches as an unsharded one. n_ranks <= 1: nothing is exchanged
    P2pDev p2p;
    // Gauss-Newton with the finish done by the consumer (MatchArgs::gn_iter): the correspondence kernel of iteration i >= 1 completes iteration i - 1 first
    PreFinish pre_finish;    // its records: the pre_tiles records the previous fit launch left in `partials`
    int pre_tiles;
    int pre_from_init;       // the previous iteration's pose is init_pose (kernel arguments); otherwise *x_prev
    int pre_from_state;      // ... or the state's own poses (x for block 0, xb[b] otherwise): iteration 1 of a solve over pose blocks
    // (x_prev / x_next / pose0 are the poses of block 0; block b's sit 7 doubles x b further)
    const double *x_prev;
    double *x_next;          // the workgroup that serves tile 0 stores the new pose here (the fit kernel of the same iteration reads it as pose0)
    const double *pose0;     // block 0's pose of this launch when it is neither init_pose nor the state's x / cand (iterations >= 1 of a deferred-finish solve)
    int warm;                // the neighbour records hold the previous iteration's neighbours of the same features in the same map
    // PRE_SOLVE (MatchArgs::pre_final): the records are the PREVIOUS solve's last iteration; its pose is published from here, then this frame's start pose chained from it
    HostPublish *pre_publish;
    unsigned long long pre_publish_seq;
    double pre_thre;
    int pre_freeze;
    double chain_prev[7], chain_cur[7];
    // Levenberg-Marquardt with the step done by the consumer (lm_consume_kernel): the records the previous launch left, the state its writer left, the state this
    // launch's writer leaves
    const double *partials_in;
    const LmState *lm_in;
    LmState *lm_out;
    // feature counts read on the DEVICE (mlh_downsample_scan2map: the solve is enqueued behind the thinning without the host reading what the thinning kept): the
    // launches are sized for an upper bound (KindP::m, tiles_*), the DEVM kernel variants take the counts -- and the tiles that follow from them -- from here
    const int *m_dev;        // [2]: surf, corner
    unsigned long long loop_timeout_ticks;   // lm_loop_kernel: a barrier wait longer than this (100 MHz wall clock) gives the loop up (mlh_ctx::caps)
    unsigned long long *loop_tagged;   // lm_loop_kernel: two sets of tagged records (64 words per tile), or null: records + grid barrier (MLH_LOOP_TAGGED=0)
    unsigned loop_tag_base;  // this launch's tag: (launch number << 8); the iteration goes into the low byte
    int debug_stall;         // MLH_DEBUG_LOOP_STALL=1 (tests): one workgroup of lm_loop_kernel never arrives at its second barrier -- the loop must end with the error bit, not hang
    // The fit in the tail of the search launch (knn_features_wide_kernel<.., FIT>). Appended behind everything else: no other field's offset moves.
    // (16 bytes, one load)
    double *rows_out;        // a fused launch: where its fits' wavefront rows go -- row (tile256 * 4 + wave) * NE_STRIDE, surf tiles, then corner tiles; the other set than `partials`
    int pre_rows;            // how the records the prologue sums (`partials`, pre_tiles tiles) are laid out: 1 = one record per 256-feature tile (fit_linearize_kernel's),
                             // 4 = four wavefront rows per tile (a fused launch's), summed ((w0 + w1) + w2) + w3 as the fit kernel's workgroup sums them. 0 reads as 1
    int fit_pad_;
};

}  // namespace mlh
