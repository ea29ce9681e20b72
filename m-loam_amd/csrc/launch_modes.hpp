// The solver's launch modes. Plain C++, no HIP: ctx.hpp includes it for every unit, and the launch planner (match_plan_host.hpp) and its stand-alone test program
// read the same names.
#pragma once

namespace mlh {

// Named once, here; the hosts (solve_host.hip, the launchers of match.hip / track.hip) and the kernels use the names, never the numbers. Unscoped, `int` underneath and
// the values the fields have always had: the parameter blocks' layouts and the kernels' comparisons are what they were.
enum LaunchTail : int {   // ::finish -- what the last workgroup of a fit / linearise launch does behind its tiles' records
    TAIL_RECORDS = 0,     // nothing: the launch leaves the records (a consumer sums them)
    TAIL_GN = 1,          // the Gauss-Newton finish: reduce + 6 x 6 solve + Plus
    TAIL_REDUCE = 2,      // the local reduce into SolverState::ne only (an RCCL all-reduce and an update kernel follow)
    TAIL_LM_BEGIN = 3,    // the Levenberg-Marquardt begin (match_launch; linearize_launch on the rows a selection kept; track_linearize_launch)
    TAIL_LM_STEP = 4      // the Levenberg-Marquardt step (linearize_launch, track_linearize_launch)
};
// MatchArgs::lmc -- the consumer-side LM launches (lm_consume_launch): every workgroup sums the records its predecessor left, then runs the LM begin (BEGIN: behind a
// match launch that left records) or step (STEP) and evaluates at the candidate -- or (LOOP) the whole loop of an outer iteration in this launch (lm_loop_kernel)
enum LmConsumer : int { LMC_NONE = 0, LMC_BEGIN = 1, LMC_STEP = 2, LMC_LOOP = 3 };
// ::lm_expect_done -- what an LM begin may assume about the previous outer iteration's loop: there is none, this is the first of a solve (clears lm_overflow and
// lm_used_max); the host READ its verdict before it enqueued this launch; or it did not (UNREAD): if that loop has not terminated, SolverState::lm_overflow is raised
// (the launches go on; the host discards the result). Ordered: >= LM_VERDICT_READ is "not the first".
enum LmExpect : int { LM_FIRST_OF_SOLVE = -1, LM_VERDICT_READ = 0, LM_VERDICT_UNREAD = 1 };
// KParams::pre_finish (the kernels' PRE template argument carries the same values as an int) -- the prologue of a correspondence launch completes the previous
// Gauss-Newton ITERATION of its own solve from the records that iteration's fit launch left, or the predecessor SOLVE's last iteration: publishes that solve's pose
// and chains this frame's start pose from it
enum PreFinish : int { PRE_NONE = 0, PRE_ITERATION = 1, PRE_SOLVE = 2 };

}  // namespace mlh
