// What a solver launch pays before and after its body: chains of 200 dependent launches on one non-blocking stream, grids of 88 x 256 and 1 016 x 256 threads,
// each variant timed by the chain's period (stream launches as fast as the host issues them; the same with the host a whole chain ahead, by events; the chain replayed
// as a captured graph); run it under
// rocprofv3 --kernel-trace --stats for the dispatches' own durations (every variant x grid is a kernel of its own name). Results: profiles/r07_launch_floor.txt.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I m-loam_amd/csrc scripts/exp/launch_floor.hip -o launch_floor
//   hipcc ... -DPRELOAD -mllvm -amdgpu-kernarg-preload-count=10 ... -o launch_floor_preload      (variants d / e with their few arguments preloaded into SGPRs)
// Variants:
//   a    no arguments, empty body
//   b    the real KParams by value; body: read one int field, leave
//   c    as b + one dependent load through a pointer field (lm_consume_kernel finding `done`)
//   c8   as c, in front of it eight fields spread over the block, each read at an offset the previous one's VALUE decides (eight scalar round trips in series)
//   c1   the same eight fields at constant offsets: one group behind one wait
//   d_b  arguments = pointer to a device-resident KParams + 32 bytes of scalars; body b (the int field comes out of the resident block)
//   d_c  ... body c (resident block -> pointer field -> word: three trips)
//   d_s  ... body c with the word's address among the scalars (argument segment -> word: c's two trips, from a 40-byte segment)
//   d_L  d_s with three 7-double poses behind the scalars, unread (the first launch of a chained frame)
#include "kparams.hpp"
#include "dev_math.hpp"
#include <chrono>
#include <cstdio>
#include <cstring>
using namespace mlh;

// the 32 bytes of per-launch scalars go as arguments of their own: only plain leading arguments are preloaded, a by-value struct ends the preloaded run
#define SCAL32 const int *done, unsigned long long seq, int slot, int publish, int tag, int pad
struct Scal32 { const int *done; unsigned long long seq; int slot, publish, tag, pad; };
struct Poses { double a[7], b[7], c[7]; };

template <int TAG> __global__ __launch_bounds__(256) void k_a() {}
template <int TAG> __global__ __launch_bounds__(256) void k_b(KParams P) { if (P.pre_tiles == 0x7fffffff) *P.ticket = 1u; }
template <int TAG> __global__ __launch_bounds__(256) void k_c(KParams P)
{
    if (int(blockIdx.x) >= P.k[0].tiles_b + P.k[1].tiles_b) return;     // (never: tiles_b are set to the grid)
    if (P.lm_in->done) return;                                          // (always)
    *P.ticket = 1u;
}
// word offsets of eight int fields the fit kernel reads, all zero in the probe's block
#define OFFS8(P) {int(offsetof(KParams, n_blocks) / 4), int(offsetof(KParams, use_init) / 4), int(offsetof(KParams, own_mode) / 4), int(offsetof(KParams, pose_sel) / 4), \
                  int(offsetof(KParams, finish) / 4), int(offsetof(KParams, pre_finish) / 4), int(offsetof(KParams, warm) / 4), int(offsetof(KParams, debug_stall) / 4)}
template <int TAG> __global__ __launch_bounds__(256) void k_c8(KParams P)
{
    const int *w = reinterpret_cast<const int *>(&P);
    constexpr int off[8] = OFFS8(P);
    int v = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) v = w[off[i] + v];      // the next offset waits for this value
    if (int(blockIdx.x) + v >= P.k[0].tiles_b + P.k[1].tiles_b) return;
    if (P.lm_in->done) return;
    *P.ticket = 1u;
}
template <int TAG> __global__ __launch_bounds__(256) void k_c1(KParams P)
{
    const int *w = reinterpret_cast<const int *>(&P);
    constexpr int off[8] = OFFS8(P);
    int v = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) v += w[off[i]];
    if (int(blockIdx.x) + v >= P.k[0].tiles_b + P.k[1].tiles_b) return;
    if (P.lm_in->done) return;
    *P.ticket = 1u;
}
template <int TAG> __global__ __launch_bounds__(256) void k_d_b(const KParams *__restrict__ R, SCAL32) { if (R->pre_tiles == 0x7fffffff) *R->ticket = unsigned(tag) + unsigned(seq) + unsigned(publish + pad); }
template <int TAG> __global__ __launch_bounds__(256) void k_d_c(const KParams *__restrict__ R, SCAL32)
{
    if (int(blockIdx.x) >= R->k[0].tiles_b + R->k[1].tiles_b) return;
    if (R->lm_in->done) return;
    *R->ticket = unsigned(tag) + unsigned(seq) + unsigned(publish + pad);
}
template <int TAG> __global__ __launch_bounds__(256) void k_d_s(const KParams *__restrict__ R, SCAL32)
{
    if (int(blockIdx.x) >= slot) return;       // (slot = the grid)
    if (*done) return;
    *R->ticket = unsigned(tag) + unsigned(seq) + unsigned(publish + pad);
}
template <int TAG> __global__ __launch_bounds__(256) void k_d_L(const KParams *__restrict__ R, SCAL32, Poses ps)
{
    if (int(blockIdx.x) >= slot) return;
    if (*done) return;
    *R->ticket = unsigned(ps.a[0] + ps.b[1] + ps.c[2]);
}

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

// holds the stream for ~ms so that the host is a whole chain ahead when the chain's first launch starts (bounded: leaves after `ticks` of the 100 MHz clock)
__global__ void k_hold(unsigned long long ticks) { const unsigned long long t0 = wall_clock64(); while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32); }
static bool g_graph = true;

template <typename F>
static int time_chain(const char *name, int wgs, hipStream_t st, int reps, F launch)
{
    constexpr int CH = 200;
    for (int i = 0; i < CH; ++i) launch();
    CK(hipStreamSynchronize(st));
    double t0 = now();
    for (int r = 0; r < reps; ++r) for (int i = 0; i < CH; ++i) launch();
    CK(hipStreamSynchronize(st));
    const double t_stream = (now() - t0) / (double(reps) * CH);
    // the same stream launches with the host ahead: the chain is enqueued while a holding kernel occupies the stream, and timed by events around it
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    double t_ahead = 0.0;
    const int areps = reps < 10 ? reps : 10;
    for (int r = 0; r < areps; ++r) {
        hipLaunchKernelGGL(k_hold, dim3(1), dim3(64), 0, st, 300000ull);       // 3 ms
        CK(hipEventRecord(e0, st));
        for (int i = 0; i < CH; ++i) launch();
        CK(hipEventRecord(e1, st));
        CK(hipStreamSynchronize(st));
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, e0, e1));
        t_ahead += double(ms) * 1e-3 / CH;
    }
    t_ahead /= areps;
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
    double t_graph = 0.0;
    if (g_graph) {
        hipGraph_t g; hipGraphExec_t ge;
        CK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        for (int i = 0; i < CH; ++i) launch();
        CK(hipStreamEndCapture(st, &g));
        CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        for (int r = 0; r < 3; ++r) CK(hipGraphLaunch(ge, st));
        CK(hipStreamSynchronize(st));
        t0 = now();
        for (int r = 0; r < reps; ++r) CK(hipGraphLaunch(ge, st));
        CK(hipStreamSynchronize(st));
        t_graph = (now() - t0) / (double(reps) * CH);
        CK(hipGraphExecDestroy(ge)); CK(hipGraphDestroy(g));
    }
    std::printf("%-5s grid %4d: period per launch, chain of %d: stream %.2f us, stream with the host ahead %.2f us, graph replay %.2f us\n", name, wgs, CH, 1e6 * t_stream, 1e6 * t_ahead,
                1e6 * t_graph);
    return 0;
}

template <int TAG>
static int run_grid(hipStream_t st, int reps, const KParams &P0, const KParams *dP, const int *d_done)
{
    KParams P = P0;
    P.k[0].tiles_b = TAG - TAG / 3; P.k[1].tiles_b = TAG / 3;
    KParams *dR = const_cast<KParams *>(dP) + (TAG == 88 ? 0 : 1);
    CK(hipMemcpy(dR, &P, sizeof(P), hipMemcpyHostToDevice));
    Scal32 s{d_done, 7ull, TAG, 0, 3, 0};
    Poses ps;
    std::memset(&ps, 0, sizeof(ps));
    const dim3 g(TAG), b(256);
#ifndef PRELOAD
    if (time_chain("a", TAG, st, reps, [&] { hipLaunchKernelGGL(k_a<TAG>, g, b, 0, st); })) return 1;
    if (time_chain("b", TAG, st, reps, [&] { hipLaunchKernelGGL(k_b<TAG>, g, b, 0, st, P); })) return 1;
    if (time_chain("c", TAG, st, reps, [&] { hipLaunchKernelGGL(k_c<TAG>, g, b, 0, st, P); })) return 1;
    if (time_chain("c8", TAG, st, reps, [&] { hipLaunchKernelGGL(k_c8<TAG>, g, b, 0, st, P); })) return 1;
    if (time_chain("c1", TAG, st, reps, [&] { hipLaunchKernelGGL(k_c1<TAG>, g, b, 0, st, P); })) return 1;
#endif
    if (time_chain("d_b", TAG, st, reps, [&] { hipLaunchKernelGGL(k_d_b<TAG>, g, b, 0, st, dR, s.done, s.seq, s.slot, s.publish, s.tag, s.pad); })) return 1;
    if (time_chain("d_c", TAG, st, reps, [&] { hipLaunchKernelGGL(k_d_c<TAG>, g, b, 0, st, dR, s.done, s.seq, s.slot, s.publish, s.tag, s.pad); })) return 1;
    if (time_chain("d_s", TAG, st, reps, [&] { hipLaunchKernelGGL(k_d_s<TAG>, g, b, 0, st, dR, s.done, s.seq, s.slot, s.publish, s.tag, s.pad); })) return 1;
    if (time_chain("d_L", TAG, st, reps, [&] { hipLaunchKernelGGL(k_d_L<TAG>, g, b, 0, st, dR, s.done, s.seq, s.slot, s.publish, s.tag, s.pad, ps); })) return 1;
    return 0;
}

int main(int argc, char **argv)
{
    const int reps = argc > 1 ? std::atoi(argv[1]) : 50;
    g_graph = !(argc > 2 && std::strcmp(argv[2], "nograph") == 0);      // (graph replay 0.00 = not run)
    hipStream_t st;
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    LmState *d_lm = nullptr;
    unsigned *d_ticket = nullptr;
    KParams *dP = nullptr;
    CK(hipMalloc(&d_lm, sizeof(LmState)));
    CK(hipMalloc(&d_ticket, 64));
    CK(hipMalloc(&dP, 2 * sizeof(KParams)));
    LmState h;
    std::memset(&h, 0, sizeof(h));
    h.done = 1;
    CK(hipMemcpy(d_lm, &h, sizeof(h), hipMemcpyHostToDevice));
    CK(hipMemset(d_ticket, 0, 64));
    KParams P;
    std::memset(&P, 0, sizeof(P));
    P.lm_in = d_lm;
    P.ticket = d_ticket;
    const char *env = std::getenv("HIP_FORCE_DEV_KERNARG");
#ifdef PRELOAD
    std::printf("sizeof(KParams) = %zu, kernarg preload build, HIP_FORCE_DEV_KERNARG=%s\n", sizeof(KParams), env ? env : "(unset)");
#else
    std::printf("sizeof(KParams) = %zu, HIP_FORCE_DEV_KERNARG=%s\n", sizeof(KParams), env ? env : "(unset)");
#endif
    if (run_grid<88>(st, reps, P, dP, &d_lm->done)) return 1;
    if (run_grid<1016>(st, reps, P, dP, &d_lm->done)) return 1;
    CK(hipStreamSynchronize(st));
    return 0;
}
