// InitialExtrinsics through the facade (the initial extrinsic calibration on the device, include/mloam_hip.h (f16)) over a motion sequence read from a file of
// doubles: n_lidar, idx_ref, planar_movement, n_frames, then n_frames x n_lidar poses [t, q(xyzw)].
//   initext_selftest callsite <file>     the block of estimator.cpp:437-467 as the reference writes it: addPose, cov_rot_state_, calibExRotation, calibExTranslation
//   initext_selftest step <file>         the same block as ONE fused call per frame (InitialExtrinsics::step); must print the same lines
//   initext_selftest cpu <file> <reps>   no device: the same arithmetic as a plain single-threaded loop over csrc/initext_host.hpp (the bookkeeping, the block, the
//                                        host Jacobi of csrc/svd_dev.hpp), every frame calibrated for every LiDAR; the last frame's rotation + translation solve
//                                        repeated <reps> times and timed (scripts/iebench.py's CPU leg)
// Lines: "A <frame> <accepted>"; "R <frame> <lidar> <converged> <rot_cov>" per rotation stage that ran; "T <frame> <lidar> qx qy qz qw tx ty tz" per extrinsic
// obtained; "E <full_cov_rot_state_> <full_cov_pos_state_>"; cpu: "C <lidar> <sigma x 4> <q x 4> <t x 3>" for the last frame and "U <microseconds> ..." per repetition.
// Exit status 0 = ran.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mloam_facade.hpp"
#include "../csrc/initext_host.hpp"

using namespace mloam_hip;

namespace {

struct Sequence {
    int n_lidar = 0, idx_ref = 0, planar = 0, n_frames = 0;
    std::vector<double> poses;
};

bool read_sequence(const char *path, Sequence &s)
{
    FILE *f = std::fopen(path, "rb");
    double h[4];
    if (!f || std::fread(h, sizeof(double), 4, f) != 4) return false;
    s.n_lidar = int(h[0]); s.idx_ref = int(h[1]); s.planar = int(h[2]); s.n_frames = int(h[3]);
    if (s.n_lidar < 1 || s.n_lidar > MLH_INITEXT_MAX_LIDAR || s.n_frames < 0 || s.n_frames > 100000) { std::fclose(f); return false; }
    s.poses.resize(size_t(s.n_frames) * size_t(s.n_lidar) * 7);
    const bool ok = std::fread(s.poses.data(), sizeof(double), s.poses.size(), f) == s.poses.size();
    std::fclose(f);
    return ok;
}

void print_ext(int frame, size_t n, const Pose &p)
{
    std::printf("T %d %zu %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", frame, n, p.q_.x, p.q_.y, p.q_.z, p.q_.w, p.t_(0), p.t_(1), p.t_(2));
}

int run_device(const Sequence &s, bool fused)
{
    Device dev(0);
    InitialExtrinsics<Pose> initial_extrinsics_(dev);
    initial_extrinsics_.options().n_lidar = s.n_lidar; initial_extrinsics_.options().idx_ref = s.idx_ref; initial_extrinsics_.options().planar_movement = s.planar;
    initial_extrinsics_.clearState();
    initial_extrinsics_.setParameter();
    const size_t NUM_OF_LASER = size_t(s.n_lidar), IDX_REF = size_t(s.idx_ref);
    const int WINDOW_SIZE = initial_extrinsics_.options().window_size, cir_buf_cnt_ = WINDOW_SIZE;
    std::vector<Pose> pose_rlt_(NUM_OF_LASER), ext(NUM_OF_LASER);
    for (int k = 0; k < s.n_frames; ++k) {
        for (size_t n = 0; n < NUM_OF_LASER; ++n) pose_rlt_[n].fromParam(s.poses.data() + (size_t(k) * NUM_OF_LASER + n) * 7);
        std::vector<size_t> cov_before(NUM_OF_LASER);
        for (size_t n = 0; n < NUM_OF_LASER; ++n) cov_before[n] = initial_extrinsics_.v_rot_cov_[n].size();
        bool accepted = false;
        std::vector<size_t> solved;
        if (fused) {
            solved = initial_extrinsics_.step(pose_rlt_, cir_buf_cnt_ == WINDOW_SIZE, &accepted);
        } else if (initial_extrinsics_.addPose(pose_rlt_) && (cir_buf_cnt_ == WINDOW_SIZE)) {
            accepted = true;
            for (size_t n = 0; n < NUM_OF_LASER; n++)
            {
                if (initial_extrinsics_.cov_rot_state_[n]) continue;
                Pose calib_result;
                if (initial_extrinsics_.calibExRotation(IDX_REF, n, calib_result))
                {
                    if (initial_extrinsics_.calibExTranslation(IDX_REF, n, calib_result))
                    {
                        ext[n] = calib_result;
                        solved.push_back(n);
                    }
                }
            }
        }
        std::printf("A %d %d\n", k, accepted ? 1 : 0);
        for (size_t n = 0; n < NUM_OF_LASER; ++n)
            if (initial_extrinsics_.v_rot_cov_[n].size() > cov_before[n])
                std::printf("R %d %zu %d %.17g\n", k, n, initial_extrinsics_.cov_rot_state_[n] ? 1 : 0, initial_extrinsics_.v_rot_cov_[n].back());
        for (size_t n : solved) print_ext(k, n, fused ? initial_extrinsics_.calib_ext_[n] : ext[n]);
        if ((initial_extrinsics_.full_cov_rot_state_) && (initial_extrinsics_.full_cov_pos_state_)) initial_extrinsics_.saveStatistics();
    }
    std::printf("E %d %d\n", initial_extrinsics_.full_cov_rot_state_ ? 1 : 0, initial_extrinsics_.full_cov_pos_state_ ? 1 : 0);
    return 0;
}

int run_cpu(const Sequence &s, int reps)
{
    using namespace mlh;
    mlh_initext_opts o;
    ie_opts_defaults(o);
    o.n_lidar = s.n_lidar; o.idx_ref = s.idx_ref; o.planar_movement = s.planar;
    IeBook B;
    B.reset(o);
    const size_t nl = size_t(s.n_lidar);
    std::vector<double> Q(nl * IE_Q_ROWS * 4, 0.0), sets(size_t(IE_N_POSE) * nl * 7, 0.0);
    std::vector<IeHostSolve> last(nl);
    const auto calibrate = [&](int l, IeHostSolve &S) {
        std::memset(&S, 0, sizeof(S));
        double *Ql = Q.data() + size_t(l) * IE_Q_ROWS * 4, *ext = B.calib_ext + 7 * l;
        ie_rot_block(B.add_poses + 7 * o.idx_ref, B.add_poses + 7 * l, ext, Ql + size_t(B.add_first) * 16);
        ie_host_rotation(Ql, B.rot_cov_thre, S);
        ext[3] = S.q[0]; ext[4] = S.q[1]; ext[5] = S.q[2]; ext[6] = S.q[3];
        if (S.rot_converged) {
            const double q[4] = {S.q[0], S.q[1], S.q[2], S.q[3]};
            ie_host_translation(sets.data(), int(B.n_sets), s.n_lidar, o.idx_ref, l, s.planar, q, S);
            ext[0] = S.t[0]; ext[1] = S.t[1]; ext[2] = S.t[2]; ext[3] = S.q[0]; ext[4] = S.q[1]; ext[5] = S.q[2]; ext[6] = S.q[3];
        }
    };
    for (int k = 0; k < s.n_frames; ++k) {
        const double *p = s.poses.data() + size_t(k) * nl * 7;
        if (!B.screw_ok(p)) continue;
        const size_t slot = B.accept(p);
        std::memcpy(sets.data() + slot * nl * 7, p, sizeof(double) * nl * 7);
        if (!B.window_full()) continue;
        for (int l = 0; l < s.n_lidar; ++l)
            if (l != o.idx_ref) calibrate(l, last[size_t(l)]);
    }
    if (B.add_first < 0 || !B.window_full()) return 3;
    for (int l = 0; l < s.n_lidar; ++l)
        if (l != o.idx_ref) {
            const IeHostSolve &S = last[size_t(l)];
            std::printf("C %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", l, S.rot_sv[0], S.rot_sv[1], S.rot_sv[2], S.rot_sv[3], S.q[0], S.q[1],
                        S.q[2], S.q[3], S.t[0], S.t[1], S.t[2]);
        }
    std::printf("U");
    for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int l = 0; l < s.n_lidar; ++l)
            if (l != o.idx_ref) { IeHostSolve S; calibrate(l, S); }
        std::printf(" %.3f", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    std::printf("\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    Sequence s;
    if (argc < 3 || !read_sequence(argv[2], s)) { std::printf("usage: initext_selftest callsite|step|cpu <file> [reps]\n"); return 2; }
    int rc = 2;
    try {
        if (std::strcmp(argv[1], "callsite") == 0) rc = run_device(s, false);
        else if (std::strcmp(argv[1], "step") == 0) rc = run_device(s, true);
        else if (std::strcmp(argv[1], "cpu") == 0) rc = run_cpu(s, argc > 3 ? std::atoi(argv[3]) : 1);
    } catch (const std::exception &e) {
        std::printf("initext_selftest: %s\n", e.what());
        return 1;
    }
    if (rc == 0) std::printf("initext_selftest: ok\n");
    return rc;
}
