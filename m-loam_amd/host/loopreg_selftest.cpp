// PoseGraph::checkGeometricConsistency's device steps through the facade (LoopLocalMap::constructLocalMap, LoopRegistration::performLocalRegistration) on a scene
// of a floor, two walls and six poles driven twice -- the second pass displaced by 25 degrees of yaw and (0.6, -0.4, 0.1) m, its stored poses drifted -- with a
// gap of missing keyframe indices between the passes:
//   - the facade chooses the keyframes of cpp:374-410 (windows clipped at 0 and at que_index, missing indices skipped);
//   - its clouds equal the clouds of a plain mlh_loop_build_clouds call with hand-made lists on a second context, record for record;
//   - registering the clouds left on the device and registering the same clouds fetched to the host and handed back (the reference's signature shape) give the
//     same bits, the transform that made the scene within 5 cm, accepted;
//   - a start 30 m above the scene matches nothing: T_ini comes back bit for bit with cost 1e7, not accepted.
// Usage: loopreg_selftest  (exit status 0 = pass)
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "mloam_facade.hpp"

using namespace mloam_hip;

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

Mat4 yaw_T(double deg, double x, double y, double z)
{
    const double c = std::cos(deg * M_PI / 180.0), s = std::sin(deg * M_PI / 180.0);
    return Mat4{c, -s, 0, x, s, c, 0, y, 0, 0, 1, z, 0, 0, 0, 1};
}
Mat4 mul(const Mat4 &A, const Mat4 &B) { Mat4 C; mlh::loop_mat_mul(A.data(), B.data(), C.data()); return C; }
Mat4 inv(const Mat4 &A) { Mat4 C; mlh::loop_rigid_inverse(A.data(), C.data()); return C; }

const double POLES[6][2] = {{-5.0, -5.0}, {-2.0, 5.5}, {3.0, -6.0}, {6.0, 4.0}, {9.5, -3.0}, {10.0, 6.5}};

// the world seen from keyframe pose T (floor z = 0, wall y = 8, wall x = 12, the poles), 0.02 m jitter, in the keyframe's frame
void sample(std::mt19937 &rng, const Mat4 &T, int n_surf, int n_corner, PointICloud &surf, PointICloud &corner)
{
    std::uniform_real_distribution<double> ux(-8.0, 12.0), uy(-8.0, 8.0), uh(0.0, 3.0), u01(0.0, 1.0);
    std::normal_distribution<double> g(0.0, 0.02);
    const Mat4 Ti = inv(T);
    const auto put = [&](PointICloud &c, double x, double y, double z) {
        x += g(rng); y += g(rng); z += g(rng);
        PointI p;
        p.x = float(Ti[0] * x + Ti[1] * y + Ti[2] * z + Ti[3]); p.y = float(Ti[4] * x + Ti[5] * y + Ti[6] * z + Ti[7]); p.z = float(Ti[8] * x + Ti[9] * y + Ti[10] * z + Ti[11]);
        p.intensity = 0.f;
        c.push_back(p);
    };
    for (int i = 0; i < n_surf; ++i) {
        const double r = u01(rng);
        if (r < 0.6) put(surf, ux(rng), uy(rng), 0.0);
        else if (r < 0.8) put(surf, ux(rng), 8.0, uh(rng));
        else put(surf, 12.0, uy(rng), uh(rng));
    }
    for (int i = 0; i < n_corner; ++i) { const int k = int(rng() % 6u); put(corner, POLES[k][0], POLES[k][1], uh(rng)); }
}

void to_pose(const Mat4 &T, double pose[7]) { mlh::loop_pose_of(T.data(), pose); }

bool same_cloud(Device &a, int which, Device &b, bool filtered)
{
    const void *pa = nullptr, *pb = nullptr;
    int32_t na = 0, nb = 0;
    a.check(mlh_loop_cloud(a.ctx(), which, filtered, &pa, &na));
    b.check(mlh_loop_cloud(b.ctx(), which, filtered, &pb, &nb));
    if (na != nb) return false;
    if (na == 0) return true;
    a.check(mlh_synchronize(a.ctx())); b.check(mlh_synchronize(b.ctx()));
    std::vector<float> ha(size_t(na) * 4), hb(size_t(nb) * 4);
    if (hipMemcpy(ha.data(), pa, ha.size() * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hb.data(), pb, hb.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
    return std::memcmp(ha.data(), hb.data(), ha.size() * 4) == 0;
}

}  // namespace

int main()
{
    std::mt19937 rng(5);
    const Mat4 truth = yaw_T(25.0, 0.6, -0.4, 0.1), drift = yaw_T(3.0, 1.5, -2.0, 0.3);
    Device dev_a(0), dev_b(0);
    std::map<int, LoopLocalMap::Keyframe> kfs;
    std::vector<PointICloud> surf(10), corner(10);
    std::vector<Mat4> stored(10);
    for (int k = 0; k < 10; ++k) {
        const Mat4 base = yaw_T(0.0, double(k % 5), 0.0, 1.0);
        const Mat4 T = k < 5 ? base : mul(base, truth);
        stored[size_t(k)] = k < 5 ? T : mul(drift, T);
        sample(rng, T, 300 + int(rng() % 301u), 40 + int(rng() % 41u), surf[size_t(k)], corner[size_t(k)]);
        double pose[7], cov[36] = {0};
        to_pose(stored[size_t(k)], pose);
        for (Device *d : {&dev_a, &dev_b}) {
            int32_t key = -1;
            d->check(mlh_keyframe_save(d->ctx(), pose, cov, surf[size_t(k)].points.data(), int(surf[size_t(k)].size()), corner[size_t(k)].points.data(),
                                       int(corner[size_t(k)].size()), int(sizeof(PointI)), int(offsetof(PointI, intensity)), MLH_MEM_HOST, &key));
            EXPECT(key == k);
        }
        // the first pass is keyframes 0..4, the second 100..104: the indices in between are missing keyframes
        kfs[k < 5 ? k : 95 + k] = LoopLocalMap::Keyframe{k, stored[size_t(k)]};
    }
    const int que_index = 102, match_index = 2;
    const Mat4 pose_ini = yaw_T(0.0, 0.0, 0.0, 0.0);

    LoopLocalMap lmap(dev_a);
    lmap.options().history_search_num = 3;
    lmap.constructLocalMap(que_index, match_index, pose_ini, kfs);
    EXPECT((lmap.dataKeyframes() == std::vector<int>{100, 101, 102}));           // 99 is missing; nothing beyond the query
    EXPECT((lmap.modelKeyframes() == std::vector<int>{0, 1, 2, 3, 4}));          // -1 is clipped, 5 is missing
    // the same lists by hand, on the second context
    {
        const int dk_idx[3] = {100, 101, 102}, mk_idx[5] = {0, 1, 2, 3, 4};
        std::vector<int32_t> dk, mk;
        std::vector<float> dT(16 * 3), mT(16 * 5);
        for (int e = 0; e < 3; ++e) {
            dk.push_back(kfs.at(dk_idx[e]).key);
            const Mat4 M = mul(pose_ini, mul(inv(kfs.at(que_index).T), kfs.at(dk_idx[e]).T));
            for (int i = 0; i < 16; ++i) dT[size_t(16 * e + i)] = float(M[size_t(i)]);
        }
        for (int e = 0; e < 5; ++e) {
            mk.push_back(kfs.at(mk_idx[e]).key);
            const Mat4 M = mul(inv(kfs.at(match_index).T), kfs.at(mk_idx[e]).T);
            for (int i = 0; i < 16; ++i) mT[size_t(16 * e + i)] = float(M[size_t(i)]);
        }
        int32_t n_pre[4], n_ds[4];
        dev_b.check(mlh_loop_build_clouds(dev_b.ctx(), dk.data(), dT.data(), 3, mk.data(), mT.data(), 5, nullptr, n_pre, n_ds));
        for (int c = 0; c < 4; ++c) {
            EXPECT(size_t(n_pre[c]) == lmap.size(c, false) && size_t(n_ds[c]) == lmap.size(c, true) && n_ds[c] > 0 && n_ds[c] <= n_pre[c]);
            EXPECT(same_cloud(dev_a, c, dev_b, false));
            EXPECT(same_cloud(dev_a, c, dev_b, true));
        }
    }
    // registration: the device clouds, and the same clouds through the host (the reference's signature shape)
    const Mat4 T_ini = yaw_T(24.0, 0.0, 0.0, 0.0);           // the Scan Context yaw on the 6-degree grid, zero translation
    LoopRegistration reg_a(dev_a), reg_b(dev_b);
    const std::pair<bool, Mat4> ra = reg_a.performLocalRegistration(T_ini);
    const auto copy = [](void *dst, const void *src, size_t bytes) { if (hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) throw Error("hipMemcpy"); };
    PointICloud c4[4];
    for (int c = 0; c < 4; ++c) lmap.fetchCloud(c, c4[c], copy);
    const std::pair<bool, Mat4> rb = reg_b.performLocalRegistration(&c4[0], &c4[1], &c4[2], &c4[3], T_ini);
    EXPECT(ra.first && rb.first);
    EXPECT(std::memcmp(ra.second.data(), rb.second.data(), sizeof(double) * 16) == 0);
    EXPECT(reg_a.lastResult().opti_cost == reg_b.lastResult().opti_cost && reg_a.lastResult().n_outer == 2);
    double worst = 0.0;
    for (int i = 0; i < 16; ++i) worst = std::max(worst, std::fabs(ra.second[size_t(i)] - truth[size_t(i)]));
    std::printf("loopreg_selftest: |T - truth| = %.4f, cost %.4f, surf %d corner %d\n", worst, reg_a.lastResult().opti_cost, reg_a.lastResult().outer[1].surf_num,
                reg_a.lastResult().outer[1].corner_num);
    EXPECT(worst < 0.05);
    // a start that matches nothing
    const Mat4 T_far = yaw_T(24.0, 0.0, 0.0, 30.0);
    const std::pair<bool, Mat4> rf = reg_a.performLocalRegistration(T_far);
    EXPECT(!rf.first && std::memcmp(rf.second.data(), T_far.data(), sizeof(double) * 16) == 0);
    EXPECT(reg_a.lastResult().opti_cost == 1e7 && reg_a.lastResult().n_outer == 1 && reg_a.lastResult().outer[0].ran == 0);

    std::printf(fails ? "loopreg_selftest: %d FAILED\n" : "loopreg_selftest: ok\n", fails);
    return fails ? 1 : 0;
}
