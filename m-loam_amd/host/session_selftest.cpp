// The session image through the facade (SessionImage, saveSession / loadSession, PoseGraph::savePoseGraph / loadPoseGraph, SCManager::rebuildFromKeyframes,
// KeyframePolicy::restore): a context with 12 keyframes (outlier clouds attached late on some), a place index built in one batch and a pose graph with two loop
// edges is saved to a file, loaded into a second context and must then export the same bytes, answer a loop query and an optimisation with the same bits, and
// leave the mapper's keyframe policy where 12 saves would have; a damaged file must be refused and change nothing; the place index rebuilt under another grid
// must equal the one a third context builds keyframe by keyframe.
// Usage: session_selftest  (exit status 0 = pass)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "mloam_facade.hpp"

using namespace mloam_hip;

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

struct P4 { float x, y, z, lidar; };

std::vector<P4> cloud(std::mt19937 &rng, int n)
{
    std::uniform_real_distribution<float> u(-60.f, 60.f), h(-2.f, 8.f);
    std::vector<P4> c;
    for (int i = 0; i < n; ++i) c.push_back(P4{u(rng), u(rng), h(rng), float(i % 2)});
    return c;
}

}  // namespace

int main()
{
    const int K = 12;
    std::mt19937 rng(11);
    Device dev_a(0), dev_b(0), dev_c(0);
    std::vector<std::vector<P4>> surf, corner, outlier;
    std::vector<Pose> poses;
    KeyframePolicy policy_a(0.5f, 5.f, 50.f), policy_b(0.5f, 5.f, 50.f);
    double cov[36] = {0};
    for (int d = 0; d < 6; ++d) cov[7 * d] = 1e-4;
    for (int i = 0; i < K; ++i) {
        surf.push_back(cloud(rng, 200 + 57 * i)); corner.push_back(cloud(rng, i == 3 ? 0 : 256)); outlier.push_back(cloud(rng, i % 3 == 1 ? 90 + i : 0));
        Pose p;
        p.t_(0) = 2.0 * i; p.t_(1) = 0.3 * i; p.t_(2) = 0.05; p.q_.z = std::sin(0.02 * i); p.q_.w = std::cos(0.02 * i);
        poses.push_back(p);
        double pp[7];
        p.toParam(pp);
        for (Device *d : {&dev_a, &dev_c}) {
            int32_t key = -1;
            d->check(mlh_keyframe_save(d->ctx(), pp, cov, surf[i].data(), int(surf[i].size()), corner[i].data(), int(corner[i].size()), 16, 12, MLH_MEM_HOST, &key));
            EXPECT(key == i);
        }
        EXPECT(policy_a.save(p) == i);
    }
    for (int i = 0; i < K; ++i)
        if (!outlier[i].empty())
            for (Device *d : {&dev_a, &dev_c}) d->check(mlh_keyframe_attach_outlier(d->ctx(), i, outlier[i].data(), int(outlier[i].size()), 16, 12, MLH_MEM_HOST));
    SCManager sc_a(dev_a);
    sc_a.setParameter(2.0, 20, 60, 80.0, 6.0, 4.0, 2, 4, 0.1, 0.5, 3, -1.0);
    EXPECT(sc_a.rebuildFromKeyframes(0, K) == 0 && int(sc_a.getDataBaseSize()) == K);
    sc_a.detectLoopClosureID(7);
    PoseGraph<Pose> pg_a(dev_a);
    for (int i = 0; i < K; ++i) EXPECT(pg_a.addKeyFrame(poses[i]) == i);
    Pose rel;
    rel.t_(0) = 0.1;
    pg_a.updateLoopInfo(8, 2, rel);
    pg_a.updateLoopInfo(11, 4, rel);

    // save, through a file, load
    const char *tmp = std::getenv("TMPDIR");
    const std::string path = std::string(tmp && *tmp ? tmp : "/tmp") + "/mloam_session_selftest_" + std::to_string(long(std::random_device{}())) + ".img";
    const SessionImage image = saveSession(dev_a);
    mlh_session_info info, ex;
    dev_a.check(mlh_session_last_info(dev_a.ctx(), &ex));
    EXPECT(ex.host_waits == 1);
    EXPECT(image.inspect(info) && info.sections == 7u && info.count[0] == K && info.count[2] == K && info.count[3] == K && info.total_bytes == int64_t(image.bytes.size()));
    EXPECT(image.save(path));
    SessionImage loaded;
    EXPECT(loaded.load(path) && loaded.bytes == image.bytes);
    const mlh_session_info got = loadSession(dev_b, loaded, MLH_SESSION_KEYFRAMES | MLH_SESSION_SC | MLH_SESSION_PG, &policy_b);
    EXPECT(got.host_waits == 1 && got.count[1] == info.count[1]);
    EXPECT(saveSession(dev_b).bytes == image.bytes);
    // the keyframe policy stands where K saves left it
    EXPECT(policy_b.pose_keyframes_3d.size() == size_t(K) && policy_b.pose_keyframes_6d.size() == size_t(K));
    Pose probe = poses[K - 1];
    probe.t_(0) += 0.3;
    EXPECT(policy_a.wouldSave(probe) == policy_b.wouldSave(probe) && !policy_b.wouldSave(probe));
    probe.t_(0) += 0.3;
    EXPECT(policy_a.wouldSave(probe) && policy_b.wouldSave(probe) && policy_a.surrounding(probe) == policy_b.surrounding(probe));
    // the same answers
    SCManager sc_b(dev_b);                                   // (no setParameter: the image brought the options)
    for (int que : {9, 11, 10, 11}) {
        const QueryResult qa = sc_a.detectLoopClosureID(que), qb = sc_b.detectLoopClosureID(que);
        EXPECT(qa.match_index_ == qb.match_index_ && qa.score_ == qb.score_ && qa.yaw_diff_rad_ == qb.yaw_diff_rad_);
    }
    mlh_pg_result ra, rb;
    dev_a.check(mlh_pg_optimize(dev_a.ctx(), K - 1, nullptr, &ra));
    dev_b.check(mlh_pg_optimize(dev_b.ctx(), K - 1, nullptr, &rb));
    std::vector<double> pa(7 * K), pb(7 * K);
    dev_a.check(mlh_pg_poses(dev_a.ctx(), 0, K, pa.data(), nullptr));
    dev_b.check(mlh_pg_poses(dev_b.ctx(), 0, K, pb.data(), nullptr));
    EXPECT(ra.final_cost == rb.final_cost && ra.num_iterations == rb.num_iterations && !std::memcmp(pa.data(), pb.data(), sizeof(double) * pa.size()));
    // a damaged file: refused, nothing changed
    const std::vector<unsigned char> before = saveSession(dev_b).bytes;
    SessionImage bad = image;
    bad.bytes[bad.bytes.size() / 2] ^= 0x20;
    bool threw = false;
    try { loadSession(dev_b, bad); } catch (const Error &) { threw = true; }
    EXPECT(threw && !bad.inspect(info) && saveSession(dev_b).bytes == before);
    // savePoseGraph / loadPoseGraph with the reference's names: the pose graph alone
    PoseGraph<Pose> pg_c(dev_c);
    EXPECT(pg_a.savePoseGraph(path) && pg_c.loadPoseGraph(path) && pg_c.getKeyFrameSize() == K && pg_c.earliestLoopIndex() == 2);
    EXPECT(saveSession(dev_c, MLH_SESSION_PG).bytes == saveSession(dev_a, MLH_SESSION_PG).bytes);
    EXPECT(!pg_c.loadPoseGraph(path + ".none"));
    std::remove(path.c_str());
    // the place index rebuilt under another grid in one batch = keyframe by keyframe
    SCManager sc_b8(dev_b), sc_c8(dev_c);
    sc_b8.setParameter(1.0, 8, 12, 40.0, 30.0, 5.0, 2, 4, 0.1, 0.5, 3, -1.0);
    sc_c8.setParameter(1.0, 8, 12, 40.0, 30.0, 5.0, 2, 4, 0.1, 0.5, 3, -1.0);
    EXPECT(sc_b8.rebuildFromKeyframes(0, K) == 0);
    for (int i = 0; i < K; ++i) EXPECT(sc_c8.makeAndSaveScancontextAndKeysFromKeyframe(i) == i);
    for (int i = 0; i < K; ++i) EXPECT(sc_b8.fetchScanContext(i) == sc_c8.fetchScanContext(i));
    std::printf("session_selftest: %d keyframes, %lld points, image of %lld bytes, export %d launches / %d waits, import %d / %d: %s\n", K, (long long)got.count[1],
                (long long)got.total_bytes, ex.launches, ex.host_waits, got.launches, got.host_waits, fails ? "FAILED" : "ok");
    return fails ? 1 : 0;
}
