// Loop-corrected poses applied to the mapper's keyframe store (keyframes.hip; include/mloam_hip.h section (f15)): the host arithmetic and bookkeeping of
// mlh_keyframes_update_poses, written once -- for the library and for a stand-alone host program that runs it under a sanitizer (tests/host/kf_update_host_main.cpp).
// The reference has nothing here: updateKeyframe() (estimator/src/lidarMapper/lidar_mapper_keyframe.cpp:685-688) is a stub under "TODO: using loop info to update
// keyframes". Every rule below is CHOSEN (the header's section lists them); the one line taken from the reference is the drift of optimizePoseGraph
// (mloam_loop/src/pose_graph.cpp:630-641: pose_drift = cur * last^-1, left-multiplied onto every later keyframe), through pg_pose_mul / pg_pose_inverse of pg_host.hpp.
// The store's types are template parameters (a key has pose[7], cov[36], pos[3]; a cache entry has id and slot), so this header needs neither ctx.hpp nor HIP.
// Translation units that include this header are compiled with -ffp-contract=off (pg_host.hpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "pg_host.hpp"

namespace mlh {

// the argument at fault, or nullptr: n > 0, poses given, first_key .. first_key + n - 1 inside the store, every pose finite (what bad_pose refuses at save time),
// every covariance entry finite when covariances are given
inline const char *kf_update_fault(size_t n_keys, int32_t first_key, int32_t n, const double *poses, const double *covs)
{
    if (n <= 0) return "n must be > 0";
    if (!poses) return "null poses";
    if (first_key < 0 || size_t(first_key) + size_t(n) > n_keys) return "the range lies outside the store";
    for (size_t i = 0; i < 7 * size_t(n); ++i) if (!std::isfinite(poses[i])) return "non-finite pose";
    if (covs) for (size_t i = 0; i < 36 * size_t(n); ++i) if (!std::isfinite(covs[i])) return "non-finite covariance";
    return nullptr;
}

// "changed" is a statement about bits: -0.0 against 0.0 is a change, the same NaN-free doubles are not (mlh_pg_optimize leaves keyframes before `first` bit-identical)
inline bool kf_bits_differ(const double *a, const double *b, int n) { return std::memcmp(a, b, sizeof(double) * size_t(n)) != 0; }

// drift = new_last * old_last^-1 (pose_graph.cpp:630-633)
inline void kf_drift(const double new_last[7], const double old_last[7], double drift[7])
{
    double inv[7];
    pg_pose_inverse(old_last, inv);
    pg_pose_mul(new_last, inv, drift);
}

// The update on validated arguments (kf_update_fault == nullptr). Keys first_key .. first_key + n - 1 take the given pose (and covariance, when given) and
// pos = float(t); changed[k] <- 1 where any bit of them differed. With drift_tail and a changed LAST key of the range, drift = new(last) * old(last)^-1 goes onto
// every key beyond the range (pose <- drift * pose, pos = float(t); each counts as changed); otherwise drift is the identity. Returns the number of changed keys.
template <class Key>
int kf_update_apply(std::vector<Key> &keys, int32_t first_key, int32_t n, const double *poses, const double *covs, int drift_tail, std::vector<char> &changed,
                    double drift[7])
{
    changed.assign(keys.size(), 0);
    for (int c = 0; c < 7; ++c) drift[c] = c == 6 ? 1.0 : 0.0;
    const size_t last = size_t(first_key) + size_t(n) - 1;
    double old_last[7];
    std::memcpy(old_last, keys[last].pose, sizeof(old_last));
    int n_changed = 0;
    for (int32_t i = 0; i < n; ++i) {
        Key &key = keys[size_t(first_key) + size_t(i)];
        const double *p = poses + 7 * size_t(i), *c = covs ? covs + 36 * size_t(i) : nullptr;
        if (!kf_bits_differ(key.pose, p, 7) && !(c && kf_bits_differ(key.cov, c, 36))) continue;
        std::memcpy(key.pose, p, sizeof(double) * 7);
        if (c) std::memcpy(key.cov, c, sizeof(double) * 36);
        for (int d = 0; d < 3; ++d) key.pos[d] = float(key.pose[d]);
        changed[size_t(first_key) + size_t(i)] = 1;
        ++n_changed;
    }
    if (drift_tail && changed[last]) {
        kf_drift(keys[last].pose, old_last, drift);
        for (size_t k = last + 1; k < keys.size(); ++k) {
            double moved[7];
            pg_pose_mul(drift, keys[k].pose, moved);
            std::memcpy(keys[k].pose, moved, sizeof(moved));
            for (int d = 0; d < 3; ++d) keys[k].pos[d] = float(moved[d]);
            changed[k] = 1;
            ++n_changed;
        }
    }
    return n_changed;
}

// the cache entries of changed keyframes erased, their slots recycled, the order of the rest kept (the erase of extractSurroundingKeyFrames, cpp:274-293, with
// "changed" in the place of "left the radius")
template <class Entry>
void kf_erase_changed(std::vector<Entry> &entries, std::vector<int> &free_slots, const std::vector<char> &changed)
{
    std::vector<Entry> kept;
    kept.reserve(entries.size());
    for (const Entry &e : entries) {
        if (changed[size_t(e.id)]) free_slots.push_back(e.slot);
        else kept.push_back(e);
    }
    entries.swap(kept);
}

}  // namespace mlh
