// TEST INFRASTRUCTURE ONLY. m-loam_amd/csrc/kf_update_host.hpp (the host rules of mlh_keyframes_update_poses) in a stand-alone program, so that
// tests/test_kf_update_cases.py can build it with -fsanitize=address,undefined and run it directly. Every expectation is computed here, by hand or from the
// quaternion algebra written out in this file (not through pg_host.hpp):
//   the bitwise "changed" rule (-0.0 against 0.0 is a change, an equal pose with a changed covariance is a change, equal bits are not);
//   erase-keeps-order and slot recycling on a hand-made entry list;
//   the drift of a hand-made pose pair (a quarter turn of yaw and a translation), applied to the keys beyond the range;
//   the identity drift when the last key of the range did not change, and without drift_tail;
//   range validation.
#include "kf_update_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace mlh;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("kf_update_host: CHECK FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

struct Key { double pose[7], cov[36]; float pos[3]; };
struct Entry { int id; size_t off[2]; int n[2]; int slot; };

static Key make_key(double x, double y, double z, double yaw)
{
    Key k;
    k.pose[0] = x; k.pose[1] = y; k.pose[2] = z; k.pose[3] = 0.0; k.pose[4] = 0.0; k.pose[5] = std::sin(yaw / 2); k.pose[6] = std::cos(yaw / 2);
    for (int i = 0; i < 36; ++i) k.cov[i] = i % 7 == 0 ? 1e-4 : 0.0;
    for (int d = 0; d < 3; ++d) k.pos[d] = float(k.pose[d]);
    return k;
}

static std::vector<Key> make_store(int n)
{
    std::vector<Key> keys;
    for (int i = 0; i < n; ++i) keys.push_back(make_key(1.0 * i, 0.25 * i, 0.1, 0.05 * i));
    return keys;
}

static bool same_bits(const Key &a, const Key &b) { return !std::memcmp(a.pose, b.pose, sizeof(a.pose)) && !std::memcmp(a.cov, b.cov, sizeof(a.cov)) && !std::memcmp(a.pos, b.pos, sizeof(a.pos)); }
static bool is_identity(const double d[7]) { return d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0 && d[3] == 0.0 && d[4] == 0.0 && d[5] == 0.0 && d[6] == 1.0; }

static void check_changed_rule()
{
    std::vector<Key> keys = make_store(6);
    const std::vector<Key> before = keys;
    std::vector<char> changed;
    double drift[7];
    // the stored poses back: nothing changes, whatever drift_tail says
    std::vector<double> p;
    for (int i = 1; i <= 3; ++i) p.insert(p.end(), keys[size_t(i)].pose, keys[size_t(i)].pose + 7);
    CHECK(kf_update_apply(keys, 1, 3, p.data(), nullptr, 1, changed, drift) == 0);
    CHECK(is_identity(drift));
    for (size_t i = 0; i < keys.size(); ++i) CHECK(!changed[i] && same_bits(keys[i], before[i]));
    // ... and with the stored covariances given as well
    std::vector<double> c;
    for (int i = 1; i <= 3; ++i) c.insert(c.end(), keys[size_t(i)].cov, keys[size_t(i)].cov + 36);
    CHECK(kf_update_apply(keys, 1, 3, p.data(), c.data(), 0, changed, drift) == 0);
    // one ulp in one double of key 2; -0.0 for the 0.0 of key 3's qx: both are changes, key 1 is not
    std::vector<double> q = p;
    q[7 * 1 + 1] = std::nextafter(q[7 * 1 + 1], 1e9);
    CHECK(q[7 * 2 + 3] == 0.0);
    q[7 * 2 + 3] = -0.0;
    CHECK(kf_update_apply(keys, 1, 3, q.data(), nullptr, 0, changed, drift) == 2);
    CHECK(!changed[0] && !changed[1] && changed[2] && changed[3] && !changed[4] && !changed[5]);
    CHECK(is_identity(drift));
    CHECK(std::signbit(keys[3].pose[3]) && keys[2].pose[1] == q[8] && keys[2].pos[1] == float(q[8]));
    CHECK(same_bits(keys[1], before[1]) && same_bits(keys[4], before[4]));
    CHECK(!std::memcmp(keys[2].cov, before[2].cov, sizeof(before[2].cov)));          // covs == NULL: the stored covariance stays
    // the same poses again with ONE covariance entry of key 1 changed: key 1 alone is changed, its pose bits stay
    std::vector<double> c2 = c;
    c2[5] = 3e-5;
    CHECK(kf_update_apply(keys, 1, 3, q.data(), c2.data(), 0, changed, drift) == 1);
    CHECK(changed[1] && !changed[2] && !changed[3]);
    CHECK(keys[1].cov[5] == 3e-5 && !std::memcmp(keys[1].pose, before[1].pose, sizeof(before[1].pose)));
    // the position follows the translation
    std::vector<double> r(q.begin(), q.begin() + 7);
    r[0] = 123.456789012345; r[1] = -7.000000123; r[2] = 1e-3;
    CHECK(kf_update_apply(keys, 5, 1, r.data(), nullptr, 0, changed, drift) == 1 && changed[5]);
    CHECK(keys[5].pos[0] == float(123.456789012345) && keys[5].pos[1] == float(-7.000000123) && keys[5].pos[2] == float(1e-3));
}

static void check_erase()
{
    // cache order 7 2 9 4 0 with slots 3 0 4 1 2; keyframes 2 and 0 and (uncached) 5 changed
    std::vector<Entry> entries;
    const int ids[5] = {7, 2, 9, 4, 0}, slots[5] = {3, 0, 4, 1, 2};
    for (int j = 0; j < 5; ++j) entries.push_back(Entry{ids[j], {size_t(100 * j), size_t(100 * j + 50)}, {50, 40}, slots[j]});
    std::vector<int> free_slots = {6};
    std::vector<char> changed(10, 0);
    changed[2] = changed[0] = changed[5] = 1;
    kf_erase_changed(entries, free_slots, changed);
    CHECK(entries.size() == 3 && entries[0].id == 7 && entries[1].id == 9 && entries[2].id == 4);
    CHECK(entries[0].slot == 3 && entries[1].slot == 4 && entries[2].slot == 1 && entries[1].off[0] == 200 && entries[2].off[1] == 350);
    CHECK(free_slots.size() == 3 && free_slots[0] == 6 && free_slots[1] == 0 && free_slots[2] == 2);      // in cache order behind what was free
    // nothing changed: nothing moves; everything changed: every slot comes back
    std::vector<char> none(10, 0), all(10, 1);
    kf_erase_changed(entries, free_slots, none);
    CHECK(entries.size() == 3 && free_slots.size() == 3);
    kf_erase_changed(entries, free_slots, all);
    CHECK(entries.empty() && free_slots.size() == 6 && free_slots[3] == 3 && free_slots[4] == 4 && free_slots[5] == 1);
    std::vector<Entry> empty;
    kf_erase_changed(empty, free_slots, all);
    CHECK(empty.empty() && free_slots.size() == 6);
}

static void check_drift()
{
    // old(last) = identity rotation at (1, 2, 3); new(last) = a quarter turn about z at (4, 6, 3). drift = new * old^-1: rotation = the quarter turn,
    // translation = t_new - R (t_old) = (4, 6, 3) - (-2, 1, 3) = (6, 5, 0)
    const double h = std::sqrt(0.5);
    std::vector<Key> keys = make_store(5);
    keys[2] = make_key(1.0, 2.0, 3.0, 0.0);
    const std::vector<Key> before = keys;
    double nw[14];
    std::memcpy(nw, keys[1].pose, sizeof(double) * 7);          // key 1 unchanged
    const double last[7] = {4.0, 6.0, 3.0, 0.0, 0.0, h, h};
    std::memcpy(nw + 7, last, sizeof(last));
    std::vector<char> changed;
    double drift[7];
    CHECK(kf_update_apply(keys, 1, 2, nw, nullptr, 1, changed, drift) == 3);         // key 2 and the two keys beyond the range
    CHECK(!changed[0] && !changed[1] && changed[2] && changed[3] && changed[4]);
    const double want[7] = {6.0, 5.0, 0.0, 0.0, 0.0, h, h};
    for (int c = 0; c < 7; ++c) CHECK(std::fabs(drift[c] - want[c]) < (c < 3 ? 1e-14 : 4e-16));     // a few ulps of 6; one ulp of a unit quaternion's entry
    double d2[7];
    kf_drift(last, before[2].pose, d2);
    CHECK(!std::memcmp(d2, drift, sizeof(d2)));
    CHECK(!std::memcmp(keys[2].pose, last, sizeof(last)));      // taken as given
    // a key beyond the range: R_z(90) (x, y, z) + (6, 5, 0) = (-y + 6, x + 5, z); its yaw gains a quarter turn
    for (size_t k = 3; k < 5; ++k) {
        const double *o = before[k].pose, *n = keys[k].pose;
        CHECK(std::fabs(n[0] - (-o[1] + 6.0)) < 1e-14 && std::fabs(n[1] - (o[0] + 5.0)) < 1e-14 && std::fabs(n[2] - o[2]) < 1e-15);
        const double yaw_o = 2.0 * std::atan2(o[5], o[6]), yaw_n = 2.0 * std::atan2(n[5], n[6]);
        CHECK(std::fabs(yaw_n - yaw_o - M_PI / 2) < 1e-14 && n[3] == 0.0 && n[4] == 0.0);
        for (int d = 0; d < 3; ++d) CHECK(keys[k].pos[d] == float(n[d]));
        CHECK(!std::memcmp(keys[k].cov, before[k].cov, sizeof(before[k].cov)));
    }
    CHECK(same_bits(keys[0], before[0]) && same_bits(keys[1], before[1]));
    // the last key of the range unchanged (an earlier one changed): the identity, nothing beyond the range moves
    keys = before;
    std::memcpy(nw, last, sizeof(last));
    std::memcpy(nw + 7, before[2].pose, sizeof(double) * 7);
    CHECK(kf_update_apply(keys, 1, 2, nw, nullptr, 1, changed, drift) == 1);
    CHECK(is_identity(drift) && changed[1] && !changed[2] && !changed[3] && !changed[4]);
    CHECK(same_bits(keys[3], before[3]) && same_bits(keys[4], before[4]));
    // the last key changed but no drift_tail asked for: the identity, nothing beyond the range moves
    keys = before;
    std::memcpy(nw, before[1].pose, sizeof(double) * 7);
    std::memcpy(nw + 7, last, sizeof(last));
    CHECK(kf_update_apply(keys, 1, 2, nw, nullptr, 0, changed, drift) == 1);
    CHECK(is_identity(drift) && changed[2] && !changed[3] && same_bits(keys[3], before[3]));
    // a range that ends at the store's end: a drift, nothing to put it on
    keys = before;
    double tail[7];
    std::memcpy(tail, last, sizeof(last));
    CHECK(kf_update_apply(keys, 4, 1, tail, nullptr, 1, changed, drift) == 1);
    CHECK(!is_identity(drift) && changed[4]);
}

static void check_validation()
{
    std::vector<double> p(7 * 4, 0.0), c(36 * 4, 0.0);
    for (int i = 0; i < 4; ++i) p[size_t(7 * i + 6)] = 1.0;
    CHECK(kf_update_fault(10, 0, 4, p.data(), nullptr) == nullptr);
    CHECK(kf_update_fault(10, 6, 4, p.data(), c.data()) == nullptr);             // the last four keys
    CHECK(kf_update_fault(10, 7, 4, p.data(), nullptr) != nullptr);              // one past the store
    CHECK(kf_update_fault(10, -1, 4, p.data(), nullptr) != nullptr);
    CHECK(kf_update_fault(10, 10, 1, p.data(), nullptr) != nullptr);
    CHECK(kf_update_fault(0, 0, 1, p.data(), nullptr) != nullptr);               // an empty store
    CHECK(kf_update_fault(10, 0, 0, p.data(), nullptr) != nullptr);
    CHECK(kf_update_fault(10, 0, -3, p.data(), nullptr) != nullptr);
    CHECK(kf_update_fault(10, 0, 4, nullptr, nullptr) != nullptr);
    CHECK(kf_update_fault(10, INT32_MAX, INT32_MAX, p.data(), nullptr) != nullptr);      // no overflow on the way to the answer
    std::vector<double> bad = p;
    bad[7 * 3 + 2] = NAN;
    CHECK(kf_update_fault(10, 0, 4, bad.data(), nullptr) != nullptr);
    CHECK(kf_update_fault(10, 0, 3, bad.data(), nullptr) == nullptr);            // the NaN lies beyond the three poses read
    bad = p; bad[4] = INFINITY;
    CHECK(kf_update_fault(10, 0, 4, bad.data(), nullptr) != nullptr);
    std::vector<double> badc = c;
    badc[36 * 3 + 35] = INFINITY;
    CHECK(kf_update_fault(10, 0, 4, p.data(), badc.data()) != nullptr);
    badc[36 * 3 + 35] = NAN;
    CHECK(kf_update_fault(10, 0, 4, p.data(), badc.data()) != nullptr);
    CHECK(kf_update_fault(10, 0, 3, p.data(), badc.data()) == nullptr);
}

int main()
{
    check_changed_rule();
    check_erase();
    check_drift();
    check_validation();
    if (failures) { std::printf("kf_update_host: %d checks failed\n", failures); return 1; }
    std::printf("kf_update_host: ok\n");
    return 0;
}
