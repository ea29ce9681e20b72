// Host logic check (no GPU): mlh::records_fault, the one validation of a caller's record buffer (m-loam_amd/csrc/records.hpp), accepts every record layout in
// use and names the argument at fault for everything a kernel would read outside the record. Compiled and run by tests/test_abi.py::test_records_validation.
#include "records.hpp"
#include <cstdio>
#include <cstring>

static int bad = 0, cases = 0;
static unsigned char buf[64];

static void expect(const char *what, const mlh::Records &r, bool allow_empty, const char *fault)
{
    const char *got = mlh::records_fault(r, allow_empty);
    ++cases;
    if ((got == nullptr) != (fault == nullptr) || (got && std::strcmp(got, fault) != 0)) {
        ++bad;
        std::printf("MISMATCH %s: fault %s, expected %s\n", what, got ? got : "none", fault ? fault : "none");
    }
}

int main()
{
    using mlh::records_of;
    const char *I = "intensity_offset_bytes", *C = "cov_offset_bytes", *T = "trace_offset_bytes";
    // ---- the layouts in use, host and device
    for (int mem = 0; mem < 2; ++mem) {
        expect("float4 {x y z i}", records_of(buf, 16, 100, mem, 12), false, nullptr);
        expect("44-byte {x y z i cov6 trace} (Python wrapper, device clouds)", records_of(buf, 44, 100, mem, 12, 16, 40), false, nullptr);
        expect("facade PointI (32 bytes)", records_of(buf, 32, 100, mem, 16), false, nullptr);
        expect("facade PointIWithCov (48 bytes)", records_of(buf, 48, 100, mem, 16, 20, 44), false, nullptr);
        expect("48-byte layout of mloam_hip.h", records_of(buf, 48, 100, mem, 12, 16, 40), false, nullptr);
        expect("bare xyz", records_of(buf, 12, 100, mem), false, nullptr);
        expect("bare xyz, every offset -1", records_of(buf, 12, 100, mem, -1, -1, -1), false, nullptr);
    }
    // ---- each field exactly fitting (off + size == stride), one word and one byte past, misaligned
    expect("intensity fits exactly", records_of(buf, 16, 1, 0, 12), false, nullptr);
    expect("intensity one word past", records_of(buf, 16, 1, 0, 16), false, I);
    expect("intensity one byte past", records_of(buf, 16, 1, 0, 13), false, I);
    expect("intensity misaligned inside", records_of(buf, 32, 1, 0, 14), false, I);
    expect("covariance fits exactly", records_of(buf, 40, 1, 0, 12, 16), false, nullptr);
    expect("covariance one word past", records_of(buf, 40, 1, 0, 12, 20), false, C);
    expect("covariance one byte past", records_of(buf, 40, 1, 0, 12, 17), false, C);
    expect("covariance misaligned inside", records_of(buf, 48, 1, 0, 12, 18), false, C);
    expect("covariance in a float4 record", records_of(buf, 16, 1, 0, 12, 12), false, C);
    expect("trace fits exactly", records_of(buf, 44, 1, 0, 12, 16, 40), false, nullptr);
    expect("trace one word past", records_of(buf, 44, 1, 0, 12, 16, 44), false, T);
    expect("trace one byte past", records_of(buf, 44, 1, 0, 12, 16, 41), false, T);
    expect("trace misaligned inside", records_of(buf, 48, 1, 0, 12, 16, 42), false, T);
    expect("trace far outside", records_of(buf, 16, 1, 1, 12, -1, 4096), false, T);
    // ---- stride
    expect("stride 8", records_of(buf, 8, 1, 0), false, "stride_bytes");
    expect("stride 14", records_of(buf, 14, 1, 0), false, "stride_bytes");
    expect("stride 10 (test_status_codes)", records_of(buf, 10, 100, 0), false, "stride_bytes");
    expect("stride 0", records_of(buf, 0, 1, 0), false, "stride_bytes");
    expect("negative stride", records_of(buf, -16, 1, 0), false, "stride_bytes");
    expect("stride 12", records_of(buf, 12, 1, 0), false, nullptr);
    // ---- base pointer and count
    expect("null, n > 0", records_of(nullptr, 16, 5, 0, 12), false, "points");
    expect("null, n > 0, empty allowed", records_of(nullptr, 16, 5, 0, 12), true, "points");
    expect("n == 0", records_of(buf, 16, 0, 0, 12), false, "n");
    expect("n == 0 where the call allows it", records_of(buf, 16, 0, 0, 12), true, nullptr);
    expect("null, n == 0 where the call allows it", records_of(nullptr, 16, 0, 1, 12), true, nullptr);
    expect("null, n == 0", records_of(nullptr, 16, 0, 1, 12), false, "n");
    expect("n < 0", records_of(buf, 16, -1, 0, 12), false, "n");
    expect("n < 0, empty allowed", records_of(buf, 16, -1, 0, 12), true, "n");
    // ---- mem
    expect("mem 2", records_of(buf, 16, 1, 2, 12), false, "mem");
    expect("mem -1", records_of(buf, 16, 1, -1, 12), false, "mem");
    // ---- n * stride in size_t
    const mlh::Records big = records_of(buf, 48, 1 << 27, 1, 12, 16, 40);
    expect("2^27 records of 48 bytes", big, false, nullptr);
    ++cases;
    if (big.bytes() != size_t(48) << 27) { ++bad; std::printf("MISMATCH bytes(): %zu\n", big.bytes()); }
    std::printf("%d cases, %d mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
