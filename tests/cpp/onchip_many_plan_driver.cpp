// onchip_many_plan_driver.cpp -- the host arithmetic of the batched on-chip solves (csrc/onchip_plan.h) on the
// CPU, under the sanitizers (tests/test_onchip_many_cpu.py).
//
// For every even N from 6 to kOnchipMaxN: the LDS bytes of one workgroup cover the image of that grid and the side data, stay within
// one CU's LDS, are a multiple of 16 and grow with N; the workspace bytes of 1, 2, 40 and MANY_MAX systems are restated here from the
// documented formula (three packed vectors, 456 bytes of small data per system, 8 bytes once).  Sizes the plan refuses give 0.
// Prints "N=<n> lds=<bytes> cells=<c> unknowns=<u> per_cu=<floor(160 KiB / lds)> ws1=<bytes> ws40=<bytes>" per size, "FAIL ..." per
// violation and "ok <failures>" at the end.
#include "../../iterative_solvers_amd/csrc/onchip_plan.h"

#include <cstdio>

using namespace mi355cg;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

int main() {
    int prev = 0;
    for (int n = 6; n <= kOnchipMaxN; n += 2) {
        const OnchipPlan pl = onchip_plan(n);
        const int lds = onchip_many_lds_bytes(n);
        CHECK(lds >= pl.cells * 8 + kOnchipSideBytes, "N=%d: %d bytes do not hold the image and the side data", n, lds);
        CHECK(lds >= pl.lds_bytes && lds < pl.lds_bytes + 16, "N=%d: %d bytes against the plan's %d", n, lds, pl.lds_bytes);
        CHECK(lds <= kOnchipLdsLimit && kOnchipLdsLimit == 160 * 1024, "N=%d: %d bytes exceed one CU's LDS", n, lds);
        CHECK(lds % 16 == 0, "N=%d: %d bytes are no multiple of 16", n, lds);
        CHECK(lds > prev, "N=%d: %d bytes after %d", n, lds, prev);
        prev = lds;
        const int unknowns = (n / 2 - 1) * (3 * n / 2 - 1);
        CHECK(pl.unknowns == unknowns, "N=%d: %d unknowns", n, pl.unknowns);
        for (int nsys : {1, 2, 40, 65536}) {
            const long long want = (long long)nsys * (3LL * 8 * unknowns + 2 * 184 + 9 * 8 + 8 + 8) + 8;
            CHECK(onchip_many_workspace_bytes(n, nsys) == want, "N=%d nsys=%d: %lld workspace bytes, not %lld", n, nsys,
                  onchip_many_workspace_bytes(n, nsys), want);
        }
        std::printf("N=%d lds=%d cells=%d unknowns=%d per_cu=%d ws1=%lld ws40=%lld\n", n, lds, pl.cells, unknowns, kOnchipLdsLimit / lds,
                    onchip_many_workspace_bytes(n, 1), onchip_many_workspace_bytes(n, 40));
    }
    for (int n : {0, 4, 7, kOnchipMaxN + 1, kOnchipMaxN + 2}) {
        CHECK(onchip_many_lds_bytes(n) == 0, "N=%d has LDS bytes", n);
        CHECK(onchip_many_workspace_bytes(n, 3) == 0, "N=%d has workspace bytes", n);
    }
    CHECK(onchip_many_workspace_bytes(10, 0) == 0 && onchip_many_workspace_bytes(10, -1) == 0, "an empty batch has workspace bytes");
    CHECK(kOnchipLdsLimit / onchip_many_lds_bytes(kOnchipMaxN) == 1, "two workgroups of the largest grid on one CU");
    CHECK(kOnchipLdsLimit / onchip_many_lds_bytes(10) >= 32, "N=10: fewer than 32 workgroups' LDS on one CU");
    std::printf("cap %d\n", kOnchipMaxN);
    std::printf("ok %d\n", failures);
    return failures ? 1 : 0;
}
