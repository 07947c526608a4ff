// Prints the plan of prompt-GEMM calls from csrc/gemm_plan.h alone, built with a plain host C++ compiler (no HIP):
//   c++ -std=c++17 tools/gemm_plan_dump.cpp -o gemm_plan_dump
// stdin:  one call per line   kind M N K group epilogue norm_kind          (kind 0 bf16, 1 int4, 2 codebook)
// stdout: one line per call   rc route tile ksplit norm_fused xn_off xn_len xs_off xs_len part_off part_len part2_off part2_len total
// The tile variant has no slot in parrot_gemm_plan's out[12]; tests/test_gemm_plan_host.py pins it through this program.
#include <stdio.h>

#include "../lit-parrot_amd/csrc/gemm_plan.h"

namespace parrot {
void set_error(const char*, ...) {}
}  // namespace parrot

int main() {
    using namespace parrot;
    int kind, M, N, K, group, epilogue, norm_kind;
    while (scanf("%d %d %d %d %d %d %d", &kind, &M, &N, &K, &group, &epilogue, &norm_kind) == 7) {
        W4Plan w4;
        GemmPlan p = {};
        int rc = kind == GEMM_BF16 ? PARROT_OK : w4_make_plan(N, K, group, &w4);
        if (rc == PARROT_OK) rc = gemm_make_plan(kind, M, N, K, &w4, epilogue, norm_kind, &p);
        printf("%d %d %d %d %d %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", rc, p.route, p.tile, p.ksplit, p.norm_fused, (long long)p.xn.off,
               (long long)p.xn.len, (long long)p.xs.off, (long long)p.xs.len, (long long)p.part.off, (long long)p.part.len, (long long)p.part2.off,
               (long long)p.part2.len, (long long)p.total);
    }
    return 0;
}
