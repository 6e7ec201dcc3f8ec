// Stand-alone driver of the pair orientation (csrc/dgm_plan.h dgm_orient) for
// tests/test_wasserstein_cpu.py: host C++ only.  One case on stdin, whitespace-separated:
//     S  offsets[S + 1]  rows  points[2 * rows]  P  pairs[2 * P]
// Coordinates are read with strtod, so nan, inf, -inf and -0 are values.  The calls are those of
// ws_plan: dgm_check_layout, dgm_gather, dgm_classify (max(n1, n2) <= 64 / 256 / 512), dgm_orient.
// Output: "err <code> <message>", or one line per pair: first second swapped.
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "dgm_plan.h"

int main() {
    using namespace tda;
    long long S, rows, P;
    if (!(std::cin >> S)) return 2;
    std::vector<int64_t> off((size_t)S + 1);
    for (auto& o : off) std::cin >> o;
    std::cin >> rows;
    std::vector<double> pts((size_t)rows * 2);
    for (auto& x : pts) {
        std::string tok;
        std::cin >> tok;
        x = strtod(tok.c_str(), nullptr);
    }
    std::cin >> P;
    std::vector<int32_t> prs((size_t)P * 2 + 1);  // never empty: something to point at
    for (size_t q = 0; q < (size_t)P * 2; ++q) std::cin >> prs[q];
    if (!std::cin) return 2;

    PairPlan pl;
    std::string msg;
    const int limits[kPairClasses] = {64, 256, 512};
    int rc = dgm_check_layout(pts.data(), off.data(), S, prs.data(), P, "test", msg);
    if (!rc) rc = dgm_gather(pts.data(), off.data(), S, prs.data(), P, pl, msg);
    if (!rc) rc = dgm_classify(pl, PairSize::kMax, limits, "too large", msg);
    if (rc) {
        printf("err %d %s\n", rc, msg.c_str());
        return 0;
    }
    const std::vector<int32_t> order = pl.order;
    std::vector<uint8_t> swapped;
    dgm_orient(pl, swapped);
    if (pl.order != order || (int64_t)swapped.size() != P) return 3;  // the orientation leaves the classes alone
    for (long long p = 0; p < P; ++p) printf("%d %d %d\n", (int)pl.pairs[2 * p], (int)pl.pairs[2 * p + 1], (int)swapped[p]);
    return 0;
}
