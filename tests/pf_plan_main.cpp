// Stand-alone driver of the persistence Fisher plan (csrc/dgm_plan.h pf_plan) for
// tests/test_fisher_cpu.py: host C++ only.  One case on stdin, whitespace-separated:
//     pf  S  offsets[S + 1] | null  rows  points[2 * rows]  npairs  pairs[2 * npairs]  P  sigma  reserved
//     null                  args == NULL
// ("null" in place of the offsets passes NULL; rows = -1 passes points = NULL; npairs = -1 passes
// pairs = NULL; P is what the call names, which need not be npairs.)  Coordinates and sigma are read
// with strtod, so nan, inf, -inf and -0 are values.  Output: "err <code> <message>", or the plan:
//     P <P> / c <c2, %a> / off <S + 1> / pairs <2 P, oriented> / swapped <P> / order <P> /
//     cnt <3> / cls_parts <3> / part_off <P + 1> / pts <2 * finite, %a>
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "dgm_plan.h"

static double num() {
    std::string tok;
    std::cin >> tok;
    return strtod(tok.c_str(), nullptr);
}

int main() {
    using namespace tda;
    std::string mode, tok;
    if (!(std::cin >> mode)) return 2;
    PfPlan fp;
    std::string msg;
    if (mode == "null") {
        const int code = pf_plan(nullptr, fp, msg);
        printf("err %d %s\n", code, msg.c_str());
        return 0;
    }
    if (mode != "pf") return 2;
    long long S = 0, rows = 0, npairs = 0, P = 0, reserved = 0;
    if (!(std::cin >> S)) return 2;
    std::vector<int64_t> off;
    bool have_off = true;
    if (S >= 0) {
        off.resize((size_t)S + 1);
        for (size_t i = 0; i < off.size(); ++i) {
            std::cin >> tok;
            if (i == 0 && tok == "null") {
                have_off = false;
                break;
            }
            off[i] = strtoll(tok.c_str(), nullptr, 10);
        }
    } else {
        off.resize(1);
    }
    if (!(std::cin >> rows) || rows > (1 << 24)) return 2;
    std::vector<double> pts((size_t)(rows > 0 ? rows : 0) * 2 + 1);
    for (long long i = 0; i < 2 * rows; ++i) pts[(size_t)i] = num();
    if (!(std::cin >> npairs) || npairs > (1 << 24)) return 2;
    std::vector<int32_t> pairs((size_t)(npairs > 0 ? npairs : 0) * 2 + 1);
    for (long long i = 0; i < 2 * npairs; ++i) {
        long long v;
        std::cin >> v;
        pairs[(size_t)i] = (int32_t)v;
    }
    std::cin >> P;
    tda_pf_args a = {};
    a.sigma = num();
    std::cin >> reserved;
    if (!std::cin) return 2;
    a.points = rows < 0 ? nullptr : pts.data();
    a.offsets = have_off ? off.data() : nullptr;
    a.S = S;
    a.pairs = npairs < 0 ? nullptr : pairs.data();
    a.P = P;
    a.reserved = (int32_t)reserved;
    if (int rc = pf_plan(&a, fp, msg)) {
        printf("err %d %s\n", rc, msg.c_str());
        return 0;
    }
    const PairPlan& pl = fp.pl;
    printf("P %lld\nc %a\noff", (long long)pl.P, fp.c2);
    for (int64_t o : pl.off) printf(" %lld", (long long)o);
    printf("\npairs");
    for (int32_t o : pl.pairs) printf(" %d", (int)o);
    printf("\nswapped");
    for (uint8_t o : fp.swapped) printf(" %d", (int)o);
    printf("\norder");
    for (int32_t o : pl.order) printf(" %d", (int)o);
    printf("\ncnt");
    for (int c = 0; c < kPairClasses; ++c) printf(" %lld", (long long)pl.cls_cnt[c]);
    printf("\ncls_parts");
    for (int c = 0; c < kPairClasses; ++c) printf(" %d", fp.cls_parts[c]);
    printf("\npart_off");
    for (int64_t o : fp.part_off) printf(" %lld", (long long)o);
    printf("\npts");
    for (double x : pl.pts) printf(" %a", x);
    printf("\n");
    return 0;
}
