// Stand-alone driver of the persistence curves' plan (csrc/dgm_plan.h pc_plan) for
// tests/test_persistence_curves_cpu.py: host C++ only.  One case on stdin, whitespace-separated:
//     pc  S  offsets[S + 1] | null  rows  points[2 * rows]  G  kernel  flags  reserved  ngrid  grid[ngrid] | -1  ncoef  coef[ncoef] | -1
//     null 0      args == NULL
// ("null" in place of the offsets passes NULL; rows = -1 passes points = NULL; -1 in place of a
// count passes NULL for that array.)  Values are read with strtod, so nan, inf, -inf and -0 are
// values.  Output: "err <code> <message>", or the plan:
//     off <S + 1 numbers> / order <S> / cnt <4> / cls_n <4> / pts <2 * kept, %a> / wgt <kept or none, %a> / W <S, %a>
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "dgm_plan.h"

static double num() {
    std::string tok;
    std::cin >> tok;
    return strtod(tok.c_str(), nullptr);
}

static bool array(std::vector<double>& v) {  // false: NULL
    long long n;
    std::cin >> n;
    if (n < 0) return false;
    v.resize((size_t)n + 1);  // never empty: something to point at
    for (long long i = 0; i < n; ++i) v[(size_t)i] = num();
    return true;
}

int main() {
    using namespace tda;
    std::string mode, tok;
    long long S = 0, rows = 0;
    if (!(std::cin >> mode >> S)) return 2;
    PcPlan pp;
    std::string msg;
    if (mode == "null") {
        const int code = pc_plan(nullptr, pp, msg);
        printf("err %d %s\n", code, msg.c_str());
        return 0;
    }
    if (mode != "pc") return 2;
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

    tda_pc_args a = {};
    long long G, kernel, flags, reserved;
    std::cin >> G >> kernel >> flags >> reserved;
    std::vector<double> grid, coef;
    const bool have_grid = array(grid), have_coef = array(coef);
    if (!std::cin) return 2;
    a.points = rows < 0 ? nullptr : pts.data();
    a.offsets = have_off ? off.data() : nullptr;
    a.S = S;
    a.coef = have_coef ? coef.data() : nullptr;
    a.grid = have_grid ? grid.data() : nullptr;
    a.G = (int32_t)G;
    a.kernel = (int32_t)kernel;
    a.flags = (int32_t)flags;
    a.reserved = (int32_t)reserved;
    if (int rc = pc_plan(&a, pp, msg)) {
        printf("err %d %s\n", rc, msg.c_str());
        return 0;
    }
    const VecPlan& pl = pp.v;
    printf("off");
    for (int64_t o : pl.off) printf(" %lld", (long long)o);
    printf("\norder");
    for (int32_t o : pl.order) printf(" %d", (int)o);
    printf("\ncnt");
    for (int c = 0; c < kVecClasses; ++c) printf(" %lld", (long long)pl.cls_cnt[c]);
    printf("\ncls_n");
    for (int c = 0; c < kVecClasses; ++c) printf(" %d", pl.cls_n[c]);
    printf("\npts");
    for (double x : pl.pts) printf(" %a", x);
    printf("\nwgt");
    for (double x : pl.wgt) printf(" %a", x);
    printf("\nW");
    for (double x : pp.W) printf(" %a", x);
    printf("\n");
    return 0;
}
