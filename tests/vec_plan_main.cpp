// Stand-alone driver of the per-diagram plan (csrc/dgm_plan.h pl_plan / pi_plan) for
// tests/test_vectorize_cpu.py: host C++ only.  One case on stdin, whitespace-separated:
//     pl  S  offsets[S + 1] | null  rows  points[2 * rows]  G  K  reserved  ngrid  grid[ngrid] | -1 (NULL)
//     pi  S  offsets[S + 1] | null  rows  points[2 * rows]  W  H  reserved  sigma  power  nx  x_edges[nx] | -1  ny  y_edges[ny] | -1
//     null 0 | null 1      args == NULL for tda_landscape | tda_persistence_image
// ("null" in place of the offsets passes NULL; rows = -1 passes points = NULL.)  Coordinates are read
// with strtod, so nan, inf, -inf and -0 are values.  Output: "err <code> <message>", or the plan:
//     off <S + 1 numbers> / order <S> / cnt <4> / cls_n <4> / pts <2 * finite, %a> / wgt <finite, %a>
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
    if (mode == "null") {  // args == NULL: S picks the entry
        VecPlan none;
        std::string why;
        const int code = S ? pi_plan(nullptr, none, why) : pl_plan(nullptr, none, why);
        printf("err %d %s\n", code, why.c_str());
        return 0;
    }
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

    VecPlan pl;
    std::string msg;
    int rc;
    if (mode == "pl") {
        tda_pl_args a = {};
        long long G, K, reserved;
        std::cin >> G >> K >> reserved;
        std::vector<double> grid;
        const bool have_grid = array(grid);
        if (!std::cin) return 2;
        a.points = rows < 0 ? nullptr : pts.data();
        a.offsets = have_off ? off.data() : nullptr;
        a.S = S;
        a.grid = have_grid ? grid.data() : nullptr;
        a.G = (int32_t)G;
        a.K = (int32_t)K;
        a.reserved = (int32_t)reserved;
        rc = pl_plan(&a, pl, msg);
    } else if (mode == "pi") {
        tda_pi_args a = {};
        long long W, H, reserved;
        std::cin >> W >> H >> reserved;
        a.sigma = num();
        a.weight_power = num();
        std::vector<double> xe, ye;
        const bool have_x = array(xe), have_y = array(ye);
        if (!std::cin) return 2;
        a.points = rows < 0 ? nullptr : pts.data();
        a.offsets = have_off ? off.data() : nullptr;
        a.S = S;
        a.x_edges = have_x ? xe.data() : nullptr;
        a.y_edges = have_y ? ye.data() : nullptr;
        a.W = (int32_t)W;
        a.H = (int32_t)H;
        a.reserved = (int32_t)reserved;
        rc = pi_plan(&a, pl, msg);
    } else {
        return 2;
    }
    if (rc) {
        printf("err %d %s\n", rc, msg.c_str());
        return 0;
    }
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
    printf("\n");
    return 0;
}
