// Stand-alone driver of the diagram-distance plan (csrc/dgm_plan.h) for tests/test_dgm_plan_cpu.py:
// host C++ only.  Cases on stdin, whitespace-separated:
//     measure(0 = sum, 1 = max)  l0 l1 l2  S  offsets[S + 1]  rows  points[2 * rows]  P  pairs[2 * P]
// rows = -1: points == NULL.  P = -1: pairs == NULL (every i < j); P = -2: a pairs pointer with
// P = -1.  Coordinates are read with strtod, so nan, inf and -inf are values.  The calls are those
// of sw_plan / bn_plan: dgm_check_layout, dgm_gather, dgm_classify.  Per case either
// "err <code> <message>" or "ok" and six lines: pts, off, pairs, order, cls_cnt, cls_n.
// A case that starts with sw, bn or ws instead calls that entry's whole plan on an args struct:
//     entry  args(0 = NULL, 1)  S  noff  offsets[noff]  rows  points[2 * rows]  P  pairs[2 * P]  extra
// noff = -1: offsets == NULL (S is given apart, so that it can be negative); extra is M (sw),
// reserved (bn) or flags (ws).  The output is the same; the pairs of ws are as oriented.
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "dgm_plan.h"

template <typename T>
static void line(const char* name, const T* v, size_t n) {
    printf("%s", name);
    for (size_t i = 0; i < n; ++i) printf(" %lld", (long long)v[i]);
    printf("\n");
}

int main() {
    using namespace tda;
    int measure = 0, limits[kPairClasses] = {}, have_args = 1, extra = 0;
    long long S, rows, P, noff;
    std::string head;
    while (std::cin >> head) {
        const bool whole = head == "sw" || head == "bn" || head == "ws";
        if (whole) {
            std::cin >> have_args >> S >> noff;
        } else {
            measure = atoi(head.c_str());
            std::cin >> limits[0] >> limits[1] >> limits[2] >> S;
            noff = S + 1;
        }
        if (!std::cin) return 2;
        std::vector<int64_t> off(noff > 0 ? (size_t)noff : 0);
        for (auto& o : off) std::cin >> o;
        std::cin >> rows;
        std::vector<double> pts(rows > 0 ? (size_t)rows * 2 : 0);
        for (auto& x : pts) {
            std::string tok;
            std::cin >> tok;
            x = strtod(tok.c_str(), nullptr);
        }
        std::cin >> P;
        std::vector<int32_t> prs(P > 0 ? (size_t)P * 2 : 0);
        for (auto& q : prs) std::cin >> q;
        if (whole) std::cin >> extra;
        if (!std::cin) return 2;
        static const int32_t none = 0;  // something to point at for a list that is empty or refused
        const int32_t* pairs = P == -1 ? nullptr : prs.empty() ? &none : prs.data();
        const int64_t Parg = P == -2 ? -1 : P;

        PairPlan pl;
        WsPlan wp;
        std::string msg;
        int rc;
        if (whole) {
            const double* points = rows < 0 ? nullptr : pts.data();
            const int64_t* offsets = noff < 0 ? nullptr : off.data();
            if (head == "sw") {
                tda_sw_args a = {};
                a.points = points, a.offsets = offsets, a.S = S, a.pairs = pairs, a.P = Parg, a.M = extra;
                rc = sw_plan(have_args ? &a : nullptr, pl, msg);
            } else if (head == "bn") {
                tda_bn_args a = {};
                a.points = points, a.offsets = offsets, a.S = S, a.pairs = pairs, a.P = Parg, a.reserved = extra;
                rc = bn_plan(have_args ? &a : nullptr, pl, msg);
            } else {
                tda_ws_args a = {};
                a.points = points, a.offsets = offsets, a.S = S, a.pairs = pairs, a.P = Parg, a.flags = extra;
                rc = ws_plan(have_args ? &a : nullptr, wp, msg);
                pl = wp.pl;
            }
        } else {
            rc = dgm_check_layout(rows < 0 ? nullptr : pts.data(), off.data(), S, pairs, Parg, "test", msg);
            if (!rc) rc = dgm_gather(pts.data(), off.data(), S, pairs, pairs ? Parg : S * (S - 1) / 2, pl, msg);
            if (!rc) rc = dgm_classify(pl, measure ? PairSize::kMax : PairSize::kSum, limits, "too large", msg);
        }
        if (rc) {
            printf("err %d %s\n", rc, msg.c_str());
            continue;
        }
        printf("ok\npts");
        for (double x : pl.pts) printf(" %.17g", x);
        printf("\n");
        line("off", pl.off.data(), pl.off.size());
        line("pairs", pl.pairs.data(), pl.pairs.size());
        line("order", pl.order.data(), pl.order.size());
        line("cls_cnt", pl.cls_cnt, (size_t)kPairClasses);
        line("cls_n", pl.cls_n, (size_t)kPairClasses);
    }
    return 0;
}
