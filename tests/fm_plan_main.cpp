// Stand-alone driver of the Frechet mean's plan (csrc/fm_plan.h fm_plan, fm_class, fm_g_entries) for
// tests/test_frechet_cpu.py: host C++ only.  One case per line on stdin, whitespace-separated:
//     null                                   args == NULL
//     cls K n                                prints "cls <fm_class(K, n)> <fm_g_entries(3, K)>"
//     fm S offsets[S + 1] | null  rows points[2 * rows]  init_index  init_rows init[2 * init_rows]  max_iter flags reserved
// ("null" in place of the offsets passes NULL and is followed by nothing of them; rows = -1 passes
// points = NULL, init_rows = -1 passes init_points = NULL with init_n = 0, init_rows = -2 passes
// init_n = -1, init_rows = -3 passes init_points = NULL with init_n = 4.)  Coordinates are read with
// strtod, so nan, inf, -inf and -0 are values.
// Output per case: "err <code> <message>", or
//     ok <S> <K0> <n_max> <class of the first step> / off <S + 1> / pts <2 * finite, %a> / y0 <2 * K0, %a>
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "fm_plan.h"

static double num() {
    std::string tok;
    std::cin >> tok;
    return strtod(tok.c_str(), nullptr);
}

int main() {
    using namespace tda;
    std::string mode, tok;
    while (std::cin >> mode) {
        FmPlan fp;
        std::string msg;
        if (mode == "null") {
            const int code = fm_plan(nullptr, fp, msg);
            printf("err %d %s\n", code, msg.c_str());
            continue;
        }
        if (mode == "cls") {
            long long K, n;
            if (!(std::cin >> K >> n)) return 2;
            printf("cls %d %zu\n", fm_class((int)K, (int)n), fm_g_entries(3, (int)K));
            continue;
        }
        if (mode != "fm") return 2;
        long long S = 0, rows = 0, init_index = 0, init_rows = 0, max_iter = 0, flags = 0, reserved = 0;
        if (!(std::cin >> S) || S > (1 << 20)) return 2;
        std::vector<int64_t> off((size_t)(S > 0 ? S : 0) + 1);
        bool have_off = true;
        for (size_t i = 0; i < off.size(); ++i) {
            std::cin >> tok;
            if (i == 0 && tok == "null") {
                have_off = false;
                break;
            }
            off[i] = strtoll(tok.c_str(), nullptr, 10);
        }
        if (!(std::cin >> rows) || rows > (1 << 24)) return 2;
        std::vector<double> pts((size_t)(rows > 0 ? rows : 0) * 2 + 1);
        for (long long i = 0; i < 2 * rows; ++i) pts[(size_t)i] = num();
        if (!(std::cin >> init_index >> init_rows) || init_rows > (1 << 24)) return 2;
        std::vector<double> init((size_t)(init_rows > 0 ? init_rows : 0) * 2 + 1);
        for (long long i = 0; i < 2 * init_rows; ++i) init[(size_t)i] = num();
        if (!(std::cin >> max_iter >> flags >> reserved)) return 2;
        tda_fm_args a = {};
        a.points = rows < 0 ? nullptr : pts.data();
        a.offsets = have_off ? off.data() : nullptr;
        a.S = S;
        a.init_index = init_index;
        a.init_points = init_rows < 0 ? nullptr : init.data();
        a.init_n = init_rows == -3 ? 4 : init_rows == -2 ? -1 : init_rows < 0 ? 0 : init_rows;
        a.max_iter = (int32_t)max_iter;
        a.flags = (int32_t)flags;
        a.reserved = (int32_t)reserved;
        if (int rc = fm_plan(&a, fp, msg)) {
            printf("err %d %s\n", rc, msg.c_str());
            continue;
        }
        if ((int64_t)fp.y0.size() != 2 * (int64_t)fp.K0 || (int64_t)fp.pts.size() != 2 * fp.off[(size_t)S]) return 3;
        printf("ok %lld %d %d %d\noff", (long long)fp.S, fp.K0, fp.n_max, fm_class(fp.K0, fp.n_max));
        for (int64_t o : fp.off) printf(" %lld", (long long)o);
        printf("\npts");
        for (double x : fp.pts) printf(" %a", x);
        printf("\ny0");
        for (double x : fp.y0) printf(" %a", x);
        printf("\n");
    }
    return 0;
}
