// Runs geo_plan (csrc/geo_plan.h) with a host compiler alone (tests/test_shortest_paths_cpu.py builds it
// under the address and undefined-behaviour sanitizers).  One case per line of stdin:
//   args cap x dtype x_on_device L N D is_dist n_neighbors graph_only radius <bad>
// x is a mode: 0 NULL; 1 present.  A host distance matrix (is_dist, not on the device) is read by the
// plan, so it is given at its full size, zero-filled (a read-only mapping of zero pages, kept and
// grown from case to case), or, when <bad> is not "-", as a heap copy of L * N * N ones in which
// entry <bad> = index:value is set.  Point input is never read: 16 bytes stand for it.
// One line per case on stdout: "err <code> <message>" or "ok name=value ...", every field of the plan.
#include <sys/mman.h>

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <vector>

#include "geo_plan.h"

using namespace tda;

namespace {

alignas(16) char g_dummy[16];
std::string g_out;
void* g_zero = nullptr;
size_t g_zero_bytes = 0;

template <typename T>
void put(const char* name, T v) {
    g_out += std::string(" ") + name + "=" + std::to_string(v);
}

int64_t rd_int(std::istream& in) {
    int64_t v;
    in >> v;
    return v;
}

// at least `bytes` of zeros, never written: untouched pages cost nothing
const void* zeros(size_t bytes) {
    if (bytes > g_zero_bytes) {
        if (g_zero) munmap(g_zero, g_zero_bytes);
        g_zero = mmap(nullptr, bytes, PROT_READ, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (g_zero == MAP_FAILED) return fprintf(stderr, "mmap of %zu bytes failed\n", bytes), exit(3), nullptr;
        g_zero_bytes = bytes;
    }
    return g_zero;
}

int run(std::istream& in, std::string& msg) {
    const bool args = rd_int(in) != 0;
    tda_geodesic_args a = {};
    const size_t cap = (size_t)rd_int(in);
    const bool have_x = rd_int(in) != 0;
    a.dtype = (int32_t)rd_int(in), a.x_on_device = (int32_t)rd_int(in), a.L = rd_int(in), a.N = rd_int(in), a.D = rd_int(in);
    a.is_dist = (int32_t)rd_int(in), a.n_neighbors = (int32_t)rd_int(in), a.graph_only = (int32_t)rd_int(in);
    std::string rad, bad;
    in >> rad >> bad;
    a.radius = strtod(rad.c_str(), nullptr);  // decimal, hex, inf, nan
    std::vector<float> m32;
    std::vector<double> m64;
    if (have_x) {
        a.x = g_dummy;
        // the plan reads a host matrix only after the size limits: within them, hand it a real one
        const bool read = a.is_dist && !a.x_on_device && a.L >= 1 && a.N >= 1 && a.N <= 8192 && (unsigned __int128)a.L * a.N * a.N <= (1u << 28);
        if (read) {
            const size_t n = (size_t)a.L * a.N * a.N;
            if (bad == "-") {
                a.x = zeros(n * 8);
            } else {
                const size_t at = strtoull(bad.c_str(), nullptr, 10);
                const double v = strtod(bad.c_str() + bad.find(':') + 1, nullptr);
                if (a.dtype == TDA_F64) m64.assign(n, 1.0), m64.at(at) = v, a.x = m64.data();
                else m32.assign(n, 1.0f), m32.at(at) = (float)v, a.x = m32.data();
            }
        }
    }
    GeoPlan p;
    if (int rc = geo_plan(args ? &a : nullptr, cap, p, msg)) return rc;
    put("L", p.L), put("N", p.N), put("is_dist", (int)p.is_dist), put("knn", (int)p.knn), put("graph_only", (int)p.graph_only);
    put("resident", (int)p.resident), put("k", p.k), put("lds_n", p.lds_n), put("tiles", p.tiles), put("padded", p.padded);
    put("lds_select", p.lds_select), put("lds_resident", p.lds_resident), put("lds_diag", p.lds_diag), put("lds_product", p.lds_product);
    const SqDistPlan& s = p.sq;
    put("x_layer", s.x_layer), put("per_layer", s.per_layer), put("Lc", s.Lc), put("mfma", (int)s.sel.mfma), put("dsplit", s.sel.dsplit);
    put("gram_layer", (int)s.sel.gram_layer), put("o_x", s.o_x), put("o_dm", s.o_dm), put("o_rm", s.o_rm), put("o_gp", s.o_gp), put("o_np", s.o_np);
    put("o_ne", p.o_ne), put("o_nc", p.o_nc), put("o_thr", p.o_thr), put("total", p.total);
    return 0;
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string msg;
        g_out.clear();
        const int rc = run(in, msg);
        if (in.fail()) return fprintf(stderr, "short case: %s\n", line.c_str()), 2;
        if (rc) printf("err %d %s\n", rc, msg.c_str());
        else printf("ok%s\n", g_out.c_str());
    }
    return 0;
}
