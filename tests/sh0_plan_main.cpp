// Runs sh0_plan (csrc/sh0_plan.h) with a host compiler alone (tests/test_subsample_h0_cpu.py builds it
// under the address and undefined-behaviour sanitizers).  One case per line of stdin:
//   args cap x dtype x_on_device L N D is_dist B m idx_per_layer want_deaths alpha <idx> <sizes>
// A table is given as a mode: 0 NULL; 1 present and zero-filled at its full size (a read-only mapping
// of zero pages, kept and grown from case to case: the plan reads the first sizes[b] entries of every
// row, however large the table); 2 the count of its values and the values follow.  sizes in mode 1
// holds B times the value that follows the mode.  One line per case on stdout:
// "err <code> <message>" or "ok name=value ...", every field of the plan.
#include <sys/mman.h>

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <vector>

#include "sh0_plan.h"

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
const int32_t* zeros(size_t bytes) {
    if (bytes > g_zero_bytes) {
        if (g_zero) munmap(g_zero, g_zero_bytes);
        g_zero = mmap(nullptr, bytes, PROT_READ, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (g_zero == MAP_FAILED) return fprintf(stderr, "mmap of %zu bytes failed\n", bytes), exit(3), nullptr;
        g_zero_bytes = bytes;
    }
    return (const int32_t*)g_zero;
}

int run(std::istream& in, std::string& msg) {
    const bool args = rd_int(in) != 0;
    tda_subsample_h0_args a = {};
    const size_t cap = (size_t)rd_int(in);
    a.x = rd_int(in) ? g_dummy : nullptr;
    a.dtype = (int32_t)rd_int(in), a.x_on_device = (int32_t)rd_int(in), a.L = rd_int(in), a.N = rd_int(in), a.D = rd_int(in);
    a.is_dist = (int32_t)rd_int(in), a.B = rd_int(in), a.m = (int32_t)rd_int(in), a.idx_per_layer = (int32_t)rd_int(in);
    a.want_deaths = (int32_t)rd_int(in);
    std::string al;
    in >> al;
    a.alpha = strtod(al.c_str(), nullptr);  // decimal, hex, inf, nan
    const bool sane = a.L >= 1 && a.B >= 1 && a.m >= 1;
    std::vector<int32_t> idx, sizes;
    int mode = (int)rd_int(in);
    if (mode == 2) {
        idx.resize((size_t)rd_int(in));
        for (int32_t& v : idx) v = (int32_t)rd_int(in);
        a.idx = idx.data();
    } else if (mode == 1) {
        a.idx = sane ? zeros((size_t)(a.idx_per_layer ? a.L : 1) * a.B * a.m * 4) : (const int32_t*)g_dummy;
    }
    mode = (int)rd_int(in);
    if (mode == 2) {
        sizes.resize((size_t)rd_int(in));
        for (int32_t& v : sizes) v = (int32_t)rd_int(in);
        a.sizes = sizes.data();
    } else if (mode == 1) {
        const int32_t v = (int32_t)rd_int(in);
        sizes.assign(sane ? (size_t)a.B : 0, v);
        a.sizes = sane ? sizes.data() : (const int32_t*)g_dummy;
    }
    Sh0Plan p;
    if (int rc = sh0_plan(args ? &a : nullptr, cap, p, msg)) return rc;
    put("L", p.L), put("N", p.N), put("B", p.B), put("m", p.m), put("is_dist", (int)p.is_dist), put("per_layer_idx", (int)p.per_layer_idx);
    put("want_deaths", (int)p.want_deaths), put("resident", (int)p.resident), put("mode", p.mode), put("Bc", p.Bc), put("idx_lstride", p.idx_lstride);
    put("d_lstride", p.d_lstride), put("lds", p.lds);
    const SqDistPlan& s = p.sq;
    put("x_layer", s.x_layer), put("per_layer", s.per_layer), put("Lc", s.Lc), put("mfma", (int)s.sel.mfma), put("dsplit", s.sel.dsplit);
    put("gram_layer", (int)s.sel.gram_layer), put("o_x", s.o_x), put("o_dm", s.o_dm), put("o_rm", s.o_rm), put("o_gp", s.o_gp), put("o_np", s.o_np);
    put("o_E", p.o_E), put("o_sz", p.o_sz), put("o_idx", p.o_idx), put("o_deaths", p.o_deaths), put("total", p.total);
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
