// Runs the plans of csrc/side_plan.h with a host compiler alone (tests/test_side_plan_cpu.py builds it
// under the address and undefined-behaviour sanitizers).  One case per line of stdin, its first word the
// plan; a pointer is given as a mode: 0 NULL, 1 present (never read by the checks the case reaches, or
// zero-filled where the plan scans it), 2 the count of its values and the values follow.  One line per case on stdout:
// "err <code> <message>" or "ok name=value ...", every field of the plan.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <vector>

#include "side_plan.h"

using namespace tda;

namespace {

alignas(16) char g_dummy[16];
std::string g_out;

template <typename T>
void put(const char* name, T v) {
    g_out += std::string(" ") + name + "=" + std::to_string(v);
}
void put_sq(const SqDistPlan& s) {
    put("x_layer", s.x_layer), put("per_layer", s.per_layer), put("Lc", s.Lc), put("mfma", (int)s.sel.mfma), put("dsplit", s.sel.dsplit);
    put("gram_layer", (int)s.sel.gram_layer), put("o_x", s.o_x), put("o_dm", s.o_dm), put("o_rm", s.o_rm), put("o_gp", s.o_gp), put("o_np", s.o_np);
}
void put_job(const EdJob& j) {
    put("B", j.B), put("N", j.N), put("D", j.D), put("src_items", j.src_items), put("src_rows", j.src_rows), put("keep_rows", j.keep_rows);
    put("per_item", j.per_item), put("m", j.m), put("esz", j.esz), put("o_x", j.o_x), put("o_g", j.o_g), put("total", j.total), put("n_out", j.n_out);
    put("pinned", j.pinned), put("stage", (int)j.stage());
}

int64_t rd_int(std::istream& in);
// a pointer of `count` elements by its mode
template <typename T, typename Read>
const T* ptr(std::istream& in, std::vector<T>& store, size_t count, bool scanned, Read&& read) {
    int mode;
    in >> mode;
    if (mode == 0) return nullptr;
    if (mode == 1 && !scanned) return (const T*)g_dummy;
    store.assign(mode == 2 ? (size_t)rd_int(in) : count, T());  // mode 2: the count, then the values
    if (mode == 2)
        for (T& v : store) v = read(in);
    return store.data();
}
int64_t rd_int(std::istream& in) {
    int64_t v;
    in >> v;
    return v;
}
double rd_f64(std::istream& in) {
    std::string t;
    in >> t;
    return strtod(t.c_str(), nullptr);  // decimal, hex, inf, nan
}

int run(const std::string& what, std::istream& in, std::string& msg) {
    const bool args = rd_int(in) != 0;
    if (what == "cap") {  // the cap the entries pass their plans
        put("cap", side_ws_cap());
    } else if (what == "greedy") {
        tda_greedy_args a = {};
        const size_t cap = (size_t)rd_int(in);
        a.x = rd_int(in) ? g_dummy : nullptr;
        a.dtype = (int32_t)rd_int(in), a.x_on_device = (int32_t)rd_int(in), a.L = rd_int(in), a.N = rd_int(in), a.D = rd_int(in);
        a.is_dist = (int32_t)rd_int(in), a.n_perm = (int32_t)rd_int(in), a.want_dperm2all = (int32_t)rd_int(in);
        GreedyPlan p;
        if (int rc = greedy_plan(args ? &a : nullptr, cap, p, msg)) return rc;
        put("L", p.L), put("N", p.N), put("k", p.k), put("is_dist", (int)p.is_dist), put("want_dp", (int)p.want_dp);
        put_sq(p.sq);
        put("o_idx", p.o_idx), put("o_lam", p.o_lam), put("o_dp", p.o_dp), put("total", p.total), put("sub_bytes", p.sub_bytes);
    } else if (what == "resample") {
        tda_resample_args a = {};
        const size_t cap = (size_t)rd_int(in);
        a.x = rd_int(in) ? g_dummy : nullptr;
        a.dtype = (int32_t)rd_int(in), a.x_on_device = (int32_t)rd_int(in), a.L = rd_int(in), a.N = rd_int(in), a.D = rd_int(in);
        a.is_dist = (int32_t)rd_int(in), a.B = rd_int(in), a.m = (int32_t)rd_int(in), a.idx_per_layer = (int32_t)rd_int(in);
        const bool sane = a.L >= 1 && a.B >= 1 && a.m >= 1 && (unsigned __int128)a.L * (uint64_t)a.B <= (uint64_t)TDA_RESAMPLE_MAX_OUT;
        std::vector<int32_t> idx;
        a.idx = ptr(in, idx, sane ? (size_t)(a.idx_per_layer ? a.L : 1) * a.B * a.m : 0, sane, [](std::istream& s) { return (int32_t)rd_int(s); });
        ResamplePlan p;
        if (int rc = resample_plan(args ? &a : nullptr, cap, p, msg)) return rc;
        put("L", p.L), put("N", p.N), put("B", p.B), put("m", p.m), put("is_dist", (int)p.is_dist), put("per_layer_idx", (int)p.per_layer_idx);
        put("Bc", p.Bc), put("idx_lstride", p.idx_lstride);
        put_sq(p.sq);
        put("o_h", p.o_h), put("o_idx", p.o_idx), put("total", p.total);
    } else if (what == "perm") {
        tda_perm_args a = {};
        a.S = rd_int(in), a.B = rd_int(in), a.G = (int32_t)rd_int(in), a.reserved = (int32_t)rd_int(in);
        const bool sane = a.S >= 2 && a.S <= TDA_PERM_MAX_S && a.B >= 1 && (unsigned __int128)a.B * (uint64_t)a.S <= (uint64_t)TDA_PERM_MAX_TABLE;
        std::vector<double> w;
        std::vector<uint8_t> obs, lab;
        const auto byte = [](std::istream& s) { return (uint8_t)rd_int(s); };
        a.w = ptr(in, w, sane ? (size_t)a.S * a.S : 0, sane, rd_f64);
        a.obs = ptr(in, obs, sane ? (size_t)a.S : 0, sane, byte);
        a.lab = ptr(in, lab, sane ? (size_t)a.B * a.S : 0, sane, byte);
        PermPlan p;
        if (int rc = perm_plan(args ? &a : nullptr, p, msg)) return rc;
        put("S", p.S), put("B", p.B), put("rows", p.rows), put("chunk", p.chunk), put("resident", (int)p.resident);
        put("o_w", p.o_w), put("o_c", p.o_c), put("o_out", p.o_out), put("o_lab", p.o_lab), put("total", p.total);
        char t[64];
        for (int g = 0; g < a.G; ++g) snprintf(t, sizeof t, " cw%d=%a", g, p.cw[g]), g_out += t;
    } else if (what == "ed") {
        tda_ed_args a = {};
        const bool out = rd_int(in) != 0;
        a.x = rd_int(in) ? g_dummy : nullptr;
        a.dtype = (int32_t)rd_int(in), a.x_on_device = (int32_t)rd_int(in), a.B = rd_int(in), a.N = rd_int(in), a.D = rd_int(in);
        EdJob j;
        if (int rc = ed_plan(args ? &a : nullptr, out ? (const float*)g_dummy : nullptr, j, msg)) return rc;
        put_job(j);
    } else if (what == "windows" || what == "entropy") {
        tda_spectral_args a = {};
        const bool out = rd_int(in) != 0;
        a.x = rd_int(in) ? g_dummy : nullptr;
        a.dtype = (int32_t)rd_int(in), a.x_on_device = (int32_t)rd_int(in), a.B = rd_int(in), a.S = rd_int(in), a.D = rd_int(in);
        a.n_windows = rd_int(in), a.n_alpha = (int32_t)rd_int(in), a.eps = rd_f64(in);
        std::vector<double> alphas;
        const bool sane = a.n_alpha >= 1 && a.n_alpha <= kSideEdMaxAlpha;
        a.alphas = ptr(in, alphas, sane ? (size_t)a.n_alpha : 0, sane, rd_f64);
        EdJob j;
        const float* o = out ? (const float*)g_dummy : nullptr;
        if (int rc = what == "entropy" ? entropy_plan(args ? &a : nullptr, o, j, msg)
                                       : spectral_plan("windowed effective dimensionality", args ? &a : nullptr, o, true, j, msg))
            return rc;
        put_job(j);
    } else if (what == "umap") {
        tda_umap_args a = {};
        a.x = rd_int(in) ? g_dummy : nullptr, a.out = rd_int(in) ? (float*)g_dummy : nullptr;
        a.dtype = (int32_t)rd_int(in), a.x_on_device = (int32_t)rd_int(in), a.L = rd_int(in), a.N = rd_int(in), a.D = rd_int(in);
        a.metric = (int32_t)rd_int(in), a.n_neighbors = (int32_t)rd_int(in), a.n_components = (int32_t)rd_int(in), a.n_epochs = (int32_t)rd_int(in);
        a.init = (int32_t)rd_int(in), a.negative_sample_rate = (int32_t)rd_int(in), a.a = (float)rd_f64(in), a.b = (float)rd_f64(in);
        UmapPlan p;
        if (int rc = umap_plan(args ? &a : nullptr, p, msg)) return rc;
        put("L", p.L), put("N", p.N), put("D", p.D), put("k", p.k), put("c", p.c), put("esz", p.esz), put("ecap", p.ecap), put("o_x", p.o_x);
        put("o_dist", p.o_dist), put("o_rmax", p.o_rmax), put("o_kd", p.o_kd), put("o_ki", p.o_ki), put("o_P", p.o_P), put("o_S", p.o_S);
        put("o_smax", p.o_smax), put("o_ne", p.o_ne), put("o_head", p.o_head), put("o_tail", p.o_tail), put("o_eps", p.o_eps), put("o_nxt", p.o_nxt);
        put("o_nxn", p.o_nxn), put("o_deg", p.o_deg), put("o_emb", p.o_emb), put("total", p.total), put("spectral", (int)p.spectral);
        put("spec_lds", p.spec_lds), put("sgd_lds", p.sgd_lds);
    } else if (what == "transform") {
        tda_umap_transform_args a = {};
        a.x_train = rd_int(in) ? g_dummy : nullptr, a.emb_train = rd_int(in) ? (const float*)g_dummy : nullptr;
        a.y = rd_int(in) ? g_dummy : nullptr, a.out = rd_int(in) ? (float*)g_dummy : nullptr;
        a.dtype = (int32_t)rd_int(in), a.x_on_device = (int32_t)rd_int(in), a.L = rd_int(in), a.M = rd_int(in), a.N = rd_int(in), a.D = rd_int(in);
        a.metric = (int32_t)rd_int(in), a.n_neighbors = (int32_t)rd_int(in), a.n_components = (int32_t)rd_int(in), a.n_epochs = (int32_t)rd_int(in);
        a.negative_sample_rate = (int32_t)rd_int(in), a.a = (float)rd_f64(in), a.b = (float)rd_f64(in);
        UmapTransformPlan p;
        if (int rc = umap_transform_plan(args ? &a : nullptr, p, msg)) return rc;
        put("L", p.L), put("M", p.M), put("N", p.N), put("D", p.D), put("NM", p.NM), put("k", p.k), put("c", p.c), put("esz", p.esz);
        put("ecap", p.ecap), put("o_xt", p.o_xt), put("o_y", p.o_y), put("o_z", p.o_z), put("o_dist", p.o_dist), put("o_rmax", p.o_rmax);
        put("o_kd", p.o_kd), put("o_ki", p.o_ki), put("o_val", p.o_val), put("o_eps", p.o_eps), put("o_nxt", p.o_nxt), put("o_nxn", p.o_nxn);
        put("o_temb", p.o_temb), put("o_emb", p.o_emb), put("total", p.total), put("lds", p.lds), put("tw", p.tw), put("lw", p.lw);
    } else {
        return msg = "unknown plan " + what, 1;
    }
    return 0;
}

}  // namespace

int main() {
    std::string line, what;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> what)) continue;
        std::string msg;
        g_out.clear();
        const int rc = run(what, in, msg);
        if (in.fail()) return fprintf(stderr, "short case: %s\n", line.c_str()), 2;
        if (rc) printf("err %d %s\n", rc, msg.c_str());
        else printf("ok%s\n", g_out.c_str());
    }
    return 0;
}
