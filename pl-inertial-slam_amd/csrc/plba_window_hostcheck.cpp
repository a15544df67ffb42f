// Host-compiled wrapper around plba_window.h used ONLY by tests/test_slide_plan_cpu.py: a Window is filled member by member from
// arrays, slide_plan() runs, and the next window and the plan are read back by name.  That this file compiles without any HIP header
// is the check that plba_window.h is standard-library code.  Not linked into libplba_hip.so and never used by the product path.
#include <string>
#include <type_traits>
#include "plba_window.h"
using namespace plba;

namespace {
struct Check { Window cur, next; SlidePlan plan; };

// every vector member by name; f(name, vector&)
template <class W, class F> void window_fields(W& w, F f) {
    f("vid_pvr", w.vid_pvr); f("vid_bias", w.vid_bias); f("kf0", w.kf0); f("fix_pvr", w.fix_pvr); f("fix_bias", w.fix_bias);
    f("pts", w.pts); f("lns", w.lns); f("pt_fixed", w.pt_fixed); f("ln_fixed", w.ln_fixed);
    f("po_pt", w.po_pt); f("po_kf", w.po_kf); f("lo_ln", w.lo_ln); f("lo_kf", w.lo_kf);
    f("po_uv", w.po_uv); f("po_w", w.po_w); f("lo_l", w.lo_l); f("lo_w", w.lo_w); f("level", w.level);
    f("imu_i", w.imu_i); f("imu_j", w.imu_j); f("imu_pre", w.imu_pre); f("imu_ipvr", w.imu_ipvr); f("imu_ibias", w.imu_ibias);
}
template <class F> void plan_fields(SlidePlan& p, F f) {
    f("pmap", p.pmap); f("lmap", p.lmap); f("src_lm", p.src_lm); f("src_ob", p.src_ob); f("kf_add", p.kf_add); f("add_lm", p.add_lm); f("add_ob", p.add_ob);
}
Window& pick(Check* c, int which) { return which == 0 ? c->cur : c->next; }
}  // namespace

extern "C" {
void* wc_new() { return new Check; }
void wc_free(void* h) { delete (Check*)h; }
// cur.<name> = the nbytes at data; -1: no such member
long wc_put(void* h, const char* name, const void* data, long nbytes) {
    long done = -1;
    window_fields(((Check*)h)->cur, [&](const char* n, auto& v) {
        if (std::string(n) != name) return;
        using T = typename std::remove_reference<decltype(v)>::type::value_type;
        v.assign((const T*)data, (const T*)data + nbytes / (long)sizeof(T));
        done = nbytes;
    });
    return done;
}
// bytes of <name> in cur (which 0), next (1) or the plan (2), copied to out when it has room; -1: no such member
long wc_get(void* h, int which, const char* name, void* out, long cap) {
    long bytes = -1;
    auto take = [&](const char* n, auto& v) {
        if (std::string(n) != name) return;
        bytes = (long)(v.size() * sizeof(v[0]));
        if (out && bytes && bytes <= cap) memcpy(out, v.data(), (size_t)bytes);
    };
    if (which == 2) plan_fields(((Check*)h)->plan, take); else window_fields(pick((Check*)h, which), take);
    return bytes;
}
// [K, Np, Nl, Ep, El, M, have_cam, carry_pts, carry_lns, carry_kf, carry_po, carry_lo] and [fx, fy, cx, cy, Rbc 9, Pbc 3, gw 3]
void wc_put_scalars(void* h, const int32_t* i12, const double* d19) {
    Window& w = ((Check*)h)->cur;
    w.K = i12[0]; w.Np = i12[1]; w.Nl = i12[2]; w.Ep = i12[3]; w.El = i12[4]; w.M = i12[5];
    w.have_cam = i12[6]; w.carry_pts = i12[7]; w.carry_lns = i12[8]; w.carry_kf = i12[9]; w.carry_po = i12[10]; w.carry_lo = i12[11];
    w.fx = d19[0]; w.fy = d19[1]; w.cx = d19[2]; w.cy = d19[3];
    memcpy(w.Rbc, d19 + 4, 72); memcpy(w.Pbc, d19 + 13, 24); memcpy(w.gw, d19 + 16, 24);
}
void wc_get_scalars(void* h, int which, int32_t* i12, double* d19) {
    const Window& w = pick((Check*)h, which);
    const int32_t v[12] = {w.K, w.Np, w.Nl, w.Ep, w.El, w.M, w.have_cam, w.carry_pts, w.carry_lns, w.carry_kf, w.carry_po, w.carry_lo};
    memcpy(i12, v, sizeof v);
    d19[0] = w.fx; d19[1] = w.fy; d19[2] = w.cx; d19[3] = w.cy;
    memcpy(d19 + 4, w.Rbc, 72); memcpy(d19 + 13, w.Pbc, 24); memcpy(d19 + 16, w.gw, 24);
}
// slide_plan(cur, *s, next, plan); kept[2] = the plan's Npk, Nlk
int wc_plan(void* h, const plba_slide* s, char* err, long errcap, int32_t* kept) {
    Check* c = (Check*)h;
    const int rc = slide_plan(c->cur, *s, c->next, c->plan, err, (size_t)errcap);
    kept[0] = c->plan.Npk; kept[1] = c->plan.Nlk;
    return rc;
}
// Window::clear() on next keeps the storage: returns 1 when every vector is empty, the scalars are a new Window's and no capacity shrank
int wc_clear_next_keeps_capacity(void* h) {
    Window& w = ((Check*)h)->next;
    size_t before = 0, after = 0; bool empty = true;
    window_fields(w, [&](const char*, auto& v) { before += v.capacity(); });
    w.clear();
    window_fields(w, [&](const char*, auto& v) { after += v.capacity(); empty = empty && v.empty(); });
    const bool zero = !w.have_cam && !w.K && !w.Np && !w.Nl && !w.Ep && !w.El && !w.M && !w.carry_pts && !w.carry_lns && !w.carry_kf && !w.carry_po && !w.carry_lo && w.fx == 0 && w.gw[2] == 0;
    return empty && zero && after == before && before > 0;
}
}
