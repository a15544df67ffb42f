// plba_covis.hip — the covisibility graph on the device (plba_covis_*, include/plba.h): a resident map of observation lists and the
// queries the loop thread makes on it, in place of the reference's dense full_graph (include/mapHandler.h; grown by expandGraphs,
// src/mapHandler.cpp:874-885, read by the double loop of :4373-4393).  Definition and predicates: plba_covis_dev.h.
//
// The resident map is one device block: [live | landmark starts | landmark lists || keyframe starts | keyframe lists], the landmark CSR
// as uploaded (points, then lines) and its keyframe -> landmark transpose, which the device builds: k_covis_count, k_covis_scan,
// k_covis_fill.  The fill takes a keyframe's slots with an integer atomic cursor, so the order INSIDE a keyframe's transposed list
// differs from run to run; everything downstream is an order-independent integer sum, and no output shows that order.
//
// k_covis_row, one workgroup per requested row i: it walks i's landmarks through the transpose (16 lanes to an occurrence, 16
// occurrences at a time), each landmark's list with those 16 lanes, and adds into an LDS histogram of 32-bit counters over a tile of
// COVIS_W keyframe columns with LDS integer atomics.  The tile's entries that pass the mode's predicate are then compacted in ascending
// column order, 256 columns at a time: a ballot per wave, the four waves' counts through LDS.  K > COVIS_W: a first walk finds the
// lowest and highest column the row touches, and only the tiles between them are visited; inside a tile only the touched span is
// scanned.  The kernel runs twice per query, to count and to fill (the fill checks the caller's capacity on the device), with
// k_covis_scan between the two: no size is read back first, and a query blocks the host once.
//  mode ROWS   entries C >= max(1, min_count) of the whole row                                    (plba_covis_rows)
//  mode EDGES  columns j > i, j < nv that pass covis::edge                                        (plba_covis_pose_graph)
//  mode DENSE  the counts themselves for the columns below `limit`, into a cleared array          (plba_covis_column, _local_map)
// No floating-point atomics, no waiting between workgroups, every loop bounded by a list length or by K.
#include "plba_batch_call.h"
#include "plba_covis_dev.h"

#include <cmath>

namespace plba {

constexpr int COVIS_W = 8192;      // columns of a histogram tile: 32 KiB of static LDS, 4 workgroups to a CU by LDS
constexpr int COVIS_TPB = 256, COVIS_SUB = 16;

struct CovisState {
    int K = 0, n_live = 0, Np = 0, Nl = 0;
    size_t Ep = 0, El = 0;
    DArr<char> blk;
    size_t o_live = 0, o_ls = 0, o_lk = 0, o_ks = 0, o_kl = 0;
};

namespace {

namespace cv = covis;

struct MapDev {
    int K, L, E;
    const uint8_t* live;
    const int32_t *lm_start, *lm_kf;      // L + 1, E
    const int32_t *kf_start, *kf_lm;      // K + 1, E
};

MapDev map_dev(const CovisState& st) {
    MapDev m{};
    m.K = st.K; m.L = st.Np + st.Nl; m.E = (int)(st.Ep + st.El);
    m.live = reinterpret_cast<const uint8_t*>(st.blk.p + st.o_live);
    m.lm_start = reinterpret_cast<const int32_t*>(st.blk.p + st.o_ls); m.lm_kf = reinterpret_cast<const int32_t*>(st.blk.p + st.o_lk);
    m.kf_start = reinterpret_cast<const int32_t*>(st.blk.p + st.o_ks); m.kf_lm = reinterpret_cast<const int32_t*>(st.blk.p + st.o_kl);
    return m;
}

// ---- the transpose: count, scan, fill ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_covis_count(const int32_t* lm_kf, int E, int32_t* kf_cnt) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < E) atomicAdd(&kf_cnt[lm_kf[e]], 1);      // (integer; the sum does not depend on the order)
}

// start[0 .. n] from cnt[0 .. n): one workgroup, 256 entries at a time; sums in 64 bits, stored clamped to INT32_MAX
__global__ __launch_bounds__(256) void k_covis_scan(const int32_t* cnt, int32_t* start, int n) {
    __shared__ long long sc[256];
    const int tid = threadIdx.x;
    long long carry = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + tid;
        const long long v = i < n ? cnt[i] : 0;
        sc[tid] = v;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const long long a = tid >= off ? sc[tid - off] : 0;
            __syncthreads();
            sc[tid] += a;
            __syncthreads();
        }
        const long long excl = carry + sc[tid] - v;
        if (i < n) start[i] = excl > INT32_MAX ? INT32_MAX : (int32_t)excl;
        carry += sc[255];
        __syncthreads();
    }
    if (tid == 0) start[n] = carry > INT32_MAX ? INT32_MAX : (int32_t)carry;
}

// one lane per landmark; a keyframe's slots are handed out by an integer cursor (order inside a keyframe's list: see the head of the file)
__global__ __launch_bounds__(256) void k_covis_fill(const int32_t* lm_start, const int32_t* lm_kf, int L, const int32_t* kf_start, int32_t* cursor, int32_t* kf_lm) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= L) return;
    for (int e = lm_start[l]; e < lm_start[l + 1]; ++e) {
        const int k = lm_kf[e];
        kf_lm[kf_start[k] + atomicAdd(&cursor[k], 1)] = l;
    }
}

// ---- a row ---------------------------------------------------------------------------------------------------------------------------
enum { MODE_ROWS = 0, MODE_EDGES = 1, MODE_DENSE = 2 };
struct RowDev {
    MapDev m;
    int n;                       // requested rows
    const int32_t* kf;           // their keyframes; null: row r is keyframe r
    int min_count, ess, cov, nv, limit;
    int fill;                    // 0: count into row_cnt; 1: write at row_start, provided row_start[n] + extra <= cap
    int cap, extra;
    int32_t* row_cnt;            // n
    const int32_t* row_start;    // n + 1
    int32_t *out_a, *out_b;      // ROWS: col, cnt; EDGES: ei, ej; DENSE: out_a = the dense row
};

template <int MODE>
__global__ __launch_bounds__(COVIS_TPB) void k_covis_row(RowDev d) {
    __shared__ int32_t hist[COVIS_W];
    __shared__ int s_lo, s_hi;
    __shared__ int wsum[2][4];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = tid / COVIS_SUB, sl = tid % COVIS_SUB;
    const int i = d.kf ? d.kf[r] : r;
    if (MODE != MODE_DENSE && d.fill && (long long)d.row_start[d.n] + d.extra > (long long)d.cap) return;      // too small a capacity: nothing is written
    const bool live_i = d.m.live[i] != 0;
    const int jlo = MODE == MODE_EDGES ? i + 1 : 0;
    const int jhi = MODE == MODE_EDGES ? d.nv : MODE == MODE_DENSE ? d.limit : d.m.K;
    if (!live_i || jlo >= jhi) {      // (block-uniform) a dead keyframe's row is 0; the dense row has been cleared
        if (MODE != MODE_DENSE && !d.fill && tid == 0) d.row_cnt[r] = 0;
        return;
    }
    const int chain = (MODE == MODE_EDGES && i + 1 < d.nv) ? i + 1 : -1;      // the column that is an edge without a count
    const int b0 = d.m.kf_start[i], b1 = d.m.kf_start[i + 1];
    // the walk over row i's occurrences; add(j - lo) once per entry j != i of [lo, hi)
    auto walk = [&](int lo, int hi, auto add) {
        for (int o = b0 + sub; o < b1; o += COVIS_TPB / COVIS_SUB) {
            const int l = d.m.kf_lm[o];
            cv::add_occurrence(d.m.lm_kf, d.m.lm_start[l], d.m.lm_start[l + 1], sl, COVIS_SUB, i, lo, hi, add);
        }
    };
    int t0 = jlo / COVIS_W, t1 = (jhi - 1) / COVIS_W;
    if (t1 > t0) {      // several tiles: the span of columns the row touches
        if (tid == 0) { s_lo = INT32_MAX; s_hi = -1; }
        __syncthreads();
        int lo = INT32_MAX, hi = -1;
        walk(jlo, jhi, [&](int c) { lo = c < lo ? c : lo; hi = c > hi ? c : hi; });
        if (hi >= 0) { atomicMin(&s_lo, lo + jlo); atomicMax(&s_hi, hi + jlo); }
        __syncthreads();
        lo = s_lo; hi = s_hi;
        if (chain >= 0) { lo = chain < lo ? chain : lo; hi = chain > hi ? chain : hi; }
        __syncthreads();      // (s_lo / s_hi are set again below)
        if (hi < 0) {
            if (MODE != MODE_DENSE && !d.fill && tid == 0) d.row_cnt[r] = 0;
            return;
        }
        t0 = lo / COVIS_W; t1 = hi / COVIS_W;
    }
    int total = 0, par = 0;      // entries compacted so far (the same in every lane)
    const int base_out = (MODE != MODE_DENSE && d.fill) ? d.row_start[r] : 0;
    for (int t = t0; t <= t1; ++t) {
        const int c0 = t * COVIS_W, c1 = c0 + COVIS_W < jhi ? c0 + COVIS_W : jhi;
        const int wlo = c0 > jlo ? c0 : jlo;      // the tile's column window [wlo, c1)
        for (int c = tid; c < c1 - c0; c += COVIS_TPB) hist[c] = 0;
        if (tid == 0) { s_lo = INT32_MAX; s_hi = -1; }
        __syncthreads();
        int lo = INT32_MAX, hi = -1;
        walk(wlo, c1, [&](int c) {
            const int col = c + wlo - c0;
            atomicAdd(&hist[col], 1);      // (LDS, integer, 32-bit counters)
            lo = col < lo ? col : lo; hi = col > hi ? col : hi;
        });
        if (hi >= 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
        __syncthreads();
        lo = s_lo; hi = s_hi;      // tile-relative
        if (chain >= c0 && chain < c1) { lo = chain - c0 < lo ? chain - c0 : lo; hi = chain - c0 > hi ? chain - c0 : hi; }
        if (hi >= 0) {      // (block-uniform) a tile nobody touched has no entry
            if (MODE == MODE_DENSE) {
                for (int c = lo + tid; c <= hi; c += COVIS_TPB) d.out_a[c0 + c] = cv::count(hist[c], live_i, d.m.live[c0 + c] != 0);
            } else {
                for (int cb = lo & ~(COVIS_TPB - 1); cb <= hi; cb += COVIS_TPB) {
                    const int c = cb + tid;
                    const bool in = c >= lo && c <= hi;
                    const int j = c0 + c;
                    const bool live_j = in && d.m.live[j] != 0;
                    const int cnt = in ? cv::count(hist[c], live_i, live_j) : 0;
                    const bool keep = in && (MODE == MODE_ROWS ? cv::row_entry(cnt, d.min_count) : cv::edge(cnt, i, j, live_i, live_j, d.ess, d.cov));
                    const unsigned long long mask = __ballot(keep);
                    if (lane == 0) wsum[par][wave] = __popcll(mask);
                    __syncthreads();      // (wsum alternates between two sets: the next chunk writes the other one)
                    int before = 0, all = 0;
                    for (int w = 0; w < 4; ++w) { const int s = wsum[par][w]; all += s; before += w < wave ? s : 0; }
                    if (keep && d.fill) {
                        const long long at = (long long)base_out + total + before + __popcll(mask & ((1ull << lane) - 1ull));
                        if (at < (long long)d.cap) {      // (holds by the check above; a store is never let out of the caller's capacity)
                            if (MODE == MODE_ROWS) { d.out_a[at] = j; d.out_b[at] = cnt; }
                            else { d.out_a[at] = i; d.out_b[at] = j; }
                        }
                    }
                    total += all;
                    par ^= 1;
                }
            }
        }
        __syncthreads();      // the histogram and the span are the next tile's
    }
    if (MODE != MODE_DENSE && !d.fill && tid == 0) d.row_cnt[r] = total;
}

// ---- the measurements of the covisibility edges: one lane per edge, as many as the fill wrote -----------------------------------------
__global__ __launch_bounds__(256) void k_covis_meas(const int32_t* n_edges, int extra, int cap, const int32_t* ei, const int32_t* ej, const double* pose12, double* meas12) {
    const int ne = *n_edges;
    if ((long long)ne + extra > (long long)cap) return;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < ne; e += gridDim.x * 256) {
        double Ti[12], Tj[12], Z[12];
        for (int k = 0; k < 12; ++k) { Ti[k] = pose12[12 * (size_t)ei[e] + k]; Tj[k] = pose12[12 * (size_t)ej[e] + k]; }
        cv::relative_pose(Ti, Tj, Z);
        for (int k = 0; k < 12; ++k) meas12[12 * (size_t)e + k] = Z[k];
    }
}

// ---- the local map --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_covis_local_kf(MapDev m, const int32_t* row, int kf, int cov, int min_kf, uint8_t* kf_local) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < m.K) kf_local[i] = cv::local_keyframe(m.live[i] != 0, row[i], kf, i, cov, min_kf) ? 1 : 0;
}
// a landmark is local when any keyframe of its list is (an empty list: a removed landmark, never local)
__global__ __launch_bounds__(256) void k_covis_local_lm(MapDev m, const uint8_t* kf_local, uint8_t* lm_local) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= m.L) return;
    uint8_t any = 0;
    for (int e = m.lm_start[l]; e < m.lm_start[l + 1]; ++e) any |= kf_local[m.lm_kf[e]];
    lm_local[l] = any;
}

unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

template <int MODE>
void launch_row(const RowDev& d, hipStream_t s) {
    if (d.n > 0) hipLaunchKernelGGL(k_covis_row<MODE>, dim3((unsigned)d.n), dim3(COVIS_TPB), 0, s, d);
}

const char* check_options(const plba_covis_options* o) {
    if (!o) return "no options";
    if (o->min_lm_ess_graph < 0 || o->min_lm_cov_graph < 0 || o->min_kf_local_map < 0) return "a negative option";
    return nullptr;
}

}  // namespace
}  // namespace plba

using namespace plba;

void plba_covis_discard(plba_problem* p) {
    if (!p || !p->covis) return;
    delete p->covis;
    p->covis = nullptr;
}
void plba_covis_describe(const plba_problem* p, double out6[6]) {
    for (int i = 0; i < 6; ++i) out6[i] = 0.0;
    const CovisState* st = p->covis;
    if (!st) return;
    out6[0] = st->K; out6[1] = st->n_live; out6[2] = st->Np + st->Nl; out6[3] = (double)st->Ep; out6[4] = (double)st->El; out6[5] = (double)st->blk.cls;
}

extern "C" {

void plba_covis_default_options(plba_covis_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->min_lm_ess_graph = 150; o->min_lm_cov_graph = 75; o->min_kf_local_map = 3;      // src/slamConfig.cpp:60-62
}

int plba_covis_set_map(plba_problem* p, int K, const uint8_t* live, int Np, const int32_t* pt_start, const int32_t* pt_kf, int Nl, const int32_t* ln_start,
                       const int32_t* ln_kf, double* info6) {
    if (!p) return PLBA_ERR_INVALID;
    if (K < 1) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_set_map: K = %d", K);
    if (Np < 0 || Nl < 0) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_set_map: a negative landmark count");
    if ((size_t)Np + (size_t)Nl >= (size_t)INT32_MAX) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_set_map: the landmark count does not fit int32");
    if ((Np && !pt_start) || (Nl && !ln_start)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_set_map: missing start array");
    for (int k = 0; k < 2; ++k) {
        const int n = k ? Nl : Np;
        const int32_t* st = k ? ln_start : pt_start;
        if (n)
            if (const char* why = check_starts(n, st)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_set_map: %s", why);
    }
    const size_t Ep = Np ? (size_t)pt_start[Np] : 0, El = Nl ? (size_t)ln_start[Nl] : 0, E = Ep + El;
    if (E > (size_t)INT32_MAX) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_set_map: %zu observations do not fit int32", E);
    if ((Ep && !pt_kf) || (El && !ln_kf)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_set_map: missing array");
    for (int k = 0; k < 2; ++k) {
        const size_t n = k ? El : Ep;
        const int32_t* a = k ? ln_kf : pt_kf;
        for (size_t e = 0; e < n; ++e)
            if (a[e] < 0 || a[e] >= K) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_set_map: keyframe %d in a list is outside [0, %d)", a[e], K);
    }
    const size_t L = (size_t)Np + Nl;
    // the call's block: [live | landmark starts | landmark lists || the transpose's element count]; the map's block has the same first
    // three sections at the same offsets, then [keyframe starts | keyframe lists | cursors]
    Layout Lc;
    const size_t o_live = Lc.take((size_t)K), o_ls = Lc.take(4 * (L + 1)), o_lk = Lc.take(4 * E), up_end = Lc.off, o_chk = Lc.take(16);
    Layout Lm;
    Lm.take((size_t)K); Lm.take(4 * (L + 1)); Lm.take(4 * E);
    const size_t o_ks = Lm.take(4 * ((size_t)K + 1)), o_kl = Lm.take(4 * E), o_cur = Lm.take(4 * (size_t)K);
    BatchCall call(p);
    PLBA_TRY(call.open(Lc.off, up_end, o_chk, Lc.off));
    hipStream_t s = call.s;
    int n_live = K;
    if (live) {
        uint8_t* lv = call.up<uint8_t>(o_live);
        n_live = 0;
        for (int k = 0; k < K; ++k) { lv[k] = live[k] ? 1 : 0; n_live += lv[k]; }
        memset(lv + K, 0, (0 - (size_t)K) & 15);
    } else {
        memset(call.up<uint8_t>(o_live), 1, (size_t)K);
        memset(call.up<uint8_t>(o_live) + K, 0, (0 - (size_t)K) & 15);
    }
    {      // the two CSRs as one: the lines' starts follow the points', shifted by the points' observations
        int32_t* ls = call.up<int32_t>(o_ls);
        ls[0] = 0;
        for (int l = 0; l < Np; ++l) ls[l + 1] = pt_start[l + 1];
        for (int l = 0; l < Nl; ++l) ls[(size_t)Np + l + 1] = (int32_t)(Ep + (size_t)ln_start[l + 1]);
        memset(ls + L + 1, 0, (0 - 4 * (L + 1)) & 15);
    }
    call.put(o_lk, pt_kf, 4 * Ep);
    if (El) memcpy(call.up<char>(o_lk) + 4 * Ep, ln_kf, 4 * El);
    memset(call.up<char>(o_lk) + 4 * E, 0, (0 - 4 * E) & 15);
    PLBA_TRY(call.upload());
    DArr<char> nb;      // the new map; the resident one stays until this call has succeeded
    PLBA_HIPCK(p, nb.alloc(Lm.off, false));
    PLBA_HIPCK(p, hipMemcpyAsync(nb.p, call.blk.p, up_end, hipMemcpyDeviceToDevice, s));
    int32_t *ks = reinterpret_cast<int32_t*>(nb.p + o_ks), *kl = reinterpret_cast<int32_t*>(nb.p + o_kl), *cur = reinterpret_cast<int32_t*>(nb.p + o_cur);
    const int32_t *dls = reinterpret_cast<const int32_t*>(nb.p + o_ls), *dlk = reinterpret_cast<const int32_t*>(nb.p + o_lk);
    PLBA_HIPCK(p, hipMemsetAsync(cur, 0, 4 * (size_t)K, s));
    if (E) hipLaunchKernelGGL(k_covis_count, dim3(blocks_of(E)), dim3(256), 0, s, dlk, (int)E, cur);
    hipLaunchKernelGGL(k_covis_scan, dim3(1), dim3(256), 0, s, cur, ks, K);
    PLBA_HIPCK(p, hipMemsetAsync(cur, 0, 4 * (size_t)K, s));
    if (L) hipLaunchKernelGGL(k_covis_fill, dim3(blocks_of(L)), dim3(256), 0, s, dls, dlk, (int)L, ks, cur, kl);
    PLBA_HIPCK(p, hipGetLastError());
    PLBA_HIPCK(p, hipMemcpyAsync(call.dev<char>(o_chk), ks + K, 4, hipMemcpyDeviceToDevice, s));
    PLBA_TRY(call.download());
    if ((size_t)*call.down<int32_t>(o_chk) != E) PLBA_FAIL(p, PLBA_ERR_INTERNAL, "plba_covis_set_map: the transpose holds %d entries, the lists %zu", *call.down<int32_t>(o_chk), E);
    if (!p->covis) p->covis = new CovisState;
    CovisState* st = p->covis;
    st->blk.swap(nb);      // (the former block goes back to the pool here, after the wait)
    st->K = K; st->n_live = n_live; st->Np = Np; st->Nl = Nl; st->Ep = Ep; st->El = El;
    st->o_live = o_live; st->o_ls = o_ls; st->o_lk = o_lk; st->o_ks = o_ks; st->o_kl = o_kl;
    if (info6) plba_covis_describe(p, info6);
    return PLBA_OK;
}

int plba_covis_reset(plba_problem* p) {
    if (!p) return PLBA_ERR_INVALID;
    if (!p->covis) return PLBA_OK;
    PLBA_HIPCK(p, hipSetDevice(p->device));
    PLBA_HIPCK(p, plba_stream_wait(p->stream));      // (uncounted; the calls that use the map have waited already)
    plba_covis_discard(p);
    return PLBA_OK;
}

int plba_covis_rows(plba_problem* p, int n, const int32_t* kf, int min_count, int32_t* row_start, int cap, int32_t* col, int32_t* cnt) {
    if (!p) return PLBA_ERR_INVALID;
    const CovisState* st = p->covis;
    if (!st) PLBA_FAIL(p, PLBA_ERR_STATE, "plba_covis_rows: no map (plba_covis_set_map)");
    if (n < 0 || cap < 0 || min_count < 0) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_rows: a negative count");
    if (!row_start || (n && !kf) || (cap && (!col || !cnt))) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_rows: missing array");
    for (int r = 0; r < n; ++r)
        if (kf[r] < 0 || kf[r] >= st->K) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_rows: keyframe %d is outside [0, %d)", kf[r], st->K);
    // [keyframes || row starts | col | cnt | row counts]
    Layout L;
    const size_t o_kf = L.take(4 * (size_t)n), up_end = L.off, o_rs = L.take(4 * ((size_t)n + 1)), o_col = L.take(4 * (size_t)cap), o_cnt = L.take(4 * (size_t)cap),
                 down_end = L.off, o_rc = L.take(4 * (size_t)n);
    BatchCall call(p);
    PLBA_TRY(call.open(L.off, up_end, o_rs, down_end));
    call.put(o_kf, kf, 4 * (size_t)n);
    PLBA_TRY(call.upload());
    RowDev d{};
    d.m = map_dev(*st); d.n = n; d.kf = call.dev<int32_t>(o_kf); d.min_count = min_count; d.cap = cap;
    d.row_cnt = call.dev<int32_t>(o_rc); d.row_start = call.dev<int32_t>(o_rs); d.out_a = call.dev<int32_t>(o_col); d.out_b = call.dev<int32_t>(o_cnt);
    launch_row<MODE_ROWS>(d, call.s);
    hipLaunchKernelGGL(k_covis_scan, dim3(1), dim3(256), 0, call.s, d.row_cnt, call.dev<int32_t>(o_rs), n);
    d.fill = 1;
    launch_row<MODE_ROWS>(d, call.s);
    PLBA_HIPCK(p, hipGetLastError());
    PLBA_TRY(call.download());
    const int32_t* rs = call.down<int32_t>(o_rs);
    if (rs[n] > cap) {
        row_start[n] = rs[n];      // the needed capacity, and nothing else
        PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_rows: cap = %d, the rows have %d entries%s", cap, rs[n], rs[n] == INT32_MAX ? " or more" : "");
    }
    memcpy(row_start, rs, 4 * ((size_t)n + 1));
    if (rs[n]) { memcpy(col, call.down<int32_t>(o_col), 4 * (size_t)rs[n]); memcpy(cnt, call.down<int32_t>(o_cnt), 4 * (size_t)rs[n]); }
    return PLBA_OK;
}

int plba_covis_column(plba_problem* p, int idx, int32_t* cov) {
    if (!p) return PLBA_ERR_INVALID;
    const CovisState* st = p->covis;
    if (!st) PLBA_FAIL(p, PLBA_ERR_STATE, "plba_covis_column: no map (plba_covis_set_map)");
    if (idx < 0 || idx >= st->K) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_column: keyframe %d is outside [0, %d)", idx, st->K);
    if (idx && !cov) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_column: missing array");
    if (!idx) return PLBA_OK;
    Layout L;
    const size_t o_kf = L.take(4), up_end = L.off, o_row = L.take(4 * (size_t)idx);
    BatchCall call(p);
    PLBA_TRY(call.open(L.off, up_end, o_row, L.off));
    const int32_t kf = idx;
    call.put(o_kf, &kf, 4);
    PLBA_TRY(call.upload());
    PLBA_HIPCK(p, hipMemsetAsync(call.dev<char>(o_row), 0, 4 * (size_t)idx, call.s));
    RowDev d{};
    d.m = map_dev(*st); d.n = 1; d.kf = call.dev<int32_t>(o_kf); d.limit = idx; d.out_a = call.dev<int32_t>(o_row);
    launch_row<MODE_DENSE>(d, call.s);
    PLBA_HIPCK(p, hipGetLastError());
    PLBA_TRY(call.download());
    memcpy(cov, call.down<int32_t>(o_row), 4 * (size_t)idx);
    return PLBA_OK;
}

int plba_covis_pose_graph(plba_problem* p, const plba_covis_options* opt, int nv, const double* pose12, int n_loop, const int32_t* loop_ij, const double* loop_meas12,
                          int edge_cap, int32_t* ei, int32_t* ej, double* meas12, int* ne) {
    if (!p) return PLBA_ERR_INVALID;
    const CovisState* st = p->covis;
    if (!st) PLBA_FAIL(p, PLBA_ERR_STATE, "plba_covis_pose_graph: no map (plba_covis_set_map)");
    if (const char* why = check_options(opt)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_pose_graph: %s", why);
    if (nv < 1 || nv > st->K) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_pose_graph: nv = %d is outside 1 .. K = %d", nv, st->K);
    if (n_loop < 0 || edge_cap < 0) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_pose_graph: a negative count");
    if (!pose12 || !ne || (n_loop && (!loop_ij || !loop_meas12)) || (edge_cap && (!ei || !ej || !meas12))) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_pose_graph: missing array");
    for (int e = 0; e < n_loop; ++e) {
        const int a = loop_ij[2 * e], b = loop_ij[2 * e + 1];
        if (a < 0 || a >= nv || b < 0 || b >= nv || a == b) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_pose_graph: loop edge %d joins %d and %d", e, a, b);
    }
    for (size_t k = 0; k < 12 * (size_t)nv; ++k) if (!std::isfinite(pose12[k])) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_pose_graph: a non-finite pose");
    for (size_t k = 0; k < 12 * (size_t)n_loop; ++k) if (!std::isfinite(loop_meas12[k])) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_pose_graph: a non-finite loop measurement");
    // [poses || row starts | the covisibility edges' count | ei | ej | meas12 | row counts]; the down span begins at the count
    Layout L;
    const size_t o_pose = L.take(96 * (size_t)nv), up_end = L.off, o_rs = L.take(4 * ((size_t)nv + 1)), o_ne = L.take(4);
    const size_t o_ei = L.take(4 * (size_t)edge_cap), o_ej = L.take(4 * (size_t)edge_cap), o_z = L.take(96 * (size_t)edge_cap), down_end = L.off, o_rc = L.take(4 * (size_t)nv);
    BatchCall call(p);
    PLBA_TRY(call.open(L.off, up_end, o_ne, down_end));
    call.put(o_pose, pose12, 96 * (size_t)nv);
    PLBA_TRY(call.upload());
    RowDev d{};
    d.m = map_dev(*st); d.n = nv; d.kf = nullptr; d.ess = opt->min_lm_ess_graph; d.cov = opt->min_lm_cov_graph; d.nv = nv; d.cap = edge_cap; d.extra = n_loop;
    d.row_cnt = call.dev<int32_t>(o_rc); d.row_start = call.dev<int32_t>(o_rs); d.out_a = call.dev<int32_t>(o_ei); d.out_b = call.dev<int32_t>(o_ej);
    launch_row<MODE_EDGES>(d, call.s);
    hipLaunchKernelGGL(k_covis_scan, dim3(1), dim3(256), 0, call.s, d.row_cnt, call.dev<int32_t>(o_rs), nv);
    PLBA_HIPCK(p, hipMemcpyAsync(call.dev<char>(o_ne), call.dev<int32_t>(o_rs) + nv, 4, hipMemcpyDeviceToDevice, call.s));
    d.fill = 1;
    launch_row<MODE_EDGES>(d, call.s);
    if (edge_cap)
        hipLaunchKernelGGL(k_covis_meas, dim3(std::min(blocks_of((size_t)edge_cap), 1024u)), dim3(256), 0, call.s, call.dev<int32_t>(o_ne), n_loop, edge_cap, d.out_a, d.out_b,
                           call.dev<double>(o_pose), call.dev<double>(o_z));
    PLBA_HIPCK(p, hipGetLastError());
    PLBA_TRY(call.download());
    const int n_cov = *call.down<int32_t>(o_ne);
    const long long need = (long long)n_cov + n_loop;
    if (need > (long long)edge_cap) {
        *ne = need > INT32_MAX ? INT32_MAX : (int)need;      // the needed capacity, and nothing else
        PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_pose_graph: edge_cap = %d, the graph has %lld edges", edge_cap, need);
    }
    if (n_cov) {
        memcpy(ei, call.down<int32_t>(o_ei), 4 * (size_t)n_cov); memcpy(ej, call.down<int32_t>(o_ej), 4 * (size_t)n_cov);
        memcpy(meas12, call.down<double>(o_z), 96 * (size_t)n_cov);
    }
    for (int e = 0; e < n_loop; ++e) { ei[n_cov + e] = loop_ij[2 * e]; ej[n_cov + e] = loop_ij[2 * e + 1]; }      // the loop edges follow, in the order given
    if (n_loop) memcpy(meas12 + 12 * (size_t)n_cov, loop_meas12, 96 * (size_t)n_loop);
    *ne = (int)need;
    return PLBA_OK;
}

int plba_covis_local_map(plba_problem* p, const plba_covis_options* opt, int kf, uint8_t* kf_local, uint8_t* pt_local, uint8_t* ln_local, int32_t* counts3) {
    if (!p) return PLBA_ERR_INVALID;
    const CovisState* st = p->covis;
    if (!st) PLBA_FAIL(p, PLBA_ERR_STATE, "plba_covis_local_map: no map (plba_covis_set_map)");
    if (const char* why = check_options(opt)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_local_map: %s", why);
    if (kf < 0 || kf >= st->K) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_local_map: keyframe %d is outside [0, %d)", kf, st->K);
    if (!kf_local || !counts3 || (st->Np && !pt_local) || (st->Nl && !ln_local)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_covis_local_map: missing array");
    const size_t K = (size_t)st->K, Lm = (size_t)st->Np + st->Nl;
    // [keyframe || keyframe flags | landmark flags | the dense row]
    Layout L;
    const size_t o_kf = L.take(4), up_end = L.off, o_fk = L.take(K), o_fl = L.take(Lm), down_end = L.off, o_row = L.take(4 * K);
    BatchCall call(p);
    PLBA_TRY(call.open(L.off, up_end, o_fk, down_end));
    const int32_t k32 = kf;
    call.put(o_kf, &k32, 4);
    PLBA_TRY(call.upload());
    PLBA_HIPCK(p, hipMemsetAsync(call.dev<char>(o_row), 0, 4 * K, call.s));
    RowDev d{};
    d.m = map_dev(*st); d.n = 1; d.kf = call.dev<int32_t>(o_kf); d.limit = st->K; d.out_a = call.dev<int32_t>(o_row);
    launch_row<MODE_DENSE>(d, call.s);
    hipLaunchKernelGGL(k_covis_local_kf, dim3(blocks_of(K)), dim3(256), 0, call.s, d.m, call.dev<int32_t>(o_row), kf, opt->min_lm_cov_graph, opt->min_kf_local_map,
                       call.dev<uint8_t>(o_fk));
    if (Lm) hipLaunchKernelGGL(k_covis_local_lm, dim3(blocks_of(Lm)), dim3(256), 0, call.s, d.m, call.dev<uint8_t>(o_fk), call.dev<uint8_t>(o_fl));
    PLBA_HIPCK(p, hipGetLastError());
    PLBA_TRY(call.download());
    memcpy(kf_local, call.down<uint8_t>(o_fk), K);
    const uint8_t* fl = call.down<uint8_t>(o_fl);
    if (st->Np) memcpy(pt_local, fl, (size_t)st->Np);
    if (st->Nl) memcpy(ln_local, fl + st->Np, (size_t)st->Nl);
    int32_t c3[3] = {0, 0, 0};
    for (size_t i = 0; i < K; ++i) c3[0] += kf_local[i];
    for (size_t l = 0; l < Lm; ++l) c3[l < (size_t)st->Np ? 1 : 2] += fl[l];
    memcpy(counts3, c3, sizeof c3);
    return PLBA_OK;
}

}  // extern "C"
