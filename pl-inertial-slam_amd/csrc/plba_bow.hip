// plba_bow.hip — place recognition on the device (plba_bow_*, include/plba.h): DBoW2's vocabulary-tree transform, the L1 score against
// a device-resident database of bag-of-words vectors, the three insertKFBowVector* scores (src/mapHandler.cpp:3116-3237) and
// lookForLoopCandidates (:3239-3299).
//
// Mapping, all B keyframes and both kinds in each launch:
//  k_bow_descend   one lane per descriptor, the descriptor in 8 registers.  The root's children pass through LDS in tiles (every lane
//                  reads them: a broadcast read); deeper levels read a node's children, which the plan made contiguous, from memory.
//  k_bow_build     one workgroup per (keyframe, kind): the word ids are sorted in LDS (bitonic, stopped words behind the others), the
//                  run heads are numbered by a scan, a head's lane adds the word's weight once per occurrence, lane 0 sums the norm in
//                  ascending word id; the vector goes to the call's output and, for an insert, to the database.  Waves 0 and 1 first
//                  compute vector_stdv of x and y in the lane-tree order.
//  k_bow_score     work items over (inserted keyframe, chunk of database keyframes, kind): the query vector sits sorted in LDS, a
//                  wave takes one stored vector at a time, reads it coalesced, looks every word up by bisection and sums the terms in
//                  the lane-tree order.
//  k_bow_decide    one workgroup per inserted keyframe: the mode's score, the float column, lc_min_score as a minimum, the eligible
//                  count, the best entries by repeated (first index, arg-max) reductions, n_closest as a count.
// The database keeps, per kind, one pool of ids and one of values, a keyframe's vector at the offset its descriptor rows gave it (a
// vector has at most as many entries as the keyframe has descriptors, so the offsets are known before the device has counted), and
// (offset, nnz) per keyframe.  The pools grow geometrically by a copy on the stream; the blocks they leave are released after the
// call's wait.  The arithmetic is plba_bow_dev.h, shared with the host check and include/plba_g2o/bow.h.  The host side of the
// transform and the insert (one block, one copy up, one down, one wait) is plba_batch_call.h's.
#include "plba_batch_call.h"
#include "plba_bow_dev.h"

namespace plba {

struct BowVoc {
    bool set = false;
    int n_nodes = 0, n_words = 0, weighting = 0;
    DArr<char> blk;      // [desc | child0 | nchild | word | weight | word_weight]
    size_t o_desc = 0, o_c0 = 0, o_nc = 0, o_word = 0, o_w = 0, o_ww = 0;
};
struct BowState {
    BowVoc voc[2];
    int n = 0, n_live = 0;
    std::vector<uint8_t> live;
    size_t used[2] = {0, 0}, nnz[2] = {0, 0};      // pool entries handed out; entries the vectors really have
    DArr<char> ids[2], vals[2], meta[2];           // int32 | double | int2 (offset, nnz) per keyframe
    void drop_db() {
        n = n_live = 0; live.clear();
        for (int k = 0; k < 2; ++k) { used[k] = nnz[k] = 0; ids[k].release(); vals[k].release(); meta[k].release(); }
    }
};

namespace {

namespace mt = match;
namespace bw = bow;

struct VocDev {
    const uint4* desc;
    const int32_t *child0, *nchild, *word;
    const double *weight, *word_weight;
    int weighting;
};

__device__ __forceinline__ mt::Desc to_desc(const uint4& lo, const uint4& hi) {
    mt::Desc d;
    d.w[0] = lo.x; d.w[1] = lo.y; d.w[2] = lo.z; d.w[3] = lo.w; d.w[4] = hi.x; d.w[5] = hi.y; d.w[6] = hi.z; d.w[7] = hi.w;
    return d;
}

// ---- (a) descent ------------------------------------------------------------------------------------------------------------------
constexpr int ROOT_TILE = 128;      // children of the root that pass through LDS at a time
struct DescendDev {
    VocDev vp, vl;
    const uint4* desc;      // the points' rows, then the lines'
    int Np, Nl;
    int32_t* word;          // per row
};

__global__ __launch_bounds__(256) void k_bow_descend(DescendDev d) {
    __shared__ uint4 tile[2 * ROOT_TILE];
    const int nbp = (d.Np + 255) >> 8;
    const int kind = (int)blockIdx.x >= nbp ? 1 : 0;
    // (every field chosen into a local: indexing the argument block by `kind` would put it in scratch)
    const uint4* vdesc = kind ? d.vl.desc : d.vp.desc;
    const int32_t *child0 = kind ? d.vl.child0 : d.vp.child0, *nchild = kind ? d.vl.nchild : d.vp.nchild, *vword = kind ? d.vl.word : d.vp.word;
    const double* weight = kind ? d.vl.weight : d.vp.weight;
    const int n = kind ? d.Nl : d.Np, tid = threadIdx.x;
    const int g = ((int)blockIdx.x - (kind ? nbp : 0)) * 256 + tid;
    const size_t row = (size_t)(kind ? d.Np : 0) + (size_t)g;
    const bool live = g < n;
    uint4 ql = make_uint4(0, 0, 0, 0), qh = make_uint4(0, 0, 0, 0);
    if (live) { ql = d.desc[2 * row]; qh = d.desc[2 * row + 1]; }
    const mt::Desc q = to_desc(ql, qh);
    const int nroot = nchild[0], c0 = child0[0];
    int node = c0, bd = mt::NONE;
    for (int t0 = 0; t0 < nroot; t0 += ROOT_TILE) {
        const int m = nroot - t0 < ROOT_TILE ? nroot - t0 : ROOT_TILE;
        __syncthreads();      // the previous tile has been compared
        for (int e = tid; e < 2 * m; e += 256) tile[e] = vdesc[2 * (size_t)(c0 + t0) + e];
        __syncthreads();
        for (int r = 0; r < m; ++r) {
            const int dist = mt::distance(q, to_desc(tile[2 * r], tile[2 * r + 1]));
            if (dist < bd) { bd = dist; node = c0 + t0 + r; }      // strict: the first of equal distances stays
        }
    }
    if (!live) return;
    for (;;) {
        const int nc = nchild[node];
        if (nc == 0) break;
        const int cc = child0[node];
        int best = cc;
        bd = mt::NONE;
        for (int c = 0; c < nc; ++c) {
            const uint4 lo = vdesc[2 * (size_t)(cc + c)], hi = vdesc[2 * (size_t)(cc + c) + 1];
            const int dist = mt::distance(q, to_desc(lo, hi));
            if (dist < bd) { bd = dist; best = cc + c; }
        }
        node = best;      // a child's index is above its parent's: the walk ends
    }
    d.word[row] = weight[node] > 0.0 ? vword[node] : -1;      // :1073: "not stopped" is w > 0
}

// ---- the lane-tree sum of a wave (plba_bow_dev.h): lane l holds the chain of the terms l, l + 64, ...; every lane gets the sum -------
__device__ __forceinline__ double wave_tree(double part) {
#pragma unroll
    for (int o = bw::LANES / 2; o >= 1; o >>= 1) part = part + __shfl_xor(part, o);
    return part;
}

// ---- (b) the bag-of-words vector ----------------------------------------------------------------------------------------------------
struct BuildDev {
    int B, n0, Np, NP;                        // keyframes; database size before the call; point rows; LDS entries (a power of two)
    const int32_t *start_p, *start_l;         // B + 1 each
    const int32_t* word;                      // per row (points, then lines)
    const double *ww_p, *ww_l;                // a word's weight
    int acc_p, acc_l;                         // addWeight (1) or addIfNotExist (0)
    int32_t* out_id; double* out_val;         // per row; a set's vector begins at its first row
    int32_t* out_nnz;                         // [kind * B + b]
    int32_t *db_id_p, *db_id_l;               // the database (null: plba_bow_transform)
    double *db_val_p, *db_val_l;
    int2 *meta_p, *meta_l;
    int used_p, used_l;                       // pool offset of the call's first row
    const double *pos_p, *pos_l;              // 2 / 4 doubles per row of the kind (null: no dispersion term)
    double* stat;                             // [2 * b + kind]: vector_stdv(x) + vector_stdv(y)
};

// vector_stdv (stvo-pl/src/auxiliar.cpp:504-513) of one coordinate by one wave; lines: the midpoint (spl + epl) * 0.5
__device__ __forceinline__ double wave_stdv(const double* pos, int n, int kind, int coord, int lane) {
    auto at = [&](int j) { return kind ? (pos[4 * (size_t)j + coord] + pos[4 * (size_t)j + 2 + coord]) * 0.5 : pos[2 * (size_t)j + coord]; };
    double part = 0.0;
    for (int j = lane; j < n; j += bw::LANES) part += at(j);
    const double mean = wave_tree(part) / (double)n;
    part = 0.0;
    for (int j = lane; j < n; j += bw::LANES) { const double c = at(j) - mean; part += c * c; }
    return bw::stdv_finish(n, wave_tree(part));
}

__global__ __launch_bounds__(256) void k_bow_build(BuildDev d) {
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    __shared__ int sc[256];
    __shared__ int carry;
    __shared__ double s_norm, s_std[2];
    double* vals = s_dyn;
    int32_t* keys = reinterpret_cast<int32_t*>(s_dyn + d.NP);
    const int b = blockIdx.x, kind = blockIdx.y, tid = threadIdx.x;
    const int32_t* start = kind ? d.start_l : d.start_p;
    const int r0 = start[b], n = start[b + 1] - r0;
    const size_t row0 = (size_t)(kind ? d.Np : 0) + (size_t)r0;
    const double* ww = kind ? d.ww_l : d.ww_p;
    const int acc = kind ? d.acc_l : d.acc_p;
    int32_t* db_id = kind ? d.db_id_l : d.db_id_p;
    double* db_val = kind ? d.db_val_l : d.db_val_p;
    int2* meta = kind ? d.meta_l : d.meta_p;
    const int db0 = (kind ? d.used_l : d.used_p) + r0;
    const double* pos = kind ? d.pos_l : d.pos_p;
    if (d.stat && tid < 2 * bw::LANES) {
        const double s = pos ? wave_stdv(pos + (kind ? 4 : 2) * (size_t)r0, n, kind, tid >> 6, tid & 63) : 0.0;
        if ((tid & 63) == 0) s_std[tid >> 6] = s;
    }
    int npad = 1;
    while (npad < n) npad <<= 1;
    for (int i = tid; i < npad; i += 256) {
        const int w = i < n ? d.word[row0 + i] : -1;
        keys[i] = w >= 0 ? w : bw::STOPPED;
    }
    if (tid == 0) carry = 0;
    __syncthreads();
    if (d.stat && tid == 0) d.stat[2 * (size_t)b + kind] = s_std[0] + s_std[1];
    for (int k = 2; k <= npad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < npad; i += 256) {
                const int x = i ^ j;
                if (x > i) {
                    const int a = keys[i], c = keys[x];
                    if (((i & k) == 0) ? (a > c) : (a < c)) { keys[i] = c; keys[x] = a; }
                }
            }
            __syncthreads();
        }
    for (int base = 0; base < n; base += 256) {
        const int i = base + tid;
        const int key = i < n ? keys[i] : bw::STOPPED;
        const int head = (key != bw::STOPPED && (i == 0 || keys[i - 1] != key)) ? 1 : 0;
        sc[tid] = head;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int a = tid >= off ? sc[tid - off] : 0;
            __syncthreads();
            sc[tid] += a;
            __syncthreads();
        }
        if (head) {
            const int at = carry + sc[tid] - 1;
            const double w = ww[key];
            double v = w;
            if (acc) for (int c = i + 1; c < n && keys[c] == key; ++c) v += w;      // addWeight: once per occurrence
            vals[at] = v;
            d.out_id[row0 + at] = key;
            if (db_id) db_id[(size_t)db0 + at] = key;
        }
        __syncthreads();
        if (tid == 255) carry += sc[255];
        __syncthreads();
    }
    const int nnz = carry;
    if (tid == 0) {
        double norm = 0.0;
        for (int e = 0; e < nnz; ++e) norm += fabs(vals[e]);      // BowVector.cpp:68-69, ascending word id
        s_norm = norm;
        d.out_nnz[(size_t)kind * d.B + b] = nnz;
        if (meta) meta[d.n0 + b] = make_int2(db0, nnz);
    }
    __syncthreads();
    const double norm = s_norm;
    for (int e = tid; e < nnz; e += 256) {
        const double v = norm > 0.0 ? vals[e] / norm : vals[e];
        d.out_val[row0 + e] = v;
        if (db_val) db_val[(size_t)db0 + e] = v;
    }
}

// ---- (c) scores ----------------------------------------------------------------------------------------------------------------------
constexpr int SCORE_CHUNK = 64;      // database keyframes of one work item: 16 per wave
struct ScoreDev {
    int B, n0, NQ;                   // NQ: LDS entries, at least the longest query vector
    const uint8_t* live;             // n0
    const int32_t *id_p, *id_l;
    const double *val_p, *val_l;
    const int2 *meta_p, *meta_l;
    double *sp, *sl;                 // rows as bow::score_row
    int use_p, use_l;
};

__global__ __launch_bounds__(256) void k_bow_score(ScoreDev d) {
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    double* qv = s_dyn;
    int32_t* qi = reinterpret_cast<int32_t*>(s_dyn + d.NQ);
    const int b = blockIdx.y >> 1, kind = blockIdx.y & 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int idx = d.n0 + b, i0 = (int)blockIdx.x * SCORE_CHUNK;
    if (i0 > idx) return;
    const int i1 = i0 + SCORE_CHUNK < idx + 1 ? i0 + SCORE_CHUNK : idx + 1;
    double* out = (kind ? d.sl : d.sp) + bw::score_row(b, d.n0);
    if (!(kind ? d.use_l : d.use_p)) {
        for (int i = i0 + tid; i < i1; i += 256) out[i] = 0.0;
        return;
    }
    const int32_t* ids = kind ? d.id_l : d.id_p;
    const double* vals = kind ? d.val_l : d.val_p;
    const int2* meta = kind ? d.meta_l : d.meta_p;
    const int2 mq = meta[idx];
    const int nq = mq.y;
    for (int e = tid; e < nq; e += 256) { qi[e] = ids[(size_t)mq.x + e]; qv[e] = vals[(size_t)mq.x + e]; }
    __syncthreads();
    for (int i = i0 + wave; i < i1; i += 4) {
        if (i < d.n0 && !d.live[i]) {      // map_keyframes[i] == NULL: the entry is never written
            if (lane == 0) out[i] = 0.0;
            continue;
        }
        const int2 m = meta[i];
        double part = 0.0;
        for (int j = lane; j < m.y; j += bw::LANES) {
            const int k = bw::find_word(qi, nq, ids[(size_t)m.x + j]);
            part += k >= 0 ? bw::l1_term(qv[k], vals[(size_t)m.x + j]) : 0.0;
        }
        const double s = bw::l1_finish(wave_tree(part));
        if (lane == 0) out[i] = s;
    }
}

// ---- (d) the decision ---------------------------------------------------------------------------------------------------------------
constexpr int CAND_I = 4 + bw::TOPK_MAX, CAND_D = 2 + bw::TOPK_MAX;
struct DecideDev {
    int B, n0, mode, topk, lc_kf_dist, lc_kf_max_dist, lc_nkf_closest, min_lm_cov_graph, min_kf_local_map;
    const uint8_t* live;
    const int32_t *start_p, *start_l;
    const double* stat;
    const double *sp, *sl;
    double* s; float* sf;
    const int32_t* cov;      // rows as bow::cov_row; null: no decision
    int32_t* cand_i;         // B x CAND_I: is_candidate, kf_prev, n_closest, n_eligible, topk
    double* cand_d;          // B x CAND_D: best_score, lc_min_score, topk_score
};

__device__ __forceinline__ int block_sum(int v, int* sh) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) sh[tid] += sh[tid + o]; __syncthreads(); }
    return sh[0];
}
__device__ __forceinline__ int block_min(int v, int* sh) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o && sh[tid + o] < sh[tid]) sh[tid] = sh[tid + o]; __syncthreads(); }
    return sh[0];
}
__device__ __forceinline__ double block_min(double v, double* sh) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o && sh[tid + o] < sh[tid]) sh[tid] = sh[tid + o]; __syncthreads(); }
    return sh[0];
}
// the entry with the largest value, the lowest index among equal ones; an index of INT32_MAX is "none"
__device__ __forceinline__ void arg_better(float& v, int& i, float v2, int i2) {
    if (i2 == INT32_MAX) return;
    if (i == INT32_MAX || v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}
__device__ __forceinline__ int block_argmax(float v, int i, float* shv, int* shi) {
    const int tid = threadIdx.x;
    __syncthreads();
    shv[tid] = v; shi[tid] = i;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { float a = shv[tid]; int ai = shi[tid]; arg_better(a, ai, shv[tid + o], shi[tid + o]); shv[tid] = a; shi[tid] = ai; }
        __syncthreads();
    }
    return shi[0];
}

__global__ __launch_bounds__(256) void k_bow_decide(DecideDev d) {
    __shared__ int shi[256];
    __shared__ float shf[256];
    __shared__ double shd[256];
    __shared__ int taken[bw::TOPK_MAX];
    const int b = blockIdx.x, tid = threadIdx.x, idx = d.n0 + b;
    const size_t row = bw::score_row(b, d.n0);
    const int n_pt = d.start_p[b + 1] - d.start_p[b], n_ls = d.start_l[b + 1] - d.start_l[b];
    const double std_pt = d.stat[2 * (size_t)b], std_ls = d.stat[2 * (size_t)b + 1];
    for (int i = tid; i <= idx; i += 256) {
        double s = 0.0;
        if (!(i < d.n0 && !d.live[i])) s = bw::mode_score(d.mode, d.sp[row + i], d.sl[row + i], n_pt, n_ls, std_pt, std_ls);
        d.s[row + i] = s;
        d.sf[row + i] = (float)s;      // conf_matrix is vector<vector<float>>
    }
    if (!d.cov) return;
    __syncthreads();      // the column is read by other lanes below
    const float* col = d.sf + row;
    const int32_t* cov = d.cov + bw::cov_row(b, d.n0);
    auto is_live = [&](int i) { return i >= d.n0 || d.live[i] != 0; };
    int n_el = 0;
    double mn = 1.0;
    for (int i = tid; i < idx; i += 256) {
        n_el += bw::eligible(i, idx, d.lc_kf_dist, is_live(i)) ? 1 : 0;
        if (bw::in_min_scan(cov[i], i, idx, d.min_lm_cov_graph, d.min_kf_local_map)) {
            const double s = col[i];
            if (s < mn && s > 0.001) mn = s;
        }
    }
    n_el = block_sum(n_el, shi);
    const double lc_min = block_min(mn, shd);
    int32_t* ci = d.cand_i + (size_t)CAND_I * b;
    double* cd = d.cand_d + (size_t)CAND_D * b;
    const int rounds = d.topk > 1 ? d.topk : 1;
    int idx_max = -1, n_taken = 0;
    float best = 0.0f;
    for (int r = 0; r < rounds; ++r) {
        // the pinned scan: its start is the first entry left; a NaN there stays, otherwise the largest entry wins, the lowest index first
        int first = INT32_MAX, ai = INT32_MAX;
        float av = 0.0f;
        for (int i = tid; i < idx; i += 256) {
            if (!bw::eligible(i, idx, d.lc_kf_dist, is_live(i))) continue;
            bool gone = false;
            for (int t = 0; t < n_taken; ++t) gone = gone || taken[t] == i;
            if (gone) continue;
            if (i < first) first = i;
            const float v = col[i];
            if (v == v) arg_better(av, ai, v, i);
        }
        first = block_min(first, shi);
        if (first == INT32_MAX) break;      // (block-uniform)
        const int am = block_argmax(av, ai, shf, shi);
        const float fv = col[first];
        const int pick = (fv != fv) ? first : am;
        if (r == 0) { idx_max = pick; best = col[pick]; }
        __syncthreads();
        if (tid == 0) {
            taken[n_taken] = pick;
            if (r < d.topk) { ci[4 + r] = pick; cd[2 + r] = (double)col[pick]; }
        }
        ++n_taken;
        __syncthreads();
    }
    int n_closest = 0;
    const bool passes = idx_max >= 0 && (double)best >= lc_min;
    if (passes)
        for (int i = tid; i < idx; i += 256) {
            if (i == idx_max || !bw::eligible(i, idx, d.lc_kf_dist, is_live(i))) continue;
            const int gap = i > idx_max ? i - idx_max : idx_max - i;
            n_closest += (gap <= d.lc_kf_max_dist && (double)col[i] >= lc_min * 0.8) ? 1 : 0;
        }
    n_closest = block_sum(n_closest, shi);
    if (tid == 0) {
        const int is_cand = (n_el > d.lc_kf_max_dist && passes && n_closest >= d.lc_nkf_closest) ? 1 : 0;
        ci[0] = is_cand; ci[1] = is_cand ? idx_max : -1; ci[2] = n_closest; ci[3] = n_el;
        cd[0] = idx_max >= 0 ? (double)best : 0.0; cd[1] = lc_min;
        for (int r = n_taken < d.topk ? n_taken : d.topk; r < bw::TOPK_MAX; ++r) { ci[4 + r] = -1; cd[2 + r] = 0.0; }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// the text for a keyframe with more than bw::MAX_DESC rows of one kind
constexpr const char* TOO_MANY_DESC = "more than 8192 descriptors of one kind in one keyframe";
static_assert(bw::MAX_DESC == 8192, "TOO_MANY_DESC names the limit");
int max_rows(int B, const int32_t* st) {
    int m = 0;
    for (int b = 0; b < B; ++b) m = std::max(m, st[b + 1] - st[b]);
    return m;
}
int pow2_at_least(int n) { int p = 1; while (p < n) p <<= 1; return p; }

VocDev voc_dev(const BowVoc& v) {
    VocDev d{};
    if (!v.set) return d;
    d.desc = reinterpret_cast<const uint4*>(v.blk.p + v.o_desc);
    d.child0 = reinterpret_cast<const int32_t*>(v.blk.p + v.o_c0); d.nchild = reinterpret_cast<const int32_t*>(v.blk.p + v.o_nc);
    d.word = reinterpret_cast<const int32_t*>(v.blk.p + v.o_word);
    d.weight = reinterpret_cast<const double*>(v.blk.p + v.o_w); d.word_weight = reinterpret_cast<const double*>(v.blk.p + v.o_ww);
    d.weighting = v.weighting;
    return d;
}

// room for `need` bytes in a pool that holds `used`: a larger block and a copy on the stream; the old block goes to `old`, which the
// caller releases after its wait
hipError_t grow(DArr<char>& a, size_t used, size_t need, DArr<char>& old, hipStream_t s) {
    if (a.p && need <= a.cls) return hipSuccess;
    DArr<char> nb;
    hipError_t e = nb.alloc(std::max(need, 2 * a.cls), false);
    if (e != hipSuccess) return e;
    if (a.p && used) e = hipMemcpyAsync(nb.p, a.p, used, hipMemcpyDeviceToDevice, s);
    a.swap(nb);
    old.swap(nb);
    return e;
}

// the descent and the build of one call; dyn LDS of the build: NP entries
hipError_t transform_launch(const DescendDev& t, const BuildDev& bd, hipStream_t s) {
    const int blocks = ((t.Np + 255) >> 8) + ((t.Nl + 255) >> 8);
    if (blocks) hipLaunchKernelGGL(k_bow_descend, dim3((unsigned)blocks), dim3(256), 0, s, t);
    const size_t lds = 12 * (size_t)bd.NP;
    hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(k_bow_build), 12 * bw::MAX_DESC);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bow_build, dim3((unsigned)bd.B, 2), dim3(256), lds, s, bd);
    return hipGetLastError();
}

}  // namespace
}  // namespace plba

using namespace plba;

void plba_bow_discard(plba_problem* p) {
    if (!p || !p->bow) return;
    delete p->bow;
    p->bow = nullptr;
}
void plba_bow_describe(const plba_problem* p, double out5[5]) {
    for (int i = 0; i < 5; ++i) out5[i] = 0.0;
    const BowState* st = p->bow;
    if (!st) return;
    out5[0] = st->n; out5[1] = st->n_live; out5[2] = (double)st->nnz[0]; out5[3] = (double)st->nnz[1];
    size_t bytes = 0;
    for (int k = 0; k < 2; ++k) bytes += st->ids[k].cls + st->vals[k].cls + st->meta[k].cls;
    out5[4] = (double)bytes;
}

extern "C" {

void plba_bow_default_options(plba_bow_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->mode = bw::MODE_COMBINED;
    o->topk = 8;
    o->lc_kf_dist = 50; o->lc_kf_max_dist = 50; o->lc_nkf_closest = 4;      // src/slamConfig.cpp:80-82
    o->min_lm_cov_graph = 75; o->min_kf_local_map = 3;                      // :61-62
}

int plba_bow_set_vocabulary(plba_problem* p, int kind, int k, int L, int weighting, int scoring, int n_nodes, const int32_t* parent,
                            const uint8_t* desc32, const double* weight, const int32_t* word_id) {
    (void)k; (void)L;
    if (!p) return PLBA_ERR_INVALID;
    if (kind != 0 && kind != 1) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_set_vocabulary: kind = %d", kind);
    if (weighting < 0 || weighting > 3) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_set_vocabulary: weighting = %d", weighting);
    if (scoring != 0) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_set_vocabulary: only L1_NORM scoring (0) is supported, not %d", scoring);
    if (!parent || !desc32 || !weight || !word_id) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_set_vocabulary: missing array");
    bw::VocPlan pl = bw::plan_vocabulary(n_nodes, parent, word_id);
    if (!pl.err.empty()) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_set_vocabulary: %s", pl.err.c_str());
    const size_t N = (size_t)n_nodes, W = (size_t)pl.n_words;
    Layout Lo;
    const size_t o_desc = Lo.take(32 * N), o_c0 = Lo.take(4 * N), o_nc = Lo.take(4 * N), o_word = Lo.take(4 * N), o_w = Lo.take(8 * N), o_ww = Lo.take(8 * W),
                 total = Lo.off;
    std::vector<char> h(total, 0);
    for (size_t at = 0; at < N; ++at) {
        const size_t old = (size_t)pl.order[at];
        memcpy(h.data() + o_desc + 32 * at, desc32 + 32 * old, 32);
        reinterpret_cast<double*>(h.data() + o_w)[at] = weight[old];
        if (pl.word[at] >= 0) reinterpret_cast<double*>(h.data() + o_ww)[pl.word[at]] = weight[old];
    }
    memcpy(h.data() + o_c0, pl.child0.data(), 4 * N); memcpy(h.data() + o_nc, pl.nchild.data(), 4 * N); memcpy(h.data() + o_word, pl.word.data(), 4 * N);
    PLBA_HIPCK(p, hipSetDevice(p->device));
    if (!p->bow) p->bow = new BowState;
    BowState* st = p->bow;
    PLBA_HIPCK(p, plba_stream_wait(p->stream));      // (uncounted: nothing of this library may still read the tree or the database)
    BowVoc& v = st->voc[kind];
    v.set = false;
    st->drop_db();
    PLBA_HIPCK(p, v.blk.alloc(total, false));
    PLBA_HIPCK(p, plba_h2d(p, v.blk.p, h.data(), total));
    v.o_desc = o_desc; v.o_c0 = o_c0; v.o_nc = o_nc; v.o_word = o_word; v.o_w = o_w; v.o_ww = o_ww;
    v.n_nodes = n_nodes; v.n_words = pl.n_words; v.weighting = weighting; v.set = true;
    return PLBA_OK;
}

int plba_bow_transform(plba_problem* p, int kind, int B, const int32_t* start, const uint8_t* desc32, int32_t* word, int32_t* bow_id, double* bow_val,
                       int32_t* nnz) {
    if (!p) return PLBA_ERR_INVALID;
    if (kind != 0 && kind != 1) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_transform: kind = %d", kind);
    if (B < 1 || B > 32767) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_transform: B = %d is outside 1 .. 32767", B);
    if (!start || !nnz) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_transform: missing start array or nnz");
    if (const char* why = check_starts(B, start, bw::MAX_DESC, TOO_MANY_DESC)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_transform: %s", why);
    const size_t N = (size_t)start[B];
    if (N && (!desc32 || !word || !bow_id || !bow_val)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_transform: missing array");
    if (!p->bow || !p->bow->voc[kind].set) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_transform: no vocabulary of kind %d", kind);
    const BowState* st = p->bow;
    std::vector<int32_t> zero((size_t)B + 1, 0);
    // one device block: [starts | empty starts | desc || words | ids | values | nnz]; up: before the bar, down: behind it
    Layout L;
    const size_t n_st = 4 * ((size_t)B + 1);
    const size_t o_st = L.take(n_st), o_z = L.take(n_st), o_d = L.take(32 * N), up_end = L.off, o_w = L.take(4 * N), o_id = L.take(4 * N), o_val = L.take(8 * N),
                 o_nnz = L.take(8 * (size_t)B);
    BatchCall call(p);
    PLBA_TRY(call.open(L.off, up_end, up_end, L.off));
    call.put(o_st, start, n_st); call.put(o_z, zero.data(), n_st); call.put(o_d, desc32, 32 * N);
    PLBA_TRY(call.upload());
    DescendDev t{};
    t.vp = voc_dev(st->voc[0]); t.vl = voc_dev(st->voc[1]);
    t.desc = call.dev<uint4>(o_d); t.Np = kind ? 0 : (int)N; t.Nl = kind ? (int)N : 0; t.word = call.dev<int32_t>(o_w);
    BuildDev bd{};
    bd.B = B; bd.n0 = 0; bd.Np = 0; bd.NP = pow2_at_least(std::max(max_rows(B, start), 1));
    bd.start_p = call.dev<int32_t>(kind ? o_z : o_st); bd.start_l = call.dev<int32_t>(kind ? o_st : o_z);
    bd.word = t.word; bd.ww_p = t.vp.word_weight; bd.ww_l = t.vl.word_weight;
    bd.acc_p = bw::accumulates(t.vp.weighting); bd.acc_l = bw::accumulates(t.vl.weighting);
    bd.out_id = call.dev<int32_t>(o_id); bd.out_val = call.dev<double>(o_val); bd.out_nnz = call.dev<int32_t>(o_nnz);
    PLBA_HIPCK(p, transform_launch(t, bd, call.s));
    PLBA_TRY(call.download());
    if (N) { memcpy(word, call.down<int32_t>(o_w), 4 * N); memcpy(bow_id, call.down<int32_t>(o_id), 4 * N); memcpy(bow_val, call.down<double>(o_val), 8 * N); }
    memcpy(nnz, call.down<int32_t>(o_nnz) + (kind ? (size_t)B : 0), 4 * (size_t)B);
    return PLBA_OK;
}

int plba_bow_insert_keyframes(plba_problem* p, const plba_bow_options* opt, int B, const int32_t* pt_start, const uint8_t* pt_desc32, const double* pt_pl2,
                              const int32_t* ln_start, const uint8_t* ln_desc32, const double* ln_spl_epl4, const int32_t* cov_start, const int32_t* cov,
                              plba_bow_result* out) {
    if (!p) return PLBA_ERR_INVALID;
    if (!opt || !out) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_insert_keyframes: no options or no output");
    if (B < 1 || B > 32767) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_insert_keyframes: B = %d is outside 1 .. 32767", B);
    if (opt->mode < 0 || opt->mode > 2) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_insert_keyframes: mode = %d", opt->mode);
    if (opt->topk < 0 || opt->topk > bw::TOPK_MAX) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_insert_keyframes: topk = %d is outside 0 .. 16", opt->topk);
    if (opt->lc_kf_dist < 0 || opt->lc_kf_max_dist < 0 || opt->lc_nkf_closest < 0 || opt->min_lm_cov_graph < 0 || opt->min_kf_local_map < 0)
        PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_insert_keyframes: a negative option");
    const bool use_p = opt->mode != bw::MODE_LINES, use_l = opt->mode != bw::MODE_POINTS;
    if ((use_p && !pt_start) || (use_l && !ln_start)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_insert_keyframes: missing start array");
    std::vector<int32_t> zero((size_t)B + 1, 0);
    const int32_t *ps = use_p ? pt_start : zero.data(), *ls = use_l ? ln_start : zero.data();
    for (const int32_t* st : {ps, ls})
        if (const char* why = check_starts(B, st, bw::MAX_DESC, TOO_MANY_DESC)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_insert_keyframes: %s", why);
    const size_t Np = (size_t)ps[B], Nl = (size_t)ls[B];
    const bool want_std = opt->mode == bw::MODE_COMBINED;
    if ((Np && (!pt_desc32 || (want_std && !pt_pl2))) || (Nl && (!ln_desc32 || (want_std && !ln_spl_epl4))))
        PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_insert_keyframes: missing array");
    BowState* st = p->bow;
    if (!st || (use_p && !st->voc[0].set) || (use_l && !st->voc[1].set)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_insert_keyframes: no vocabulary for a kind the mode uses");
    const int n0 = st->n;
    if ((size_t)n0 + (size_t)B > (size_t)INT32_MAX / 2 || st->used[0] + Np > (size_t)INT32_MAX || st->used[1] + Nl > (size_t)INT32_MAX)
        PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_insert_keyframes: the database would pass 2^31 - 1 entries");
    const size_t R = bw::score_row(B, n0), C = bw::cov_row(B, n0);
    if (cov_start || cov) {
        if (!cov_start || !out->cand || (C && !cov)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_insert_keyframes: a covisibility column needs cov_start, cov and cand");
        for (int b = 0; b <= B; ++b)
            if ((size_t)cov_start[b] != bw::cov_row(b, n0)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_insert_keyframes: cov_start[%d] does not fit: keyframe b has first_index + b entries", b);
        for (size_t i = 0; i < C; ++i) if (cov[i] < 0) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_insert_keyframes: a negative covisibility count");
    }
    const bool decide = cov_start != nullptr;
    if ((out->score_p || out->score_l || out->score || out->score_f32) && (out->score_cap < 0 || (size_t)out->score_cap < R))
        PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_insert_keyframes: score_cap = %lld, the call writes %zu entries", (long long)out->score_cap, R);

    // one device block: [starts | live | desc | positions | cov || words | ids | values | nnz | stat | cand | float | score | score_p | score_l];
    // up: before the bar; down: behind it, as far as the last score column the caller asked for
    Layout L;
    const size_t n_st = 4 * ((size_t)B + 1);
    const size_t o_ps = L.take(n_st), o_ls = L.take(n_st), o_live = L.take((size_t)n0), o_d = L.take(32 * (Np + Nl)), o_pp = L.take(want_std ? 16 * Np : 0),
                 o_pl = L.take(want_std ? 32 * Nl : 0), o_cov = L.take(decide ? 4 * C : 0), up_end = L.off;
    const size_t o_w = L.take(4 * (Np + Nl)), o_id = L.take(4 * (Np + Nl)), o_val = L.take(8 * (Np + Nl)), o_nnz = L.take(8 * (size_t)B), o_stat = L.take(16 * (size_t)B),
                 o_ci = L.take(4 * (size_t)CAND_I * B), o_cd = L.take(8 * (size_t)CAND_D * B), o_sf = L.take(4 * R), o_s = L.take(8 * R), o_sp = L.take(8 * R),
                 o_sl = L.take(8 * R);
    // (the score columns are the bulk of a large database's read-back: a caller that asks for none of them gets none copied)
    const size_t down_end = (out->score_p || out->score_l) ? L.off : out->score ? o_sp : out->score_f32 ? o_s : o_sf;
    BatchCall call(p);
    PLBA_TRY(call.open(L.off, up_end, up_end, down_end));
    hipStream_t s = call.s;
    call.put(o_ps, ps, n_st); call.put(o_ls, ls, n_st); call.put(o_live, st->live.data(), (size_t)n0);
    call.put(o_d, pt_desc32, 32 * Np); call.put(o_d + 32 * Np, ln_desc32, 32 * Nl);
    if (want_std) { call.put(o_pp, pt_pl2, 16 * Np); call.put(o_pl, ln_spl_epl4, 32 * Nl); }
    if (decide) call.put(o_cov, cov, 4 * C);
    PLBA_TRY(call.upload());
    DArr<char> old[6];      // the pools' former blocks: released when the call returns, which is after its wait
    const size_t rows[2] = {Np, Nl};
    for (int k = 0; k < 2; ++k) {
        PLBA_HIPCK(p, grow(st->ids[k], 4 * st->used[k], 4 * (st->used[k] + rows[k]), old[3 * k], s));
        PLBA_HIPCK(p, grow(st->vals[k], 8 * st->used[k], 8 * (st->used[k] + rows[k]), old[3 * k + 1], s));
        PLBA_HIPCK(p, grow(st->meta[k], 8 * (size_t)n0, 8 * ((size_t)n0 + B), old[3 * k + 2], s));
    }
    DescendDev t{};
    t.vp = voc_dev(st->voc[0]); t.vl = voc_dev(st->voc[1]);
    t.desc = call.dev<uint4>(o_d); t.Np = (int)Np; t.Nl = (int)Nl; t.word = call.dev<int32_t>(o_w);
    const int longest = std::max(std::max(max_rows(B, ps), max_rows(B, ls)), 1);
    BuildDev bd{};
    bd.B = B; bd.n0 = n0; bd.Np = (int)Np; bd.NP = pow2_at_least(longest);
    bd.start_p = call.dev<int32_t>(o_ps); bd.start_l = call.dev<int32_t>(o_ls); bd.word = t.word; bd.ww_p = t.vp.word_weight; bd.ww_l = t.vl.word_weight;
    bd.acc_p = bw::accumulates(t.vp.weighting); bd.acc_l = bw::accumulates(t.vl.weighting);
    bd.out_id = call.dev<int32_t>(o_id); bd.out_val = call.dev<double>(o_val); bd.out_nnz = call.dev<int32_t>(o_nnz);
    bd.db_id_p = reinterpret_cast<int32_t*>(st->ids[0].p); bd.db_id_l = reinterpret_cast<int32_t*>(st->ids[1].p);
    bd.db_val_p = reinterpret_cast<double*>(st->vals[0].p); bd.db_val_l = reinterpret_cast<double*>(st->vals[1].p);
    bd.meta_p = reinterpret_cast<int2*>(st->meta[0].p); bd.meta_l = reinterpret_cast<int2*>(st->meta[1].p);
    bd.used_p = (int)st->used[0]; bd.used_l = (int)st->used[1];
    bd.pos_p = want_std ? call.dev<double>(o_pp) : nullptr; bd.pos_l = want_std ? call.dev<double>(o_pl) : nullptr; bd.stat = call.dev<double>(o_stat);
    PLBA_HIPCK(p, transform_launch(t, bd, s));
    ScoreDev sc{};
    sc.B = B; sc.n0 = n0; sc.NQ = longest; sc.live = call.dev<uint8_t>(o_live);
    sc.id_p = bd.db_id_p; sc.id_l = bd.db_id_l; sc.val_p = bd.db_val_p; sc.val_l = bd.db_val_l; sc.meta_p = bd.meta_p; sc.meta_l = bd.meta_l;
    sc.sp = call.dev<double>(o_sp); sc.sl = call.dev<double>(o_sl); sc.use_p = use_p; sc.use_l = use_l;
    PLBA_HIPCK(p, ensure_dyn_lds(reinterpret_cast<const void*>(k_bow_score), 12 * bw::MAX_DESC));
    const unsigned chunks = (unsigned)(((size_t)n0 + B + SCORE_CHUNK - 1) / SCORE_CHUNK);
    hipLaunchKernelGGL(k_bow_score, dim3(chunks, 2 * (unsigned)B), dim3(256), 12 * (size_t)sc.NQ, s, sc);
    DecideDev dc{};
    dc.B = B; dc.n0 = n0; dc.mode = opt->mode; dc.topk = opt->topk; dc.lc_kf_dist = opt->lc_kf_dist; dc.lc_kf_max_dist = opt->lc_kf_max_dist;
    dc.lc_nkf_closest = opt->lc_nkf_closest; dc.min_lm_cov_graph = opt->min_lm_cov_graph; dc.min_kf_local_map = opt->min_kf_local_map;
    dc.live = sc.live; dc.start_p = bd.start_p; dc.start_l = bd.start_l; dc.stat = bd.stat; dc.sp = sc.sp; dc.sl = sc.sl; dc.s = call.dev<double>(o_s);
    dc.sf = call.dev<float>(o_sf); dc.cov = decide ? call.dev<int32_t>(o_cov) : nullptr; dc.cand_i = call.dev<int32_t>(o_ci); dc.cand_d = call.dev<double>(o_cd);
    hipLaunchKernelGGL(k_bow_decide, dim3((unsigned)B), dim3(256), 0, s, dc);
    PLBA_HIPCK(p, hipGetLastError());
    PLBA_TRY(call.download());

    const int32_t* nz = call.down<int32_t>(o_nnz);
    st->n = n0 + B; st->n_live += B; st->live.resize((size_t)n0 + B, 1);
    st->used[0] += Np; st->used[1] += Nl;
    for (int b = 0; b < B; ++b) { st->nnz[0] += (size_t)nz[b]; st->nnz[1] += (size_t)nz[B + b]; }
    out->first_index = n0;
    if (out->score_p) memcpy(out->score_p, call.down<double>(o_sp), 8 * R);
    if (out->score_l) memcpy(out->score_l, call.down<double>(o_sl), 8 * R);
    if (out->score) memcpy(out->score, call.down<double>(o_s), 8 * R);
    if (out->score_f32) memcpy(out->score_f32, call.down<float>(o_sf), 4 * R);
    if (use_p) {
        if (out->pt_word && Np) memcpy(out->pt_word, call.down<int32_t>(o_w), 4 * Np);
        if (out->pt_bow_id && Np) memcpy(out->pt_bow_id, call.down<int32_t>(o_id), 4 * Np);
        if (out->pt_bow_val && Np) memcpy(out->pt_bow_val, call.down<double>(o_val), 8 * Np);
        if (out->pt_nnz) memcpy(out->pt_nnz, nz, 4 * (size_t)B);
    }
    if (use_l) {
        if (out->ln_word && Nl) memcpy(out->ln_word, call.down<int32_t>(o_w) + Np, 4 * Nl);
        if (out->ln_bow_id && Nl) memcpy(out->ln_bow_id, call.down<int32_t>(o_id) + Np, 4 * Nl);
        if (out->ln_bow_val && Nl) memcpy(out->ln_bow_val, call.down<double>(o_val) + Np, 8 * Nl);
        if (out->ln_nnz) memcpy(out->ln_nnz, nz + B, 4 * (size_t)B);
    }
    if (decide) {
        const int32_t* ci = call.down<int32_t>(o_ci);
        const double* cd = call.down<double>(o_cd);
        for (int b = 0; b < B; ++b) {
            plba_bow_candidate& c = out->cand[b];
            const int32_t* i4 = ci + (size_t)CAND_I * b;
            const double* d2 = cd + (size_t)CAND_D * b;
            c.is_candidate = i4[0]; c.kf_prev = i4[1]; c.n_closest = i4[2]; c.n_eligible = i4[3];
            c.best_score = d2[0]; c.lc_min_score = d2[1];
            for (int r = 0; r < bw::TOPK_MAX; ++r) { c.topk[r] = i4[4 + r]; c.topk_score[r] = d2[2 + r]; }
        }
    }
    return PLBA_OK;
}

int plba_bow_remove_keyframe(plba_problem* p, int kf) {
    if (!p) return PLBA_ERR_INVALID;
    BowState* st = p->bow;
    if (!st || kf < 0 || kf >= st->n) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_bow_remove_keyframe: keyframe %d is not in the database", kf);
    if (st->live[(size_t)kf]) { st->live[(size_t)kf] = 0; --st->n_live; }
    return PLBA_OK;
}

int plba_bow_reset(plba_problem* p) {
    if (!p) return PLBA_ERR_INVALID;
    if (!p->bow) return PLBA_OK;
    PLBA_HIPCK(p, hipSetDevice(p->device));
    PLBA_HIPCK(p, plba_stream_wait(p->stream));      // (uncounted; the calls that use the database have waited already)
    p->bow->drop_db();
    return PLBA_OK;
}

}  // extern "C"
