// plba_match.hip — descriptor matching (plba_match_descriptors, include/plba.h): StVO::match (stvo-pl/src/matching.cpp:41-109) for B
// problems, and the composed loop-candidate check (plba_verify_loop_candidates): MapHandler::isLoopClosure (src/mapHandler.cpp:3301-3409)
// from the descriptors to the decision with one upload, one read-back and one wait.
//
// Mapping.  k_match_nn: ONE launch over a host-built work list of (problem, direction, query tile).  A work item is one wave; a lane
// keeps one query descriptor in 8 registers, the train rows pass through LDS in tiles of TRAIN_TILE rows (the next tile is fetched into
// registers while the current one is compared), every lane reads the same LDS row (a broadcast read), and the rows are visited in
// ascending index, so the strict `<` of match::nn_update is the tie rule.  8 xor and 8 population counts per pair.  k_match_finish: one
// block per problem applies the ratio test and the mutual rule to the stored (index, d0, d1) triples and counts the matches: integer
// sums only, no order to depend on.  The composed call appends k_loop_gate (one block: the inlier-ratio gate per candidate and the scan
// of the surviving feature counts over B), k_loop_gather (the matched pairs in ascending i1 into k_relpose's arrays) and k_relpose itself
// (plba_relpose.hip, through plba_relpose_launch.h).  The arithmetic is plba_match_dev.h, shared with the host check and the drop-in.
// The host side of both calls (one block, one copy up, one down, one wait) is plba_batch_call.h's.
#include "plba_batch_call.h"
#include "plba_match_dev.h"
#include "plba_relpose_launch.h"

namespace plba {
namespace {

namespace mt = match;

struct MatchDev {
    int P;                                  // problems
    const int32_t *a_start, *b_start;       // P + 1 each: rows of desc1 / desc2
    const uint4 *descA, *descB;             // two uint4 per row
    const int4* work;                       // (problem, direction, query tile, -)
    const float* nnr;                       // P
    const int32_t* flags;                   // P: match::BEST_LR | match::SKIP
    int32_t *nnA, *nnB;                     // 3 per row: the search 1 -> 2 and 2 -> 1
    int32_t *m12, *count;                   // rows of desc1; P
};

__device__ __forceinline__ mt::Desc to_desc(const uint4& lo, const uint4& hi) {
    mt::Desc d;
    d.w[0] = lo.x; d.w[1] = lo.y; d.w[2] = lo.z; d.w[3] = lo.w; d.w[4] = hi.x; d.w[5] = hi.y; d.w[6] = hi.z; d.w[7] = hi.w;
    return d;
}

constexpr int TILE_VEC = 2 * mt::TRAIN_TILE;                 // uint4 of a train tile
constexpr int FETCH = TILE_VEC / mt::QUERY_TILE;             // uint4 a lane moves per tile
static_assert(TILE_VEC % mt::QUERY_TILE == 0, "a train tile is moved by whole lanes");

__global__ __launch_bounds__(mt::QUERY_TILE) void k_match_nn(MatchDev d) {
    __shared__ uint4 tile[TILE_VEC];
    const int4 w = d.work[blockIdx.x];
    const int a0 = d.a_start[w.x], na = d.a_start[w.x + 1] - a0, b0 = d.b_start[w.x], nb = d.b_start[w.x + 1] - b0;
    const int dir = w.y;
    // (both sides in locals first: a choice between two FIELDS of the argument block would index it dynamically and put it in scratch)
    const uint4 *rowsA = d.descA + 2 * (size_t)a0, *rowsB = d.descB + 2 * (size_t)b0;
    int32_t *outA = d.nnA + 3 * (size_t)a0, *outB = d.nnB + 3 * (size_t)b0;
    const uint4* Q = dir ? rowsB : rowsA;
    const uint4* T = dir ? rowsA : rowsB;
    const int nq = dir ? nb : na, nt = dir ? na : nb;
    const int lane = threadIdx.x, q = w.z * mt::QUERY_TILE + lane;
    const bool live = q < nq;
    uint4 ql = make_uint4(0, 0, 0, 0), qh = make_uint4(0, 0, 0, 0);
    if (live) { ql = Q[2 * (size_t)q]; qh = Q[2 * (size_t)q + 1]; }
    const mt::Desc qd = to_desc(ql, qh);
    mt::NN2 s;
    mt::nn_init(s);
    uint4 nx[FETCH];
#pragma unroll
    for (int k = 0; k < FETCH; ++k) {
        const int e = lane + mt::QUERY_TILE * k;
        nx[k] = make_uint4(0, 0, 0, 0);
        if ((e >> 1) < nt) nx[k] = T[e];
    }
    for (int t0 = 0; t0 < nt; t0 += mt::TRAIN_TILE) {
        __syncthreads();      // the previous tile has been compared
#pragma unroll
        for (int k = 0; k < FETCH; ++k) tile[lane + mt::QUERY_TILE * k] = nx[k];
        __syncthreads();
        const int t1 = t0 + mt::TRAIN_TILE;
        if (t1 < nt) {
#pragma unroll
            for (int k = 0; k < FETCH; ++k) {
                const int e = lane + mt::QUERY_TILE * k;
                nx[k] = make_uint4(0, 0, 0, 0);
                if (t1 + (e >> 1) < nt) nx[k] = T[2 * (size_t)t1 + e];
            }
        }
        const int m = nt - t0 < mt::TRAIN_TILE ? nt - t0 : mt::TRAIN_TILE;
        for (int r = 0; r < m; ++r) mt::nn_update(s, mt::distance(qd, to_desc(tile[2 * r], tile[2 * r + 1])), t0 + r);
    }
    if (live) mt::nn_store(s, (dir ? outB : outA) + 3 * (size_t)q);
}

// sum of v over the block's 256 threads, in every thread (integers: any order gives the same sum)
__device__ __forceinline__ int block_sum_256(int v, int* sh4) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh4[0] + sh4[1] + sh4[2] + sh4[3];
}

__global__ __launch_bounds__(256) void k_match_finish(MatchDev d) {
    __shared__ int sh4[4];
    const int pb = blockIdx.x;
    const int a0 = d.a_start[pb], na = d.a_start[pb + 1] - a0, b0 = d.b_start[pb], nb = d.b_start[pb + 1] - b0;
    const int flags = d.flags[pb];
    const float nnr = d.nnr[pb];
    const bool searched = !(flags & mt::SKIP) && nb > 0;      // else no work item wrote this problem's triples
    int cnt = 0;
    for (int i = threadIdx.x; i < na; i += 256) {
        int32_t* t = d.nnA + 3 * ((size_t)a0 + i);
        int m = -1;
        if (searched) m = mt::resolve(t, d.nnB + 3 * (size_t)b0, i, na, nb, nnr, flags & mt::BEST_LR);
        else { t[0] = -1; t[1] = -1; t[2] = -1; }
        d.m12[(size_t)a0 + i] = m;
        cnt += m >= 0 ? 1 : 0;
    }
    cnt = block_sum_256(cnt, sh4);
    if (threadIdx.x == 0) d.count[pb] = cnt;
}

struct LoopDev {
    int B;
    const int32_t *a_start, *b_start;       // 2B + 1 each: the point problems, then the line problems
    const int32_t *m12, *count;             // of the 2B problems
    int use_points, use_lines;
    double lc_inlier_ratio;
    int32_t* gate_i;                        // B
    double* gate_d;                         // B x 2: inl_ratio_pt, inl_ratio_ls
    int32_t *rp_ps, *rp_ls;                 // B + 1 each: k_relpose's starts
    const double *P3A, *uvB, *pq6A, *l3B;   // the keyframes' features, rows as the descriptors'
    int NpA, NpB;                           // point rows in front of the line rows
    double *gP3, *guv, *gpq, *gl3;          // the matched pairs
    uint8_t *pm, *lm;
};

__global__ __launch_bounds__(256) void k_loop_gate(LoopDev d) {
    __shared__ int sp[256], sl[256], carry[2];
    const int tid = threadIdx.x, B = d.B;
    if (tid == 0) { carry[0] = 0; carry[1] = 0; d.rp_ps[0] = 0; d.rp_ls[0] = 0; }
    for (int base = 0; base < B; base += 256) {
        __syncthreads();
        const int b = base + tid;
        int np = 0, nl = 0;
        if (b < B) {
            const int cp = d.count[b], cl = d.count[B + b];
            const double rpt = mt::inlier_ratio(cp, d.a_start[b + 1] - d.a_start[b], d.b_start[b + 1] - d.b_start[b]);
            const double rls = mt::inlier_ratio(cl, d.a_start[B + b + 1] - d.a_start[B + b], d.b_start[B + b + 1] - d.b_start[B + b]);
            const int ok = mt::gate(rpt, rls, d.use_points, d.use_lines, d.lc_inlier_ratio);
            d.gate_i[b] = ok; d.gate_d[2 * (size_t)b] = rpt; d.gate_d[2 * (size_t)b + 1] = rls;
            if (ok) { np = cp; nl = cl; }
        }
        sp[tid] = np; sl[tid] = nl;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int a = tid >= off ? sp[tid - off] : 0, c = tid >= off ? sl[tid - off] : 0;
            __syncthreads();
            sp[tid] += a; sl[tid] += c;
            __syncthreads();
        }
        if (b < B) { d.rp_ps[b + 1] = carry[0] + sp[tid]; d.rp_ls[b + 1] = carry[1] + sl[tid]; }
        __syncthreads();
        if (tid == 255) { carry[0] += sp[255]; carry[1] += sl[255]; }
    }
}

__global__ __launch_bounds__(256) void k_loop_gather(LoopDev d) {
    __shared__ int wsum[4];
    const int B = d.B, pb = blockIdx.x, kind = pb >= B ? 1 : 0, b = pb - kind * B;
    const int32_t* rs = kind ? d.rp_ls : d.rp_ps;
    const int dst0 = rs[b];
    if (rs[b + 1] == dst0) return;      // the gate failed, or nothing matched
    const int a0 = d.a_start[pb], na = d.a_start[pb + 1] - a0, b0 = d.b_start[pb];
    const size_t fa = (size_t)a0 - (kind ? (size_t)d.NpA : 0), fb = (size_t)b0 - (kind ? (size_t)d.NpB : 0);      // feature rows of this kind
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int run = 0;
    for (int base = 0; base < na; base += 256) {
        const int i = base + tid;
        const int m = i < na ? d.m12[(size_t)a0 + i] : -1;
        const unsigned long long bal = __ballot(m >= 0);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int before = 0;
        for (int v = 0; v < wave; ++v) before += wsum[v];
        const int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (m >= 0) {
            const size_t k = (size_t)dst0 + run + before + __popcll(bal & ((1ull << lane) - 1ull));
            if (!kind) {
                const double *s = d.P3A + 3 * (fa + i), *u = d.uvB + 2 * (fb + m);
                d.gP3[3 * k] = s[0]; d.gP3[3 * k + 1] = s[1]; d.gP3[3 * k + 2] = s[2];
                d.guv[2 * k] = u[0]; d.guv[2 * k + 1] = u[1];
                d.pm[k] = 1;
            } else {
                const double *s = d.pq6A + 6 * (fa + i), *u = d.l3B + 3 * (fb + m);
#pragma unroll
                for (int c = 0; c < 6; ++c) d.gpq[6 * k + c] = s[c];
                d.gl3[3 * k] = u[0]; d.gl3[3 * k + 1] = u[1]; d.gl3[3 * k + 2] = u[2];
                d.lm[k] = 1;
            }
        }
        run += tot;
        __syncthreads();      // wsum is written again
    }
}

// (problem, direction, query tile) of every search that resolve() will read: 1 -> 2 wherever both sides have a row (its triples are
// also nn3), 2 -> 1 only where the mutual rule can keep a match
void build_work(int P, const int32_t* a_start, const int32_t* b_start, const int32_t* flags, std::vector<int4>& work) {
    work.clear();
    for (int pb = 0; pb < P; ++pb) {
        if (flags[pb] & mt::SKIP) continue;
        const int na = a_start[pb + 1] - a_start[pb], nb = b_start[pb + 1] - b_start[pb];
        if (na < 1 || nb < 1) continue;
        for (int t = 0; t * mt::QUERY_TILE < na; ++t) work.push_back(make_int4(pb, 0, t, 0));
        if ((flags[pb] & mt::BEST_LR) && na >= 2 && nb >= 2)
            for (int t = 0; t * mt::QUERY_TILE < nb; ++t) work.push_back(make_int4(pb, 1, t, 0));
    }
}

bool nnr_valid(float v) { return std::isfinite(v) && v > 0.0f; }

// the two matching launches
hipError_t match_launch(const MatchDev& d, size_t n_work, hipStream_t s) {
    if (n_work) hipLaunchKernelGGL(k_match_nn, dim3((unsigned)n_work), dim3(mt::QUERY_TILE), 0, s, d);
    hipLaunchKernelGGL(k_match_finish, dim3((unsigned)d.P), dim3(256), 0, s, d);
    return hipGetLastError();
}

}  // namespace
}  // namespace plba

using namespace plba;

extern "C" {

void plba_match_default_options(plba_match_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->nnr = 0.9f;      // Config::minRatio12P / minRatio12L, stvo-pl/src/config.cpp
    o->best_lr = 1;     // Config::bestLRMatches
}

int plba_match_descriptors(plba_problem* p, const plba_match_options* opt, int B, const int32_t* a_start, const uint8_t* descA32,
                           const int32_t* b_start, const uint8_t* descB32, const float* nnr_b, int32_t* matches_12, int32_t* n_matches, int32_t* nn3) {
    if (!p) return PLBA_ERR_INVALID;
    if (!opt || !n_matches) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_match_descriptors: no options or no output");
    if (B < 1) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_match_descriptors: B = %d", B);
    if (!a_start || !b_start) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_match_descriptors: missing start array");
    for (const int32_t* st : {a_start, b_start})
        if (const char* why = check_starts(B, st)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_match_descriptors: %s", why);
    const size_t NA = (size_t)a_start[B], NB = (size_t)b_start[B];
    if ((NA && (!descA32 || !matches_12)) || (NB && !descB32)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_match_descriptors: missing array");
    if (!nnr_valid(opt->nnr)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_match_descriptors: nnr is not finite or not positive");
    if (nnr_b) for (int b = 0; b < B; ++b) if (!nnr_valid(nnr_b[b])) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_match_descriptors: nnr_b[%d] is not finite or not positive", b);

    std::vector<int32_t> flags((size_t)B, opt->best_lr ? mt::BEST_LR : 0);
    std::vector<int4> work;
    build_work(B, a_start, b_start, flags.data(), work);
    // one device block: [starts | nnr | flags | work | desc1 | desc2 || triples 2 -> 1 || matches | counts | triples 1 -> 2]; the copy up takes
    // what is before the first bar, the copy down what is behind the second; the section between them stays on the device
    Layout L;
    const size_t n_st = 4 * ((size_t)B + 1);
    const size_t o_as = L.take(n_st), o_bs = L.take(n_st), o_nnr = L.take(4 * (size_t)B), o_fl = L.take(4 * (size_t)B), o_wk = L.take(16 * work.size()),
                 o_dA = L.take(32 * NA), o_dB = L.take(32 * NB), up_end = L.off, o_nB = L.take(12 * NB), down_begin = L.off, o_m = L.take(4 * NA),
                 o_cnt = L.take(4 * (size_t)B), o_nA = L.take(12 * NA);
    BatchCall call(p);
    PLBA_TRY(call.open(L.off, up_end, down_begin, L.off));
    call.put(o_as, a_start, n_st); call.put(o_bs, b_start, n_st);
    for (int b = 0; b < B; ++b) call.up<float>(o_nnr)[b] = nnr_b ? nnr_b[b] : opt->nnr;
    call.put(o_fl, flags.data(), 4 * (size_t)B); call.put(o_wk, work.data(), 16 * work.size());
    call.put(o_dA, descA32, 32 * NA); call.put(o_dB, descB32, 32 * NB);
    PLBA_TRY(call.upload());
    MatchDev d;
    d.P = B;
    d.a_start = call.dev<int32_t>(o_as); d.b_start = call.dev<int32_t>(o_bs);
    d.descA = call.dev<uint4>(o_dA); d.descB = call.dev<uint4>(o_dB);
    d.work = call.dev<int4>(o_wk); d.nnr = call.dev<float>(o_nnr); d.flags = call.dev<int32_t>(o_fl);
    d.nnA = call.dev<int32_t>(o_nA); d.nnB = call.dev<int32_t>(o_nB); d.m12 = call.dev<int32_t>(o_m); d.count = call.dev<int32_t>(o_cnt);
    PLBA_HIPCK(p, match_launch(d, work.size(), call.s));
    PLBA_TRY(call.download());
    if (NA) memcpy(matches_12, call.down<int32_t>(o_m), 4 * NA);
    memcpy(n_matches, call.down<int32_t>(o_cnt), 4 * (size_t)B);
    if (nn3 && NA) memcpy(nn3, call.down<int32_t>(o_nA), 12 * NA);
    return PLBA_OK;
}

void plba_loop_default_options(plba_loop_options* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    plba_match_default_options(&o->match_pt); plba_match_default_options(&o->match_ln);
    o->use_points = 1; o->use_lines = 1;      // SlamConfig::hasPoints / hasLines
    o->lc_inlier_ratio = 30.0;                // SlamConfig::lcInlierRatio, src/slamConfig.cpp
    plba_relpose_default_options(&o->relpose);
}

int plba_verify_loop_candidates(plba_problem* p, const plba_loop_options* opt, int B, const int32_t* pa_start, const uint8_t* descPA32, const double* P3A,
                                const int32_t* pb_start, const uint8_t* descPB32, const double* uvB, const int32_t* la_start, const uint8_t* descLA32,
                                const double* sPeP6A, const int32_t* lb_start, const uint8_t* descLB32, const double* l3B, double fx, double fy, double cx,
                                double cy, int32_t* pt_match, int32_t* ln_match, uint8_t* pt_inlier, uint8_t* ln_inlier, plba_loop_result* out) {
    if (!p) return PLBA_ERR_INVALID;
    if (!opt || !out) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_verify_loop_candidates: no options or no output");
    if (B < 1) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_verify_loop_candidates: B = %d", B);
    if (!pa_start || !pb_start || !la_start || !lb_start) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_verify_loop_candidates: missing start array");
    for (const int32_t* st : {pa_start, pb_start, la_start, lb_start})
        if (const char* why = check_starts(B, st)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_verify_loop_candidates: %s", why);
    const size_t NpA = (size_t)pa_start[B], NpB = (size_t)pb_start[B], NlA = (size_t)la_start[B], NlB = (size_t)lb_start[B];
    const size_t NA = NpA + NlA, NB = NpB + NlB;
    if (NA > (size_t)INT32_MAX || NB > (size_t)INT32_MAX) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_verify_loop_candidates: more than 2^31 - 1 rows on a side");
    if ((NpA && (!descPA32 || !P3A || !pt_match)) || (NpB && (!descPB32 || !uvB)) || (NlA && (!descLA32 || !sPeP6A || !ln_match)) || (NlB && (!descLB32 || !l3B)))
        PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_verify_loop_candidates: missing array");
    if (!nnr_valid(opt->match_pt.nnr) || !nnr_valid(opt->match_ln.nnr)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_verify_loop_candidates: nnr is not finite or not positive");
    if (!std::isfinite(opt->lc_inlier_ratio)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_verify_loop_candidates: lc_inlier_ratio is not finite");
    if (const char* why = relpose_check_options(opt->relpose, fx, fy, cx, cy)) PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_verify_loop_candidates: %s", why);
    if (!all_finite(P3A, 3 * NpA) || !all_finite(uvB, 2 * NpB) || !all_finite(sPeP6A, 6 * NlA) || !all_finite(l3B, 3 * NlB))
        PLBA_FAIL(p, PLBA_ERR_INVALID, "plba_verify_loop_candidates: non-finite input");

    // 2B matching problems: the candidates' points, then their lines; rows of desc1 / desc2 likewise
    const int P = 2 * B;
    std::vector<int32_t> as((size_t)P + 1), bs((size_t)P + 1), flags((size_t)P);
    for (int b = 0; b <= B; ++b) { as[b] = pa_start[b]; bs[b] = pb_start[b]; as[B + b] = (int32_t)NpA + la_start[b]; bs[B + b] = (int32_t)NpB + lb_start[b]; }
    for (int b = 0; b < B; ++b) {
        flags[b] = (opt->match_pt.best_lr ? mt::BEST_LR : 0) | (opt->use_points ? 0 : mt::SKIP);
        flags[B + b] = (opt->match_ln.best_lr ? mt::BEST_LR : 0) | (opt->use_lines ? 0 : mt::SKIP);
    }
    std::vector<int4> work;
    build_work(P, as.data(), bs.data(), flags.data(), work);
    // one device block: [starts | nnr | flags | work | desc1 | desc2 | features || triples | k_relpose's starts and arrays || matches | counts | gate |
    // masks | k_relpose's results]; the copy up takes what is before the first bar, the copy down what is behind the second; the section
    // between them stays on the device
    Layout L;
    const size_t n_st = 4 * ((size_t)P + 1), n_rst = 4 * ((size_t)B + 1);
    const size_t o_as = L.take(n_st), o_bs = L.take(n_st), o_nnr = L.take(4 * (size_t)P), o_fl = L.take(4 * (size_t)P), o_wk = L.take(16 * work.size()),
                 o_dA = L.take(32 * NA), o_dB = L.take(32 * NB), o_P3 = L.take(24 * NpA), o_uv = L.take(16 * NpB), o_pq = L.take(48 * NlA),
                 o_l3 = L.take(24 * NlB), up_end = L.off;
    const size_t o_nA = L.take(12 * NA), o_nB = L.take(12 * NB), o_rps = L.take(n_rst), o_rls = L.take(n_rst), o_gP = L.take(24 * NpA), o_gu = L.take(16 * NpA),
                 o_gq = L.take(48 * NlA), o_gl = L.take(24 * NlA), down_begin = L.off;
    const size_t o_m = L.take(4 * NA), o_cnt = L.take(4 * (size_t)P), o_gi = L.take(4 * (size_t)B), o_gd = L.take(16 * (size_t)B), o_pm = L.take(NpA),
                 o_lm = L.take(NlA), o_od = L.take(8 * (size_t)RP_OUT_D * B), o_oi = L.take(4 * (size_t)RP_OUT_I * B);
    BatchCall call(p);
    PLBA_TRY(call.open(L.off, up_end, down_begin, L.off));
    call.put(o_as, as.data(), n_st); call.put(o_bs, bs.data(), n_st);
    for (int b = 0; b < B; ++b) { call.up<float>(o_nnr)[b] = opt->match_pt.nnr; call.up<float>(o_nnr)[B + b] = opt->match_ln.nnr; }
    call.put(o_fl, flags.data(), 4 * (size_t)P); call.put(o_wk, work.data(), 16 * work.size());
    call.put(o_dA, descPA32, 32 * NpA); call.put(o_dA + 32 * NpA, descLA32, 32 * NlA); call.put(o_P3, P3A, 24 * NpA); call.put(o_pq, sPeP6A, 48 * NlA);
    call.put(o_dB, descPB32, 32 * NpB); call.put(o_dB + 32 * NpB, descLB32, 32 * NlB); call.put(o_uv, uvB, 16 * NpB); call.put(o_l3, l3B, 24 * NlB);
    PLBA_TRY(call.upload());
    MatchDev d;
    d.P = P;
    d.a_start = call.dev<int32_t>(o_as); d.b_start = call.dev<int32_t>(o_bs);
    d.descA = call.dev<uint4>(o_dA); d.descB = call.dev<uint4>(o_dB);
    d.work = call.dev<int4>(o_wk); d.nnr = call.dev<float>(o_nnr); d.flags = call.dev<int32_t>(o_fl);
    d.nnA = call.dev<int32_t>(o_nA); d.nnB = call.dev<int32_t>(o_nB); d.m12 = call.dev<int32_t>(o_m); d.count = call.dev<int32_t>(o_cnt);
    PLBA_HIPCK(p, match_launch(d, work.size(), call.s));
    LoopDev g;
    g.B = B; g.a_start = d.a_start; g.b_start = d.b_start; g.m12 = d.m12; g.count = d.count;
    g.use_points = opt->use_points ? 1 : 0; g.use_lines = opt->use_lines ? 1 : 0; g.lc_inlier_ratio = opt->lc_inlier_ratio;
    g.gate_i = call.dev<int32_t>(o_gi); g.gate_d = call.dev<double>(o_gd); g.rp_ps = call.dev<int32_t>(o_rps); g.rp_ls = call.dev<int32_t>(o_rls);
    g.P3A = call.dev<double>(o_P3); g.uvB = call.dev<double>(o_uv); g.pq6A = call.dev<double>(o_pq); g.l3B = call.dev<double>(o_l3);
    g.NpA = (int)NpA; g.NpB = (int)NpB;
    g.gP3 = call.dev<double>(o_gP); g.guv = call.dev<double>(o_gu); g.gpq = call.dev<double>(o_gq); g.gl3 = call.dev<double>(o_gl);
    g.pm = call.dev<uint8_t>(o_pm); g.lm = call.dev<uint8_t>(o_lm);
    hipLaunchKernelGGL(k_loop_gate, dim3(1), dim3(256), 0, call.s, g);
    hipLaunchKernelGGL(k_loop_gather, dim3((unsigned)P), dim3(256), 0, call.s, g);
    PLBA_HIPCK(p, hipGetLastError());
    RelposeDev r;
    relpose_set_options(opt->relpose, fx, fy, cx, cy, r.o);
    r.pt_start = g.rp_ps; r.ln_start = g.rp_ls; r.P3 = g.gP3; r.uv2 = g.guv; r.pq6 = g.gpq; r.l3 = g.gl3; r.T0 = nullptr;
    r.pt_in = g.pm; r.ln_in = g.lm; r.out_d = call.dev<double>(o_od); r.out_i = call.dev<int32_t>(o_oi);
    PLBA_HIPCK(p, relpose_launch(r, B, call.s));
    PLBA_TRY(call.download());

    const int32_t *m12 = call.down<int32_t>(o_m), *cnt = call.down<int32_t>(o_cnt), *gi = call.down<int32_t>(o_gi), *oi = call.down<int32_t>(o_oi);
    const double *gd = call.down<double>(o_gd), *od = call.down<double>(o_od);
    const uint8_t *pm = call.down<uint8_t>(o_pm), *lm = call.down<uint8_t>(o_lm);
    if (NpA) memcpy(pt_match, m12, 4 * NpA);
    if (NlA) memcpy(ln_match, m12 + NpA, 4 * NlA);
    size_t kp = 0, kl = 0;      // where a candidate's pairs begin in k_relpose's arrays: the device's scan, repeated
    for (int b = 0; b < B; ++b) {
        plba_loop_result& o = out[b];
        memset(&o, 0, sizeof o);
        o.common_pt = cnt[b]; o.common_ls = cnt[B + b]; o.ratio_ok = gi[b];
        o.inl_ratio_pt = gd[2 * (size_t)b]; o.inl_ratio_ls = gd[2 * (size_t)b + 1];
        if (o.ratio_ok) relpose_assemble(opt->relpose, o.common_pt + o.common_ls, od + (size_t)RP_OUT_D * b, oi + (size_t)RP_OUT_I * b, o.relpose);
        if (pt_inlier)
            for (int32_t i = pa_start[b]; i < pa_start[b + 1]; ++i) pt_inlier[i] = (o.ratio_ok && m12[i] >= 0) ? pm[kp++] : 0;
        if (ln_inlier)
            for (int32_t i = la_start[b]; i < la_start[b + 1]; ++i) ln_inlier[i] = (o.ratio_ok && m12[NpA + i] >= 0) ? lm[kl++] : 0;
        if (!pt_inlier && o.ratio_ok) kp += (size_t)o.common_pt;
        if (!ln_inlier && o.ratio_ok) kl += (size_t)o.common_ls;
    }
    return PLBA_OK;
}

}  // extern "C"
