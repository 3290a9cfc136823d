// Loop candidate search: stage 1 of the reference's loop closure, LoopClosure::LoopKeyframeCandidate
// (src/loopclosure.cpp:227-284), with SimilarityScore (:173-180) and the normalisation of :128, over a store of normalised global
// descriptors that stays on the device.
//
// The contract (include/svslam.h has it in full; tests/ref_loop_candidates.py is its second reading):
//   similarity   64 accumulators from +0; accumulator l takes the elements l, l + 64, l + 128, ... below dim in that order, each step
//                acc = acc + (a[e] * b[e]) with the product and the sum rounded to f32 (no FMA); then acc[l] += acc[l + s] for l < s,
//                s = 32, 16, 8, 4, 2, 1; the similarity is acc[0].
//   normalise    n2 = similarity(a, a); v[e] = a[e] / sqrtf(n2), IEEE; n2 zero or not finite: BAD_VECTOR.
//   selection    rows in ascending keyframe id; kf_id - id < min_gap skipped; best = largest sim > 0, lowest id on a tie; n_weak
//                counts sim > weak; NONE, then best < strong, then n_weak > max_num_weak, then FOUND.
//
// Layout of a stored row: padded with +0 to dp = a multiple of 256 floats and permuted inside every 256, so that the 16 bytes lane l
// loads from chunk c are the elements c 256 + l, + 64, + 128, + 192: the four consecutive terms of accumulator l.  One wave-wide
// 16-byte load therefore feeds every accumulator in the contract's order.  The padding is inert: a term (+0 * +0) = +0, and an
// accumulator is never -0 (it starts at +0, and a sum rounds to -0 only from two -0), so acc + +0 == acc bit for bit.
//
// k_lc_candidates: one workgroup of 256 threads per job.  The query goes into LDS in the row layout, wave 0 sums its n2, all threads
// divide; then wave w takes the rows 16 g + 4 w ... + 3 of every group g of 16: four rows per pass, so every LDS read of the query
// serves four rows and four 16-byte global loads per lane are in flight per chunk.  The 64 accumulators of a row are one per lane;
// the device build sums them by a butterfly acc += acc[l ^ s] (every lane ends with the halving tree's acc[0], as float addition
// commutes), the host build by the tree itself.  No barrier inside the row loop.  Each wave keeps its best (sim, id) and counts;
// thread 0 combines the four with the same tie rule.
// k_lc_append: one wave per vector; with commit == 0 it only reports BAD_VECTOR, with commit == 1 it writes the normalised row.
//
// The file is plain C++ between the HIP qualifiers: with LC_HOST_EMU (tests/cpp/lc_host_emu) a wave becomes a loop over 64 lane
// numbers, a workgroup a loop over its waves, and a per-lane value an array of 64.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#pragma clang fp contract(off)

#define LC_THREADS 256
#define LC_WAVES 4
#define LC_ROWS 4                 // rows a wave reduces per pass
#define LC_MAX_DIM 4096
#define LC_CHUNK 256              // floats of a row that one 16-byte load per lane covers

enum { LC_FOUND = 0, LC_NONE = 1, LC_BELOW_STRONG = 2, LC_TOO_MANY_WEAK = 3, LC_BAD_VECTOR = 4 };

#ifdef LC_HOST_EMU
#define LC_DEV
#define LC_HD
#define LC_LANES for (int lane = 0; lane < 64; ++lane)
#define LC_WAVE_LOOP for (int wave = 0; wave < LC_WAVES; ++wave)
#define LC_SYNC
struct LcLaneF { float v[64]; };
#define LC_AT(x) (x).v[lane]
#else
#define LC_DEV __device__
#define LC_HD __host__ __device__
#define LC_LANES for (int lane = (int)(threadIdx.x & 63), once_ = 1; once_; once_ = 0)
#define LC_WAVE_LOOP for (int wave = (int)(threadIdx.x >> 6), wonce_ = 1; wonce_; wonce_ = 0)
#define LC_SYNC __syncthreads();
struct LcLaneF { float v; };
#define LC_AT(x) (x).v
#endif

struct alignas(16) LcF4 { float x, y, z, w; };
struct LcStore { float *rows; int *ids; int nstreams, capacity, dim, dp; };      // rows [nstreams][capacity][dp], ids [nstreams][capacity]
struct LcParams { float weak, strong; int max_num_weak, min_gap; };
struct LcJob { int stream, kf_id, count; int status, cand_kf, best_kf, n_weak, n_compared; float best_sim; int pad; };
struct LcApp { int stream, slot, kf_id, status; };
struct LcBest { float sim; int id, n_weak, n_cmp; };
struct LcShared { alignas(16) float q[LC_MAX_DIM]; float n2; LcBest w[LC_WAVES]; };

static inline int lc_padded(int dim) { return (dim + LC_CHUNK - 1) / LC_CHUNK * LC_CHUNK; }
// which element of the vector sits at place p of a row
LC_HD static inline int lc_elem(int p) { const int r = p % LC_CHUNK; return p - r + 64 * (r % 4) + r / 4; }

// ---- host side: the store's bookkeeping and every refusal, shared by the library and the host emulation --------------------------
struct LcHost { int nstreams = 0, capacity = 0, dim = 0, dp = 0; std::vector<int> count, last_id; };

static inline const char *lc_check_configure(int nstreams, int capacity, int dim)
{
    if (nstreams < 1 || capacity < 1) return "nstreams and capacity must be at least 1";
    if (dim < 1 || dim > LC_MAX_DIM) return "dim must be 1 .. 4096";
    return nullptr;
}

// the slot every row of an append call takes, or why the call is refused; the same stream may come more than once, ascending
static inline const char *lc_check_append(const LcHost &H, int n, const int *streams, const int *kf_ids, LcApp *out)
{
    if (H.nstreams == 0) return "the store is not configured";
    std::vector<int> cnt(H.count), last(H.last_id);
    for (int i = 0; i < n; ++i) {
        const int s = streams[i];
        if (s < 0 || s >= H.nstreams) return "unknown stream";
        if (kf_ids[i] < 0) return "negative keyframe id";
        if (cnt[(size_t)s] >= H.capacity) return "the stream is full";
        if (kf_ids[i] <= last[(size_t)s]) return "keyframe ids must ascend strictly within a stream";
        out[i] = LcApp{ s, cnt[(size_t)s], kf_ids[i], 0 };
        cnt[(size_t)s]++; last[(size_t)s] = kf_ids[i];
    }
    return nullptr;
}

static inline const char *lc_check_jobs(const LcHost &H, int njobs, const int *streams, const int *kf_ids, const LcParams &P, LcJob *out)
{
    if (H.nstreams == 0) return "the store is not configured";
    if (P.min_gap < 0) return "negative min_gap";
    if (P.max_num_weak < 0) return "negative max_num_weak";
    if (!(fabsf(P.weak) <= FLT_MAX) || !(fabsf(P.strong) <= FLT_MAX)) return "a threshold is not finite";
    for (int j = 0; j < njobs; ++j) {
        const int s = streams[j];
        if (s < 0 || s >= H.nstreams) return "unknown stream";
        if (j && s <= streams[j - 1]) return "streams must ascend, one job per stream";
        if (kf_ids[j] <= H.last_id[(size_t)s]) return "kf_id must be above the stream's last stored id";
        memset(&out[j], 0, sizeof(LcJob));
        out[j].stream = s; out[j].kf_id = kf_ids[j]; out[j].count = H.count[(size_t)s];
    }
    return nullptr;
}

static inline void lc_host_configure(LcHost &H, int nstreams, int capacity, int dim)
{
    H.nstreams = nstreams; H.capacity = capacity; H.dim = dim; H.dp = lc_padded(dim);
    H.count.assign((size_t)nstreams, 0); H.last_id.assign((size_t)nstreams, -1);
}
static inline void lc_host_appended(LcHost &H, int n, const LcApp *apps)
{
    for (int i = 0; i < n; ++i) { H.count[(size_t)apps[i].stream] = apps[i].slot + 1; H.last_id[(size_t)apps[i].stream] = apps[i].kf_id; }
}
// a stored row back in the vector's own order
static inline void lc_unpermute(const float *row, int dim, int dp, float *out)
{
    for (int p = 0; p < dp; ++p) { const int e = lc_elem(p); if (e < dim) out[e] = row[p]; }
}

// ---- device side ------------------------------------------------------------------------------------------------------------------
// the halving tree over a row's 64 accumulators
#ifdef LC_HOST_EMU
static inline float lc_wave_sum(LcLaneF &a)
{
    for (int s = 32; s >= 1; s >>= 1)
        for (int l = 0; l < s; ++l) a.v[l] = a.v[l] + a.v[l + s];
    return a.v[0];
}
#else
__device__ static inline float lc_wave_sum(LcLaneF &a)
{
    for (int s = 32; s >= 1; s >>= 1) a.v = a.v + __shfl_xor(a.v, s);
    return a.v;
}
#endif

// lane's accumulator over a vector in its own order: the elements lane, lane + 64, ... below dim
LC_DEV static inline float lc_lane_self(const float *a, int dim, int lane)
{
    float acc = 0.0f;
    for (int e = lane; e < dim; e += 64) acc = acc + a[e] * a[e];
    return acc;
}

// lane's accumulators of LC_ROWS stored rows against the query, both in the row layout
LC_DEV static inline void lc_lane_dots(const float *const *rows, const float *q, int dp, int lane, float *acc)
{
    for (int k = 0; k < LC_ROWS; ++k) acc[k] = 0.0f;
    for (int c = 4 * lane; c < dp; c += LC_CHUNK) {
        const LcF4 y = *(const LcF4 *)(q + c);
        LcF4 x[LC_ROWS];
        for (int k = 0; k < LC_ROWS; ++k) x[k] = *(const LcF4 *)(rows[k] + c);
        for (int k = 0; k < LC_ROWS; ++k) {
            acc[k] = acc[k] + x[k].x * y.x;
            acc[k] = acc[k] + x[k].y * y.y;
            acc[k] = acc[k] + x[k].z * y.z;
            acc[k] = acc[k] + x[k].w * y.w;
        }
    }
}

LC_DEV static inline bool lc_norm_ok(float n2) { return n2 > 0.0f && n2 <= FLT_MAX; }      // not zero, not infinite, not NaN

// a compared row, in ascending id inside a wave
LC_DEV static inline void lc_take(LcBest &B, float sim, int id, float weak)
{
    B.n_cmp++;
    if (sim > B.sim) { B.sim = sim; B.id = id; }
    if (sim > weak) B.n_weak++;
}

// another wave's result: the larger similarity, the lower id on a tie, whichever comes first
LC_DEV static inline void lc_merge(LcBest &A, const LcBest &b)
{
    if (b.id >= 0 && (b.sim > A.sim || (b.sim == A.sim && b.id < A.id))) { A.sim = b.sim; A.id = b.id; }
    A.n_weak += b.n_weak; A.n_cmp += b.n_cmp;
}

LC_DEV static inline void lc_decide(const LcBest &B, const LcParams &P, LcJob &J)
{
    int st = LC_FOUND;
    if (B.id < 0) st = LC_NONE;
    else if (B.sim < P.strong) st = LC_BELOW_STRONG;
    else if (B.n_weak > P.max_num_weak) st = LC_TOO_MANY_WEAK;
    J.status = st; J.cand_kf = st == LC_FOUND ? B.id : -1;
    J.best_sim = B.sim; J.best_kf = B.id; J.n_weak = B.n_weak; J.n_compared = B.n_cmp;
}

LC_DEV static inline void lc_run(const LcStore &S, const LcParams &P, LcJob &J, const float *vec, LcShared &Sh)
{
    const int dp = S.dp;
    LC_WAVE_LOOP LC_LANES {                                     // the query in the row layout
        for (int p = wave * 64 + lane; p < dp; p += LC_THREADS) { const int e = lc_elem(p); Sh.q[p] = e < S.dim ? vec[e] : 0.0f; }
    }
    LC_SYNC
    LC_WAVE_LOOP {
        if (wave == 0) {
            LcLaneF acc;
            LC_LANES {
                float a = 0.0f;
                for (int c = 4 * lane; c < dp; c += LC_CHUNK) {
                    const LcF4 y = *(const LcF4 *)(Sh.q + c);
                    a = a + y.x * y.x; a = a + y.y * y.y; a = a + y.z * y.z; a = a + y.w * y.w;
                }
                LC_AT(acc) = a;
            }
            const float n2 = lc_wave_sum(acc);
            LC_LANES { if (lane == 0) Sh.n2 = n2; }
        }
    }
    LC_SYNC
    const float n2 = Sh.n2;
    if (!lc_norm_ok(n2)) {
        LC_WAVE_LOOP LC_LANES {
            if (wave == 0 && lane == 0) {
                J.status = LC_BAD_VECTOR; J.cand_kf = -1; J.best_sim = 0.0f; J.best_kf = -1; J.n_weak = 0; J.n_compared = 0;
            }
        }
        return;
    }
    const float norm = sqrtf(n2);
    LC_WAVE_LOOP LC_LANES {
        for (int p = wave * 64 + lane; p < dp; p += LC_THREADS) Sh.q[p] = Sh.q[p] / norm;
    }
    LC_SYNC
    const float *rows = S.rows + (size_t)J.stream * S.capacity * dp;
    const int *ids = S.ids + (size_t)J.stream * S.capacity;
    LC_WAVE_LOOP {
        LcBest B = { 0.0f, -1, 0, 0 };
        for (int r0 = wave * LC_ROWS; r0 < J.count; r0 += LC_WAVES * LC_ROWS) {
            int id[LC_ROWS];
            bool use[LC_ROWS], any = false;
            const float *rp[LC_ROWS];
            for (int k = 0; k < LC_ROWS; ++k) {
                const int r = r0 + k;
                id[k] = r < J.count ? ids[r] : 0;
                use[k] = r < J.count && !(J.kf_id - id[k] < P.min_gap);
                any = any || use[k];
                rp[k] = rows + (size_t)(use[k] ? r : r0) * dp;           // a row that is not compared reads row r0 and drops the sum
            }
            if (!any) continue;
            LcLaneF acc[LC_ROWS];
            LC_LANES {
                float a[LC_ROWS];
                lc_lane_dots(rp, Sh.q, dp, lane, a);
                for (int k = 0; k < LC_ROWS; ++k) LC_AT(acc[k]) = a[k];
            }
            for (int k = 0; k < LC_ROWS; ++k) {
                const float sim = lc_wave_sum(acc[k]);
                if (use[k]) lc_take(B, sim, id[k], P.weak);
            }
        }
        LC_LANES { if (lane == 0) Sh.w[wave] = B; }
    }
    LC_SYNC
    LC_WAVE_LOOP LC_LANES {
        if (wave == 0 && lane == 0) {
            LcBest B = { 0.0f, -1, 0, 0 };
            for (int w = 0; w < LC_WAVES; ++w) lc_merge(B, Sh.w[w]);
            lc_decide(B, P, J);
        }
    }
}

// one wave per vector: commit == 0 reports whether it can be normalised, commit == 1 writes the normalised row and its id
LC_DEV static inline void lc_append_run(const LcStore &S, LcApp &A, const float *vec, int commit)
{
    LcLaneF acc;
    LC_LANES { LC_AT(acc) = lc_lane_self(vec, S.dim, lane); }
    const float n2 = lc_wave_sum(acc);
    const bool ok = lc_norm_ok(n2);
    if (!commit) {
        LC_LANES { if (lane == 0) A.status = ok ? 0 : LC_BAD_VECTOR; }
        return;
    }
    if (!ok) return;
    const float norm = sqrtf(n2);
    const size_t at = (size_t)A.stream * S.capacity + A.slot;
    float *row = S.rows + at * S.dp;
    LC_LANES {
        for (int c = 0; c < S.dp; c += LC_CHUNK) {
            const int e = c + lane;
            LcF4 v;
            v.x = e < S.dim ? vec[e] / norm : 0.0f;
            v.y = e + 64 < S.dim ? vec[e + 64] / norm : 0.0f;
            v.z = e + 128 < S.dim ? vec[e + 128] / norm : 0.0f;
            v.w = e + 192 < S.dim ? vec[e + 192] / norm : 0.0f;
            *(LcF4 *)(row + c + 4 * lane) = v;
        }
        if (lane == 0) S.ids[at] = A.kf_id;
    }
}

#ifndef LC_HOST_EMU
__global__ void __launch_bounds__(LC_THREADS) k_lc_candidates(LcStore S, LcParams P, LcJob *jobs, const float *vecs)
{
    __shared__ LcShared Sh;
    lc_run(S, P, jobs[blockIdx.x], vecs + (size_t)blockIdx.x * S.dim, Sh);
}

__global__ void __launch_bounds__(64) k_lc_append(LcStore S, LcApp *apps, const float *vecs, int commit)
{
    lc_append_run(S, apps[blockIdx.x], vecs + (size_t)blockIdx.x * S.dim, commit);
}
#endif
