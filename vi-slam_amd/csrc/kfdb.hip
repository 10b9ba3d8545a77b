// kfdb.hip -- loop-closure candidates: a keyframe database on the device and a brute-force scorer (include/vislam_hip.h has the contract,
// tests/kfdb_ref.py restates it).
//
// k_kfdb_rows    expands descriptor rows into the FP4 operand (k_expand's bit trick, match.hip) and, for an add, copies pixels, count and id
//                into the ring slots the HOST chose.
// k_loop_score   one workgroup per (query, slot) couple: both directions of the Hamming 2-NN with k_knn_mfma's chain, the winners kept in LDS
//                tables instead of key rows in global memory, then computeSymMatches' mutual test.  EMIT = false: one int32 per couple.
//                EMIT = true: the couple's match list and the pixel rows the pose calls read.
// k_loop_topk    one workgroup per query: topk selections over its score row, fixed order, no atomics; the vis_loop_query record.
//
// The 2-NN chain (v_mfma_scale_f32_32x32x64_f8f6f4 on +-1 FP4, keys in the accumulator's start value aged by 16 per tile, the v_med3_i32 /
// v_min_i32 merges, the tail form) is a COPY of k_knn_mfma<2, false>'s text, not a shared header: match.hip is untouched, so the matcher's
// resource lines cannot move.
#include "vis_internal.h"

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

// Where the rows of a call come from.  ids == nullptr: id = id0 + i (the batch forms; links = the keyframe gate's table or nullptr).
struct KfRows { const int32_t* nkp; const int32_t* ids; const int32_t* links; int id0, step, cap; };
// the count a row takes part with -- clamped to [0, cap]; 0 for a negative id, a frame the gate did not save or one off the step -- and its id
__device__ __forceinline__ void kf_meta(const KfRows& r, int i, int& n, int& id) {
    id = r.ids ? r.ids[i] : r.id0 + i;
    n = min(max(r.nkp[i], 0), r.cap);
    if (id < 0 || (r.links && r.links[i] == VIS_KF_NOT_SAVED) || (r.step > 1 && id % r.step != 0)) n = 0;
}
struct KfDev { const int8_t* X; const float2* xy; const int32_t* cnt; const int32_t* id; int entry_cap, kp_cap; };
// the queries of a call: operand rows of xstride descriptors, keypoint rows of kps_row bytes (EMIT only)
struct KfQuery { KfRows rows; const int8_t* X; size_t xstride; const char* kps; size_t kps_row; };

// Row k of the call = source row first + k * every.  ring > 0 (an add): destination = slot (head + k) % ring, and a row that a LATER row of the
// same call overwrites (k + ring < m) is not written at all, so no two workgroups write one slot.  ring == 0: destination = k (the query operands).
// desc: raw 32-byte rows of src_stride descriptors, or srcX: rows that are expanded already.
__global__ __launch_bounds__(256) void k_kfdb_rows(KfRows R, int first, int every, const uint8_t* __restrict__ desc, const int8_t* __restrict__ srcX,
                                                   size_t src_stride, const char* __restrict__ kps, size_t kps_row, int m, int head, int ring,
                                                   size_t dst_stride, int8_t* __restrict__ X, float2* __restrict__ xy, int32_t* __restrict__ cnt,
                                                   int32_t* __restrict__ idv) {
    const int k = blockIdx.x;                                         // (rows on x: a call may bring more than 65535)
    if (ring > 0 && (long long)k + ring < m) return;
    const int i = first + k * every, dst = ring > 0 ? (head + k) % ring : k;
    int n, id;
    kf_meta(R, i, n, id);
    if (cnt && blockIdx.y == 0 && threadIdx.x == 0) { cnt[dst] = n; idv[dst] = id; }
    const int gid = blockIdx.y * 256 + threadIdx.x, j = gid >> 3, part = gid & 7;
    if (j >= n) return;
    uint4 o;
    if (srcX) o = *reinterpret_cast<const uint4*>(srcX + ((size_t)i * src_stride + j) * 128 + 16 * part);
    else {
        const uint32_t bits = *reinterpret_cast<const uint32_t*>(desc + ((size_t)i * src_stride + j) * 32 + 4 * part);
        uint32_t w[4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            uint32_t x = (bits >> (8 * b)) & 0xFFu;                   // 8 bits -> bit 4 k of a dword
            x = (x | (x << 12)) & 0x000F000Fu;
            x = (x | (x << 6)) & 0x03030303u;
            x = (x | (x << 3)) & 0x11111111u;
            w[b] = 0x22222222u | ((~x & 0x11111111u) << 3);          // magnitude 1, sign bit set where the descriptor bit is 0
        }
        o = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *reinterpret_cast<uint4*>(X + ((size_t)dst * dst_stride + j) * 128 + 16 * part) = o;
    if (xy && part == 0) {
        const float* kp = reinterpret_cast<const float*>(kps + (size_t)i * kps_row + (size_t)j * sizeof(vis_keypoint));
        xy[(size_t)dst * dst_stride + j] = make_float2(kp[0], kp[1]);
    }
}

#define KM_ROW 9             // uint4 per LDS row: 128 B of descriptor + 16 B pad
#define KNN_NONE 0x7F000000
static __device__ __forceinline__ int imed3(int a, int b, int c) {
    int d;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
static __device__ __forceinline__ bool ratio_survives(uint32_t k0, uint32_t k1, double ratio) {
    if (k0 == 0xFFFFFFFFu || k1 == 0xFFFFFFFFu) return false;               // fewer than 2 neighbours
    const double d0 = (double)(float)(k0 >> 16), d1 = (double)(float)(k1 >> 16);
    return !(d0 > ratio * d1);
}
// a winner table's word: the best neighbour's row (14 bits), its Hamming distance (9 bits), whether the ratio test was passed, whether there is a neighbour
#define KT_ROW(w) ((int)((w) & 0x3FFFu))
#define KT_DIST(w) (((w) >> 14) & 0x1FFu)
#define KT_SURV(w) (((w) >> 23) & 1u)
#define KT_HAVE(w) (((w) >> 24) & 1u)

// One direction of a couple: for every descriptor of the fixed set (nf rows at xf) its two nearest rows of the swept set (ns >= 1 rows at xs), in
// chunks of 256 fixed descriptors (4 waves x 2 column groups of 32) so that one workgroup covers any count; tab[f] = the winner's word.  The chain
// is k_knn_mfma<2, false>'s (match.hip has the derivation of the key form and the ageing); every thread of the workgroup must call it.
static __device__ __forceinline__ void loop_sweep(const int8_t* __restrict__ xf, int nf, const int8_t* __restrict__ xs, int ns, uint32_t* tab,
                                                  uint4 (*tile)[32 * KM_ROW], double ratio) {
    constexpr int NC = 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    const int ntiles = (ns + 31) / 32;
    const int st_row = tid >> 3, st_c = tid & 7;
    v16f cstart;
#pragma unroll
    for (int r = 0; r < 16; r++) cstart[r] = 1048576.f + 8192.f + (float)r;
    for (int fbase = 0; fbase < nf; fbase += 128 * NC) {
        const int fidx0 = fbase + wave * (32 * NC) + col;
        v8i bf[NC][4];
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const int8_t* p = xf + (size_t)min(fidx0 + 32 * c, nf - 1) * 128 + 16 * h;
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
                const v4i x = *reinterpret_cast<const v4i*>(p + 32 * ks);         // negated: the chain adds 4096 * (2 * Hamming - 256)
                bf[c][ks] = v8i{x[0] ^ (int)0x88888888, x[1] ^ (int)0x88888888, x[2] ^ (int)0x88888888, x[3] ^ (int)0x88888888, 0, 0, 0, 0};
            }
        }
        uint4 pre;
#define STAGE_LOAD(t_) pre = *reinterpret_cast<const uint4*>(xs + (size_t)min((t_) * 32 + st_row, ns - 1) * 128 + 16 * st_c)
#define STAGE_STORE(buf_) tile[buf_][st_row * KM_ROW + st_c] = pre
        int k0[NC], k1[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) { k0[c] = KNN_NONE; k1[c] = KNN_NONE; }
        STAGE_LOAD(0); STAGE_STORE(0);
        __syncthreads();
        for (int t = 0; t < ntiles; t++) {
            if (t + 1 < ntiles) STAGE_LOAD(t + 1);
            const uint4* tb = tile[t & 1] + col * KM_ROW + h;
            v16f acc[NC];
#pragma unroll
            for (int c = 0; c < NC; c++) acc[c] = cstart;
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
                const uint4 au = tb[2 * ks];
                const v8i a = {(int)au.x, (int)au.y, (int)au.z, (int)au.w, 0, 0, 0, 0};
#pragma unroll
                for (int c = 0; c < NC; c++)      // cbsz = blgp = 4: FP4 e2m1 on both sides; scales 2^6 (e8m0 133): products +-4096
                    acc[c] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, bf[c][ks], acc[c], 4, 4, 0, 133, 0, 133);
            }
#pragma unroll
            for (int c = 0; c < NC; c++) {                                 // age the running keys by one tile; exact float subtractions
                k0[c] = __float_as_int(__int_as_float(k0[c]) - 16.f);
                k1[c] = __float_as_int(__int_as_float(k1[c]) - 16.f);
            }
            if (t * 32 + 32 <= ns) {
#pragma unroll
                for (int c = 0; c < NC; c++)
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {                      // two distinct keys per step, three instructions
                        const int x = __float_as_int(acc[c][r]), y = __float_as_int(acc[c][r + 1]);
                        k1[c] = min(k1[c], imed3(k0[c], x, y));
                        k0[c] = min(min(k0[c], x), y);
                    }
            } else {
                const int toff = t * 32 + 4 * h;
#pragma unroll
                for (int c = 0; c < NC; c++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int trow = toff + (r & 3) + 8 * (r >> 2);
                        const int key = trow < ns ? __float_as_int(acc[c][r]) : KNN_NONE;
                        k1[c] = imed3(k0[c], k1[c], key);
                        k0[c] = min(k0[c], key);
                    }
            }
            if (t + 1 < ntiles) STAGE_STORE((t + 1) & 1);
            __syncthreads();
        }
#undef STAGE_LOAD
#undef STAGE_STORE
        auto true_key = [&](int k) -> uint32_t {                           // (Hamming << 16) | row: the record format of k_filter
            const uint32_t w = (uint32_t)__int_as_float(k) + 16u * (uint32_t)(ntiles - 1);
            const uint32_t lo = w & 8191u, r = lo & 15u;
            const uint32_t row = (lo >> 4) * 32u + 4u * (uint32_t)h + (r & 3u) + 8u * (r >> 2);
            return k == KNN_NONE ? 0xFFFFFFFFu : ((((w >> 13) - 1u) << 16) | row);
        };
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const uint32_t a0 = true_key(k0[c]), a1 = true_key(k1[c]);
            const uint32_t o0 = __shfl_xor(a0, 32), o1 = __shfl_xor(a1, 32);   // lanes l and l + 32 hold the two row halves of one column
            const uint32_t m0 = min(a0, o0), m1 = min(max(a0, o0), min(a1, o1));
            const int fidx = fidx0 + 32 * c;
            if (h == 0 && fidx < nf)
                tab[fidx] = m0 == 0xFFFFFFFFu ? 0u : ((m0 & 0x3FFFu) | ((m0 >> 16) << 14) | ((ratio_survives(m0, m1, ratio) ? 1u : 0u) << 23) | (1u << 24));
        }
    }
}

// computeSymMatches' test of entry keypoint e (k_filter, match.hip): ratio on direction 1, mutual best, ratio on direction 2 when INTENDED
static __device__ __forceinline__ bool loop_mutual(const uint32_t* tabE, const uint32_t* tabQ, int e, int sym_mode, uint32_t& a) {
    a = tabE[e];
    if (!KT_SURV(a)) return false;
    const uint32_t b = tabQ[KT_ROW(a)];
    return KT_HAVE(b) && KT_ROW(b) == e && (sym_mode != VIS_SYM_INTENDED || KT_SURV(b));
}

// EMIT = false: the m queries qfirst, qfirst + qevery ... (the rows on the step: a query off it launches no workgroup, k_loop_topk writes its row);
// grid 8 * ceil(entry_cap / 8) * m; workgroups are dealt round-robin over the 8 XCDs (private L2 each) and all couples of one slot go to ONE XCD,
// so an entry is fetched into one L2 once while the queries stream past it.  EMIT = true: grid n, the couple is the candidate's.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_loop_score(KfDev D, KfQuery Q, int m, int qfirst, int qevery, long long min_gap, double ratio, int sym_mode, int32_t* __restrict__ scores,
                                                    const vis_loop_cand* __restrict__ cand, int cand_stride, int max_pts, vis_dmatch* __restrict__ matches,
                                                    float* __restrict__ p1, float* __restrict__ p2, int32_t* __restrict__ npts) {
    __shared__ __attribute__((aligned(16))) uint4 tile[2][32 * KM_ROW];
    __shared__ int red[260];
    extern __shared__ __attribute__((aligned(16))) uint32_t tab[];          // tabE[nE] | tabQ[nQ]
    const int tid = threadIdx.x;
    int q, slot;
    if constexpr (EMIT) { q = blockIdx.x; slot = cand[(size_t)q * cand_stride].slot; }
    else {
        const int xcd = blockIdx.x & 7, jb = blockIdx.x >> 3;
        slot = (jb / m) * 8 + xcd; q = qfirst + (jb % m) * qevery;
        if (slot >= D.entry_cap) return;
    }
    int nQ, idQ;
    kf_meta(Q.rows, q, nQ, idQ);
    int nE = 0;
    if constexpr (EMIT) {
        const bool live = slot >= 0 && slot < D.entry_cap && nQ > 0;
        if (live) nE = D.cnt[slot];
        if (!live || nE <= 0 || D.id[slot] != cand[(size_t)q * cand_stride].id) { if (tid == 0) npts[q] = 0; return; }
    } else {
        nE = D.cnt[slot];
        if (!(nQ > 0 && nE > 0 && idQ >= 0 && (long long)D.id[slot] + min_gap <= (long long)idQ)) {
            if (tid == 0) scores[(size_t)q * D.entry_cap + slot] = -1;
            return;
        }
    }
    uint32_t* tabE = tab;
    uint32_t* tabQ = tab + nE;
    const int8_t* xe = D.X + (size_t)slot * D.kp_cap * 128;
    const int8_t* xq = Q.X + (size_t)q * Q.xstride * 128;
    loop_sweep(xe, nE, xq, nQ, tabE, tile, ratio);
    loop_sweep(xq, nQ, xe, nE, tabQ, tile, ratio);
    __syncthreads();
    if constexpr (!EMIT) {
        const int lane = tid & 63, wave = tid >> 6;
        int c = 0;
        for (int base = wave * 64; base < nE; base += 256) {               // (wave-uniform bound: the ballot sees whole waves)
            const int e = base + lane;
            uint32_t a;
            const bool ok = e < nE && loop_mutual(tabE, tabQ, e, sym_mode, a);
            c += __popcll(__ballot(ok));
        }
        if (lane == 0) red[wave] = c;
        __syncthreads();
        if (tid == 0) scores[(size_t)q * D.entry_cap + slot] = (red[0] + red[1]) + (red[2] + red[3]);
    } else {
        // ordered compaction over e (chunk per thread + block scan), as k_filter does
        const int chunk = (nE + 255) / 256, eb = tid * chunk, ee = min(nE, eb + chunk);
        int c = 0;
        uint32_t a;
        for (int e = eb; e < ee; e++) c += loop_mutual(tabE, tabQ, e, sym_mode, a) ? 1 : 0;
        red[tid] = c;
        __syncthreads();
        if (tid == 0) { int acc = 0; for (int i = 0; i < 256; i++) { const int v = red[i]; red[i] = acc; acc += v; } red[256] = acc; }
        __syncthreads();
        int pos = red[tid];
        const float2* exy = D.xy + (size_t)slot * D.kp_cap;
        const char* qk = Q.kps + (size_t)q * Q.kps_row;
        for (int e = eb; e < ee && pos < max_pts; e++) {
            if (!loop_mutual(tabE, tabQ, e, sym_mode, a)) continue;
            const int t = KT_ROW(a);
            const size_t o = (size_t)q * max_pts + pos;
            if (matches) { vis_dmatch m; m.queryIdx = e; m.trainIdx = t; m.imgIdx = slot; m.distance = (float)KT_DIST(a); matches[o] = m; }
            const float2 pe = exy[e];
            const float* kp = reinterpret_cast<const float*>(qk + (size_t)t * sizeof(vis_keypoint));
            p1[2 * o] = pe.x; p1[2 * o + 1] = pe.y;
            p2[2 * o] = kp[0]; p2[2 * o + 1] = kp[1];
            pos++;
        }
        if (tid == 0) npts[q] = red[256];
    }
}

// One workgroup per query.  A selection takes the smallest (key, slot) above the one before it, key = (0x7FFFFFFF - score) << 32 | id: score falling,
// id rising, slot rising.  Integers, a fixed reduction tree, no atomics.
__global__ __launch_bounds__(256) void k_loop_topk(KfDev D, KfRows R, int32_t* __restrict__ scores, int topk, int min_score,
                                                   vis_loop_cand* __restrict__ cand, vis_loop_query* __restrict__ qrec) {
    __shared__ unsigned long long skey[256];
    __shared__ int sslot[256], sa[256], sb[256];
    const int q = blockIdx.x, tid = threadIdx.x;
    int nQ, idQ;
    kf_meta(R, q, nQ, idQ);
    int32_t* s = scores + (size_t)q * D.entry_cap;
    if (nQ <= 0) {                                                        // a skipped query: no workgroup scored it, its row is written here
        for (int e = tid; e < D.entry_cap; e += 256) s[e] = -1;
        __syncthreads();
    }
    int nsc = 0, best = -1;
    for (int e = tid; e < D.entry_cap; e += 256) { const int v = s[e]; nsc += v >= 0; best = max(best, v); }
    sa[tid] = nsc; sb[tid] = best;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) { sa[tid] += sa[tid + w]; sb[tid] = max(sb[tid], sb[tid + w]); } __syncthreads(); }
    nsc = sa[0]; best = sb[0];
    __syncthreads();
    unsigned long long pkey = 0; int pslot = -1, ncand = 0;               // the selection before: nothing is at or below (0, -1)
    for (int r = 0; r < topk; r++) {
        unsigned long long bk = ~0ull; int bs = 0x7FFFFFFF;
        for (int e = tid; e < D.entry_cap; e += 256) {
            const int v = s[e];
            if (v < 0 || v < min_score) continue;
            const unsigned long long key = ((unsigned long long)(uint32_t)(0x7FFFFFFF - v) << 32) | (uint32_t)D.id[e];
            const bool above = key > pkey || (key == pkey && e > pslot);
            if (above && (key < bk || (key == bk && e < bs))) { bk = key; bs = e; }
        }
        skey[tid] = bk; sslot[tid] = bs;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) {
                const unsigned long long ok = skey[tid + w]; const int os = sslot[tid + w];
                if (ok < skey[tid] || (ok == skey[tid] && os < sslot[tid])) { skey[tid] = ok; sslot[tid] = os; }
            }
            __syncthreads();
        }
        bk = skey[0]; bs = sslot[0];
        __syncthreads();
        const bool found = bs != 0x7FFFFFFF;
        if (tid == 0) {
            vis_loop_cand c;
            if (found) { c.id = D.id[bs]; c.slot = bs; c.score = s[bs]; c.n_keypoints = D.cnt[bs]; }
            else { c.id = -1; c.slot = -1; c.score = 0; c.n_keypoints = 0; }
            cand[(size_t)q * topk + r] = c;
        }
        if (found) { pkey = bk; pslot = bs; ncand++; }
        else { pkey = ~0ull; pslot = 0x7FFFFFFF; }                        // nothing is above this: the rest of the row is filled
    }
    if (tid == 0) {
        vis_loop_query o;
        o.id = idQ; o.n_keypoints = nQ; o.n_scored = nsc; o.n_cand = ncand; o.best_score = best;
        o.flags = nQ > 0 ? 0 : VIS_LOOP_SKIPPED; o.reserved_[0] = o.reserved_[1] = 0;
        qrec[q] = o;
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct vis_kfdb {
    vis_ctx* ctx = nullptr;
    int entry_cap = 0, kp_cap = 0, head = 0;
    long long total = 0;
    int8_t* d_x = nullptr; float2* d_xy = nullptr; int32_t* d_cnt = nullptr; int32_t* d_id = nullptr;
    // score rows of the calls that pass no d_scores: grow-only (a call that grows it drains the context's streams); such a call is queued as a WRITER
    // of the database, so two of them never share the block
    DevBlock scores;
    // Call order on one database whichever stream a call rides: a writer (add, reset) waits for the readers noted since the last writer and for that
    // writer; a reader (query, match) waits for the last writer.  One reader event per stream slot of the guard.
    ReaderGuard readers; hipEvent_t ev_rd[4] = {}; hipEvent_t ev_wr = nullptr; bool wr_valid = false;
    bool lds_set[2] = {false, false};
};

static bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
static KfDev kf_dev(const vis_kfdb* db) { return KfDev{db->d_x, db->d_xy, db->d_cnt, db->d_id, db->entry_cap, db->kp_cap}; }

static int kf_begin(vis_kfdb* db, bool writer) {
    vis_ctx* ctx = db->ctx;
    if (db->wr_valid) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, db->ev_wr, 0));
    if (writer) HIPCHK(ctx, db->readers.wait(ctx->stream));
    return VIS_OK;
}
static int kf_end(vis_kfdb* db, bool writer) {
    vis_ctx* ctx = db->ctx;
    const hipStream_t s = ctx->stream;
    if (writer) {
        HIPCHK(ctx, hipEventRecord(db->ev_wr, s));
        db->wr_valid = true; db->readers.clear();
        return VIS_OK;
    }
    int i = 0;
    while (i < 3 && db->readers.stream[i] && db->readers.stream[i] != s) i++;          // (ReaderGuard::note's slot)
    // a fifth stream takes the last slot over: it waits for the reader it displaces, so its event stands for both
    if (db->readers.stream[i] && db->readers.stream[i] != s) HIPCHK(ctx, hipStreamWaitEvent(s, db->readers.event[i], 0));
    HIPCHK(ctx, hipEventRecord(db->ev_rd[i], s));
    db->readers.note(s, db->ev_rd[i]);
    return VIS_OK;
}

extern "C" void vis_default_loop_params(vis_loop_params* lp) {
    if (!lp) return;
    lp->ratio = 0.8f; lp->sym_mode = VIS_SYM_INTENDED; lp->min_gap = 30; lp->topk = 4; lp->min_score = 30; lp->reserved_ = 0;
}
static bool loop_params_ok(const vis_loop_params* lp) {
    return lp && (lp->sym_mode == VIS_SYM_REFERENCE_EFFECTIVE || lp->sym_mode == VIS_SYM_INTENDED) && lp->min_gap >= 0 && lp->topk >= 1 && lp->topk <= 16;
}

extern "C" void vis_kfdb_destroy(vis_kfdb* db) {
    if (!db) return;
    vis_ctx* ctx = db->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->pose_stream) (void)hipStreamSynchronize(ctx->pose_stream);
    for (void* p : {(void*)db->d_x, (void*)db->d_xy, (void*)db->d_cnt, (void*)db->d_id, db->scores.p}) if (p) (void)hipFree(p);
    for (hipEvent_t e : db->ev_rd) if (e) (void)hipEventDestroy(e);
    if (db->ev_wr) (void)hipEventDestroy(db->ev_wr);
    delete db;
}

extern "C" int vis_kfdb_create(vis_ctx* ctx, int entry_cap, int kp_cap, vis_kfdb** out) {
    if (!out) return VIS_E_INVALID;
    *out = nullptr;
    if (entry_cap < 1 || entry_cap > 65536 || kp_cap < 1 || kp_cap > 16384) return VIS_E_INVALID;
    if (!ctx) return VIS_E_STATE;
    (void)hipSetDevice(ctx->device);
    vis_kfdb* db = new (std::nothrow) vis_kfdb();
    if (!db) return VIS_E_NOMEM;
    db->ctx = ctx; db->entry_cap = entry_cap; db->kp_cap = kp_cap;
    const size_t slots = (size_t)entry_cap * kp_cap;
    bool ok = hipMalloc((void**)&db->d_x, slots * 128) == hipSuccess && hipMalloc((void**)&db->d_xy, slots * sizeof(float2)) == hipSuccess &&
              hipMalloc((void**)&db->d_cnt, (size_t)entry_cap * 4) == hipSuccess && hipMalloc((void**)&db->d_id, (size_t)entry_cap * 4) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); vis_kfdb_destroy(db); ctx->err = "vis_kfdb_create: out of device memory for " + std::to_string(slots * 136) + " bytes"; return VIS_E_NOMEM; }
    for (hipEvent_t& e : db->ev_rd) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&db->ev_wr, hipEventDisableTiming) == hipSuccess;
    if (!ok) { vis_kfdb_destroy(db); ctx->err = "vis_kfdb_create: hipEventCreateWithFlags failed"; return VIS_E_HIP; }
    const int rc = vis_kfdb_reset(db);
    if (rc) { vis_kfdb_destroy(db); return rc; }
    *out = db;
    return VIS_OK;
}

extern "C" int vis_kfdb_reset(vis_kfdb* db) {
    if (!db) return VIS_E_STATE;
    vis_ctx* ctx = db->ctx;
    (void)hipSetDevice(ctx->device);
    { const int rc = kf_begin(db, true); if (rc) return rc; }
    HIPCHK(ctx, hipMemsetAsync(db->d_cnt, 0, (size_t)db->entry_cap * 4, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(db->d_id, 0xFF, (size_t)db->entry_cap * 4, ctx->stream));
    db->head = 0; db->total = 0;
    return kf_end(db, true);
}

extern "C" int vis_kfdb_info(vis_kfdb* db, vis_kfdb_info_t* info) {
    if (!info || !aligned(info, 4)) return VIS_E_INVALID;
    if (!db) return VIS_E_STATE;
    info->entry_cap = db->entry_cap; info->kp_cap = db->kp_cap; info->head = db->head; info->reserved_ = 0; info->total_added = db->total;
    return VIS_OK;
}

extern "C" int vis_kfdb_get_entry(vis_kfdb* db, int slot, int32_t* id, int32_t* count, float* xy, int cap) {
    if (!id || !count || cap < 0 || (cap > 0 && !xy) || !aligned(id, 4) || !aligned(count, 4) || !aligned(xy, 4)) return VIS_E_INVALID;
    if (!db) return VIS_E_STATE;
    if (slot < 0 || slot >= db->entry_cap) return VIS_E_INVALID;
    vis_ctx* ctx = db->ctx;
    (void)hipSetDevice(ctx->device);
    if (db->wr_valid) HIPCHK(ctx, hipEventSynchronize(db->ev_wr));
    HIPCHK(ctx, hipMemcpy(id, db->d_id + slot, 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(count, db->d_cnt + slot, 4, hipMemcpyDeviceToHost));
    const int m = std::min(std::max(*count, 0), cap);
    if (m > 0) HIPCHK(ctx, hipMemcpy(xy, db->d_xy + (size_t)slot * db->kp_cap, (size_t)m * 8, hipMemcpyDeviceToHost));
    return VIS_OK;
}

// m rows into the slots behind the head, on ctx->stream, as a writer; the head moves once the launch was queued
static int kf_add(vis_kfdb* db, const KfRows& R, int first, int every, int m, const uint8_t* desc, const int8_t* srcX, size_t src_stride, const char* kps,
                  size_t kps_row) {
    vis_ctx* ctx = db->ctx;
    if (m <= 0) return VIS_OK;
    { const int rc = kf_begin(db, true); if (rc) return rc; }
    if (R.cap > 0) {
        hipLaunchKernelGGL(k_kfdb_rows, dim3((unsigned)m, (unsigned)((R.cap * 8 + 255) / 256)), dim3(256), 0, ctx->stream, R, first, every, desc, srcX, src_stride,
                           kps, kps_row, m, db->head, db->entry_cap, (size_t)db->kp_cap, db->d_x, db->d_xy, db->d_cnt, db->d_id);
    } else {                                                              // rows without room for a keypoint: empty entries all the same
        hipLaunchKernelGGL(k_kfdb_rows, dim3((unsigned)m, 1), dim3(256), 0, ctx->stream, R, first, every, desc, srcX, src_stride, kps, kps_row, m, db->head,
                           db->entry_cap, (size_t)db->kp_cap, db->d_x, db->d_xy, db->d_cnt, db->d_id);
    }
    HIPCHK(ctx, hipGetLastError());
    { const int rc = kf_end(db, true); if (rc) return rc; }
    db->head = (int)(((long long)db->head + m) % db->entry_cap); db->total += m;
    return VIS_OK;
}

template <bool EMIT> static int kf_lds(vis_kfdb* db, size_t lds) {
    if (lds > 48 * 1024 && !db->lds_set[EMIT]) {                  // (beside 10 KB of static LDS)
        HIPCHK(db->ctx, hipFuncSetAttribute((const void*)k_loop_score<EMIT>, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * (16384 + 16384)));
        db->lds_set[EMIT] = true;
    }
    return VIS_OK;
}

// the score rows of a call that passes none: the database's own block, grown BEFORE anything of the call is queued (growing drains the context's streams)
static int kf_scores(vis_kfdb* db, int n, int32_t*& d_scores, bool& own) {
    own = !d_scores;
    if (!own || n <= 0) return VIS_OK;
    const int rc = vis_grow_block(db->ctx, db->scores, (size_t)n * db->entry_cap * 4, "vis_kfdb_query");
    d_scores = (int32_t*)db->scores.p;
    return rc;
}

// score + top-k on ctx->stream; own: d_scores is the database's block, and the call is a writer
static int kf_query(vis_kfdb* db, const vis_loop_params* lp, int n, int qfirst, int qevery, const KfQuery& Q, int32_t* d_scores, bool own, vis_loop_cand* d_cand,
                    vis_loop_query* d_query) {
    vis_ctx* ctx = db->ctx;
    if (n <= 0) return VIS_OK;
    const size_t lds = 4 * ((size_t)db->kp_cap + (size_t)Q.rows.cap);
    { const int rc = kf_lds<false>(db, lds); if (rc) return rc; }
    { const int rc = kf_begin(db, own); if (rc) return rc; }
    const int m = qfirst < n ? (n - qfirst + qevery - 1) / qevery : 0;   // the queries on the step
    if (m > 0) {
        const unsigned grid = 8u * (unsigned)((db->entry_cap + 7) / 8) * (unsigned)m;
        hipLaunchKernelGGL((k_loop_score<false>), dim3(grid), dim3(256), lds, ctx->stream, kf_dev(db), Q, m, qfirst, qevery, (long long)lp->min_gap, (double)lp->ratio,
                           lp->sym_mode, d_scores, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr);
        HIPCHK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_loop_topk, dim3((unsigned)n), dim3(256), 0, ctx->stream, kf_dev(db), Q.rows, d_scores, lp->topk, lp->min_score, d_cand, d_query);
    HIPCHK(ctx, hipGetLastError());
    return kf_end(db, own);
}

static int kf_match(vis_kfdb* db, const vis_loop_params* lp, int n, const KfQuery& Q, const vis_loop_cand* d_cand, int cand_stride, int max_pts,
                    vis_dmatch* d_matches, float* d_p1, float* d_p2, int32_t* d_npts) {
    vis_ctx* ctx = db->ctx;
    if (n <= 0) return VIS_OK;
    const size_t lds = 4 * ((size_t)db->kp_cap + (size_t)Q.rows.cap);
    { const int rc = kf_lds<true>(db, lds); if (rc) return rc; }
    { const int rc = kf_begin(db, false); if (rc) return rc; }
    hipLaunchKernelGGL((k_loop_score<true>), dim3((unsigned)n), dim3(256), lds, ctx->stream, kf_dev(db), Q, n, 0, 1, 0ll, (double)lp->ratio, lp->sym_mode, nullptr,
                       d_cand, cand_stride, max_pts, d_matches, d_p1, d_p2, d_npts);
    HIPCHK(ctx, hipGetLastError());
    return kf_end(db, false);
}

// the rows forms' query operands: n rows of cap descriptors in the context's grow-only block, expanded on ctx->stream
static int kf_expand_rows(vis_kfdb* db, const KfRows& R, int n, const uint8_t* d_desc, int row_cap, KfQuery& Q) {
    vis_ctx* ctx = db->ctx;
    Q.rows = R; Q.xstride = (size_t)R.cap; Q.X = nullptr; Q.kps = nullptr; Q.kps_row = 0;
    if (n <= 0 || R.cap <= 0) return VIS_OK;
    const int rc = vis_grow_block(ctx, ctx->kfdb_ws, (size_t)n * R.cap * 128, "vis_kfdb_query_rows");
    if (rc) return rc;
    Q.X = (const int8_t*)ctx->kfdb_ws.p;
    hipLaunchKernelGGL(k_kfdb_rows, dim3((unsigned)n, (unsigned)((R.cap * 8 + 255) / 256)), dim3(256), 0, ctx->stream, R, 0, 1, d_desc, (const int8_t*)nullptr,
                       (size_t)row_cap, (const char*)nullptr, (size_t)0, n, 0, 0, (size_t)R.cap, (int8_t*)ctx->kfdb_ws.p, (float2*)nullptr, (int32_t*)nullptr,
                       (int32_t*)nullptr);
    HIPCHK(ctx, hipGetLastError());
    return VIS_OK;
}

extern "C" int vis_kfdb_add_rows(vis_kfdb* db, int n, const vis_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_nkp, int row_cap, const int32_t* d_ids) {
    if (!d_kps || !d_desc || !d_nkp || !d_ids || !aligned(d_kps, 4) || !aligned(d_desc, 4) || !aligned(d_nkp, 4) || !aligned(d_ids, 4) || n < 0 || row_cap < 0)
        return VIS_E_INVALID;
    if (!db) return VIS_E_STATE;
    (void)hipSetDevice(db->ctx->device);
    const KfRows R{d_nkp, d_ids, nullptr, 0, 1, std::min(row_cap, db->kp_cap)};
    return kf_add(db, R, 0, 1, n, d_desc, nullptr, (size_t)row_cap, (const char*)d_kps, (size_t)row_cap * sizeof(vis_keypoint));
}

extern "C" int vis_kfdb_query_rows(vis_kfdb* db, const vis_loop_params* lp, int n, const uint8_t* d_desc, const int32_t* d_nkp, int row_cap, const int32_t* d_ids,
                                   int32_t* d_scores, vis_loop_cand* d_cand, vis_loop_query* d_query) {
    if (!loop_params_ok(lp) || !d_desc || !d_nkp || !d_ids || !d_cand || !d_query || !aligned(d_desc, 4) || !aligned(d_nkp, 4) || !aligned(d_ids, 4) ||
        !aligned(d_scores, 4) || !aligned(d_cand, 4) || !aligned(d_query, 4) || n < 0 || row_cap < 0) return VIS_E_INVALID;
    if (!db) return VIS_E_STATE;
    vis_ctx* ctx = db->ctx;
    if ((size_t)n * (size_t)db->entry_cap > ((size_t)1 << 28)) { ctx->err = "vis_kfdb_query_rows: n x entry_cap exceeds 2^28 couples"; return VIS_E_CAPACITY; }
    (void)hipSetDevice(ctx->device);
    KfQuery Q;
    bool own;
    int rc = kf_scores(db, n, d_scores, own);
    if (!rc) rc = kf_expand_rows(db, KfRows{d_nkp, d_ids, nullptr, 0, 1, std::min(row_cap, db->kp_cap)}, n, d_desc, row_cap, Q);
    return rc ? rc : kf_query(db, lp, n, 0, 1, Q, d_scores, own, d_cand, d_query);
}

static bool match_args_ok(const vis_loop_params* lp, int n, const vis_loop_cand* d_cand, int cand_stride, int max_pts, vis_dmatch* d_matches, float* d_p1,
                          float* d_p2, int32_t* d_npts) {
    return loop_params_ok(lp) && d_cand && d_p1 && d_p2 && d_npts && aligned(d_cand, 4) && aligned(d_matches, 4) && aligned(d_p1, 8) && aligned(d_p2, 8) &&
           aligned(d_npts, 4) && n >= 0 && cand_stride >= 0 && max_pts >= 0;
}

extern "C" int vis_kfdb_match_rows(vis_kfdb* db, const vis_loop_params* lp, int n, const vis_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_nkp,
                                   int row_cap, const vis_loop_cand* d_cand, int cand_stride, int max_pts, vis_dmatch* d_matches, float* d_p1, float* d_p2,
                                   int32_t* d_npts) {
    if (!match_args_ok(lp, n, d_cand, cand_stride, max_pts, d_matches, d_p1, d_p2, d_npts) || !d_kps || !d_desc || !d_nkp || !aligned(d_kps, 4) ||
        !aligned(d_desc, 4) || !aligned(d_nkp, 4) || row_cap < 0) return VIS_E_INVALID;
    if (!db) return VIS_E_STATE;
    (void)hipSetDevice(db->ctx->device);
    KfQuery Q;
    const int rc = kf_expand_rows(db, KfRows{d_nkp, nullptr, nullptr, 0, 1, std::min(row_cap, db->kp_cap)}, n, d_desc, row_cap, Q);
    if (rc) return rc;
    Q.kps = (const char*)d_kps; Q.kps_row = (size_t)row_cap * sizeof(vis_keypoint);
    return kf_match(db, lp, n, Q, d_cand, cand_stride, max_pts, d_matches, d_p1, d_p2, d_npts);
}

// ---- the batch forms: the frames of the last vis_batch_run, on the pose stream through the follow-up scaffold
static int batch_state(vis_kfdb* db, int n, bool need_match, const char* who, Plan** out) {
    if (!db || !db->ctx->batch) return VIS_E_STATE;
    vis_ctx* ctx = db->ctx;
    Plan* pl = ctx->batch;
    if (pl->last_n < 1 || n != pl->last_n) return VIS_E_STATE;
    if (!(pl->last_stages & (need_match ? VIS_STAGE_MATCH : (VIS_STAGE_DETECT | VIS_STAGE_MATCH)))) {
        ctx->err = std::string(who) + (need_match ? ": the last vis_batch_run had no VIS_STAGE_MATCH (the expanded descriptors are the matcher's)"
                                                  : ": the last vis_batch_run had no VIS_STAGE_DETECT");
        return VIS_E_STATE;
    }
    if (need_match && !pl->d_descx) { ctx->err = std::string(who) + ": the plan has no expanded descriptors"; return VIS_E_STATE; }
    if (pl->kcap > db->kp_cap) {
        ctx->err = std::string(who) + ": the plan's keypoint capacity " + std::to_string(pl->kcap) + " exceeds the database's kp_cap " + std::to_string(db->kp_cap);
        return VIS_E_CAPACITY;
    }
    *out = pl;
    return VIS_OK;
}
static KfRows plan_rows(Plan* pl, int step) {
    return KfRows{pl->d_nkp + pl->last_base + 1, nullptr, pl->kf_min ? pl->last_set().kf_link : nullptr, pl->seq0, step, pl->kcap};
}
static KfQuery plan_query(Plan* pl, int step) {
    return KfQuery{plan_rows(pl, step), pl->d_descx + (size_t)(pl->last_base + 1) * pl->kcap * 128, (size_t)pl->kcap,
                   (const char*)(pl->d_kps + (size_t)(pl->last_base + 1) * pl->kcap), (size_t)pl->kcap * sizeof(vis_keypoint)};
}
template <class Run> static int plan_follow_up(vis_ctx* ctx, Plan* pl, Run run) {
    (void)hipSetDevice(ctx->device);
    return on_pose_stream(ctx, {FU_FORK | FU_MATCHER, ctx->ev_epi_done[pl->mo_cur]}, [&] { const int rc = run(); if (!rc) ctx->pose_pending = true; return rc; },
                          {&pl->last_set().matcher, pl->kf_min ? &pl->last_set().links : nullptr});
}

extern "C" int vis_batch_kfdb_add(vis_kfdb* db, int n, int step) {
    if (n < 0 || step < 1) return VIS_E_INVALID;
    Plan* pl = nullptr;
    { const int rc = batch_state(db, n, false, "vis_batch_kfdb_add", &pl); if (rc) return rc; }
    const int first = (step - pl->seq0 % step) % step, m = first < n ? (n - first + step - 1) / step : 0;
    if (m == 0) return VIS_OK;
    const size_t rec0 = (size_t)(pl->last_base + 1);
    return plan_follow_up(db->ctx, pl, [&] {
        return kf_add(db, plan_rows(pl, step), first, step, m, pl->d_desc + rec0 * pl->kcap * 32, nullptr, (size_t)pl->kcap, (const char*)(pl->d_kps + rec0 * pl->kcap),
                      (size_t)pl->kcap * sizeof(vis_keypoint));
    });
}

extern "C" int vis_batch_kfdb_query(vis_kfdb* db, const vis_loop_params* lp, int n, int step, int32_t* d_scores, vis_loop_cand* d_cand, vis_loop_query* d_query) {
    if (!loop_params_ok(lp) || !d_cand || !d_query || !aligned(d_scores, 4) || !aligned(d_cand, 4) || !aligned(d_query, 4) || n < 0 || step < 1) return VIS_E_INVALID;
    Plan* pl = nullptr;
    { const int rc = batch_state(db, n, true, "vis_batch_kfdb_query", &pl); if (rc) return rc; }
    if ((size_t)n * (size_t)db->entry_cap > ((size_t)1 << 28)) { db->ctx->err = "vis_batch_kfdb_query: n x entry_cap exceeds 2^28 couples"; return VIS_E_CAPACITY; }
    bool own;
    { const int rc = kf_scores(db, n, d_scores, own); if (rc) return rc; }
    const int first = (step - pl->seq0 % step) % step;            // the first frame of the launch on the step: the host knows seq0
    return plan_follow_up(db->ctx, pl, [&] { return kf_query(db, lp, n, first, step, plan_query(pl, step), d_scores, own, d_cand, d_query); });
}

extern "C" int vis_batch_kfdb_match(vis_kfdb* db, const vis_loop_params* lp, int n, const vis_loop_cand* d_cand, int cand_stride, int max_pts,
                                    vis_dmatch* d_matches, float* d_p1, float* d_p2, int32_t* d_npts) {
    if (!match_args_ok(lp, n, d_cand, cand_stride, max_pts, d_matches, d_p1, d_p2, d_npts)) return VIS_E_INVALID;
    Plan* pl = nullptr;
    { const int rc = batch_state(db, n, true, "vis_batch_kfdb_match", &pl); if (rc) return rc; }
    return plan_follow_up(db->ctx, pl, [&] { return kf_match(db, lp, n, plan_query(pl, 1), d_cand, cand_stride, max_pts, d_matches, d_p1, d_p2, d_npts); });
}
