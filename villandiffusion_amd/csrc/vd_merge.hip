// Checkpoint merging (villandiffusion_amd/merge.py): task arithmetic (Ilharco et al. 2023) and TIES-Merging (Yadav et al. 2023) over whole flat
// weight buffers.  With tau_i = theta_i - theta_base the task vector of checkpoint i,
//   vd_merge_select  finds the k-th largest |tau_i[j]| EXACTLY, by radix selection over the float bits (non-negative floats order like their
//                    bits): FOUR PASSES OF 8 BITS, most significant byte first, each pass one read of w and base and a one-workgroup finish,
//                    a fixed launch sequence with no read-back in between.  It also gives n_gt (keys above the threshold), n_eq (keys equal
//                    to it) and the count of inf / NaN keys; INVARIANT for 1 <= k <= n:  n_gt < k <= n_gt + n_eq;
//   vd_merge_apply   trims every task vector at its threshold and forms the merged weights in ONE pass with no temporary, with the integer
//                    counts the read-outs come from (kept, won, support, conflict);
//   vd_merge_apply_drop  the same pass with a seeded random drop of every task vector (DARE, Yu et al. 2024) or, with VD_DROP_COPY, the
//                    mix of a fine-tune with its base (Fine-mixing, Zhang et al. 2022): Philox4x32-10 on (seed, stream, element index).
// HBM-bound, plain C++ with vector loads and stores.  No float atomics and no global atomics: the only atomics are LDS integer adds into
// histogram bins, and integer counts do not depend on order, so a repeat is bit-identical.  Compiled without FMA contraction: every difference,
// product, sum and the division is rounded to f32 on its own, so the elementwise part is the numpy float32 op sequence bit for bit.
//
// The kernels walk their n floats the way vd_curve_point does (vd_curve.hip): in ITEMS of four consecutive floats counted from the buffer's
// start, item q in thread q % (grid * 256) of the launch.  Where every data pointer of the call is 16-byte aligned a whole item is one f32x4
// access, otherwise (and for the last, partial item) four scalar ones: which thread owns an element does not depend on that choice.
//
// Two deliberate departures from the published TIES code:
//   * the k largest magnitudes are kept and ties at the threshold are ALL kept (|tau| >= threshold); the published code keeps k + 1;
//   * a sign sum of exactly zero elects +; the published code takes the majority sign of the whole vector there, a global reduction for a
//     measure-zero case.
#include "vd_common.h"
#include <math.h>

namespace {

constexpr int MRG_BLOCK = 256;      // threads of a workgroup
constexpr int MRG_FPT = 16;         // floats a thread is sized for (four items) before the grid is capped
constexpr int MRG_MAXGRID = 1024;   // workgroups at most                                             (vd_curve_plan's rule, restated)
constexpr int MRG_BINS = 256;       // 8 bits a pass
constexpr int MRG_ROW = MRG_BINS + 1;      // uint32 a workgroup writes per pass: the bins, then (pass 0) its count of non-finite keys
constexpr int MRG_COPIES = 8;       // LDS copies of the bins, by threadIdx.x % 8: trained weights crowd into a few exponents
constexpr int MRG_MAXK = 8;
constexpr int MRG_STATE_BYTES = 32;

// the head of ws, written by the finish kernel only
struct SelState {
    uint32_t prefix;        // the bytes of the threshold found so far, in the low bits
    uint32_t pad_;
    uint64_t k_rem;         // the rank still looked for among the keys that match the prefix
    uint64_t n_gt;          // keys known to lie above the threshold
    uint64_t n_nonfinite;
};
static_assert(sizeof(SelState) == MRG_STATE_BYTES, "ws layout");

inline int mrg_grid(int64_t n) {
    const int64_t per = (int64_t)MRG_BLOCK * MRG_FPT;
    const int64_t g = (n + per - 1) / per;
    return (int)(g < 1 ? 1 : (g > MRG_MAXGRID ? MRG_MAXGRID : g));
}
inline int64_t mrg_ws_bytes(int64_t n) { return MRG_STATE_BYTES + (int64_t)mrg_grid(n) * MRG_ROW * 4; }
inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

#define ITEM_STRIDE(q, n) \
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < (n); q += (int64_t)gridDim.x * blockDim.x)

__device__ __forceinline__ uint32_t key_of(float w, float b) { return __float_as_uint(w - b) & 0x7FFFFFFFu; }

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
    return v;
}
// red: >= 4 uint32 of LDS; the result is valid in every thread
__device__ __forceinline__ uint32_t block_sum_u32(uint32_t v, uint32_t* red) {
    v = wave_sum_u32(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// One pass: the keys whose bytes above `shift + 8` equal the prefix are counted by their byte at `shift`.  row[workgroup][0..255] gets the bins,
// row[workgroup][256] the workgroup's count of keys >= 0x7F800000 (FIRST pass only; otherwise 0).
template <bool VEC, bool FIRST>
__global__ __launch_bounds__(256) void merge_hist_kernel(const float* w, const float* base, int64_t n, int shift, const SelState* __restrict__ st,
                                                         uint32_t* __restrict__ rows) {
    __shared__ uint32_t bins[MRG_COPIES][MRG_BINS];
    __shared__ uint32_t red[4];
    for (int i = threadIdx.x; i < MRG_COPIES * MRG_BINS; i += MRG_BLOCK) (&bins[0][0])[i] = 0u;
    const uint32_t prefix = FIRST ? 0u : st->prefix;
    __syncthreads();
    uint32_t* mine = bins[threadIdx.x & (MRG_COPIES - 1)];
    uint32_t nonfinite = 0u;
    ITEM_STRIDE(q, (n + 3) >> 2) {
        const int64_t k0 = q << 2;
        uint32_t key[4];
        int cnt = 4;
        if (VEC && k0 + 4 <= n) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(w + k0);
            const f32x4 b = *reinterpret_cast<const f32x4*>(base + k0);
#pragma unroll
            for (int e = 0; e < 4; ++e) key[e] = key_of(a[e], b[e]);
        } else {
            cnt = (int)(n - k0 < 4 ? n - k0 : 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) key[e] = e < cnt ? key_of(w[k0 + e], base[k0 + e]) : 0u;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < cnt) {
                if (FIRST) {
                    nonfinite += key[e] >= 0x7F800000u ? 1u : 0u;
                    atomicAdd(&mine[key[e] >> 24], 1u);
                } else if ((key[e] >> (shift + 8)) == prefix) {
                    atomicAdd(&mine[(key[e] >> shift) & 255u], 1u);
                }
            }
    }
    __syncthreads();
    uint32_t* row = rows + (size_t)blockIdx.x * MRG_ROW;
    {
        uint32_t s = 0u;
#pragma unroll
        for (int c = 0; c < MRG_COPIES; ++c) s += bins[c][threadIdx.x];
        row[threadIdx.x] = s;
    }
    const uint32_t nf = block_sum_u32(nonfinite, red);
    if (threadIdx.x == 0) row[MRG_BINS] = nf;
}

// One workgroup of 1024 threads.  Thread (r, b) adds bin b of the rows r, r + 4, ... in 64 bits (four row walks side by side, the loads of each
// unrolled: the walk is latency-bound), the four are added per bin, and thread 0 walks the bins from the top until the remaining rank is met
// and moves the prefix, the rank and n_gt on.  FIRST starts the state from k; LAST writes the outputs.  k = 0: the threshold is +inf and
// nothing lies at or above it by definition (n_gt = n_eq = 0); only the first pass is launched then.
constexpr int MRG_FIN = 1024;
__global__ __launch_bounds__(1024) void merge_select_finish_kernel(const uint32_t* __restrict__ rows, int n_rows, int64_t k, int first, int last,
                                                                   SelState* __restrict__ st, float* __restrict__ thr_out,
                                                                   int64_t* __restrict__ rec) {
    __shared__ uint64_t part[MRG_FIN / MRG_BINS][MRG_BINS];
    __shared__ uint64_t nfp[MRG_FIN];
    __shared__ uint64_t tot[MRG_BINS];
    __shared__ uint64_t nf[MRG_BINS];
    const int b = threadIdx.x & (MRG_BINS - 1), r = threadIdx.x / MRG_BINS;
    uint64_t s = 0, f = 0;
#pragma unroll 8
    for (int g = r; g < n_rows; g += MRG_FIN / MRG_BINS) s += rows[(size_t)g * MRG_ROW + b];
    if (first)
        for (int g = threadIdx.x; g < n_rows; g += MRG_FIN) f += rows[(size_t)g * MRG_ROW + MRG_BINS];
    part[r][b] = s;
    nfp[threadIdx.x] = f;
    __syncthreads();
    if (threadIdx.x < MRG_BINS) {
        tot[b] = (part[0][b] + part[1][b]) + (part[2][b] + part[3][b]);
        nf[b] = (nfp[b] + nfp[b + 256]) + (nfp[b + 512] + nfp[b + 768]);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    SelState cur;
    if (first) {
        cur.prefix = 0u;
        cur.pad_ = 0u;
        cur.k_rem = (uint64_t)k;
        cur.n_gt = 0;
        uint64_t t = 0;
        for (int i = 0; i < MRG_BINS; ++i) t += nf[i];
        cur.n_nonfinite = t;
    } else {
        cur = *st;
    }
    uint64_t n_eq = 0;
    if (k > 0) {
        uint64_t above = 0;
        int digit = 0;
        for (int b = MRG_BINS - 1; b >= 0; --b) {
            if (above + tot[b] >= cur.k_rem) {
                digit = b;
                break;
            }
            above += tot[b];
        }
        cur.prefix = (cur.prefix << 8) | (uint32_t)digit;
        cur.k_rem -= above;
        cur.n_gt += above;
        n_eq = tot[digit];
    }
    *st = cur;
    if (last) {
        thr_out[0] = k > 0 ? __uint_as_float(cur.prefix) : INFINITY;
        rec[0] = k > 0 ? (int64_t)cur.n_gt : 0;
        rec[1] = k > 0 ? (int64_t)n_eq : 0;
        rec[2] = (int64_t)cur.n_nonfinite;
    }
}

__global__ void merge_select_empty_kernel(float* __restrict__ thr_out, int64_t* __restrict__ rec) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        thr_out[0] = INFINITY;
        rec[0] = rec[1] = rec[2] = 0;
    }
}

struct ApplyArgs {
    const float* task[MRG_MAXK];
    float lam[MRG_MAXK];
};

// counters of a thread: kept[0..K), won[0..K), support, conflict
template <int K>
struct Counts {
    uint32_t kept[K], won[K], support, conflict;
};

// One element: d[i] = the task's value minus the base, thr[i] the thresholds.  Returns the merged weight.
template <int MODE, int K>
__device__ __forceinline__ float merge_one(float b, const float (&tv)[K], const float (&thr)[K], const float (&lam)[K], float lam_out,
                                           Counts<K>& c) {
    float t[K];
    bool pos_any = false, neg_any = false, any = false;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const float d = tv[i] - b;
        const bool keep = fabsf(d) >= thr[i];
        t[i] = keep ? d : 0.0f;
        c.kept[i] += keep ? 1u : 0u;
        any |= t[i] != 0.0f;
        pos_any |= t[i] > 0.0f;
        neg_any |= t[i] < 0.0f;
    }
    c.support += any ? 1u : 0u;
    c.conflict += (pos_any && neg_any) ? 1u : 0u;
    if (MODE == VD_MERGE_LINEAR) {
        float acc = 0.0f;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            acc = acc + lam[i] * t[i];
            c.won[i] += t[i] != 0.0f ? 1u : 0u;
        }
        return b + acc;
    }
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < K; ++i) s = s + t[i];
    const bool plus = s >= 0.0f;
    float m = 0.0f;
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const bool in = t[i] != 0.0f && ((t[i] > 0.0f) == plus);
        if (in) {
            m = m + t[i];
            ++cnt;
        }
        c.won[i] += in ? 1u : 0u;
    }
    const float tau = cnt ? __fdiv_rn(m, (float)cnt) : 0.0f;
    return b + lam_out * tau;
}

// out may be base or one of the tasks (the same pointer): a thread reads every input of an item before it writes the item.  No __restrict__
// among out and the inputs.  partial[c * 1024 + workgroup] holds counter c of the workgroup.
template <bool VEC, int MODE, int K>
__global__ __launch_bounds__(256) void merge_apply_kernel(float* out, const float* base, ApplyArgs a, const float* __restrict__ thr_dev,
                                                          int64_t n, float lam_out, uint32_t* __restrict__ partial) {
    __shared__ uint32_t red[4];
    Counts<K> c;
    float thr[K], lam[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        c.kept[i] = c.won[i] = 0u;
        thr[i] = thr_dev[i];
        lam[i] = a.lam[i];
    }
    c.support = c.conflict = 0u;
    ITEM_STRIDE(q, (n + 3) >> 2) {
        const int64_t k0 = q << 2;
        if (VEC && k0 + 4 <= n) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(base + k0);
            f32x4 tk[K];
#pragma unroll
            for (int i = 0; i < K; ++i) tk[i] = *reinterpret_cast<const f32x4*>(a.task[i] + k0);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float tv[K];
#pragma unroll
                for (int i = 0; i < K; ++i) tv[i] = tk[i][e];
                o[e] = merge_one<MODE, K>(b[e], tv, thr, lam, lam_out, c);
            }
            *reinterpret_cast<f32x4*>(out + k0) = o;
        } else {
            for (int e = 0; e < 4 && k0 + e < n; ++e) {
                const float b = base[k0 + e];
                float tv[K];
#pragma unroll
                for (int i = 0; i < K; ++i) tv[i] = a.task[i][k0 + e];
                out[k0 + e] = merge_one<MODE, K>(b, tv, thr, lam, lam_out, c);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const uint32_t v = block_sum_u32(c.kept[i], red);
        if (threadIdx.x == 0) partial[i * MRG_MAXGRID + blockIdx.x] = v;
    }
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const uint32_t v = block_sum_u32(c.won[i], red);
        if (threadIdx.x == 0) partial[(K + i) * MRG_MAXGRID + blockIdx.x] = v;
    }
    const uint32_t sup = block_sum_u32(c.support, red);
    const uint32_t con = block_sum_u32(c.conflict, red);
    if (threadIdx.x == 0) {
        partial[(2 * K) * MRG_MAXGRID + blockIdx.x] = sup;
        partial[(2 * K + 1) * MRG_MAXGRID + blockIdx.x] = con;
    }
}

// One workgroup: per counter, thread t adds partial[t], partial[t + 256], ... in 64 bits, then thread 0 adds the 256 sums.
__global__ __launch_bounds__(256) void merge_apply_finish_kernel(const uint32_t* __restrict__ partial, int n_partial, int n_counters,
                                                                 int64_t* __restrict__ stats) {
    __shared__ uint64_t acc[MRG_BLOCK];
    for (int c = 0; c < n_counters; ++c) {
        uint64_t v = 0;
        for (int k = threadIdx.x; k < n_partial; k += MRG_BLOCK) v += partial[c * MRG_MAXGRID + k];
        __syncthreads();
        acc[threadIdx.x] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t t = 0;
            for (int i = 0; i < MRG_BLOCK; ++i) t += acc[i];
            stats[c] = (int64_t)t;
        }
    }
}

// ---- the seeded drop (DARE, Fine-mixing): vd_merge_apply_drop -------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., Random123), restated from vd_elem.hip so that nothing of the training path is built differently; both are
// pinned to tests/elem_ref.py's integer restatement.
__device__ __forceinline__ void mrg_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                                  uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

constexpr uint64_t MRG_DROP_ALL = (uint64_t)1 << 32;      // drop_thr: 0 keeps every entry, 2^32 none

// The keep bits of item q for one task: bit e = ((uint64)r[e] >= T), r the Philox words of counter (lo32(q), hi32(q), stream, 1).  T = 0 and
// T = 2^32 need no draw (the branch is uniform: T is a kernel argument).
__device__ __forceinline__ uint32_t drop_keep_bits(int64_t q, uint32_t stream_id, uint64_t T, uint32_t k0, uint32_t k1) {
    if (T == 0) return 15u;
    if (T >= MRG_DROP_ALL) return 0u;
    uint32_t r[4];
    mrg_philox4x32_10((uint32_t)(uint64_t)q, (uint32_t)((uint64_t)q >> 32), stream_id, 1u, k0, k1, r);
    const uint32_t t = (uint32_t)T;
    return (r[0] >= t ? 1u : 0u) | (r[1] >= t ? 2u : 0u) | (r[2] >= t ? 4u : 0u) | (r[3] >= t ? 8u : 0u);
}

struct DropArgs {
    const float* task[MRG_MAXK];
    uint64_t drop_thr[MRG_MAXK];
    float lam[MRG_MAXK];
    float rescale[MRG_MAXK];      // 1.0f without VD_DROP_RESCALE: d * 1.0f is d, bit for bit
    uint32_t stream[MRG_MAXK];
};

// counters of a thread: drawn[0..K), kept[0..K), won[0..K), support, conflict
template <int K>
struct DropCounts {
    uint32_t drawn[K], kept[K], won[K], support, conflict;
};

// merge_one with the keep bit of every task (bit i of `kb`) and the rescale: t_i = (|d_i| >= thr_i && keep_i) ? d_i * rescale_i : +0.0f, the
// rest word for word.
template <int MODE, int K>
__device__ __forceinline__ float merge_one_drop(float b, const float (&tv)[K], uint32_t kb, const float (&thr)[K], const float (&lam)[K],
                                                const float (&rs)[K], float lam_out, DropCounts<K>& c) {
    float t[K];
    bool pos_any = false, neg_any = false, any = false;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const float d = tv[i] - b;
        const bool keep = fabsf(d) >= thr[i] && ((kb >> i) & 1u);
        t[i] = keep ? d * rs[i] : 0.0f;
        c.kept[i] += keep ? 1u : 0u;
        any |= t[i] != 0.0f;
        pos_any |= t[i] > 0.0f;
        neg_any |= t[i] < 0.0f;
    }
    c.support += any ? 1u : 0u;
    c.conflict += (pos_any && neg_any) ? 1u : 0u;
    if (MODE == VD_MERGE_LINEAR) {
        float acc = 0.0f;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            acc = acc + lam[i] * t[i];
            c.won[i] += t[i] != 0.0f ? 1u : 0u;
        }
        return b + acc;
    }
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < K; ++i) s = s + t[i];
    const bool plus = s >= 0.0f;
    float m = 0.0f;
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const bool in = t[i] != 0.0f && ((t[i] > 0.0f) == plus);
        if (in) {
            m = m + t[i];
            ++cnt;
        }
        c.won[i] += in ? 1u : 0u;
    }
    const float tau = cnt ? __fdiv_rn(m, (float)cnt) : 0.0f;
    return b + lam_out * tau;
}

// merge_apply_kernel's walk, with one Philox call per task and item.  partial[c * 1024 + workgroup] holds counter c of the workgroup.
template <bool VEC, int MODE, int K>
__global__ __launch_bounds__(256) void merge_apply_drop_kernel(float* out, const float* base, DropArgs a, const float* __restrict__ thr_dev,
                                                               int64_t n, float lam_out, uint32_t key0, uint32_t key1,
                                                               uint32_t* __restrict__ partial) {
    __shared__ uint32_t red[4];
    DropCounts<K> c;
    float thr[K], lam[K], rs[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        c.drawn[i] = c.kept[i] = c.won[i] = 0u;
        thr[i] = thr_dev[i];
        lam[i] = a.lam[i];
        rs[i] = a.rescale[i];
    }
    c.support = c.conflict = 0u;
    ITEM_STRIDE(q, (n + 3) >> 2) {
        const int64_t k0 = q << 2;
        const int cnt = (int)(n - k0 < 4 ? n - k0 : 4);
        uint32_t kb[4] = {0u, 0u, 0u, 0u};      // per element: bit i = task i keeps it
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const uint32_t m = drop_keep_bits(q, a.stream[i], a.drop_thr[i], key0, key1) & ((1u << cnt) - 1u);
            c.drawn[i] += (uint32_t)__popc(m);
#pragma unroll
            for (int e = 0; e < 4; ++e) kb[e] |= ((m >> e) & 1u) << i;
        }
        if (VEC && cnt == 4) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(base + k0);
            f32x4 tk[K];
#pragma unroll
            for (int i = 0; i < K; ++i) tk[i] = *reinterpret_cast<const f32x4*>(a.task[i] + k0);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float tv[K];
#pragma unroll
                for (int i = 0; i < K; ++i) tv[i] = tk[i][e];
                o[e] = merge_one_drop<MODE, K>(b[e], tv, kb[e], thr, lam, rs, lam_out, c);
            }
            *reinterpret_cast<f32x4*>(out + k0) = o;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e >= cnt) break;
                const float b = base[k0 + e];
                float tv[K];
#pragma unroll
                for (int i = 0; i < K; ++i) tv[i] = a.task[i][k0 + e];
                out[k0 + e] = merge_one_drop<MODE, K>(b, tv, kb[e], thr, lam, rs, lam_out, c);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const uint32_t v = block_sum_u32(c.drawn[i], red);
        if (threadIdx.x == 0) partial[i * MRG_MAXGRID + blockIdx.x] = v;
    }
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const uint32_t v = block_sum_u32(c.kept[i], red);
        if (threadIdx.x == 0) partial[(K + i) * MRG_MAXGRID + blockIdx.x] = v;
    }
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const uint32_t v = block_sum_u32(c.won[i], red);
        if (threadIdx.x == 0) partial[(2 * K + i) * MRG_MAXGRID + blockIdx.x] = v;
    }
    const uint32_t sup = block_sum_u32(c.support, red);
    const uint32_t con = block_sum_u32(c.conflict, red);
    if (threadIdx.x == 0) {
        partial[(3 * K) * MRG_MAXGRID + blockIdx.x] = sup;
        partial[(3 * K + 1) * MRG_MAXGRID + blockIdx.x] = con;
    }
}

// VD_DROP_COPY (Fine-mixing): out[j] = keep ? task[j] : base[j], the bits moved as integers.  Counters: drawn, kept = drawn, won = drawn,
// support = #(keep and task[j] != base[j] as floats), conflict = 0.
template <bool VEC>
__global__ __launch_bounds__(256) void merge_mix_kernel(float* out, const float* base, const float* task, int64_t n, uint32_t stream_id,
                                                        uint64_t T, uint32_t key0, uint32_t key1, uint32_t* __restrict__ partial) {
    __shared__ uint32_t red[4];
    uint32_t drawn = 0u, differ = 0u;
    ITEM_STRIDE(q, (n + 3) >> 2) {
        const int64_t k0 = q << 2;
        const int cnt = (int)(n - k0 < 4 ? n - k0 : 4);
        const uint32_t m = drop_keep_bits(q, stream_id, T, key0, key1) & ((1u << cnt) - 1u);
        drawn += (uint32_t)__popc(m);
        if (VEC && cnt == 4) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(base + k0);
            const f32x4 w = *reinterpret_cast<const f32x4*>(task + k0);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool keep = (m >> e) & 1u;
                differ += (keep && w[e] != b[e]) ? 1u : 0u;
                o[e] = __uint_as_float(keep ? __float_as_uint(w[e]) : __float_as_uint(b[e]));
            }
            *reinterpret_cast<f32x4*>(out + k0) = o;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e >= cnt) break;
                const float b = base[k0 + e], w = task[k0 + e];
                const bool keep = (m >> e) & 1u;
                differ += (keep && w != b) ? 1u : 0u;
                out[k0 + e] = __uint_as_float(keep ? __float_as_uint(w) : __float_as_uint(b));
            }
        }
    }
    const uint32_t dr = block_sum_u32(drawn, red);
    const uint32_t df = block_sum_u32(differ, red);
    if (threadIdx.x == 0) {
        partial[0 * MRG_MAXGRID + blockIdx.x] = dr;
        partial[1 * MRG_MAXGRID + blockIdx.x] = dr;
        partial[2 * MRG_MAXGRID + blockIdx.x] = dr;
        partial[3 * MRG_MAXGRID + blockIdx.x] = df;
        partial[4 * MRG_MAXGRID + blockIdx.x] = 0u;
    }
}

inline bool finite_f(float v) { return v > -INFINITY && v < INFINITY; }      // NaN fails
inline bool disjoint_b(const void* a, int64_t na, const void* b, int64_t nb) {      // [a, a + na bytes) and [b, b + nb bytes)
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y ? y - x >= (uintptr_t)na : x - y >= (uintptr_t)nb;
}

template <bool VEC, int MODE>
void launch_apply(int K, int grid, hipStream_t st, float* out, const float* base, const ApplyArgs& a, const float* thr, int64_t n, float lam_out,
                  uint32_t* partial) {
#define MRG_CASE(KK)                                                                                                                  \
    case KK:                                                                                                                          \
        hipLaunchKernelGGL((merge_apply_kernel<VEC, MODE, KK>), dim3(grid), dim3(MRG_BLOCK), 0, st, out, base, a, thr, n, lam_out, partial); \
        break;
    switch (K) {
        MRG_CASE(1) MRG_CASE(2) MRG_CASE(3) MRG_CASE(4) MRG_CASE(5) MRG_CASE(6) MRG_CASE(7) MRG_CASE(8)
    }
#undef MRG_CASE
}

template <bool VEC, int MODE>
void launch_apply_drop(int K, int grid, hipStream_t st, float* out, const float* base, const DropArgs& a, const float* thr, int64_t n,
                       float lam_out, uint32_t key0, uint32_t key1, uint32_t* partial) {
#define MRG_CASE(KK)                                                                                                                       \
    case KK:                                                                                                                               \
        hipLaunchKernelGGL((merge_apply_drop_kernel<VEC, MODE, KK>), dim3(grid), dim3(MRG_BLOCK), 0, st, out, base, a, thr, n, lam_out, key0, \
                           key1, partial);                                                                                                 \
        break;
    switch (K) {
        MRG_CASE(1) MRG_CASE(2) MRG_CASE(3) MRG_CASE(4) MRG_CASE(5) MRG_CASE(6) MRG_CASE(7) MRG_CASE(8)
    }
#undef MRG_CASE
}

}  // namespace

#define ST ((hipStream_t)stream)
#define MRG_N_OK(who) \
    VD_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), who ": n = %lld lies outside [0, 2^31) (the per-workgroup counts are 32-bit)", (long long)n)

extern "C" int vd_merge_plan(int64_t n, int* grid, int* block, int* floats_per_thread, int64_t* ws_bytes) {
    VD_REQUIRE(grid && block && floats_per_thread && ws_bytes, "vd_merge_plan: null pointer");
    MRG_N_OK("vd_merge_plan");
    *grid = mrg_grid(n);
    *block = MRG_BLOCK;
    *floats_per_thread = MRG_FPT;
    *ws_bytes = mrg_ws_bytes(n);
    return 0;
}

extern "C" int vd_merge_select(const float* w, const float* base, int64_t n, int64_t k, void* ws, float* thr_out, int64_t* rec, void* stream) {
    MRG_N_OK("vd_merge_select");
    VD_REQUIRE(k >= 0 && k <= n, "vd_merge_select: k = %lld lies outside [0, n = %lld]", (long long)k, (long long)n);
    VD_REQUIRE(w && base && ws && thr_out && rec, "vd_merge_select: null pointer");
    VD_REQUIRE(((((uintptr_t)w) | ((uintptr_t)base) | ((uintptr_t)thr_out)) & 3) == 0 && ((((uintptr_t)ws) | ((uintptr_t)rec)) & 7) == 0,
               "vd_merge_select: w, base and thr_out must be 4-byte aligned, ws and rec 8-byte aligned");
    const int64_t wsb = mrg_ws_bytes(n);
    const void* in[2] = {w, base};
    for (int i = 0; i < 2; ++i)
        VD_REQUIRE(disjoint_b(in[i], n * 4, ws, wsb) && disjoint_b(in[i], n * 4, thr_out, 4) && disjoint_b(in[i], n * 4, rec, 24),
                   "vd_merge_select: ws, thr_out or rec overlaps an input");
    VD_REQUIRE(disjoint_b(ws, wsb, thr_out, 4) && disjoint_b(ws, wsb, rec, 24) && disjoint_b(thr_out, 4, rec, 24),
               "vd_merge_select: ws, thr_out and rec overlap each other");
    if (n == 0) {
        hipLaunchKernelGGL(merge_select_empty_kernel, dim3(1), dim3(64), 0, ST, thr_out, rec);
        VD_LAUNCH_CHECK("vd_merge_select");
        return 0;
    }
    const int grid = mrg_grid(n);
    SelState* st = reinterpret_cast<SelState*>(ws);
    uint32_t* rows = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(ws) + MRG_STATE_BYTES);
    const bool vec = aligned16(w) && aligned16(base);
    const int passes = k == 0 ? 1 : 4;
    for (int p = 0; p < passes; ++p) {
        const int shift = 24 - 8 * p;
        if (p == 0) {
            if (vec) hipLaunchKernelGGL((merge_hist_kernel<true, true>), dim3(grid), dim3(MRG_BLOCK), 0, ST, w, base, n, shift, st, rows);
            else hipLaunchKernelGGL((merge_hist_kernel<false, true>), dim3(grid), dim3(MRG_BLOCK), 0, ST, w, base, n, shift, st, rows);
        } else {
            if (vec) hipLaunchKernelGGL((merge_hist_kernel<true, false>), dim3(grid), dim3(MRG_BLOCK), 0, ST, w, base, n, shift, st, rows);
            else hipLaunchKernelGGL((merge_hist_kernel<false, false>), dim3(grid), dim3(MRG_BLOCK), 0, ST, w, base, n, shift, st, rows);
        }
        hipLaunchKernelGGL(merge_select_finish_kernel, dim3(1), dim3(MRG_FIN), 0, ST, rows, grid, k, p == 0 ? 1 : 0, p == passes - 1 ? 1 : 0, st,
                           thr_out, rec);
    }
    VD_LAUNCH_CHECK("vd_merge_select");
    return 0;
}

extern "C" int vd_merge_apply(float* out, const float* base, const float* const* tasks, const float* lam, const float* thr, int K, int64_t n,
                              int mode, float lam_out, uint32_t* partial, int64_t* stats, void* stream) {
    MRG_N_OK("vd_merge_apply");
    VD_REQUIRE(K >= 1 && K <= MRG_MAXK, "vd_merge_apply: K = %d lies outside [1, %d]", K, MRG_MAXK);
    VD_REQUIRE(mode == VD_MERGE_LINEAR || mode == VD_MERGE_TIES, "vd_merge_apply: unknown mode %d", mode);
    VD_REQUIRE(out && base && tasks && thr && partial && stats, "vd_merge_apply: null pointer");
    VD_REQUIRE(mode == VD_MERGE_TIES || lam, "vd_merge_apply: VD_MERGE_LINEAR needs lam");
    VD_REQUIRE(finite_f(lam_out), "vd_merge_apply: lam_out must be finite, got %g", (double)lam_out);
    VD_REQUIRE(((((uintptr_t)out) | ((uintptr_t)base) | ((uintptr_t)thr) | ((uintptr_t)partial)) & 3) == 0 && (((uintptr_t)stats) & 7) == 0,
               "vd_merge_apply: out, base, thr and partial must be 4-byte aligned, stats 8-byte aligned");
    ApplyArgs a;
    const int64_t nb = n * 4, pb = (int64_t)(2 * K + 2) * MRG_MAXGRID * 4, sb = (int64_t)(2 * K + 2) * 8;
    bool vec = aligned16(out) && aligned16(base);
    for (int i = 0; i < MRG_MAXK; ++i) {
        a.task[i] = i < K ? tasks[i] : nullptr;
        a.lam[i] = (i < K && mode == VD_MERGE_LINEAR) ? lam[i] : 0.0f;
        if (i >= K) continue;
        VD_REQUIRE(a.task[i], "vd_merge_apply: tasks[%d] is null", i);
        VD_REQUIRE((((uintptr_t)a.task[i]) & 3) == 0, "vd_merge_apply: tasks[%d] is not 4-byte aligned", i);
        VD_REQUIRE(finite_f(a.lam[i]), "vd_merge_apply: lam[%d] must be finite, got %g", i, (double)a.lam[i]);
        VD_REQUIRE((const void*)out == (const void*)a.task[i] || disjoint_b(out, nb, a.task[i], nb),
                   "vd_merge_apply: out overlaps tasks[%d] without being it", i);
        VD_REQUIRE(disjoint_b(a.task[i], nb, partial, pb) && disjoint_b(a.task[i], nb, stats, sb), "vd_merge_apply: tasks[%d] overlaps partial or stats", i);
        vec = vec && aligned16(a.task[i]);
    }
    VD_REQUIRE((const void*)out == (const void*)base || disjoint_b(out, nb, base, nb), "vd_merge_apply: out overlaps base without being it");
    VD_REQUIRE(disjoint_b(out, nb, thr, K * 4) && disjoint_b(out, nb, partial, pb) && disjoint_b(out, nb, stats, sb),
               "vd_merge_apply: out overlaps thr, partial or stats");
    VD_REQUIRE(disjoint_b(base, nb, partial, pb) && disjoint_b(base, nb, stats, sb) && disjoint_b(thr, K * 4, partial, pb) &&
                   disjoint_b(thr, K * 4, stats, sb) && disjoint_b(partial, pb, stats, sb),
               "vd_merge_apply: partial or stats overlaps an input or each other");
    int grid = 0;
    if (n > 0) {
        grid = mrg_grid(n);
        if (mode == VD_MERGE_LINEAR) {
            if (vec) launch_apply<true, VD_MERGE_LINEAR>(K, grid, ST, out, base, a, thr, n, lam_out, partial);
            else launch_apply<false, VD_MERGE_LINEAR>(K, grid, ST, out, base, a, thr, n, lam_out, partial);
        } else {
            if (vec) launch_apply<true, VD_MERGE_TIES>(K, grid, ST, out, base, a, thr, n, lam_out, partial);
            else launch_apply<false, VD_MERGE_TIES>(K, grid, ST, out, base, a, thr, n, lam_out, partial);
        }
    }
    hipLaunchKernelGGL(merge_apply_finish_kernel, dim3(1), dim3(MRG_BLOCK), 0, ST, partial, grid, 2 * K + 2, stats);      // (n = 0: all zero)
    VD_LAUNCH_CHECK("vd_merge_apply");
    return 0;
}

extern "C" int vd_merge_apply_drop(float* out, const float* base, const float* const* tasks, const float* lam, const float* thr,
                                   const uint64_t* drop_thr, const float* rescale, const uint32_t* streams, int K, int64_t n, int mode,
                                   float lam_out, uint64_t seed, int flags, uint32_t* partial, int64_t* stats, void* stream) {
    MRG_N_OK("vd_merge_apply_drop");
    VD_REQUIRE(K >= 1 && K <= MRG_MAXK, "vd_merge_apply_drop: K = %d lies outside [1, %d]", K, MRG_MAXK);
    VD_REQUIRE(mode == VD_MERGE_LINEAR || mode == VD_MERGE_TIES, "vd_merge_apply_drop: unknown mode %d", mode);
    VD_REQUIRE((flags & ~(VD_DROP_RESCALE | VD_DROP_COPY)) == 0, "vd_merge_apply_drop: unknown flag bits in %d", flags);
    const bool copy = (flags & VD_DROP_COPY) != 0, resc = (flags & VD_DROP_RESCALE) != 0;
    VD_REQUIRE(!(copy && resc), "vd_merge_apply_drop: VD_DROP_COPY moves bits and takes no VD_DROP_RESCALE");
    VD_REQUIRE(!copy || (K == 1 && mode == VD_MERGE_LINEAR), "vd_merge_apply_drop: VD_DROP_COPY takes K = 1 and VD_MERGE_LINEAR, got K = %d, mode %d",
               K, mode);
    VD_REQUIRE(out && base && tasks && partial && stats && (copy || thr), "vd_merge_apply_drop: null pointer");
    VD_REQUIRE(drop_thr && streams, "vd_merge_apply_drop: drop_thr or streams is null");
    VD_REQUIRE(!resc || rescale, "vd_merge_apply_drop: VD_DROP_RESCALE needs rescale");
    VD_REQUIRE(copy || mode == VD_MERGE_TIES || lam, "vd_merge_apply_drop: VD_MERGE_LINEAR needs lam");
    VD_REQUIRE(copy || finite_f(lam_out), "vd_merge_apply_drop: lam_out must be finite, got %g", (double)lam_out);
    VD_REQUIRE(((((uintptr_t)out) | ((uintptr_t)base) | ((uintptr_t)partial)) & 3) == 0 && (copy || (((uintptr_t)thr) & 3) == 0) &&
                   (((uintptr_t)stats) & 7) == 0,
               "vd_merge_apply_drop: out, base, thr and partial must be 4-byte aligned, stats 8-byte aligned");
    DropArgs a;
    const int nc = 3 * K + 2;
    const int64_t nb = n * 4, pb = (int64_t)nc * MRG_MAXGRID * 4, sb = (int64_t)nc * 8;
    bool vec = aligned16(out) && aligned16(base);
    for (int i = 0; i < MRG_MAXK; ++i) {
        a.task[i] = i < K ? tasks[i] : nullptr;
        a.lam[i] = (i < K && !copy && mode == VD_MERGE_LINEAR) ? lam[i] : 0.0f;
        a.rescale[i] = (i < K && resc) ? rescale[i] : 1.0f;
        a.drop_thr[i] = i < K ? drop_thr[i] : 0;
        a.stream[i] = i < K ? streams[i] : 0u;
        if (i >= K) continue;
        VD_REQUIRE(a.task[i], "vd_merge_apply_drop: tasks[%d] is null", i);
        VD_REQUIRE((((uintptr_t)a.task[i]) & 3) == 0, "vd_merge_apply_drop: tasks[%d] is not 4-byte aligned", i);
        VD_REQUIRE(finite_f(a.lam[i]), "vd_merge_apply_drop: lam[%d] must be finite, got %g", i, (double)a.lam[i]);
        VD_REQUIRE(a.drop_thr[i] <= MRG_DROP_ALL, "vd_merge_apply_drop: drop_thr[%d] = %llu lies above 2^32", i, (unsigned long long)a.drop_thr[i]);
        VD_REQUIRE(finite_f(a.rescale[i]), "vd_merge_apply_drop: rescale[%d] must be finite, got %g", i, (double)a.rescale[i]);
        VD_REQUIRE((const void*)out == (const void*)a.task[i] || disjoint_b(out, nb, a.task[i], nb),
                   "vd_merge_apply_drop: out overlaps tasks[%d] without being it", i);
        VD_REQUIRE(disjoint_b(a.task[i], nb, partial, pb) && disjoint_b(a.task[i], nb, stats, sb),
                   "vd_merge_apply_drop: tasks[%d] overlaps partial or stats", i);
        vec = vec && aligned16(a.task[i]);
    }
    VD_REQUIRE((const void*)out == (const void*)base || disjoint_b(out, nb, base, nb), "vd_merge_apply_drop: out overlaps base without being it");
    VD_REQUIRE(disjoint_b(out, nb, partial, pb) && disjoint_b(out, nb, stats, sb) && (copy || disjoint_b(out, nb, thr, K * 4)),
               "vd_merge_apply_drop: out overlaps thr, partial or stats");
    VD_REQUIRE(disjoint_b(base, nb, partial, pb) && disjoint_b(base, nb, stats, sb) && disjoint_b(partial, pb, stats, sb) &&
                   (copy || (disjoint_b(thr, K * 4, partial, pb) && disjoint_b(thr, K * 4, stats, sb))),
               "vd_merge_apply_drop: partial or stats overlaps an input or each other");
    const uint32_t key0 = (uint32_t)seed, key1 = (uint32_t)(seed >> 32);
    int grid = 0;
    if (n > 0) {
        grid = mrg_grid(n);
        if (copy) {
            if (vec) hipLaunchKernelGGL((merge_mix_kernel<true>), dim3(grid), dim3(MRG_BLOCK), 0, ST, out, base, a.task[0], n, a.stream[0],
                                        a.drop_thr[0], key0, key1, partial);
            else hipLaunchKernelGGL((merge_mix_kernel<false>), dim3(grid), dim3(MRG_BLOCK), 0, ST, out, base, a.task[0], n, a.stream[0],
                                    a.drop_thr[0], key0, key1, partial);
        } else if (mode == VD_MERGE_LINEAR) {
            if (vec) launch_apply_drop<true, VD_MERGE_LINEAR>(K, grid, ST, out, base, a, thr, n, lam_out, key0, key1, partial);
            else launch_apply_drop<false, VD_MERGE_LINEAR>(K, grid, ST, out, base, a, thr, n, lam_out, key0, key1, partial);
        } else {
            if (vec) launch_apply_drop<true, VD_MERGE_TIES>(K, grid, ST, out, base, a, thr, n, lam_out, key0, key1, partial);
            else launch_apply_drop<false, VD_MERGE_TIES>(K, grid, ST, out, base, a, thr, n, lam_out, key0, key1, partial);
        }
    }
    hipLaunchKernelGGL(merge_apply_finish_kernel, dim3(1), dim3(MRG_BLOCK), 0, ST, partial, grid, nc, stats);      // (n = 0: all zero)
    VD_LAUNCH_CHECK("vd_merge_apply_drop");
    return 0;
}
