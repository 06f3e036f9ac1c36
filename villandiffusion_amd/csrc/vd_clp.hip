// Channel Lipschitzness-based Pruning (villandiffusion_amd/clp.py): the largest singular value of every weight row of a network, the row seen
// as a [Cin, T] matrix, in one table-driven launch that reads every weight once.  Plain C++ with 16-byte loads where the data allow, no
// atomics, every product and sum rounded on its own (compiled without FMA contraction), every sum in a fixed order: a repeat is bit-identical.
//
// Layout: the neuron-table convention -- one 64-lane wave per row, four rows per 256-thread workgroup, a job owns ceil(rows / 4) workgroups.
//
// Stage 1, the Gram matrix G = W^T W (T x T; the T (T + 1) / 2 entries (i, j) with i <= j, entry e = i * 9 - i * (i - 1) / 2 + (j - i), the
// upper triangle row by row).  A row is walked in pieces of 576 contiguous floats (2304 bytes: 64 channels of nine taps, or 9 x 64 channels
// of one tap); a wave copies its piece into its own 576 floats of LDS -- f32x4 loads where the job starts 16-byte aligned and Cin * T is a
// multiple of 4, scalar loads otherwise, consecutive lanes on consecutive addresses either way -- and reads its channels back from there.
// Lane l owns the input channels l, l + 64, ... and adds them in ascending order, one f32 partial per Gram entry starting from +0:
// p_e = p_e + w[c][i] * w[c][j].  The 64 lanes are added by the xor tree of wave_sum (offsets 32, 16, ..., 1).  Which lane owns a channel and
// the order it is added in do not depend on the load width.  The longest chain of additions of an entry is ceil(Cin / 64) + 6.
//
// Stage 2, lambda_max(G) for T = 9 (T = 1: lambda_max = G_00, no arithmetic).  G is scaled by the power of two that brings its largest
// diagonal entry into [1, 2) (exact) and diagonalised by cyclic Jacobi on the upper triangle in registers: CL_SWEEPS = 8 sweeps over the pairs
// (p, q), p < q, row by row, Rutishauser's formulas
//     theta = (a_qq - a_pp) / (2 a_pq);  t = sign(theta) / (|theta| + sqrt(theta^2 + 1));  c = 1 / sqrt(t^2 + 1);  s = t c;  tau = s / (1 + c);
//     a_pp -= t a_pq;  a_qq += t a_pq;  a_pq = 0;  a_kp' = a_kp - s (a_kq + tau a_kp);  a_kq' = a_kq + s (a_kp - tau a_kq)   (k != p, q),
// division and square root correctly rounded.  A pair with |a_pq| <= 2^-30 (of the scaled matrix) is left alone: a diagonal G is returned as
// exactly max_i G_ii, and the sweeps after convergence cost nothing.  lambda_max = the largest diagonal entry after the last sweep, scaled
// back.  Error bound (u = 2^-24): a rotation replaces the rows and columns p, q by an orthogonal transform of them plus an error of at most
// 10 u in norm relative to theirs (4 roundings per updated entry, the departure of the rounded c, s, tau from an exact rotation), and their
// Frobenius norm is at most 2 lambda_max; so each of the at most 36 * 8 rotations moves lambda_max by at most 20 u lambda_max (Weyl).  The
// pairs left alone move it by at most sqrt(72) * 2^-30 < 2^-26.  With the off-diagonal norm after eight sweeps below that (cyclic Jacobi
// converges quadratically; the tests measure it) the relative error of lambda_max is at most
//     CL_EIGEN_BOUND = 36 * 8 * 20 * 2^-24 + 2^-25 = 5760.5 * 2^-24  (3.4e-4),
// a worst case over the operation count; the measured error is a few u.
//
// out[first neuron + j] = sqrtf(lambda_max) * fabsf(scale[first neuron + j]) (scale NULL: no factor).  A zero row gives +0.0.
#include <math.h>
#include "vd_common.h"

namespace {

constexpr int CL_K = 6;                 // int64 per job: weight offset, rows, Cin, T, first neuron, first workgroup
constexpr int CL_PIECE = 576;           // floats of a row a wave stages at a time
constexpr int CL_SWEEPS = 8;
constexpr int CL_GRAM = 45;             // gram slots per neuron
constexpr float CL_SKIP = 9.31322574615478515625e-10f;      // 2^-30

__host__ __device__ constexpr int tri(int i, int j) { return i * 9 - (i * (i - 1)) / 2 + (j - i); }      // i <= j
__device__ __forceinline__ constexpr int sym(int i, int j) { return i <= j ? tri(i, j) : tri(j, i); }

__host__ __device__ inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// last job whose first workgroup <= the block (block-uniform binary search; first workgroups ascend)
__device__ __forceinline__ const int64_t* lip_job(const int64_t* __restrict__ table, int n_jobs) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(int64_t)CL_K * mid + 5] <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    return table + (int64_t)CL_K * lo;
}

// lambda_max of the symmetric positive semi-definite 9 x 9 matrix whose upper triangle is a[] (the header's stage 2); a[] is destroyed.
__device__ __forceinline__ float jacobi_lambda_max(float (&a)[CL_GRAM]) {
    float m = a[tri(0, 0)];
#pragma unroll
    for (int i = 1; i < 9; ++i) m = fmaxf(m, a[tri(i, i)]);
    if (m == 0.0f) return 0.0f;                                  // a zero row: nothing to scale by
    if (!(m < INFINITY)) return m;
    const int ex = ilogbf(m);
#pragma unroll
    for (int e = 0; e < CL_GRAM; ++e) a[e] = ldexpf(a[e], -ex);
#pragma unroll 1
    for (int sweep = 0; sweep < CL_SWEEPS; ++sweep) {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
#pragma unroll
            for (int q = p + 1; q < 9; ++q) {
                const float apq = a[tri(p, q)];
                if (fabsf(apq) > CL_SKIP) {
                    const float app = a[tri(p, p)], aqq = a[tri(q, q)];
                    const float theta = (aqq - app) / (2.0f * apq);
                    const float t = copysignf(1.0f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
                    const float c = 1.0f / sqrtf(t * t + 1.0f);
                    const float s = t * c;
                    const float tau = s / (1.0f + c);
                    const float h = t * apq;
                    a[tri(p, p)] = app - h;
                    a[tri(q, q)] = aqq + h;
                    a[tri(p, q)] = 0.0f;
#pragma unroll
                    for (int k = 0; k < 9; ++k) {
                        if (k == p || k == q) continue;
                        const float x = a[sym(k, p)], y = a[sym(k, q)];
                        a[sym(k, p)] = x - s * (y + tau * x);
                        a[sym(k, q)] = y + s * (x - tau * y);
                    }
                }
            }
        }
    }
    m = a[tri(0, 0)];
#pragma unroll
    for (int i = 1; i < 9; ++i) m = fmaxf(m, a[tri(i, i)]);
    return ldexpf(m, ex);
}

// One wave's row: G in g[] (every lane holds the same bits).  Every wave of the workgroup walks the same number of pieces (one job, one Cin):
// the barriers are workgroup-uniform, and a wave without a row (`live` false) only keeps them company.
template <int T>
__device__ __forceinline__ void lip_gram(const float* __restrict__ row, int64_t Cin, bool vec, bool live, float* __restrict__ lds, int lane,
                                         float (&g)[T == 9 ? CL_GRAM : 1]) {
    constexpr int NG = T == 9 ? CL_GRAM : 1;
#pragma unroll
    for (int e = 0; e < NG; ++e) g[e] = 0.0f;
    const int64_t len = Cin * T;
    for (int64_t base = 0; base < len; base += CL_PIECE) {
        const int n = (int)(len - base < CL_PIECE ? len - base : CL_PIECE);      // floats of this piece; a multiple of 4 where vec
        if (live) {
            const float* __restrict__ src = row + base;
            if (vec) {
#pragma unroll
                for (int u = 0; u < CL_PIECE / 256; ++u) {
                    const int k = (lane + 64 * u) << 2;
                    if (k < n) *reinterpret_cast<f32x4*>(lds + k) = *reinterpret_cast<const f32x4*>(src + k);
                }
                const int k = (lane + 64 * (CL_PIECE / 256)) << 2;             // 144 items: two full rounds of 64 and 16 more
                if (k < n && k < CL_PIECE) *reinterpret_cast<f32x4*>(lds + k) = *reinterpret_cast<const f32x4*>(src + k);
            } else {
#pragma unroll
                for (int u = 0; u < CL_PIECE / 64; ++u) {
                    const int k = lane + 64 * u;
                    if (k < n) lds[k] = src[k];
                }
            }
        }
        __syncthreads();
        if (live) {
            if (T == 9) {
                if (9 * lane < n) {                                             // channel base / 9 + lane of the row
                    float w[9];
#pragma unroll
                    for (int i = 0; i < 9; ++i) w[i] = lds[9 * lane + i];
#pragma unroll
                    for (int i = 0; i < 9; ++i)
#pragma unroll
                        for (int j = i; j < 9; ++j) g[T == 9 ? tri(i, j) : 0] += w[i] * w[j];
                }
            } else {
#pragma unroll
                for (int u = 0; u < CL_PIECE / 64; ++u) {                        // channels base + lane, base + lane + 64, ...: ascending
                    const int k = lane + 64 * u;
                    if (k < n) {
                        const float w = lds[k];
                        g[0] += w * w;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (!live) return;
#pragma unroll
    for (int e = 0; e < NG; ++e) g[e] = wave_sum(g[e]);
}

__global__ __launch_bounds__(256) void channel_lipschitz_kernel(const float* __restrict__ w, const int64_t* __restrict__ table, int n_jobs,
                                                                 const float* __restrict__ scale, float* __restrict__ out,
                                                                 float* __restrict__ gram) {
    __shared__ __attribute__((aligned(16))) float sm[4][CL_PIECE];
    const int64_t* __restrict__ t = lip_job(table, n_jobs);
    const int64_t rows = t[1], Cin = t[2], T = t[3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r = ((int64_t)blockIdx.x - t[5]) * 4 + wave;
    const bool live = r < rows;                                                  // wave-uniform
    const int64_t len = Cin * T;
    const float* __restrict__ job = w + t[0];
    const bool vec = aligned16(job) && (len & 3) == 0;
    const float* __restrict__ row = job + (live ? r : 0) * len;
    const int64_t neuron = t[4] + r;
    float lam;
    if (T == 9) {
        float g[CL_GRAM];
        lip_gram<9>(row, Cin, vec, live, sm[wave], lane, g);
        if (!live) return;
        if (gram) {
#pragma unroll
            for (int e = 0; e < CL_GRAM; ++e)
                if (lane == e) gram[CL_GRAM * neuron + e] = g[e];
        }
        lam = jacobi_lambda_max(g);
    } else {
        float g[1];
        lip_gram<1>(row, Cin, vec, live, sm[wave], lane, g);
        if (!live) return;
        if (gram && lane == 0) gram[CL_GRAM * neuron] = g[0];
        lam = g[0];
    }
    if (lane == 0) {
        const float sv = sqrtf(lam);
        out[neuron] = scale ? sv * fabsf(scale[neuron]) : sv;
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int vd_channel_lipschitz_plan(int Cin, int T, int64_t* chain) {
    VD_REQUIRE(Cin > 0 && (T == 1 || T == 9) && chain, "vd_channel_lipschitz_plan: Cin = %d, T = %d (1 or 9)", Cin, T);
    *chain = ((int64_t)Cin + 63) / 64 + 6;
    return 0;
}

extern "C" int vd_channel_lipschitz(const float* w, const int64_t* host_table, const int64_t* table, int n_jobs, int64_t total_blocks,
                                    const float* scale, float* out, float* gram, void* stream) {
    VD_REQUIRE(w && host_table && table && out, "vd_channel_lipschitz: null pointer");
    VD_REQUIRE((((uintptr_t)w) & 3) == 0, "vd_channel_lipschitz: w not 4-byte aligned");
    VD_REQUIRE(n_jobs >= 1, "vd_channel_lipschitz: n_jobs = %d", n_jobs);
    int64_t neuron = 0, block = 0;
    for (int k = 0; k < n_jobs; ++k) {
        const int64_t* t = host_table + (int64_t)CL_K * k;
        VD_REQUIRE(t[0] >= 0 && t[1] >= 1 && t[2] >= 1 && t[1] <= (1 << 24) && t[2] <= (1 << 24),
                   "vd_channel_lipschitz: job %d has weight offset, rows, Cin = %lld, %lld, %lld", k, (long long)t[0], (long long)t[1], (long long)t[2]);
        VD_REQUIRE(t[3] == 1 || t[3] == 9, "vd_channel_lipschitz: job %d has T = %lld taps (1 or 9)", k, (long long)t[3]);
        VD_REQUIRE(t[4] == neuron && t[5] == block, "vd_channel_lipschitz: job %d: first neuron %lld (expected %lld), first workgroup %lld (expected %lld)",
                   k, (long long)t[4], (long long)neuron, (long long)t[5], (long long)block);
        neuron += t[1];
        block += (t[1] + 3) / 4;
    }
    VD_REQUIRE(block == total_blocks && block < (1ll << 31), "vd_channel_lipschitz: the table owns %lld workgroups, total_blocks = %lld", (long long)block,
               (long long)total_blocks);
    hipLaunchKernelGGL(channel_lipschitz_kernel, dim3((unsigned)total_blocks), dim3(256), 0, ST, w, table, n_jobs, scale, out, gram);
    VD_LAUNCH_CHECK("vd_channel_lipschitz");
    return 0;
}
