// Sharpness-aware minimisation (villandiffusion_amd/trainer.py, Trainer(sam=...)): the whole-buffer passes between the two forward + backward
// passes of a SAM step.  w <- w + e with e = rho * T^2 g / ||T g||, T = 1 (SAM), |w| + eta (ASAM), or one value per neuron, the root mean square
// of its weight row plus eta (neuron-adaptive).  All are HBM-bound, plain C++ with vector loads and stores, no atomics, every sum in a fixed
// order: a repeat is bit-identical.  Compiled without FMA contraction: every product and sum is rounded on its own, so the elementwise parts
// are the numpy float32 op sequence bit for bit.
//
// The flat kernels walk their n floats in ITEMS of four consecutive floats counted from the buffer's start.  Item q belongs to thread
// q % (grid * 256) of the launch.  Where every pointer is 16-byte aligned a whole item is one f32x4 access, otherwise (and for the last, partial
// item) four scalar ones: which thread owns an element and the order it is used in do not depend on that choice.
#include "vd_common.h"
#include <math.h>

namespace {

constexpr int SAM_BLOCK = 256;      // threads of a workgroup
constexpr int SAM_FPT = 16;         // floats a thread is sized for (four items) before the grid is capped
constexpr int SAM_MAXGRID = 1024;   // workgroups at most: `partial` holds one float each

inline int sam_grid(int64_t n) {
    const int64_t per = (int64_t)SAM_BLOCK * SAM_FPT;
    const int64_t g = (n + per - 1) / per;
    return (int)(g < 1 ? 1 : (g > SAM_MAXGRID ? SAM_MAXGRID : g));
}
__host__ __device__ inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

#define ITEM_STRIDE(q, n) \
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < (n); q += (int64_t)gridDim.x * blockDim.x)

// Stage 1 of vd_sam_norm_sq.  A thread keeps one partial per position e of its items (four chains, items in ascending order), adds them as
// (a0 + a1) + (a2 + a3); the 64 lanes of a wave are added by the xor tree of wave_sum, the four waves as (r0 + r1) + (r2 + r3).
template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void sam_norm_kernel(const float* __restrict__ g, const float* __restrict__ w, int64_t n, float eta,
                                                       float* __restrict__ partial) {
    __shared__ float red[4];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    ITEM_STRIDE(q, (n + 3) >> 2) {
        const int64_t k0 = q << 2;
        if (VEC && k0 + 4 <= n) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(g + k0);
            f32x4 y = {0.f, 0.f, 0.f, 0.f};
            if (MODE == 1) y = *reinterpret_cast<const f32x4*>(w + k0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float u = MODE == 1 ? (fabsf(y[e]) + eta) * x[e] : x[e];
                acc[e] += u * u;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (k0 + e < n) {
                    const float u = MODE == 1 ? (fabsf(w[k0 + e]) + eta) * g[k0 + e] : g[k0 + e];
                    acc[e] += u * u;
                }
        }
    }
    const float s = block_sum_256((acc[0] + acc[1]) + (acc[2] + acc[3]), red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// Stage 2: one workgroup; thread t adds partial[t], partial[t + 256], ... in that order, then the same wave tree and (r0 + r1) + (r2 + r3).
__global__ __launch_bounds__(256) void sam_norm_finish_kernel(const float* __restrict__ partial, int n_partial, float* __restrict__ out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int k = threadIdx.x; k < n_partial; k += 256) s += partial[k];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) *out = s;
}

// c = rho / (sqrtf(*norm_sq) + 1e-12f), every thread from the same device word; 0 with ok = false when *norm_sq is not finite or is 0.
__device__ __forceinline__ float sam_coef(const float* __restrict__ norm_sq, float rho, bool& ok) {
    const float ns = *norm_sq;
    ok = ns > 0.f && ns < INFINITY;                      // NaN fails both comparisons
    return ok ? rho / (sqrtf(ns) + 1e-12f) : 0.f;
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void sam_perturb_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ backup, int64_t n,
                                                          float eta, float rho, const float* __restrict__ norm_sq) {
    bool ok;
    const float c = sam_coef(norm_sq, rho, ok);
    if (!ok && !backup) return;
    ITEM_STRIDE(q, (n + 3) >> 2) {
        const int64_t k0 = q << 2;
        if (VEC && k0 + 4 <= n) {
            f32x4 x = *reinterpret_cast<const f32x4*>(w + k0);
            if (backup) *reinterpret_cast<f32x4*>(backup + k0) = x;
            if (ok) {
                const f32x4 d = *reinterpret_cast<const f32x4*>(g + k0);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float a = c;
                    if (MODE == 1) {
                        const float T = fabsf(x[e]) + eta;
                        a = (c * T) * T;
                    }
                    x[e] = x[e] + a * d[e];
                }
                *reinterpret_cast<f32x4*>(w + k0) = x;
            }
        } else {
            for (int e = 0; e < 4 && k0 + e < n; ++e) {
                const float x = w[k0 + e];
                if (backup) backup[k0 + e] = x;
                if (ok) {
                    float a = c;
                    if (MODE == 1) {
                        const float T = fabsf(x) + eta;
                        a = (c * T) * T;
                    }
                    w[k0 + e] = x + a * g[k0 + e];
                }
            }
        }
    }
}

// ---- neuron-adaptive mode: ANP's NEURON TABLE (vd_defense.hip), {weight offset, rows, row length, bias offset or -1, first neuron, first workgroup}
constexpr int NJ = 6;

__device__ __forceinline__ float neuron_T(float wsq, int64_t len, float eta) { return sqrtf(wsq / (float)len) + eta; }

// One workgroup.  Thread t walks the jobs in table order and, within a job, the rows t, t + 256, ... in that order, in ONE f32 chain of
// (T_j * T_j) * gsq_j; the 256 chains are added by the wave tree and (r0 + r1) + (r2 + r3).  A second walk writes the coefficients.
__global__ __launch_bounds__(256) void sam_neuron_coef_kernel(const float* __restrict__ wsq, const float* __restrict__ gsq,
                                                              const int64_t* __restrict__ table, int n_jobs, int64_t n_neurons, float rho, float eta,
                                                              float* __restrict__ coef, float* __restrict__ norm_sq) {
    __shared__ float red[4];
    float s = 0.f;
    for (int k = 0; k < n_jobs; ++k) {
        const int64_t rows = table[NJ * k + 1], len = table[NJ * k + 2], j0 = table[NJ * k + 4];
        for (int64_t r = threadIdx.x; r < rows; r += 256) {
            const int64_t j = j0 + r;
            if (j >= n_neurons) break;
            const float T = neuron_T(wsq[j], len, eta);
            s += (T * T) * gsq[j];
        }
    }
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) *norm_sq = s;
    const bool ok = s > 0.f && s < INFINITY;
    const float c = ok ? rho / (sqrtf(s) + 1e-12f) : 0.f;
    for (int k = 0; k < n_jobs; ++k) {
        const int64_t rows = table[NJ * k + 1], len = table[NJ * k + 2], j0 = table[NJ * k + 4];
        for (int64_t r = threadIdx.x; r < rows; r += 256) {
            const int64_t j = j0 + r;
            if (j >= n_neurons) break;
            const float T = neuron_T(wsq[j], len, eta);
            coef[j] = ok ? (c * T) * T : 0.f;
        }
    }
}

__device__ __forceinline__ const int64_t* neuron_job(const int64_t* __restrict__ table, int n_jobs) {
    int lo = 0, hi = n_jobs - 1;
    const int64_t blk = blockIdx.x;
    while (lo < hi) {                                            // last job whose first workgroup <= blk (block-uniform)
        const int mid = (lo + hi + 1) >> 1;
        if (table[(int64_t)NJ * mid + 5] <= blk) lo = mid; else hi = mid - 1;
    }
    return table + (int64_t)NJ * lo;
}

// vd_neuron_scale's layout: one wave per row, four rows per workgroup, item q of a row in lane q % 64.
__global__ __launch_bounds__(256) void neuron_axpy_kernel(float* __restrict__ w, const float* __restrict__ g, const int64_t* __restrict__ table,
                                                          int n_jobs, const float* __restrict__ coef) {
    const int64_t* __restrict__ t = neuron_job(table, n_jobs);
    const int64_t rows = t[1], len = t[2];
    const int64_t row = (blockIdx.x - t[5]) * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float a = coef[t[4] + row];
    float* __restrict__ dst = w + t[0] + row * len;
    const float* __restrict__ src = g + t[0] + row * len;
    const bool vec = aligned16(src) && aligned16(dst);
    const int64_t items = (len + 3) >> 2;
    for (int64_t q = lane; q < items; q += 64) {
        const int64_t k0 = q << 2;
        if (vec && k0 + 4 <= len) {
            f32x4 x = *reinterpret_cast<const f32x4*>(dst + k0);
            const f32x4 d = *reinterpret_cast<const f32x4*>(src + k0);
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = x[e] + a * d[e];
            *reinterpret_cast<f32x4*>(dst + k0) = x;
        } else {
            for (int e = 0; e < 4 && k0 + e < len; ++e) dst[k0 + e] = dst[k0 + e] + a * src[k0 + e];
        }
    }
}

inline bool sam_scalar_ok(float v) { return v >= 0.f && v < INFINITY; }      // NaN fails
inline bool disjoint(const void* a, const void* b, int64_t n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return (x < y ? y - x : x - y) >= (uintptr_t)n * 4;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int vd_sam_plan(int64_t n, int* grid, int* block, int* floats_per_thread) {
    VD_REQUIRE(n >= 0 && grid && block && floats_per_thread, "vd_sam_plan: bad args");
    *grid = sam_grid(n);
    *block = SAM_BLOCK;
    *floats_per_thread = SAM_FPT;
    return 0;
}

extern "C" int vd_sam_norm_sq(const float* g, const float* w, int64_t n, int mode, float eta, float* partial, float* out_sq, void* stream) {
    VD_REQUIRE(mode == 0 || mode == 1, "vd_sam_norm_sq: mode %d (0 = sam, 1 = asam)", mode);
    VD_REQUIRE(sam_scalar_ok(eta), "vd_sam_norm_sq: eta must be finite and >= 0, got %g", (double)eta);
    VD_REQUIRE(n >= 0, "vd_sam_norm_sq: n = %lld", (long long)n);
    VD_REQUIRE(g && partial && out_sq && (w || mode == 0), "vd_sam_norm_sq: null pointer");
    VD_REQUIRE(((((uintptr_t)g) | ((uintptr_t)w)) & 3) == 0, "vd_sam_norm_sq: pointers not 4-byte aligned");
    const int grid = sam_grid(n);
    const bool vec = aligned16(g) && (mode == 0 || aligned16(w));
    if (mode == 0) {
        if (vec) hipLaunchKernelGGL((sam_norm_kernel<0, true>), dim3(grid), dim3(SAM_BLOCK), 0, ST, g, w, n, eta, partial);
        else hipLaunchKernelGGL((sam_norm_kernel<0, false>), dim3(grid), dim3(SAM_BLOCK), 0, ST, g, w, n, eta, partial);
    } else {
        if (vec) hipLaunchKernelGGL((sam_norm_kernel<1, true>), dim3(grid), dim3(SAM_BLOCK), 0, ST, g, w, n, eta, partial);
        else hipLaunchKernelGGL((sam_norm_kernel<1, false>), dim3(grid), dim3(SAM_BLOCK), 0, ST, g, w, n, eta, partial);
    }
    hipLaunchKernelGGL(sam_norm_finish_kernel, dim3(1), dim3(256), 0, ST, partial, grid, out_sq);
    VD_LAUNCH_CHECK("vd_sam_norm_sq");
    return 0;
}

extern "C" int vd_sam_perturb(float* w, const float* g, float* backup, int64_t n, int mode, float eta, float rho, const float* norm_sq,
                              void* stream) {
    VD_REQUIRE(mode == 0 || mode == 1, "vd_sam_perturb: mode %d (0 = sam, 1 = asam)", mode);
    VD_REQUIRE(sam_scalar_ok(eta) && sam_scalar_ok(rho), "vd_sam_perturb: rho and eta must be finite and >= 0, got %g, %g", (double)rho, (double)eta);
    VD_REQUIRE(n >= 0, "vd_sam_perturb: n = %lld", (long long)n);
    VD_REQUIRE(w && g && norm_sq, "vd_sam_perturb: null pointer");
    VD_REQUIRE(((((uintptr_t)w) | ((uintptr_t)g) | ((uintptr_t)backup)) & 3) == 0, "vd_sam_perturb: pointers not 4-byte aligned");
    VD_REQUIRE(disjoint(w, g, n) && (!backup || (disjoint(w, backup, n) && disjoint(g, backup, n))), "vd_sam_perturb: the buffers overlap");
    if (n == 0) return 0;
    const int grid = sam_grid(n);
    const bool vec = aligned16(w) && aligned16(g) && aligned16(backup);
    if (mode == 0) {
        if (vec) hipLaunchKernelGGL((sam_perturb_kernel<0, true>), dim3(grid), dim3(SAM_BLOCK), 0, ST, w, g, backup, n, eta, rho, norm_sq);
        else hipLaunchKernelGGL((sam_perturb_kernel<0, false>), dim3(grid), dim3(SAM_BLOCK), 0, ST, w, g, backup, n, eta, rho, norm_sq);
    } else {
        if (vec) hipLaunchKernelGGL((sam_perturb_kernel<1, true>), dim3(grid), dim3(SAM_BLOCK), 0, ST, w, g, backup, n, eta, rho, norm_sq);
        else hipLaunchKernelGGL((sam_perturb_kernel<1, false>), dim3(grid), dim3(SAM_BLOCK), 0, ST, w, g, backup, n, eta, rho, norm_sq);
    }
    VD_LAUNCH_CHECK("vd_sam_perturb");
    return 0;
}

extern "C" int vd_sam_neuron_coef(const float* wsq, const float* gsq, const int64_t* table, int n_jobs, int64_t n_neurons, float rho, float eta,
                                  float* coef, float* norm_sq, void* stream) {
    VD_REQUIRE(sam_scalar_ok(eta) && sam_scalar_ok(rho), "vd_sam_neuron_coef: rho and eta must be finite and >= 0, got %g, %g", (double)rho,
               (double)eta);
    VD_REQUIRE(wsq && gsq && table && coef && norm_sq, "vd_sam_neuron_coef: null pointer");
    VD_REQUIRE(n_jobs > 0 && n_neurons > 0, "vd_sam_neuron_coef: n_jobs = %d, n_neurons = %lld", n_jobs, (long long)n_neurons);
    hipLaunchKernelGGL(sam_neuron_coef_kernel, dim3(1), dim3(256), 0, ST, wsq, gsq, table, n_jobs, n_neurons, rho, eta, coef, norm_sq);
    VD_LAUNCH_CHECK("vd_sam_neuron_coef");
    return 0;
}

extern "C" int vd_neuron_axpy(float* w, const float* g, const int64_t* table, int n_jobs, int64_t total_blocks, const float* coef, void* stream) {
    VD_REQUIRE(w && g && table && coef, "vd_neuron_axpy: null pointer");
    VD_REQUIRE(n_jobs > 0 && total_blocks > 0 && total_blocks < (1ll << 31), "vd_neuron_axpy: bad args");
    VD_REQUIRE(w != g, "vd_neuron_axpy: w must not be g");
    hipLaunchKernelGGL(neuron_axpy_kernel, dim3((unsigned)total_blocks), dim3(256), 0, ST, w, g, table, n_jobs, coef);
    VD_LAUNCH_CHECK("vd_neuron_axpy");
    return 0;
}
