// Anchored fine-tuning (villandiffusion_amd/anchor.py, Trainer(anchor=...)): the diagonal Fisher accumulation and the gradient of the penalty
// lambda / 2 * sum_i F_i (w_i - w0_i)^2 (EWC; F = 1: L2-SP), each ONE pass over the flat buffers.  HBM-bound, plain C++ with vector loads and
// stores, no atomics, every sum in a fixed order: a repeat is bit-identical.  Compiled without FMA contraction: every product, difference and sum
// is rounded on its own, so the elementwise parts are the numpy float32 op sequence bit for bit.
//
// Both kernels walk their n floats the way vd_sam_perturb does (vd_sam.hip): in ITEMS of four consecutive floats counted from the buffer's start,
// item q in thread q % (grid * 256) of the launch.  Where every pointer is 16-byte aligned a whole item is one f32x4 access, otherwise (and for
// the last, partial item) four scalar ones: which thread owns an element and the order it is used in do not depend on that choice.
#include "vd_common.h"
#include <math.h>

namespace {

constexpr int ANC_BLOCK = 256;      // threads of a workgroup
constexpr int ANC_FPT = 16;         // floats a thread is sized for (four items) before the grid is capped
constexpr int ANC_MAXGRID = 1024;   // workgroups at most: `partial` holds one float each        (vd_sam_plan's rule, restated)

inline int anc_grid(int64_t n) {
    const int64_t per = (int64_t)ANC_BLOCK * ANC_FPT;
    const int64_t g = (n + per - 1) / per;
    return (int)(g < 1 ? 1 : (g > ANC_MAXGRID ? ANC_MAXGRID : g));
}
inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

#define ITEM_STRIDE(q, n) \
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < (n); q += (int64_t)gridDim.x * blockDim.x)

// q = g * g;  F = F + s * q
template <bool VEC>
__global__ __launch_bounds__(256) void fisher_accum_kernel(float* __restrict__ F, const float* __restrict__ g, int64_t n, float s) {
    ITEM_STRIDE(q, (n + 3) >> 2) {
        const int64_t k0 = q << 2;
        if (VEC && k0 + 4 <= n) {
            f32x4 f = *reinterpret_cast<const f32x4*>(F + k0);
            const f32x4 x = *reinterpret_cast<const f32x4*>(g + k0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float sq = x[e] * x[e];
                f[e] = f[e] + s * sq;
            }
            *reinterpret_cast<f32x4*>(F + k0) = f;
        } else {
            for (int e = 0; e < 4 && k0 + e < n; ++e) {
                const float x = g[k0 + e];
                const float sq = x * x;
                F[k0 + e] = F[k0 + e] + s * sq;
            }
        }
    }
}

// d = w - w0;  t = F * d (EWC) or d (!EWC);  g = g + coef * t;  with PEN the thread also keeps one partial of t * d per position e of its items
// (four chains, items in ascending order), adds them as (a0 + a1) + (a2 + a3); the 64 lanes of a wave are added by the xor tree of wave_sum,
// the four waves as (r0 + r1) + (r2 + r3): stage 1 of vd_sam_norm_sq.
template <bool EWC, bool PEN, bool VEC>
__global__ __launch_bounds__(256) void anchor_grad_kernel(float* __restrict__ g, const float* __restrict__ w, const float* __restrict__ w0,
                                                          const float* __restrict__ F, int64_t n, float coef, float* __restrict__ partial) {
    __shared__ float red[4];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    ITEM_STRIDE(q, (n + 3) >> 2) {
        const int64_t k0 = q << 2;
        if (VEC && k0 + 4 <= n) {
            f32x4 x = *reinterpret_cast<const f32x4*>(g + k0);
            const f32x4 a = *reinterpret_cast<const f32x4*>(w + k0);
            const f32x4 b = *reinterpret_cast<const f32x4*>(w0 + k0);
            f32x4 f = {1.f, 1.f, 1.f, 1.f};
            if (EWC) f = *reinterpret_cast<const f32x4*>(F + k0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = a[e] - b[e];
                const float t = EWC ? f[e] * d : d;
                x[e] = x[e] + coef * t;
                if (PEN) acc[e] += t * d;
            }
            *reinterpret_cast<f32x4*>(g + k0) = x;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (k0 + e < n) {
                    const float d = w[k0 + e] - w0[k0 + e];
                    const float t = EWC ? F[k0 + e] * d : d;
                    g[k0 + e] = g[k0 + e] + coef * t;
                    if (PEN) acc[e] += t * d;
                }
        }
    }
    if (PEN) {
        const float s = block_sum_256((acc[0] + acc[1]) + (acc[2] + acc[3]), red);
        if (threadIdx.x == 0) partial[blockIdx.x] = s;
    }
}

// Stage 2 of vd_sam_norm_sq: one workgroup; thread t adds partial[t], partial[t + 256], ... in that order, then the wave tree and (r0 + r1) + (r2 + r3).
__global__ __launch_bounds__(256) void anchor_pen_finish_kernel(const float* __restrict__ partial, int n_partial, float* __restrict__ out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int k = threadIdx.x; k < n_partial; k += 256) s += partial[k];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) *out = s;
}

inline bool finite_f(float v) { return v > -INFINITY && v < INFINITY; }      // NaN fails
inline bool disjoint(const void* a, int64_t na, const void* b, int64_t nb) {      // [a, a + na floats) and [b, b + nb floats)
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y ? y - x >= (uintptr_t)na * 4 : x - y >= (uintptr_t)nb * 4;
}

template <bool EWC, bool PEN>
inline void launch_anchor(bool vec, int grid, hipStream_t st, float* g, const float* w, const float* w0, const float* F, int64_t n, float coef,
                          float* partial) {
    if (vec) hipLaunchKernelGGL((anchor_grad_kernel<EWC, PEN, true>), dim3(grid), dim3(ANC_BLOCK), 0, st, g, w, w0, F, n, coef, partial);
    else hipLaunchKernelGGL((anchor_grad_kernel<EWC, PEN, false>), dim3(grid), dim3(ANC_BLOCK), 0, st, g, w, w0, F, n, coef, partial);
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int vd_anchor_plan(int64_t n, int* grid, int* block, int* floats_per_thread) {
    VD_REQUIRE(n >= 0 && grid && block && floats_per_thread, "vd_anchor_plan: bad args");
    *grid = anc_grid(n);
    *block = ANC_BLOCK;
    *floats_per_thread = ANC_FPT;
    return 0;
}

extern "C" int vd_fisher_accum(float* F, const float* g, int64_t n, float s, void* stream) {
    VD_REQUIRE(finite_f(s) && s >= 0.f, "vd_fisher_accum: s must be finite and >= 0, got %g", (double)s);
    VD_REQUIRE(n >= 0, "vd_fisher_accum: n = %lld", (long long)n);
    VD_REQUIRE(F && g, "vd_fisher_accum: null pointer");
    VD_REQUIRE(((((uintptr_t)F) | ((uintptr_t)g)) & 3) == 0, "vd_fisher_accum: pointers not 4-byte aligned");
    VD_REQUIRE(disjoint(F, n, g, n), "vd_fisher_accum: the buffers overlap");
    if (n == 0) return 0;
    const int grid = anc_grid(n);
    if (aligned16(F) && aligned16(g)) hipLaunchKernelGGL((fisher_accum_kernel<true>), dim3(grid), dim3(ANC_BLOCK), 0, ST, F, g, n, s);
    else hipLaunchKernelGGL((fisher_accum_kernel<false>), dim3(grid), dim3(ANC_BLOCK), 0, ST, F, g, n, s);
    VD_LAUNCH_CHECK("vd_fisher_accum");
    return 0;
}

extern "C" int vd_anchor_grad(float* g, const float* w, const float* w0, const float* F, int64_t n, float coef, float* partial, float* pen,
                              void* stream) {
    VD_REQUIRE(finite_f(coef), "vd_anchor_grad: coef must be finite, got %g", (double)coef);
    VD_REQUIRE(n >= 0, "vd_anchor_grad: n = %lld", (long long)n);
    VD_REQUIRE(g && w && w0 && (partial || !pen), "vd_anchor_grad: null pointer");
    VD_REQUIRE(((((uintptr_t)g) | ((uintptr_t)w) | ((uintptr_t)w0) | ((uintptr_t)F) | ((uintptr_t)partial) | ((uintptr_t)pen)) & 3) == 0,
               "vd_anchor_grad: pointers not 4-byte aligned");
    const void* bufs[4] = {g, w, w0, F};
    for (int i = 0; i < 4; ++i) {
        if (!bufs[i]) continue;
        for (int j = i + 1; j < 4; ++j) VD_REQUIRE(!bufs[j] || disjoint(bufs[i], n, bufs[j], n), "vd_anchor_grad: the buffers overlap");
        if (pen) {
            VD_REQUIRE(disjoint(bufs[i], n, partial, ANC_MAXGRID) && disjoint(bufs[i], n, pen, 1), "vd_anchor_grad: a buffer overlaps the scratch");
        }
    }
    VD_REQUIRE(!pen || disjoint(partial, ANC_MAXGRID, pen, 1), "vd_anchor_grad: pen lies inside the scratch");
    if (n == 0 && !pen) return 0;      // (n = 0 with pen: the empty sum, *pen = 0)
    const int grid = anc_grid(n);
    {
        const bool vec = aligned16(g) && aligned16(w) && aligned16(w0) && aligned16(F);
        if (F) {
            if (pen) launch_anchor<true, true>(vec, grid, ST, g, w, w0, F, n, coef, partial);
            else launch_anchor<true, false>(vec, grid, ST, g, w, w0, F, n, coef, partial);
        } else {
            if (pen) launch_anchor<false, true>(vec, grid, ST, g, w, w0, F, n, coef, partial);
            else launch_anchor<false, false>(vec, grid, ST, g, w, w0, F, n, coef, partial);
        }
        if (pen) hipLaunchKernelGGL(anchor_pen_finish_kernel, dim3(1), dim3(256), 0, ST, partial, grid, pen);
    }
    VD_LAUNCH_CHECK("vd_anchor_grad");
    return 0;
}
