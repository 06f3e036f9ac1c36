// LoRA fine-tuning (villandiffusion_amd/lora.py): the merged weights W = W0 + s * B A of every adapted layer in one launch, and the chain rule
// from the ordinary weight gradient back to (A, B) in one launch.  Both are passes over the flat buffers, HBM-bound on w0 / w / g; the adapter
// itself (r rows of A per layer) is re-read from cache.  Sums run in a fixed order (no atomics): a repeat is bit-identical.  Compiled without
// FMA contraction, like the neuron kernels: every product and every sum is rounded on its own.
//
// An ADAPTER TABLE has one job of seven int64 per adapted weight tensor: {weight offset in floats, rows M, row length L, offset of A [r, L] in
// the adapter buffer, offset of B [M, r] in the adapter buffer, first row workgroup, first column workgroup}.
//   rows:    a workgroup is four waves and a wave owns one row, workgroup b of a job holds rows [4b, 4b + 4)  (vd_lora_merge, and dL/dB);
//   columns: a workgroup owns a TILE of 256 consecutive columns, tile b of a job holds columns [256 b, 256 b + 256)      (dL/dA).
// A row is walked in ITEMS of four consecutive floats counted from the row's start; item q belongs to lane q % 64.  Where L is a multiple of
// four and the job starts 16-byte aligned in every buffer an item is one f32x4 access, otherwise four scalar ones: which lane owns an element
// and the order it is used in do not depend on that choice.
#include "vd_common.h"

namespace {

constexpr int NL = 7;
constexpr int TILE = 256;   // columns of a column workgroup: 64 lanes x one item

__host__ __device__ inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

template <int COL>
__device__ __forceinline__ const int64_t* lora_job(const int64_t* __restrict__ table, int n_jobs, int64_t blk) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {                                            // last job whose first workgroup <= blk (block-uniform)
        const int mid = (lo + hi + 1) >> 1;
        if (table[(int64_t)NL * mid + COL] <= blk) lo = mid; else hi = mid - 1;
    }
    return table + (int64_t)NL * lo;
}

// The item at p[k0 .. k0 + 4) of a row of `len` floats; elements past the row's end read as 0 and are never stored.  vec implies len % 4 == 0.
__device__ __forceinline__ f32x4 load_item(const float* __restrict__ p, int64_t k0, int64_t len, bool vec) {
    if (vec) return *reinterpret_cast<const f32x4*>(p + k0);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (k0 + e < len) v[e] = p[k0 + e];
    return v;
}
__device__ __forceinline__ void store_item(float* __restrict__ p, int64_t k0, int64_t len, bool vec, f32x4 v) {
    if (vec) {
        *reinterpret_cast<f32x4*>(p + k0) = v;
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (k0 + e < len) p[k0 + e] = v[e];
}

// RC: the rank rounded up to 4 / 8 / 16 / 32, the length of the unrolled loops over q (q >= r is skipped, wave-uniformly).
template <int RC>
__global__ __launch_bounds__(256) void lora_merge_kernel(const float* __restrict__ w0, float* __restrict__ w, const int64_t* __restrict__ table,
                                                          int n_jobs, const float* __restrict__ ab, int r, float s) {
    const int64_t* __restrict__ t = lora_job<5>(table, n_jobs, blockIdx.x);
    const int64_t rows = t[1], len = t[2];
    const int64_t row = (blockIdx.x - t[5]) * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* __restrict__ A = ab + t[3];
    const float* __restrict__ Brow = ab + t[4] + row * r;
    const float* __restrict__ src = w0 + t[0] + row * len;
    float* __restrict__ dst = w + t[0] + row * len;
    const bool vec = (len & 3) == 0 && aligned16(src) && aligned16(dst) && aligned16(A);
    float b[RC];
#pragma unroll
    for (int q = 0; q < RC; ++q) b[q] = q < r ? Brow[q] : 0.f;
    const int64_t items = (len + 3) >> 2;
    for (int64_t it = lane; it < items; it += 64) {
        const int64_t k0 = it << 2;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < RC; ++q) {
            if (q < r) {
                const f32x4 a = load_item(A + q * len, k0, len, vec);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += b[q] * a[e];
            }
        }
        f32x4 x = load_item(src, k0, len, vec);
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = x[e] + s * acc[e];
        store_item(dst, k0, len, vec, x);
    }
}

// Workgroups [0, R) are row workgroups (dL/dB), workgroups [R, R + C) column workgroups (dL/dA); R follows from the last job.
//   dL/dB[j][q]: one wave per row.  A lane keeps one f32 partial per q over its items it = lane, lane + 64, ... in that order, the four elements
//   of an item added in index order; the 64 lanes are added by the xor tree of wave_sum; the sum is multiplied by s.
//   dL/dA[q][k]: a lane owns four columns of the tile.  Wave w of the four adds rows j = w, w + 4, w + 8, ... in that order in one f32 chain;
//   the four chains are added as ((c0 + c1) + c2) + c3; the sum is multiplied by s.
template <int RC>
__global__ __launch_bounds__(256) void lora_grad_kernel(const float* __restrict__ g, const int64_t* __restrict__ table, int n_jobs,
                                                         const float* __restrict__ ab, float* __restrict__ gab, int r, float s, int accumulate) {
    const int64_t* __restrict__ last = table + (int64_t)NL * (n_jobs - 1);
    const int64_t row_blocks = last[5] + ((last[1] + 3) >> 2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int64_t)blockIdx.x < row_blocks) {
        const int64_t* __restrict__ t = lora_job<5>(table, n_jobs, blockIdx.x);
        const int64_t rows = t[1], len = t[2];
        const int64_t row = (blockIdx.x - t[5]) * 4 + wave;
        if (row >= rows) return;                                 // wave-uniform: the shuffles below see whole waves
        const float* __restrict__ A = ab + t[3];
        const float* __restrict__ grow = g + t[0] + row * len;
        const bool vec = (len & 3) == 0 && aligned16(grow) && aligned16(A);
        float acc[RC];
#pragma unroll
        for (int q = 0; q < RC; ++q) acc[q] = 0.f;
        const int64_t items = (len + 3) >> 2;
        for (int64_t it = lane; it < items; it += 64) {
            const int64_t k0 = it << 2;
            const f32x4 x = load_item(grow, k0, len, vec);
#pragma unroll
            for (int q = 0; q < RC; ++q) {
                if (q < r) {
                    const f32x4 a = load_item(A + q * len, k0, len, vec);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[q] += x[e] * a[e];
                }
            }
        }
        float* __restrict__ out = gab + t[4] + row * r;
#pragma unroll
        for (int q = 0; q < RC; ++q) {
            if (q < r) {
                const float v = s * wave_sum(acc[q]);
                if (lane == 0) out[q] = accumulate ? out[q] + v : v;
            }
        }
        return;
    }
    const int64_t cb = (int64_t)blockIdx.x - row_blocks;
    const int64_t* __restrict__ t = lora_job<6>(table, n_jobs, cb);
    const int64_t rows = t[1], len = t[2];
    const int64_t first = (cb - t[6]) * TILE;
    if (first >= len) return;                                    // block-uniform (a grid larger than the table): no barrier is skipped by a part
    const int64_t k0 = first + lane * 4;
    const bool active = k0 < len;
    const float* __restrict__ G = g + t[0];
    const float* __restrict__ B = ab + t[4];
    float* __restrict__ out = gab + t[3];
    const bool vec = (len & 3) == 0 && aligned16(G) && aligned16(out);
    f32x4 acc[RC];
#pragma unroll
    for (int q = 0; q < RC; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (active) {
#pragma unroll 2
        for (int64_t j = wave; j < rows; j += 4) {
            const f32x4 x = load_item(G + j * len, k0, len, vec);
            const float* __restrict__ bj = B + j * r;
#pragma unroll
            for (int q = 0; q < RC; ++q) {
                if (q < r) {
                    const float bq = bj[q];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[q][e] += bq * x[e];
                }
            }
        }
    }
    __shared__ f32x4 red[3][64];
#pragma unroll
    for (int q = 0; q < RC; ++q) {
        if (q < r) {                                             // block-uniform
            if (wave > 0) red[wave - 1][lane] = acc[q];
            __syncthreads();
            if (wave == 0 && active) {
                f32x4 v = ((acc[q] + red[0][lane]) + red[1][lane]) + red[2][lane];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = s * v[e];
                float* __restrict__ dst = out + q * len;
                if (accumulate) {
                    const f32x4 old = load_item(dst, k0, len, vec);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = old[e] + v[e];
                }
                store_item(dst, k0, len, vec, v);
            }
            __syncthreads();
        }
    }
}

}  // namespace

#define ST ((hipStream_t)stream)
#define LORA_DISPATCH(kernel, grid, ...)                                                                             \
    do {                                                                                                             \
        if (r <= 4) hipLaunchKernelGGL(kernel<4>, dim3((unsigned)(grid)), dim3(256), 0, ST, __VA_ARGS__);            \
        else if (r <= 8) hipLaunchKernelGGL(kernel<8>, dim3((unsigned)(grid)), dim3(256), 0, ST, __VA_ARGS__);       \
        else if (r <= 16) hipLaunchKernelGGL(kernel<16>, dim3((unsigned)(grid)), dim3(256), 0, ST, __VA_ARGS__);     \
        else hipLaunchKernelGGL(kernel<32>, dim3((unsigned)(grid)), dim3(256), 0, ST, __VA_ARGS__);                  \
    } while (0)

extern "C" int vd_lora_merge(const float* w0, float* w, const int64_t* table, int n_jobs, int64_t total_blocks, const float* ab, int r, float s,
                             void* stream) {
    VD_REQUIRE(w0 && w && table && ab && n_jobs > 0 && total_blocks > 0 && total_blocks < (1ll << 31), "vd_lora_merge: bad args");
    VD_REQUIRE(r >= 1 && r <= 32, "vd_lora_merge: the rank must lie in [1, 32], got %d", r);
    VD_REQUIRE(w0 != w, "vd_lora_merge: w must not be w0 (the base weights are read for every merge)");
    LORA_DISPATCH(lora_merge_kernel, total_blocks, w0, w, table, n_jobs, ab, r, s);
    VD_LAUNCH_CHECK("vd_lora_merge");
    return 0;
}

extern "C" int vd_lora_grad(const float* g, const int64_t* table, int n_jobs, int64_t total_blocks, const float* ab, float* gab, int r, float s,
                            int accumulate, void* stream) {
    VD_REQUIRE(g && table && ab && gab && n_jobs > 0 && total_blocks > 0 && total_blocks < (1ll << 31), "vd_lora_grad: bad args");
    VD_REQUIRE(r >= 1 && r <= 32, "vd_lora_grad: the rank must lie in [1, 32], got %d", r);
    VD_REQUIRE(ab != gab, "vd_lora_grad: gab must not be ab (the adapter is read while its gradient is written)");
    LORA_DISPATCH(lora_grad_kernel, total_blocks, g, table, n_jobs, ab, gab, r, s, accumulate);
    VD_LAUNCH_CHECK("vd_lora_grad");
    return 0;
}
