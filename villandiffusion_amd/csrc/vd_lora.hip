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


// ---------------------------------------------------------------------------------------------------------------- vd_lora_act_grad
// The adapter gradient of a 1x1 layer y_b = W x_b straight from its activations (no [M, L] weight gradient is formed):
//   gab.A[q][l] += s * sum_{b,p} T[q][b,p] x[b][l][p],  T = Bm^T dy;      gab.B[m][q] += s * sum_{b,p} dy[b][m][p] Z[q][b,p],  Z = A x.
// An ACTIVATION JOB TABLE has NA int64 per row; a row is one layer, or one CHUNK of at most 768 of the layer's L + M accumulator rows (the rows
// of x, then the rows of dy) where a layer has more.  A workgroup of a row walks TILES of 32 pixels of one image, tile = wg, wg + n_wg, ...:
//   1. the four waves read the rows of x in pairs (half a wave per row, a lane per pixel: 128 contiguous bytes, a scalar per lane, so aligned and
//      unaligned rows take the same path), stage the rows of their chunk in LDS and sum Z per wave in row order; the two halves are added,
//      then the four waves as ((w0 + w1) + w2) + w3.  The same for dy and T.
//   2. thread t owns the chunk rows t, t + 256, t + 512: one fmaf chain per (row, q) over the pixels of the tile in ascending order, carried
//      in registers from tile to tile.
// After its last tile the workgroup writes its r * rows partial sums to the workspace; lora_act_reduce_kernel adds the partials of a row in
// workgroup order from 0, multiplies by s and stores or adds into gab.  No atomics: a repeat gives the same bits.
constexpr int NA = 16;
constexpr int PT = 32;                  // pixels of a tile
constexpr int PITCH = PT + 4;           // floats of a staged row: f32x4 reads of 64 consecutive rows spread over all banks
constexpr int ACT_U = 8;                // row pairs whose loads a wave issues together
constexpr int ROWS_PT = 3;              // accumulator rows of a thread
constexpr int CHUNK = 256 * ROWS_PT;    // accumulator rows of a table row
enum { J_DY, J_DBS, J_X, J_XBS, J_NB, J_M, J_L, J_N, J_AOFF, J_BOFF, J_WG0, J_NWG, J_ROW0, J_ROWS, J_WS, J_RB0 };

template <int COL>
__device__ __forceinline__ const int64_t* act_job(const int64_t* __restrict__ table, int n_rows, int64_t blk) {
    int lo = 0, hi = n_rows - 1;
    while (lo < hi) {                                            // last row whose first workgroup <= blk (block-uniform)
        const int mid = (lo + hi + 1) >> 1;
        if (table[(int64_t)NA * mid + COL] <= blk) lo = mid; else hi = mid - 1;
    }
    return table + (int64_t)NA * lo;
}

// One operand of step 1: rows [r0, r1) of `src` (channel stride N, this tile's pixels) are read, staged at stage[(row + shift) * PITCH] where
// 0 <= row + shift < rows, and contracted with coef(q, row) into out[q * PT + p].  TRANSPOSED: coef(q, row) = c[row * r + q] (B), else
// c[q * len + row] (A).
template <int RC, bool TRANSPOSED>
__device__ __forceinline__ void act_project(const float* __restrict__ src, int64_t N, int len, int r0, int r1, bool pin, int64_t shift, int64_t rows,
                                            const float* __restrict__ c, int r, float* __restrict__ stage, float* __restrict__ part,
                                            float* __restrict__ out) {
    const int lane = threadIdx.x & 63, h = lane >> 5, p = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float z[RC];
#pragma unroll
    for (int q = 0; q < RC; ++q) z[q] = 0.f;
    // ACT_U row pairs a pass: their loads are issued together (the pass is latency-bound otherwise); the sums still run in row order
    for (int j0 = (r0 >> 1) + wave; 2 * j0 < r1; j0 += 4 * ACT_U) {
        float v[ACT_U];
#pragma unroll
        for (int u = 0; u < ACT_U; ++u) {
            const int l = 2 * (j0 + 4 * u) + h;
            v[u] = (l >= r0 && l < r1 && pin) ? src[(int64_t)l * N] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < ACT_U; ++u) {
            const int j = j0 + 4 * u;
            if (2 * j < r1) {                                    // wave-uniform
                const int l0 = 2 * j, l1 = min(2 * j + 1, len - 1);
                const int l = l0 + h;
                const int64_t sr = (int64_t)l + shift;
                if (l >= r0 && l < r1 && sr >= 0 && sr < rows) stage[sr * PITCH + p] = v[u];
#pragma unroll
                for (int q = 0; q < RC; ++q) {
                    if (q < r) {
                        const float c0 = TRANSPOSED ? c[(int64_t)l0 * r + q] : c[(int64_t)q * len + l0];
                        const float c1 = TRANSPOSED ? c[(int64_t)l1 * r + q] : c[(int64_t)q * len + l1];
                        z[q] = fmaf(h ? c1 : c0, v[u], z[q]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < RC; ++q) {
        if (q < r) {
            const float t = z[q] + __shfl_xor(z[q], 32, 64);
            if (h == 0) part[(wave * r + q) * PT + p] = t;
        }
    }
    __syncthreads();
    const int n = r * PT;
    for (int i = threadIdx.x; i < n; i += 256) out[i] = ((part[i] + part[n + i]) + part[2 * n + i]) + part[3 * n + i];
    __syncthreads();
}

template <int RC>
__global__ __launch_bounds__(256) void lora_act_grad_kernel(const int64_t* __restrict__ table, int n_rows, const float* __restrict__ ab,
                                                             float* __restrict__ ws, int r) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int64_t* __restrict__ t = act_job<J_WG0>(table, n_rows, blockIdx.x);
    const int64_t wg = (int64_t)blockIdx.x - t[J_WG0], nwg = t[J_NWG];
    if (wg >= nwg) return;                                       // block-uniform (a grid larger than the table)
    const float* __restrict__ dy = reinterpret_cast<const float*>(t[J_DY]);
    const float* __restrict__ x = reinterpret_cast<const float*>(t[J_X]);
    const int64_t dbs = t[J_DBS], xbs = t[J_XBS], N = t[J_N], row0 = t[J_ROW0], rows = t[J_ROWS];
    const int nb = (int)t[J_NB], M = (int)t[J_M], L = (int)t[J_L];
    const float* __restrict__ A = ab + t[J_AOFF];
    const float* __restrict__ Bm = ab + t[J_BOFF];
    float* __restrict__ stage = lds;
    float* __restrict__ part = lds + rows * PITCH;
    float* __restrict__ Zs = part + 4 * r * PT;
    float* __restrict__ Ts = Zs + r * PT;
    // the rows this chunk accumulates: x rows [xl0, xl1) and dy rows [ym0, ym1); Z is needed where the chunk holds a dy row, T where an x row
    const int xl0 = (int)min<int64_t>(row0, L), xl1 = (int)min<int64_t>(row0 + rows, L);
    const int ym0 = (int)(max<int64_t>(row0, L) - L), ym1 = (int)(max<int64_t>(row0 + rows, L) - L);
    const bool needZ = ym1 > ym0, needT = xl1 > xl0;
    float acc[ROWS_PT][RC];
#pragma unroll
    for (int k = 0; k < ROWS_PT; ++k)
#pragma unroll
        for (int q = 0; q < RC; ++q) acc[k][q] = 0.f;
    const int p = threadIdx.x & 31;
    const int64_t tpi = (N + PT - 1) / PT, tiles = (int64_t)nb * tpi;
    for (int64_t tile = wg; tile < tiles; tile += nwg) {
        const int64_t b = tile / tpi, p0 = (tile - b * tpi) * PT;
        const bool pin = p0 + p < N;
        act_project<RC, false>(x + b * xbs + p0 + p, N, L, needZ ? 0 : xl0, needZ ? L : xl1, pin, -row0, rows, A, r, stage, part, Zs);
        act_project<RC, true>(dy + b * dbs + p0 + p, N, M, needT ? 0 : ym0, needT ? M : ym1, pin, (int64_t)L - row0, rows, Bm, r, stage, part, Ts);
#pragma unroll
        for (int k = 0; k < ROWS_PT; ++k) {
            const int64_t crow = threadIdx.x + 256 * k;
            if (crow < rows) {
                const float* __restrict__ W = (row0 + crow < L) ? Ts : Zs;
                const float* __restrict__ sr = stage + crow * PITCH;
#pragma unroll
                for (int p4 = 0; p4 < PT / 4; ++p4) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(sr + 4 * p4);
#pragma unroll
                    for (int q = 0; q < RC; ++q) {
                        if (q < r) {
                            const f32x4 w = *reinterpret_cast<const f32x4*>(W + q * PT + 4 * p4);
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[k][q] = fmaf(v[e], w[e], acc[k][q]);
                        }
                    }
                }
            }
        }
        __syncthreads();                                         // the next tile overwrites the staged rows and Z, T
    }
    float* __restrict__ out = ws + t[J_WS] + wg * rows * r;
#pragma unroll
    for (int k = 0; k < ROWS_PT; ++k) {
        const int64_t crow = threadIdx.x + 256 * k;
        if (crow < rows) {
#pragma unroll
            for (int q = 0; q < RC; ++q)
                if (q < r) out[crow * r + q] = acc[k][q];
        }
    }
}

__global__ __launch_bounds__(256) void lora_act_reduce_kernel(const int64_t* __restrict__ table, int n_rows, const float* __restrict__ ws,
                                                               float* __restrict__ gab, int r, float s, int accumulate) {
    const int64_t* __restrict__ t = act_job<J_RB0>(table, n_rows, blockIdx.x);
    const int64_t rows = t[J_ROWS], n = rows * r;
    const int64_t e = ((int64_t)blockIdx.x - t[J_RB0]) * 256 + threadIdx.x;
    if (e >= n) return;
    const float* __restrict__ src = ws + t[J_WS] + e;
    float sum = src[0];
    for (int64_t w = 1; w < t[J_NWG]; ++w) sum += src[w * n];
    const int64_t R = t[J_ROW0] + e / r, L = t[J_L];
    const int q = (int)(e % r);
    float* __restrict__ dst = R < L ? gab + t[J_AOFF] + q * L + R : gab + t[J_BOFF] + (R - L) * r + q;
    const float v = s * sum;
    *dst = accumulate ? *dst + v : v;
}

// Host-side walk of a table: VD_EINVAL-style check of every row, the grids, the LDS of the widest row and the workspace floats.
struct act_plan { int64_t wgs, rblocks, ws_floats; int lds_bytes; };
const char* act_check(const int64_t* tb, int n_rows, int r, act_plan* out) {
    int64_t wg = 0, rb = 0, wsf = 0;
    int lds = 0;
    for (int k = 0; k < n_rows; ++k) {
        const int64_t* t = tb + (int64_t)NA * k;
        if (!t[J_DY] || !t[J_X] || t[J_NB] < 1 || t[J_M] < 1 || t[J_L] < 1 || t[J_N] < 1) return "a null operand or an empty dimension";
        if (t[J_M] >= (1ll << 30) || t[J_L] >= (1ll << 30) || t[J_NB] >= (1ll << 30)) return "a dimension of 2^30 or more";
        if (t[J_DBS] < 0 || t[J_XBS] < 0 || t[J_AOFF] < 0 || t[J_BOFF] < 0) return "a negative stride or offset";
        if (t[J_ROWS] < 1 || t[J_ROWS] > CHUNK || t[J_ROW0] < 0 || t[J_ROW0] + t[J_ROWS] > t[J_L] + t[J_M]) return "a chunk outside [0, L + M) or of more than 768 rows";
        const int64_t tiles = t[J_NB] * ((t[J_N] + PT - 1) / PT);
        if (t[J_NWG] < 1 || t[J_NWG] > tiles) return "a workgroup count outside [1, tiles]";
        if (t[J_WG0] != wg || t[J_RB0] != rb || t[J_WS] != wsf) return "first workgroups or workspace offsets that do not ascend as planned";
        wg += t[J_NWG];
        rb += (t[J_ROWS] * r + 255) / 256;
        wsf += t[J_NWG] * t[J_ROWS] * r;
        const int b = (int)((t[J_ROWS] * PITCH + 6 * r * PT) * sizeof(float));
        lds = b > lds ? b : lds;
        if (wg >= (1ll << 31) || rb >= (1ll << 31)) return "more than 2^31 workgroups";
    }
    out->wgs = wg; out->rblocks = rb; out->ws_floats = wsf; out->lds_bytes = lds;
    return nullptr;
}
constexpr int ACT_LDS_MAX = (CHUNK * PITCH + 6 * 32 * PT) * (int)sizeof(float);

template <int RC>
int act_launch(const act_plan& pl, const int64_t* table, int n_rows, const float* ab, float* ws, int r, hipStream_t st) {
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(lora_act_grad_kernel<RC>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, ACT_LDS_MAX);
    VD_REQUIRE(attr == hipSuccess, "vd_lora_act_grad: cannot reserve %d bytes of LDS", ACT_LDS_MAX);
    hipLaunchKernelGGL(lora_act_grad_kernel<RC>, dim3((unsigned)pl.wgs), dim3(256), pl.lds_bytes, st, table, n_rows, ab, ws, r);
    return 0;
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

extern "C" int64_t vd_lora_act_grad_ws_floats(const int64_t* host_table, int n_rows, int r) {
    act_plan pl;
    if (!host_table || n_rows <= 0 || r < 1 || r > 32 || act_check(host_table, n_rows, r, &pl)) return -1;
    return pl.ws_floats;
}

extern "C" int vd_lora_act_grad(const int64_t* host_table, const int64_t* table, int n_rows, const float* ab, float* gab, int r, float s,
                                int accumulate, float* ws, int64_t ws_floats, void* stream) {
    VD_REQUIRE(host_table && table && ab && gab && ws && n_rows > 0, "vd_lora_act_grad: bad args");
    VD_REQUIRE(r >= 1 && r <= 32, "vd_lora_act_grad: the rank must lie in [1, 32], got %d", r);
    VD_REQUIRE(ab != gab, "vd_lora_act_grad: gab must not be ab (the adapter is read while its gradient is written)");
    act_plan pl;
    const char* why = act_check(host_table, n_rows, r, &pl);
    VD_REQUIRE(why == nullptr, "vd_lora_act_grad: the job table has %s", why);
    VD_REQUIRE(ws_floats >= pl.ws_floats, "vd_lora_act_grad: the workspace holds %lld floats, the table needs %lld", (long long)ws_floats,
               (long long)pl.ws_floats);
    int rc;
    if (r <= 4) rc = act_launch<4>(pl, table, n_rows, ab, ws, r, ST);
    else if (r <= 8) rc = act_launch<8>(pl, table, n_rows, ab, ws, r, ST);
    else if (r <= 16) rc = act_launch<16>(pl, table, n_rows, ab, ws, r, ST);
    else rc = act_launch<32>(pl, table, n_rows, ab, ws, r, ST);
    if (rc) return rc;
    VD_LAUNCH_CHECK("vd_lora_act_grad");
    hipLaunchKernelGGL(lora_act_reduce_kernel, dim3((unsigned)pl.rblocks), dim3(256), 0, ST, table, n_rows, ws, gab, r, s, accumulate);
    VD_LAUNCH_CHECK("vd_lora_act_grad (reduce)");
    return 0;
}
