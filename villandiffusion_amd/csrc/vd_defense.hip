// Backdoor mitigation (villandiffusion_amd/mitigation.py): the statistics of a sampled image set (Elijah's uniformity / total-variation features)
// and the data-free removal loss with its gradient; after them the three kernels of Adversarial Neuron Pruning (villandiffusion_amd/anp.py).
// All are HBM-bound, the reductions with sums in a fixed order (no atomics): a repeat is bit-identical.  Compiled without FMA contraction: the
// post-processing rounds every operation on its own, as vd_postprocess does, and the neuron kernels restate short torch op sequences.
//
// The removal-loss and image-set kernels walk their elements in ITEMS of four consecutive floats.  Where rows and pointers are 16-byte aligned an
// item is one f32x4 access, otherwise four scalar ones; which elements a thread owns and the order it adds them in do not depend on that choice, so
// a strided or unaligned view gives the same bits as its contiguous copy.
#include "vd_common.h"

namespace {

constexpr int MAXP = 1024;   // blocks of a reducing launch: partial[0 .. MAXP) and partial[MAXP .. 2 MAXP) hold one sum each

inline int item_grid(int64_t items) {
    int64_t g = (items + 255) / 256;
    return (int)(g < 1 ? 1 : (g > MAXP ? MAXP : g));
}
__host__ __device__ inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

#define ITEM_STRIDE(q, n) \
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < (n); q += (int64_t)gridDim.x * blockDim.x)

// Sum of `n` floats of `p` in double, by the whole block, in an order fixed by (n, thread count).  Every thread gets the result.
__device__ __forceinline__ double block_sum_partials(const float* __restrict__ p, int n, double* red) {
    double s = 0.0;
    for (int k = threadIdx.x; k < n; k += 256) s += (double)p[k];
    __syncthreads();
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// ---- removal loss ------------------------------------------------------------------------------------------------------------------------------
// Item q = elements [4q, 4q + 4) of ref's [B, chw]; its clean partner is pred row b, its shifted partner pred row B + b.
template <bool VEC>
__global__ __launch_bounds__(256) void removal_loss_kernel(const float* __restrict__ pred, const float* __restrict__ ref, float* __restrict__ dpred,
                                                            float* __restrict__ partial, int B, int64_t chw, int64_t pbs, float cc, float cs) {
    __shared__ float red[4];
    const int64_t n = (int64_t)B * chw;
    float sc = 0.f, ss = 0.f;
    ITEM_STRIDE(q, (n + 3) >> 2) {
        const int64_t f0 = q << 2;
        if (VEC) {                                       // chw % 4 == 0: an item never straddles two rows
            const int64_t b = f0 / chw, j = f0 - b * chw;
            const f32x4 r = *reinterpret_cast<const f32x4*>(ref + f0);
            const f32x4 pc = *reinterpret_cast<const f32x4*>(pred + b * pbs + j);
            const f32x4 ps = *reinterpret_cast<const f32x4*>(pred + (b + B) * pbs + j);
            f32x4 gc, gs;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dc = pc[e] - r[e], ds = ps[e] - r[e];
                sc += dc * dc;
                ss += ds * ds;
                gc[e] = cc * dc;
                gs[e] = cs * ds;
            }
            *reinterpret_cast<f32x4*>(dpred + f0) = gc;
            *reinterpret_cast<f32x4*>(dpred + n + f0) = gs;
        } else {
            for (int e = 0; e < 4; ++e) {
                const int64_t f = f0 + e;
                if (f >= n) break;
                const int64_t b = f / chw, j = f - b * chw;
                const float r = ref[f];
                const float dc = pred[b * pbs + j] - r, ds = pred[(b + B) * pbs + j] - r;
                sc += dc * dc;
                ss += ds * ds;
                dpred[f] = cc * dc;
                dpred[n + f] = cs * ds;
            }
        }
    }
    sc = block_sum_256(sc, red);
    ss = block_sum_256(ss, red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = sc;
        partial[MAXP + blockIdx.x] = ss;
    }
}

__global__ __launch_bounds__(256) void removal_loss_finish_kernel(const float* __restrict__ partial, int n_partial, double inv_n, float w_clean,
                                                                   float w_shift, float* __restrict__ terms) {
    __shared__ double red[256];
    const double c = block_sum_partials(partial, n_partial, red);
    const double s = block_sum_partials(partial + MAXP, n_partial, red);
    if (threadIdx.x == 0) {
        const float clean = (float)(c * inv_n), shift = (float)(s * inv_n);
        terms[0] = w_clean * clean + w_shift * shift;
        terms[1] = clean;
        terms[2] = shift;
    }
}

// ---- image-set statistics ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float post(float v, float mul, float add, float lo, float hi) {
    return fminf(fmaxf(__fadd_rn(__fmul_rn(v, mul), add), lo), hi);      // postprocess_kernel's sequence
}

// Pass 1: mean_img[i] = mean over n of y[n][i], the sum in double.  A block owns 32 neighbouring positions; its 8 thread rows take every 8th image
// each and their sums are added in row order.
constexpr int MP = 32, MS = 8;
__global__ __launch_bounds__(256) void image_set_mean_kernel(const float* __restrict__ x, float* __restrict__ mean_img, int N, int64_t chw,
                                                              int64_t xbs, float mul, float add, float lo, float hi) {
    __shared__ double red[MS][MP];
    const int px = threadIdx.x % MP, sl = threadIdx.x / MP;
    for (int64_t i0 = (int64_t)blockIdx.x * MP; i0 < chw; i0 += (int64_t)gridDim.x * MP) {
        const int64_t i = i0 + px;
        double s = 0.0;
        if (i < chw)
            for (int k = sl; k < N; k += MS) s += (double)post(x[(int64_t)k * xbs + i], mul, add, lo, hi);
        __syncthreads();
        red[sl][px] = s;
        __syncthreads();
        if (sl == 0 && i < chw) {
            double t = red[0][px];
#pragma unroll
            for (int k = 1; k < MS; ++k) t += red[k][px];
            mean_img[i] = (float)(t / (double)N);
        }
    }
}

// Pass 2: partial[block] = the block's share of sum_n ||y_n - mean||^2, partial[MAXP + block] = its share of sum_n TV(y_n).  An element adds its
// squared deviation, then |down - y| (h + 1 < H), then |right - y| (w + 1 < W); VEC needs W % 4 == 0, so an item lies inside one image row.
template <bool VEC>
__global__ __launch_bounds__(256) void image_set_dev_tv_kernel(const float* __restrict__ x, const float* __restrict__ mean_img,
                                                                float* __restrict__ partial, int N, int H, int W, int64_t chw, int64_t xbs,
                                                                float mul, float add, float lo, float hi) {
    __shared__ float red[4];
    const int64_t n = (int64_t)N * chw;
    float sq = 0.f, tv = 0.f;
    ITEM_STRIDE(q, (n + 3) >> 2) {
        const int64_t f0 = q << 2;
        if (VEC) {
            const int64_t img = f0 / chw, i = f0 - img * chw;
            const int w0 = (int)(i % W), h = (int)((i / W) % H);
            const float* row = x + img * xbs + i;
            const f32x4 v = *reinterpret_cast<const f32x4*>(row);
            const f32x4 m = *reinterpret_cast<const f32x4*>(mean_img + i);
            const bool down = h + 1 < H;
            f32x4 dn = v;
            if (down) dn = *reinterpret_cast<const f32x4*>(row + W);
            const float nxt = (w0 + 4 < W) ? row[4] : 0.f;
            float y[5];
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = post(v[e], mul, add, lo, hi);
            y[4] = post(nxt, mul, add, lo, hi);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = y[e] - m[e];
                sq += d * d;
                if (down) tv += fabsf(post(dn[e], mul, add, lo, hi) - y[e]);
                if (w0 + e + 1 < W) tv += fabsf(y[e + 1] - y[e]);
            }
        } else {
            for (int e = 0; e < 4; ++e) {
                const int64_t f = f0 + e;
                if (f >= n) break;
                const int64_t img = f / chw, i = f - img * chw;
                const int w = (int)(i % W), h = (int)((i / W) % H);
                const float* p = x + img * xbs + i;
                const float y = post(*p, mul, add, lo, hi);
                const float d = y - mean_img[i];
                sq += d * d;
                if (h + 1 < H) tv += fabsf(post(p[W], mul, add, lo, hi) - y);
                if (w + 1 < W) tv += fabsf(post(p[1], mul, add, lo, hi) - y);
            }
        }
    }
    sq = block_sum_256(sq, red);
    tv = block_sum_256(tv, red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = sq;
        partial[MAXP + blockIdx.x] = tv;
    }
}

__global__ __launch_bounds__(256) void image_set_finish_kernel(const float* __restrict__ partial, int n_partial, float* __restrict__ stats) {
    __shared__ double red[256];
    const double a = block_sum_partials(partial, n_partial, red);
    const double b = block_sum_partials(partial + MAXP, n_partial, red);
    if (threadIdx.x == 0) {
        stats[0] = (float)a;
        stats[1] = (float)b;
    }
}

// ---- streaming merge of image-set statistics (defense_ldm.py) ----------------------------------------------------------------------------------
// Chan et al.'s pairwise update of (mean image, sum of squared deviations): delta = mean_b - mean_a, mean_a += delta * n_b / n (in double, rounded
// once), partial[block] = the block's sum of delta^2.  Every term is added in double, a thread's items in index order, the threads of a block by
// the fixed tree, the blocks in index order by the finish kernel: no atomics, a repeat is bit-identical.  copy: n_a == 0, a becomes b.
template <bool VEC>
__global__ __launch_bounds__(256) void image_set_merge_kernel(float* __restrict__ mean_a, const float* __restrict__ mean_b,
                                                               double* __restrict__ partial, int64_t chw, double wb, bool copy) {
    __shared__ double red[256];
    double acc = 0.0;
    ITEM_STRIDE(q, (chw + 3) >> 2) {
        const int64_t f0 = q << 2;
        if (VEC) {                                       // chw % 4 == 0: every item is whole
            const f32x4 a = *reinterpret_cast<const f32x4*>(mean_a + f0);
            const f32x4 b = *reinterpret_cast<const f32x4*>(mean_b + f0);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)b[e] - (double)a[e];
                acc += d * d;
                o[e] = copy ? b[e] : (float)((double)a[e] + d * wb);
            }
            *reinterpret_cast<f32x4*>(mean_a + f0) = o;
        } else {
            for (int e = 0; e < 4; ++e) {
                const int64_t f = f0 + e;
                if (f >= chw) break;
                const float a = mean_a[f], b = mean_b[f];
                const double d = (double)b - (double)a;
                acc += d * d;
                mean_a[f] = copy ? b : (float)((double)a + d * wb);
            }
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void image_set_merge_finish_kernel(const double* __restrict__ partial, int n_partial, double between,
                                                                      float* __restrict__ stats_a, const float* __restrict__ stats_b, bool copy) {
    __shared__ double red[256];
    double s = 0.0;
    for (int k = threadIdx.x; k < n_partial; k += 256) s += partial[k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (copy) {
            stats_a[0] = stats_b[0];
            stats_a[1] = stats_b[1];
        } else {
            stats_a[0] = (float)((double)stats_a[0] + (double)stats_b[0] + between * red[0]);
            stats_a[1] = (float)((double)stats_a[1] + (double)stats_b[1]);
        }
    }
}

// ---- trigger-inversion objective of a score network (defense_ve.py) -----------------------------------------------------------------------------
// The VE counterpart of vd_trigger_inv_objective, in noise-prediction units: n[b] = -sigma * s[b],  r = mean_b n[b] - lambda * tau,  L = ||r||_2.
// Phase 1: r[i] (the batch sum in double: B is not bounded) parked in dtau, partial[block] = the block's sum of r^2.  Phase 2: every block adds the
// partials in index order (the same value in every block and in every run), then dout[b][i] = sigma * dL/ds[b][i] = -sigma^2 r / (B L) for every
// b and dtau[i] = -lambda r / L.  L = 0: zero gradients.
__global__ __launch_bounds__(256) void score_inv_residual_kernel(const float* __restrict__ s, const float* __restrict__ tau, float* __restrict__ r,
                                                                  float* __restrict__ partial, int B, int64_t n, int64_t s_bstride, float sigma,
                                                                  float lambda) {
    __shared__ float red[4];
    float acc = 0.f;
    ITEM_STRIDE(i, n) {
        double m = 0.0;
        for (int b = 0; b < B; ++b) m += (double)s[(int64_t)b * s_bstride + i];
        const float v = (float)(-(double)sigma * m / (double)B) - lambda * tau[i];
        r[i] = v;
        acc += v * v;
    }
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void score_inv_grad_kernel(const float* __restrict__ partial, int n_partial, float* __restrict__ loss,
                                                              float* __restrict__ dout, float* __restrict__ dtau, int B, int64_t n, float sigma,
                                                              float lambda) {
    __shared__ float Ls;
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < n_partial; ++k) t += (double)partial[k];
        Ls = (float)sqrt(t);
    }
    __syncthreads();
    const float L = Ls;
    const float inv = L > 0.f ? 1.0f / L : 0.f;
    const float cb = -(sigma * sigma) * (inv / (float)B);
    if (blockIdx.x == 0 && threadIdx.x == 0) *loss = L;
    ITEM_STRIDE(i, n) {
        const float v = dtau[i];
        const float gv = v * cb;
        for (int b = 0; b < B; ++b) dout[(int64_t)b * n + i] = gv;
        dtau[i] = -lambda * (v * inv);
    }
}


// ---- Adversarial Neuron Pruning (anp.py): neuron-scaled weights, mask gradients and the projected step -------------------------------------------
// A NEURON TABLE has one job of six int64 per selected weight tensor: {weight offset in floats, rows, row length, bias offset or -1, index of the
// layer's first neuron, first workgroup}.  A workgroup is four waves and a wave owns one row: workgroup b of a job holds rows [4b, 4b + 4).  A row
// is walked in ITEMS of four consecutive floats counted from the row's start; item q belongs to lane q % 64.  Where the row's start is 16-byte
// aligned in every buffer a whole item is one f32x4 access, otherwise (conv_in's 27-float rows, a base pointer off alignment) four scalar ones:
// which lane owns an element and the order it is used in do not depend on that choice.
constexpr int NJ = 6;

__device__ __forceinline__ const int64_t* neuron_job(const int64_t* __restrict__ table, int n_jobs) {
    int lo = 0, hi = n_jobs - 1;
    const int64_t blk = blockIdx.x;
    while (lo < hi) {                                            // last job whose first workgroup <= blk (block-uniform)
        const int mid = (lo + hi + 1) >> 1;
        if (table[(int64_t)NJ * mid + 5] <= blk) lo = mid; else hi = mid - 1;
    }
    return table + (int64_t)NJ * lo;
}

__global__ __launch_bounds__(256) void neuron_scale_kernel(const float* __restrict__ w0, float* __restrict__ w, const int64_t* __restrict__ table,
                                                            int n_jobs, const float* __restrict__ mask, const float* __restrict__ delta,
                                                            const float* __restrict__ xi) {
    const int64_t* __restrict__ t = neuron_job(table, n_jobs);
    const int64_t rows = t[1], len = t[2], boff = t[3];
    const int64_t row = (blockIdx.x - t[5]) * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int64_t j = t[4] + row;
    float s = mask[j];
    if (delta) s = s + delta[j];
    const float* __restrict__ src = w0 + t[0] + row * len;
    float* __restrict__ dst = w + t[0] + row * len;
    const bool vec = aligned16(src) && aligned16(dst);
    const int64_t items = (len + 3) >> 2;
    for (int64_t q = lane; q < items; q += 64) {
        const int64_t k0 = q << 2;
        if (vec && k0 + 4 <= len) {
            f32x4 v = *reinterpret_cast<const f32x4*>(src + k0);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = s * v[e];
            *reinterpret_cast<f32x4*>(dst + k0) = v;
        } else {
            for (int e = 0; e < 4 && k0 + e < len; ++e) dst[k0 + e] = s * src[k0 + e];
        }
    }
    if (lane == 0 && boff >= 0) {
        const float b = w0[boff + row];
        w[boff + row] = xi ? (1.0f + xi[j]) * b : b;
    }
}

// One wave per row.  A lane keeps one partial sum per position e of its items (four chains of ceil(items / 64) products each, items in index order),
// adds them as (a0 + a1) + (a2 + a3), and the 64 lanes are added by the xor tree of wave_sum: a fixed order, and no chain longer than
// len / 256 + 8 additions.
__global__ __launch_bounds__(256) void neuron_grad_kernel(const float* __restrict__ g, const float* __restrict__ w0, const int64_t* __restrict__ table,
                                                           int n_jobs, float* __restrict__ gmask, float* __restrict__ gxi, float scale,
                                                           int accumulate) {
    const int64_t* __restrict__ t = neuron_job(table, n_jobs);
    const int64_t rows = t[1], len = t[2], boff = t[3];
    const int64_t row = (blockIdx.x - t[5]) * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                     // wave-uniform: the shuffles below see whole waves
    const int lane = threadIdx.x & 63;
    const int64_t j = t[4] + row;
    const float* __restrict__ a = g + t[0] + row * len;
    const float* __restrict__ b = w0 + t[0] + row * len;
    const bool vec = aligned16(a) && aligned16(b);
    const int64_t items = (len + 3) >> 2;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int64_t q = lane; q < items; q += 64) {
        const int64_t k0 = q << 2;
        if (vec && k0 + 4 <= len) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(a + k0);
            const f32x4 y = *reinterpret_cast<const f32x4*>(b + k0);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += x[e] * y[e];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (k0 + e < len) acc[e] += a[k0 + e] * b[k0 + e];
        }
    }
    const float sum = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if (lane == 0) {
        const float v = scale * sum;
        gmask[j] = accumulate ? gmask[j] + v : v;
        if (gxi && boff >= 0) {
            const float u = scale * (g[boff + row] * w0[boff + row]);
            gxi[j] = accumulate ? gxi[j] + u : u;
        }
    }
}

// x = min(max(x - lr * d, lo), hi), every operation rounded on its own; d = the momentum buffer after buf = momentum * buf + g, or g, or
// sign(g) = (g > 0) - (g < 0) (0 for +-0 and NaN).
__global__ __launch_bounds__(256) void neuron_step_kernel(float* __restrict__ x, const float* __restrict__ g, float* __restrict__ buf, int64_t n,
                                                           float lr, float momentum, float lo, float hi, int use_sign) {
    ITEM_STRIDE(i, n) {
        float d = g[i];
        if (buf) {
            d = momentum * buf[i] + d;
            buf[i] = d;
        } else if (use_sign) {
            d = (float)(d > 0.f) - (float)(d < 0.f);
        }
        x[i] = fminf(fmaxf(x[i] - lr * d, lo), hi);
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int vd_score_inv_objective(const float* s, const float* tau, float sigma, float lambda, float* loss, float* dout, float* dtau,
                                      float* partial, int B, int64_t chw, int64_t s_bstride, void* stream) {
    VD_REQUIRE(s && tau && loss && dout && dtau && partial && B > 0 && chw > 0 && s_bstride >= chw, "vd_score_inv_objective: bad args");
    VD_REQUIRE(sigma > 0.f, "vd_score_inv_objective: sigma must be positive, got %g", (double)sigma);
    const int grid = item_grid(chw);
    hipLaunchKernelGGL(score_inv_residual_kernel, dim3(grid), dim3(256), 0, ST, s, tau, dtau, partial, B, chw, s_bstride, sigma, lambda);
    hipLaunchKernelGGL(score_inv_grad_kernel, dim3(grid), dim3(256), 0, ST, partial, grid, loss, dout, dtau, B, chw, sigma, lambda);
    VD_LAUNCH_CHECK("vd_score_inv_objective");
    return 0;
}

extern "C" int vd_removal_loss(const float* pred, const float* ref, float w_clean, float w_shift, float gscale, float* dpred, float* terms,
                               float* partial, int B, int64_t chw, int64_t pred_bstride, void* stream) {
    VD_REQUIRE(pred && ref && dpred && terms && partial && B > 0 && chw > 0 && pred_bstride >= chw, "vd_removal_loss: bad args");
    const int64_t n = (int64_t)B * chw;
    const int grid = item_grid((n + 3) >> 2);
    // gscale * w * 2 / n in double, rounded once: a power-of-two gscale scales dpred exactly
    const float cc = (float)((double)gscale * (double)w_clean * 2.0 / (double)n);
    const float cs = (float)((double)gscale * (double)w_shift * 2.0 / (double)n);
    const bool vec = (chw % 4 == 0) && (pred_bstride % 4 == 0) && aligned16(pred) && aligned16(ref) && aligned16(dpred);
    if (vec)
        hipLaunchKernelGGL(removal_loss_kernel<true>, dim3(grid), dim3(256), 0, ST, pred, ref, dpred, partial, B, chw, pred_bstride, cc, cs);
    else
        hipLaunchKernelGGL(removal_loss_kernel<false>, dim3(grid), dim3(256), 0, ST, pred, ref, dpred, partial, B, chw, pred_bstride, cc, cs);
    hipLaunchKernelGGL(removal_loss_finish_kernel, dim3(1), dim3(256), 0, ST, partial, grid, 1.0 / (double)n, w_clean, w_shift, terms);
    VD_LAUNCH_CHECK("vd_removal_loss");
    return 0;
}

extern "C" int vd_image_set_stats(const float* x, int N, int C, int H, int W, int64_t x_bstride, float mul, float add, float lo, float hi,
                                  float* mean_img, float* stats, float* partial, void* stream) {
    VD_REQUIRE(x && mean_img && stats && partial && N > 0 && C > 0 && H > 0 && W > 0, "vd_image_set_stats: bad args");
    const int64_t chw = (int64_t)C * H * W;
    VD_REQUIRE(x_bstride >= chw, "vd_image_set_stats: batch stride %lld < C*H*W %lld", (long long)x_bstride, (long long)chw);
    const int mgrid = (int)((chw + MP - 1) / MP > 4096 ? 4096 : (chw + MP - 1) / MP);
    hipLaunchKernelGGL(image_set_mean_kernel, dim3(mgrid), dim3(256), 0, ST, x, mean_img, N, chw, x_bstride, mul, add, lo, hi);
    const int grid = item_grid(((int64_t)N * chw + 3) >> 2);
    const bool vec = (W % 4 == 0) && (x_bstride % 4 == 0) && aligned16(x) && aligned16(mean_img);
    if (vec)
        hipLaunchKernelGGL(image_set_dev_tv_kernel<true>, dim3(grid), dim3(256), 0, ST, x, mean_img, partial, N, H, W, chw, x_bstride, mul, add,
                           lo, hi);
    else
        hipLaunchKernelGGL(image_set_dev_tv_kernel<false>, dim3(grid), dim3(256), 0, ST, x, mean_img, partial, N, H, W, chw, x_bstride, mul, add,
                           lo, hi);
    hipLaunchKernelGGL(image_set_finish_kernel, dim3(1), dim3(256), 0, ST, partial, grid, stats);
    VD_LAUNCH_CHECK("vd_image_set_stats");
    return 0;
}

extern "C" int vd_image_set_merge(float* mean_a, float* stats_a, int64_t n_a, const float* mean_b, const float* stats_b, int64_t n_b, int64_t chw,
                                  float* partial, void* stream) {
    VD_REQUIRE(mean_a && stats_a && mean_b && stats_b && partial && n_a >= 0 && n_b > 0 && chw > 0, "vd_image_set_merge: bad args");
    VD_REQUIRE((((uintptr_t)partial) & 7) == 0, "vd_image_set_merge: partial must be 8-byte aligned (it holds doubles)");
    VD_REQUIRE(mean_a != mean_b && stats_a != stats_b, "vd_image_set_merge: a and b must not alias");
    const int grid = item_grid((chw + 3) >> 2);
    const double n = (double)n_a + (double)n_b;
    const double wb = (double)n_b / n, between = (double)n_a * (double)n_b / n;
    const bool copy = n_a == 0;
    double* pd = reinterpret_cast<double*>(partial);     // MAXP doubles in the 2 * MAXP floats
    if ((chw % 4 == 0) && aligned16(mean_a) && aligned16(mean_b))
        hipLaunchKernelGGL(image_set_merge_kernel<true>, dim3(grid), dim3(256), 0, ST, mean_a, mean_b, pd, chw, wb, copy);
    else
        hipLaunchKernelGGL(image_set_merge_kernel<false>, dim3(grid), dim3(256), 0, ST, mean_a, mean_b, pd, chw, wb, copy);
    hipLaunchKernelGGL(image_set_merge_finish_kernel, dim3(1), dim3(256), 0, ST, pd, grid, between, stats_a, stats_b, copy);
    VD_LAUNCH_CHECK("vd_image_set_merge");
    return 0;
}

extern "C" int vd_neuron_scale(const float* w0, float* w, const int64_t* table, int n_jobs, int64_t total_blocks, const float* mask,
                               const float* delta, const float* xi, void* stream) {
    VD_REQUIRE(w0 && w && table && mask && n_jobs > 0 && total_blocks > 0 && total_blocks < (1ll << 31), "vd_neuron_scale: bad args");
    VD_REQUIRE(w0 != w, "vd_neuron_scale: w must not be w0 (the base weights are read for every pass)");
    hipLaunchKernelGGL(neuron_scale_kernel, dim3((unsigned)total_blocks), dim3(256), 0, ST, w0, w, table, n_jobs, mask, delta, xi);
    VD_LAUNCH_CHECK("vd_neuron_scale");
    return 0;
}

extern "C" int vd_neuron_grad(const float* g, const float* w0, const int64_t* table, int n_jobs, int64_t total_blocks, float* gmask, float* gxi,
                              float scale, int accumulate, void* stream) {
    VD_REQUIRE(g && w0 && table && gmask && n_jobs > 0 && total_blocks > 0 && total_blocks < (1ll << 31), "vd_neuron_grad: bad args");
    hipLaunchKernelGGL(neuron_grad_kernel, dim3((unsigned)total_blocks), dim3(256), 0, ST, g, w0, table, n_jobs, gmask, gxi, scale, accumulate);
    VD_LAUNCH_CHECK("vd_neuron_grad");
    return 0;
}

extern "C" int vd_neuron_step(float* x, const float* g, float* buf, int64_t n, float lr, float momentum, float lo, float hi, int use_sign,
                              void* stream) {
    VD_REQUIRE(x && g && n > 0 && lo <= hi, "vd_neuron_step: bad args");
    hipLaunchKernelGGL(neuron_step_kernel, dim3(item_grid(n)), dim3(256), 0, ST, x, g, buf, n, lr, momentum, lo, hi, use_sign);
    VD_LAUNCH_CHECK("vd_neuron_step");
    return 0;
}
