// HBM-bound elementwise / reduction kernels of the hot path:
//   K3  timestep embedding, SiLU          K8  q-sample + backdoor shift + target, MSE fwd+bwd
//   K9  global grad norm + clip + Adam    K10 sampler step (+ Philox4x32-10 noise), post-processing
//   K11 trigger stamping (poison_batch)   plus strided add / scale / lincomb helpers.
// Where the reference's arithmetic is a short torch op sequence (q-sample, scheduler step, normalisation) every
// product and sum is rounded individually (__fmul_rn/__fadd_rn, no FMA contraction) so that the results are
// bit-identical to that sequence on the CPU oracle.
#include "vd_common.h"

namespace {

constexpr int EB = 256;
inline int egrid(int64_t n, int per_thread = 1) {
    int64_t g = (n + (int64_t)EB * per_thread - 1) / ((int64_t)EB * per_thread);
    return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));  // cap + grid-stride (cdna guide G11)
}
#define GRID_STRIDE(i, n) \
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub_rn(float a, float b) { return __fsub_rn(a, b); }

// ---- K3 ----------------------------------------------------------------------------------------------------------
__global__ void temb_kernel(const float* __restrict__ t, const float* __restrict__ freqs, float* __restrict__ emb, int B,
                            int half, int flip) {
    GRID_STRIDE(i, (int64_t)B * half) {
        const int b = (int)(i / half), k = (int)(i - (int64_t)b * half);
        const float a = mul_rn(t[b], freqs[k]);
        const float sn = sinf(a), cs = cosf(a);
        float* e = emb + (int64_t)b * 2 * half;
        e[flip ? half + k : k] = sn;
        e[flip ? k : half + k] = cs;
    }
}

__global__ void silu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n) {
    GRID_STRIDE(i, n) {
        const float z = x[i];
        y[i] = z * sigmoidf_(z);
    }
}
__global__ void silu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx, int64_t n,
                                int accumulate) {
    GRID_STRIDE(i, n) {
        const float z = x[i], sg = sigmoidf_(z);
        const float g = dy[i] * sg * (1.f + z * (1.f - sg));
        dx[i] = accumulate ? dx[i] + g : g;
    }
}

__global__ void add_strided_kernel(float* __restrict__ dst, const float* __restrict__ src, int B, int64_t inner4,
                                   int64_t dst_bs, int64_t src_bs, int accumulate) {
    GRID_STRIDE(i, (int64_t)B * inner4) {
        const int b = (int)(i / inner4);
        const int64_t r = i - (int64_t)b * inner4;
        f32x4* d = reinterpret_cast<f32x4*>(dst + (int64_t)b * dst_bs) + r;
        const f32x4 s = *(reinterpret_cast<const f32x4*>(src + (int64_t)b * src_bs) + r);
        *d = accumulate ? (*d + s) : s;
    }
}
__global__ void add_strided_scalar_kernel(float* __restrict__ dst, const float* __restrict__ src, int B, int64_t inner,
                                          int64_t dst_bs, int64_t src_bs, int accumulate) {
    GRID_STRIDE(i, (int64_t)B * inner) {
        const int b = (int)(i / inner);
        const int64_t r = i - (int64_t)b * inner;
        float* d = dst + (int64_t)b * dst_bs + r;
        const float s = src[(int64_t)b * src_bs + r];
        *d = accumulate ? (*d + s) : s;
    }
}

__global__ void scale_kernel(float* __restrict__ x, int64_t n, float alpha) {
    GRID_STRIDE(i, n) x[i] = (alpha == 0.f) ? 0.f : x[i] * alpha;
}

struct LinArgs {
    const float* src[6];
    float coef[6];
    int n_src;
};
__global__ void lincomb_kernel(float* __restrict__ out, LinArgs a, int64_t n) {
    GRID_STRIDE(i, n) {
        float acc = mul_rn(a.coef[0], a.src[0][i]);
        for (int k = 1; k < a.n_src; ++k) acc = add_rn(acc, mul_rn(a.coef[k], a.src[k][i]));
        out[i] = acc;
    }
}

// ---- K8 ----------------------------------------------------------------------------------------------------------
__global__ void qsample_kernel(const float* __restrict__ x0, const float* __restrict__ R, const float* __restrict__ eps,
                               const int64_t* __restrict__ t, const float* __restrict__ tab_a, const float* __restrict__ tab_s,
                               const float* __restrict__ tab_step, const float* __restrict__ tab_coef, float* __restrict__ x_t,
                               float* __restrict__ y, int B, int64_t chw) {
    GRID_STRIDE(i, (int64_t)B * chw) {
        const int b = (int)(i / chw);
        const int64_t tt = t[b];
        const float a = tab_a ? tab_a[tt] : 1.0f, s = tab_s[tt], st = tab_step[tt], cf = tab_coef[tt];
        const float xv = x0[i], rv = R[i], ev = eps[i];
        const float noisy = tab_a ? add_rn(mul_rn(a, xv), mul_rn(s, ev)) : add_rn(xv, mul_rn(s, ev));
        x_t[i] = add_rn(noisy, mul_rn(st, rv));
        y[i] = add_rn(mul_rn(cf, rv), ev);
    }
}

// partial[block] = sum over the block's elements of norm(pred*ps - y); also writes dpred = gcoef * norm'(d) * ps.
// KIND 0: F.mse_loss (d^2; gcoef carries the factor 2), 1: F.l1_loss (|d|, gradient sign(d) with sign(0) = 0),
// 2: F.smooth_l1_loss with beta = 1 (0.5 d^2 inside |d| < 1, |d| - 0.5 outside)  -- loss.py:849-858.
template <int KIND>
__global__ __launch_bounds__(256) void mse_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                  const float* __restrict__ pscale, float* __restrict__ dpred,
                                                  float* __restrict__ partial, int B, int64_t chw, float gcoef) {
    __shared__ float red[4];
    float s = 0.f;
    GRID_STRIDE(i, (int64_t)B * chw) {
        const float ps = pscale ? pscale[i / chw] : 1.0f;
        const float d = pred[i] * ps - y[i];
        float v, g;
        if (KIND == 0) {
            v = d * d;
            g = d;
        } else if (KIND == 1) {
            v = fabsf(d);
            g = (d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f);
        } else {
            const float a = fabsf(d);
            v = (a < 1.f) ? 0.5f * d * d : a - 0.5f;
            g = (a < 1.f) ? d : ((d > 0.f) ? 1.f : -1.f);
        }
        s += v;
        if (dpred) dpred[i] = gcoef * g * ps;
    }
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void finish_sum_kernel(const float* __restrict__ partial, int n, float scale,
                                                         float* __restrict__ out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) *out = s * scale;
}

// ---- K9 ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ partial) {
    __shared__ float red[4];
    float s = 0.f;
    const int64_t n4 = n >> 2;
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    GRID_STRIDE(i, n4) {
        const f32x4 v = g4[i];
        s += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    if (blockIdx.x == 0)
        for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) s += g[i] * g[i];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// One element of torch.optim.Adam's update on the clipped, unscaled gradient g * gs: the arithmetic adam_kernel and adam_ema_kernel share, so that
// p / m / v come out of both with the same bits.
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float gs, float beta1, float beta2, float eps,
                                            float step_size, float bc2_sqrt) {
    const float gr = g * gs;
    m = m + (gr - m) * (1.f - beta1);          // exp_avg.lerp_(grad, 1-beta1)
    v = v * beta2 + (1.f - beta2) * gr * gr;   // exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2)
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = p - step_size * (m / denom);
}

// The gradient scale of this step -- 1/world, the loss scale and torch.nn.utils.clip_grad_norm_'s coefficient (max_norm/(norm+1e-6), clamped
// to 1) folded --, or false: the step is skipped.
// A non-finite gradient (f16 mixed-precision mode: an operand overflowed under the loss scale) skips the whole update, as
// torch.cuda.amp.GradScaler.step does (reference VillanDiffusion.py:260-264 -> accelerate); the skip is COUNTED (one writer: thread 0 of
// block 0) so that the host sees every skipped step at its next lazy check, not only the one the check happens to land on
__device__ __forceinline__ bool adam_grad_scale(const float* __restrict__ norm_sq, float max_norm, float inv_scale,
                                                unsigned* __restrict__ skipped, float& gs) {
    gs = inv_scale;
    if (norm_sq) {
        if (!(*norm_sq <= 3.0e38f)) {
            if (skipped && blockIdx.x == 0 && threadIdx.x == 0) *skipped += 1u;
            return false;
        }
        const float norm = sqrtf(*norm_sq) * inv_scale;
        gs *= fminf(1.0f, max_norm / (norm + 1e-6f));
    }
    return true;
}

// torch.nn.utils.clip_grad_norm_ fused into torch.optim.Adam's update.
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n, const float* __restrict__ norm_sq,
                                                   float max_norm, float inv_scale, float lr, float beta1, float beta2,
                                                   float eps, float bc1, float bc2_sqrt, unsigned* __restrict__ skipped) {
    float gs;
    if (!adam_grad_scale(norm_sq, max_norm, inv_scale, skipped, gs)) return;
    const float step_size = lr / bc1;
    const int64_t n4 = n >> 2;
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    f32x4* m4 = reinterpret_cast<f32x4*>(m);
    f32x4* v4 = reinterpret_cast<f32x4*>(v);
    GRID_STRIDE(i, n4) {
        f32x4 pv = p4[i], gv = g4[i], mv = m4[i], vv = v4[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = pv[j], mj = mv[j], vj = vv[j];
            adam_update(pj, gv[j], mj, vj, gs, beta1, beta2, eps, step_size, bc2_sqrt);
            pv[j] = pj;
            mv[j] = mj;
            vv[j] = vj;
        }
        p4[i] = pv;
        m4[i] = mv;
        v4[i] = vv;
    }
    if (blockIdx.x == 0)
        for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) adam_update(p[i], g[i], m[i], v[i], gs, beta1, beta2, eps, step_size, bc2_sqrt);
}

// adam_kernel plus the exponential moving average of the updated parameters in the same pass (diffusers EMAModel.step:
// shadow.sub_((1 - decay) * (shadow - param)), signs folded: the same bits): ema += (p_new - ema) * one_minus_decay, three individually rounded
// operations.  A skipped step leaves ema alone too.  5 f32x4 loads + 4 f32x4 stores per item (36 B/parameter; adam_kernel: 28).
__global__ __launch_bounds__(256) void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, float* __restrict__ ema, int64_t n,
                                                       const float* __restrict__ norm_sq, float max_norm, float inv_scale, float lr,
                                                       float beta1, float beta2, float eps, float bc1, float bc2_sqrt,
                                                       float one_minus_decay, unsigned* __restrict__ skipped) {
    float gs;
    if (!adam_grad_scale(norm_sq, max_norm, inv_scale, skipped, gs)) return;
    const float step_size = lr / bc1;
    const int64_t n4 = n >> 2;
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    f32x4* m4 = reinterpret_cast<f32x4*>(m);
    f32x4* v4 = reinterpret_cast<f32x4*>(v);
    f32x4* e4 = reinterpret_cast<f32x4*>(ema);
    GRID_STRIDE(i, n4) {
        f32x4 pv = p4[i], gv = g4[i], mv = m4[i], vv = v4[i], ev = e4[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = pv[j], mj = mv[j], vj = vv[j];
            adam_update(pj, gv[j], mj, vj, gs, beta1, beta2, eps, step_size, bc2_sqrt);
            pv[j] = pj;
            mv[j] = mj;
            vv[j] = vj;
            ev[j] = add_rn(ev[j], mul_rn(sub_rn(pj, ev[j]), one_minus_decay));
        }
        p4[i] = pv;
        m4[i] = mv;
        v4[i] = vv;
        e4[i] = ev;
    }
    if (blockIdx.x == 0)
        for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
            adam_update(p[i], g[i], m[i], v[i], gs, beta1, beta2, eps, step_size, bc2_sqrt);
            ema[i] = add_rn(ema[i], mul_rn(sub_rn(p[i], ema[i]), one_minus_decay));
        }
}

// a <-> b in place: bits move, nothing is rounded (NaN payloads included).  VEC: f32x4 items plus block 0's scalar tail; else scalar throughout.
template <bool VEC>
__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n) {
    if (VEC) {
        const int64_t n4 = n >> 2;
        uint4* a4 = reinterpret_cast<uint4*>(a);
        uint4* b4 = reinterpret_cast<uint4*>(b);
        GRID_STRIDE(i, n4) {
            const uint4 x = a4[i], y = b4[i];
            a4[i] = y;
            b4[i] = x;
        }
        if (blockIdx.x == 0) {
            uint32_t* au = reinterpret_cast<uint32_t*>(a);
            uint32_t* bu = reinterpret_cast<uint32_t*>(b);
            for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
                const uint32_t x = au[i], y = bu[i];
                au[i] = y;
                bu[i] = x;
            }
        }
    } else {
        uint32_t* au = reinterpret_cast<uint32_t*>(a);
        uint32_t* bu = reinterpret_cast<uint32_t*>(b);
        GRID_STRIDE(i, n) {
            const uint32_t x = au[i], y = bu[i];
            au[i] = y;
            bu[i] = x;
        }
    }
}

// ---- Philox4x32-10 + Box-Muller -------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
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
// 4 standard normals for counter value `ctr`
__device__ __forceinline__ void randn4(uint64_t seed, uint64_t ctr, float (&z)[4]) {
    uint32_t r[4];
    philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const float k = 2.3283064365386963e-10f;  // 2^-32
    const float u0 = ((float)r[0] + 0.5f) * k, u1 = ((float)r[1] + 0.5f) * k;
    const float u2 = ((float)r[2] + 0.5f) * k, u3 = ((float)r[3] + 0.5f) * k;
    const float ra = sqrtf(-2.f * __logf(fminf(u0, 0.99999994f) + 1e-12f)), rb = sqrtf(-2.f * __logf(fminf(u2, 0.99999994f) + 1e-12f));
    float s, c;
    __sincosf(6.283185307179586f * u1, &s, &c);
    z[0] = ra * c;
    z[1] = ra * s;
    __sincosf(6.283185307179586f * u3, &s, &c);
    z[2] = rb * c;
    z[3] = rb * s;
}

__global__ void randn_kernel(float* __restrict__ out, int64_t n, uint64_t seed, uint64_t offset) {
    GRID_STRIDE(q, (n + 3) >> 2) {
        float z[4];
        randn4(seed, offset + (uint64_t)q, z);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q * 4 + j < n) out[q * 4 + j] = z[j];
    }
}

// ---- K10 ---------------------------------------------------------------------------------------------------------
struct StepCoef {
    float c_eps, c_div, clip, c_x0, c_x, c_e, c_z;
};
__global__ void sched_step_kernel(const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ z,
                                  float* __restrict__ out, float* __restrict__ x0_out, int64_t n, StepCoef k, uint64_t seed,
                                  uint64_t offset) {
    GRID_STRIDE(q, (n + 3) >> 2) {
        float zz[4] = {0.f, 0.f, 0.f, 0.f};
        if (k.c_z != 0.f && !z) randn4(seed, offset + (uint64_t)q, zz);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t i = q * 4 + j;
            if (i >= n) break;
            const float xv = x[i], ev = eps[i];
            float x0 = sub_rn(xv, mul_rn(k.c_eps, ev)) / k.c_div;
            if (k.clip > 0.f) x0 = fminf(fmaxf(x0, -k.clip), k.clip);
            float o = add_rn(mul_rn(k.c_x0, x0), mul_rn(k.c_x, xv));
            if (k.c_e != 0.f) o = add_rn(o, mul_rn(k.c_e, ev));
            if (k.c_z != 0.f) o = add_rn(o, mul_rn(k.c_z, z ? z[i] : zz[j]));
            out[i] = o;
            if (x0_out) x0_out[i] = x0;
        }
    }
}

// one workgroup per sample: deterministic block reduction
__global__ __launch_bounds__(256) void batch_l2norm_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t inner) {
    __shared__ float red[4];
    const float* __restrict__ xb = x + (int64_t)blockIdx.x * inner;
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < inner; i += 256) s += xb[i] * xb[i];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = sqrtf(s);
}

__global__ void postprocess_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int C, int HW, float mul,
                                   float add, float lo, float hi, int to_nhwc) {
    GRID_STRIDE(i, (int64_t)B * C * HW) {
        const float v = fminf(fmaxf(add_rn(mul_rn(x[i], mul), add), lo), hi);
        if (to_nhwc) {
            const int p = (int)(i % HW);
            const int64_t bc = i / HW;
            const int c = (int)(bc % C);
            const int64_t b = bc / C;
            out[(b * HW + p) * C + c] = v;
        } else {
            out[i] = v;
        }
    }
}

// ---- K11 ---------------------------------------------------------------------------------------------------------
__global__ void poison_kernel(const uint8_t* __restrict__ img, const int64_t* __restrict__ idx, const uint8_t* __restrict__ flags,
                              const float* __restrict__ trigger, const float* __restrict__ target, float* __restrict__ pv,
                              float* __restrict__ tg, float* __restrict__ image_out, int B, int C, int H, int W, float vmin,
                              float vmax, float denom, int r_trigger_only) {
    const int64_t chw = (int64_t)C * H * W;
    GRID_STRIDE(i, (int64_t)B * chw) {
        const int b = (int)(i / chw);
        const int64_t r = i - (int64_t)b * chw;
        const int xw = (int)(r % W);
        const int64_t cy = r / W;
        const int yh = (int)(cy % H), c = (int)(cy / H);
        const uint8_t f = flags[b];
        const int xs = (f & 2) ? (W - 1 - xw) : xw;
        const int64_t sb = idx ? idx[b] : (int64_t)b;
        const float u = (float)img[((sb * H + yh) * W + xs) * C + c] / 255.0f;                     // ToTensor
        const float xv = add_rn(mul_rn(sub_rn(u, 0.0f) / denom, sub_rn(vmax, vmin)), vmin);        // util.normalize
        if (image_out) image_out[i] = xv;
        if (f & 1) {
            const float tr = trigger[r];
            pv[i] = r_trigger_only ? tr : ((tr > vmin) ? tr : xv);
            tg[i] = target[r];
        } else {
            pv[i] = 0.f;
            tg[i] = xv;
        }
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int vd_timestep_embedding(const float* t, const float* freqs, float* emb, int B, int half, int flip_sin_to_cos,
                                     void* stream) {
    VD_REQUIRE(t && freqs && emb && B > 0 && half > 0, "vd_timestep_embedding: bad args");
    hipLaunchKernelGGL(temb_kernel, dim3(egrid((int64_t)B * half)), dim3(EB), 0, ST, t, freqs, emb, B, half, flip_sin_to_cos);
    VD_LAUNCH_CHECK("vd_timestep_embedding");
    return 0;
}

extern "C" int vd_silu_fwd(const float* x, float* y, int64_t n, void* stream) {
    VD_REQUIRE(x && y && n > 0, "vd_silu_fwd: bad args");
    hipLaunchKernelGGL(silu_fwd_kernel, dim3(egrid(n)), dim3(EB), 0, ST, x, y, n);
    VD_LAUNCH_CHECK("vd_silu_fwd");
    return 0;
}

extern "C" int vd_silu_bwd(const float* dy, const float* x, float* dx, int64_t n, int accumulate, void* stream) {
    VD_REQUIRE(dy && x && dx && n > 0, "vd_silu_bwd: bad args");
    hipLaunchKernelGGL(silu_bwd_kernel, dim3(egrid(n)), dim3(EB), 0, ST, dy, x, dx, n, accumulate);
    VD_LAUNCH_CHECK("vd_silu_bwd");
    return 0;
}

extern "C" int vd_add_strided(float* dst, const float* src, int B, int64_t inner, int64_t dst_bstride, int64_t src_bstride,
                              int accumulate, void* stream) {
    VD_REQUIRE(dst && src && B > 0 && inner > 0, "vd_add_strided: bad args");
    const bool vec = ((inner & 3) == 0) && ((dst_bstride & 3) == 0) && ((src_bstride & 3) == 0) &&
                     ((((uintptr_t)dst) & 15) == 0) && ((((uintptr_t)src) & 15) == 0);
    if (vec)
        hipLaunchKernelGGL(add_strided_kernel, dim3(egrid((int64_t)B * inner / 4)), dim3(EB), 0, ST, dst, src, B, inner / 4,
                           dst_bstride, src_bstride, accumulate);
    else
        hipLaunchKernelGGL(add_strided_scalar_kernel, dim3(egrid((int64_t)B * inner)), dim3(EB), 0, ST, dst, src, B, inner,
                           dst_bstride, src_bstride, accumulate);
    VD_LAUNCH_CHECK("vd_add_strided");
    return 0;
}

extern "C" int vd_scale(float* x, int64_t n, float alpha, void* stream) {
    VD_REQUIRE(x && n > 0, "vd_scale: bad args");
    hipLaunchKernelGGL(scale_kernel, dim3(egrid(n, 4)), dim3(EB), 0, ST, x, n, alpha);
    VD_LAUNCH_CHECK("vd_scale");
    return 0;
}

extern "C" int vd_lincomb(float* out, const float* const* srcs, const float* coefs, int n_src, int64_t n, void* stream) {
    VD_REQUIRE(out && srcs && coefs && n_src >= 1 && n_src <= 6 && n > 0, "vd_lincomb: bad args (n_src=%d)", n_src);
    LinArgs a;
    for (int i = 0; i < 6; ++i) {
        a.src[i] = i < n_src ? srcs[i] : nullptr;
        a.coef[i] = i < n_src ? coefs[i] : 0.f;
    }
    a.n_src = n_src;
    for (int i = 0; i < n_src; ++i) VD_REQUIRE(a.src[i] != nullptr, "vd_lincomb: null source %d", i);
    hipLaunchKernelGGL(lincomb_kernel, dim3(egrid(n)), dim3(EB), 0, ST, out, a, n);
    VD_LAUNCH_CHECK("vd_lincomb");
    return 0;
}

extern "C" int vd_qsample_backdoor(const float* x0, const float* R, const float* eps, const int64_t* t, const float* tab_a,
                                   const float* tab_s, const float* tab_step, const float* tab_coef, float* x_t, float* y, int B,
                                   int64_t chw, void* stream) {
    VD_REQUIRE(x0 && R && eps && t && tab_s && tab_step && tab_coef && x_t && y, "vd_qsample_backdoor: null pointer");
    VD_REQUIRE(B > 0 && chw > 0, "vd_qsample_backdoor: bad dims");
    hipLaunchKernelGGL(qsample_kernel, dim3(egrid((int64_t)B * chw)), dim3(EB), 0, ST, x0, R, eps, t, tab_a, tab_s, tab_step,
                       tab_coef, x_t, y, B, chw);
    VD_LAUNCH_CHECK("vd_qsample_backdoor");
    return 0;
}

extern "C" int vd_loss_fwd_bwd(const float* pred, const float* y, const float* pscale, float* dpred, float* loss, float* partial,
                               int B, int64_t chw, float gscale, int kind, void* stream) {
    VD_REQUIRE(pred && y && loss && partial && B > 0 && chw > 0, "vd_loss_fwd_bwd: bad args");
    VD_REQUIRE(kind >= VD_LOSS_L2 && kind <= VD_LOSS_HUBER, "vd_loss_fwd_bwd: kind %d (0 = l2, 1 = l1, 2 = huber)", kind);
    const int64_t n = (int64_t)B * chw;
    int grid = egrid(n);
    if (grid > 1024) grid = 1024;
    const float gcoef = (kind == VD_LOSS_L2 ? 2.0f : 1.0f) * gscale / (float)n;
    if (kind == VD_LOSS_L2)
        hipLaunchKernelGGL(mse_kernel<0>, dim3(grid), dim3(256), 0, ST, pred, y, pscale, dpred, partial, B, chw, gcoef);
    else if (kind == VD_LOSS_L1)
        hipLaunchKernelGGL(mse_kernel<1>, dim3(grid), dim3(256), 0, ST, pred, y, pscale, dpred, partial, B, chw, gcoef);
    else
        hipLaunchKernelGGL(mse_kernel<2>, dim3(grid), dim3(256), 0, ST, pred, y, pscale, dpred, partial, B, chw, gcoef);
    hipLaunchKernelGGL(finish_sum_kernel, dim3(1), dim3(256), 0, ST, partial, grid, 1.0f / (float)n, loss);
    VD_LAUNCH_CHECK("vd_loss_fwd_bwd");
    return 0;
}

extern "C" int vd_mse_fwd_bwd(const float* pred, const float* y, const float* pscale, float* dpred, float* loss, float* partial,
                              int B, int64_t chw, float gscale, void* stream) {
    return vd_loss_fwd_bwd(pred, y, pscale, dpred, loss, partial, B, chw, gscale, VD_LOSS_L2, stream);
}

extern "C" int vd_l2norm_sq(const float* g, int64_t n, float* partial, float* out_sq, void* stream) {
    VD_REQUIRE(g && partial && out_sq && n > 0 && ((((uintptr_t)g) & 15) == 0), "vd_l2norm_sq: bad args");
    int grid = egrid(n, 16);
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(sumsq_kernel, dim3(grid), dim3(256), 0, ST, g, n, partial);
    hipLaunchKernelGGL(finish_sum_kernel, dim3(1), dim3(256), 0, ST, partial, grid, 1.0f, out_sq);
    VD_LAUNCH_CHECK("vd_l2norm_sq");
    return 0;
}

// ---- trigger-inversion objective (defense.py): L = || mean_b e[b] - lambda * tau ||_2 over the C*H*W elements, and its gradients --------------
// Phase 1: r[i] = mean_b e[b][i] - lambda * tau[i] (the batch sum in double: B is not bounded), parked in dtau; partial[block] = the block's sum
// of r^2.  Phase 2: every block adds the partials in index order (the same value in every block and in every run: no atomics), then
// dout[b][i] = r / (B L) for every b and dtau[i] = -lambda r / L.  L = 0: zero gradients.
__global__ __launch_bounds__(256) void trigger_inv_residual_kernel(const float* __restrict__ e, const float* __restrict__ tau, float* __restrict__ r,
                                                                    float* __restrict__ partial, int B, int64_t n, int64_t e_bstride, float lambda) {
    __shared__ float red[4];
    float s = 0.f;
    GRID_STRIDE(i, n) {
        double m = 0.0;
        for (int b = 0; b < B; ++b) m += (double)e[(int64_t)b * e_bstride + i];
        const float v = (float)(m / (double)B) - lambda * tau[i];
        r[i] = v;
        s += v * v;
    }
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void trigger_inv_grad_kernel(const float* __restrict__ partial, int n_partial, float* __restrict__ loss,
                                                                float* __restrict__ dout, float* __restrict__ dtau, int B, int64_t n, float lambda) {
    __shared__ float Ls;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < n_partial; ++k) s += (double)partial[k];
        Ls = (float)sqrt(s);
    }
    __syncthreads();
    const float L = Ls;
    const float inv = L > 0.f ? 1.0f / L : 0.f;
    const float inv_b = inv / (float)B;
    if (blockIdx.x == 0 && threadIdx.x == 0) *loss = L;
    GRID_STRIDE(i, n) {
        const float v = dtau[i];
        const float g = v * inv_b;
        for (int b = 0; b < B; ++b) dout[(int64_t)b * n + i] = g;
        dtau[i] = -lambda * (v * inv);
    }
}

extern "C" int vd_trigger_inv_objective(const float* e, const float* tau, float lambda, float* loss, float* dout, float* dtau, float* partial,
                                        int B, int64_t chw, int64_t e_bstride, void* stream) {
    VD_REQUIRE(e && tau && loss && dout && dtau && partial && B > 0 && chw > 0 && e_bstride >= chw, "vd_trigger_inv_objective: bad args");
    int grid = egrid(chw);
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(trigger_inv_residual_kernel, dim3(grid), dim3(256), 0, ST, e, tau, dtau, partial, B, chw, e_bstride, lambda);
    hipLaunchKernelGGL(trigger_inv_grad_kernel, dim3(grid), dim3(256), 0, ST, partial, grid, loss, dout, dtau, B, chw, lambda);
    VD_LAUNCH_CHECK("vd_trigger_inv_objective");
    return 0;
}

extern "C" int vd_adam_step(float* p, const float* g, float* m, float* v, int64_t n, const float* norm_sq, float max_norm,
                            float inv_scale, float lr, float beta1, float beta2, float eps, int step, unsigned* skipped, void* stream) {
    VD_REQUIRE(p && g && m && v && n > 0 && step >= 1, "vd_adam_step: bad args");
    VD_REQUIRE(((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0, "vd_adam_step: unaligned");
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(adam_kernel, dim3(egrid(n, 8)), dim3(256), 0, ST, p, g, m, v, n, norm_sq, max_norm, inv_scale, lr, beta1,
                       beta2, eps, (float)bc1, (float)sqrt(bc2), skipped);
    VD_LAUNCH_CHECK("vd_adam_step");
    return 0;
}

extern "C" int vd_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* norm_sq, float max_norm,
                                float inv_scale, float lr, float beta1, float beta2, float eps, int step, float one_minus_decay,
                                unsigned* skipped, void* stream) {
    VD_REQUIRE(p && g && m && v && ema && n > 0 && step >= 1, "vd_adam_ema_step: bad args");
    VD_REQUIRE(one_minus_decay >= 0.f && one_minus_decay <= 1.f, "vd_adam_ema_step: one_minus_decay %g outside [0, 1]", (double)one_minus_decay);
    VD_REQUIRE(((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v) | ((uintptr_t)ema)) & 15) == 0, "vd_adam_ema_step: unaligned");
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(adam_ema_kernel, dim3(egrid(n, 8)), dim3(256), 0, ST, p, g, m, v, ema, n, norm_sq, max_norm, inv_scale, lr, beta1,
                       beta2, eps, (float)bc1, (float)sqrt(bc2), one_minus_decay, skipped);
    VD_LAUNCH_CHECK("vd_adam_ema_step");
    return 0;
}

extern "C" int vd_swap(float* a, float* b, int64_t n, void* stream) {
    VD_REQUIRE(a && b && n > 0, "vd_swap: bad args");
    VD_REQUIRE(((((uintptr_t)a) | ((uintptr_t)b)) & 3) == 0, "vd_swap: pointers not 4-byte aligned");
    const uintptr_t lo = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)a : (uintptr_t)b, hi = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)b : (uintptr_t)a;
    VD_REQUIRE(hi - lo >= (uintptr_t)n * 4, "vd_swap: the two buffers overlap");
    if (((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0)
        hipLaunchKernelGGL(swap_kernel<true>, dim3(egrid(n, 8)), dim3(256), 0, ST, a, b, n);
    else
        hipLaunchKernelGGL(swap_kernel<false>, dim3(egrid(n, 2)), dim3(256), 0, ST, a, b, n);
    VD_LAUNCH_CHECK("vd_swap");
    return 0;
}

extern "C" int vd_sched_step(const float* x, const float* eps, const float* z, float* out, float* x0_out, int64_t n,
                             float c_eps, float c_div, float clip, float c_x0, float c_x, float c_e, float c_z, uint64_t seed,
                             uint64_t offset, void* stream) {
    VD_REQUIRE(x && eps && out && n > 0 && c_div != 0.f, "vd_sched_step: bad args");
    StepCoef k{c_eps, c_div, clip, c_x0, c_x, c_e, c_z};
    hipLaunchKernelGGL(sched_step_kernel, dim3(egrid((n + 3) / 4)), dim3(EB), 0, ST, x, eps, z, out, x0_out, n, k, seed, offset);
    VD_LAUNCH_CHECK("vd_sched_step");
    return 0;
}

extern "C" int vd_batch_l2norm(const float* x, float* out, int B, int64_t inner, void* stream) {
    VD_REQUIRE(x && out && B > 0 && inner > 0, "vd_batch_l2norm: bad args");
    hipLaunchKernelGGL(batch_l2norm_kernel, dim3(B), dim3(256), 0, ST, x, out, inner);
    VD_LAUNCH_CHECK("vd_batch_l2norm");
    return 0;
}

extern "C" int vd_postprocess(const float* x, float* out, int B, int C, int HW, float mul, float add, float lo, float hi,
                              int to_nhwc, void* stream) {
    VD_REQUIRE(x && out && B > 0 && C > 0 && HW > 0, "vd_postprocess: bad args");
    hipLaunchKernelGGL(postprocess_kernel, dim3(egrid((int64_t)B * C * HW)), dim3(EB), 0, ST, x, out, B, C, HW, mul, add, lo, hi,
                       to_nhwc);
    VD_LAUNCH_CHECK("vd_postprocess");
    return 0;
}

// ---- SSIM of image pairs (measure glue: torchmetrics StructuralSimilarityIndexMeasure(data_range), VillanDiffusion.py:1001-1007) ----
// One workgroup per image; a thread walks map positions (c, y, x), accumulates the five 11 x 11 gaussian-window sums with reflect indexing
// (the window of a kept position lies inside the image whenever H, W > 2 * 5: the reflect-padded border is cropped from the map), evaluates the
// SSIM expression and the workgroup averages its map in a fixed order.  win: the K x K window (outer product of the normalised 1-D gaussian).
__global__ __launch_bounds__(256) void ssim_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ win,
                                                    float* __restrict__ out, int C, int H, int W, int K, float c1, float c2) {
    __shared__ float wsh[32 * 32];
    __shared__ float red[4];
    const int n = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < K * K; i += 256) wsh[i] = win[i];
    __syncthreads();
    const int p = (K - 1) / 2;
    const bool crop = W > 2 * p && H > 2 * p;            // torchmetrics crops [p:-p] of both map dimensions when the map is larger than the border
    const int y0 = crop ? p : 0, x0 = crop ? p : 0, mh = crop ? H - 2 * p : H, mw = crop ? W - 2 * p : W;
    const int total = C * mh * mw;
    const float* __restrict__ an = a + (int64_t)n * C * H * W;
    const float* __restrict__ bn = b + (int64_t)n * C * H * W;
    float acc = 0.f;
    for (int i = tid; i < total; i += 256) {
        const int c = i / (mh * mw), r = i - c * mh * mw, y = y0 + r / mw, x = x0 + r % mw;
        const float* __restrict__ ac = an + (int64_t)c * H * W;
        const float* __restrict__ bc = bn + (int64_t)c * H * W;
        float sa = 0.f, sb = 0.f, saa = 0.f, sbb = 0.f, sab = 0.f;
        for (int dy = 0; dy < K; ++dy) {
            int yy = y + dy - p;
            yy = yy < 0 ? -yy : (yy >= H ? 2 * (H - 1) - yy : yy);
            for (int dx = 0; dx < K; ++dx) {
                int xx = x + dx - p;
                xx = xx < 0 ? -xx : (xx >= W ? 2 * (W - 1) - xx : xx);
                const float w = wsh[dy * K + dx], va = ac[yy * W + xx], vb = bc[yy * W + xx];
                sa += w * va;
                sb += w * vb;
                saa += w * (va * va);
                sbb += w * (vb * vb);
                sab += w * (va * vb);
            }
        }
        const float va_ = saa - sa * sa, vb_ = sbb - sb * sb, cab = sab - sa * sb;
        acc += ((2.f * sa * sb + c1) * (2.f * cab + c2)) / ((sa * sa + sb * sb + c1) * (va_ + vb_ + c2));
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) out[n] = ((red[0] + red[1]) + (red[2] + red[3])) / (float)total;
}

extern "C" int vd_ssim(const float* a, const float* b, const float* win, float* out, int N, int C, int H, int W, int K, float c1, float c2,
                       void* stream) {
    VD_REQUIRE(a && b && win && out && N > 0 && C > 0 && H > 0 && W > 0 && K > 0 && K <= 32 && (K & 1) && H > (K - 1) / 2 && W > (K - 1) / 2,
               "vd_ssim: bad args (odd window <= 32, image larger than the window radius)");
    hipLaunchKernelGGL(ssim_kernel, dim3(N), dim3(256), 0, ST, a, b, win, out, C, H, W, K, c1, c2);
    VD_LAUNCH_CHECK("vd_ssim");
    return 0;
}

extern "C" int vd_randn(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream) {
    VD_REQUIRE(out && n > 0, "vd_randn: bad args");
    hipLaunchKernelGGL(randn_kernel, dim3(egrid((n + 3) / 4)), dim3(EB), 0, ST, out, n, seed, offset);
    VD_LAUNCH_CHECK("vd_randn");
    return 0;
}

// ---- VQ-VAE nearest-code lookup (diffusers VectorQuantizer.forward; used by VQModel.decode of the LDM path) ------------
// One thread per latent pixel; the codebook is streamed through LDS in chunks with its squared norms.
// d(z, e) = (|z|^2 + |e|^2) - 2 z.e, first minimum wins (torch.argmin).
constexpr int VQ_CH = 1024;   // codes per LDS chunk
constexpr int VQ_MAXD = 16;
__global__ __launch_bounds__(256) void vq_nearest_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                         float* __restrict__ zq, int64_t* __restrict__ idx_out, int B, int D,
                                                         int HW, int n_e, int64_t z_bs, int64_t q_bs) {
    extern __shared__ float vq_sh[];                 // [VQ_CH * D] codes + [VQ_CH] norms
    float* __restrict__ sh_n = vq_sh + VQ_CH * D;
    const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const bool live = p < (int64_t)B * HW;
    const int b = live ? (int)(p / HW) : 0;
    const int pix = live ? (int)(p - (int64_t)b * HW) : 0;
    float zv[VQ_MAXD];
    float zz = 0.f;
#pragma unroll
    for (int k = 0; k < VQ_MAXD; ++k) {
        zv[k] = (k < D) ? z[(int64_t)b * z_bs + (int64_t)k * HW + pix] : 0.f;
        zz += zv[k] * zv[k];
    }
    float best = INFINITY;
    int besti = 0;
    for (int c0 = 0; c0 < n_e; c0 += VQ_CH) {
        const int nc = min(VQ_CH, n_e - c0);
        __syncthreads();
        for (int i = threadIdx.x; i < nc * D; i += blockDim.x) vq_sh[i] = cb[(int64_t)c0 * D + i];
        __syncthreads();
        for (int j = threadIdx.x; j < nc; j += blockDim.x) {
            float ee = 0.f;
            for (int k = 0; k < D; ++k) ee += vq_sh[j * D + k] * vq_sh[j * D + k];
            sh_n[j] = ee;
        }
        __syncthreads();
        for (int j = 0; j < nc; ++j) {
            float dot = 0.f;
#pragma unroll
            for (int k = 0; k < VQ_MAXD; ++k)
                if (k < D) dot += zv[k] * vq_sh[j * D + k];
            const float dist = (zz + sh_n[j]) - 2.f * dot;
            if (dist < best) {
                best = dist;
                besti = c0 + j;
            }
        }
    }
    if (live) {
        for (int k = 0; k < D; ++k) zq[(int64_t)b * q_bs + (int64_t)k * HW + pix] = cb[(int64_t)besti * D + k];
        if (idx_out) idx_out[p] = besti;
    }
}

extern "C" int vd_vq_nearest(const float* z, const float* codebook, float* zq, int64_t* idx, int B, int D, int HW, int n_e,
                             int64_t z_bstride, int64_t q_bstride, void* stream) {
    VD_REQUIRE(z && codebook && zq && B > 0 && HW > 0 && n_e > 0, "vd_vq_nearest: bad args");
    VD_REQUIRE(D >= 1 && D <= VQ_MAXD, "vd_vq_nearest: embedding dim %d not in [1, %d]", D, VQ_MAXD);
    const int64_t n = (int64_t)B * HW;
    const size_t shmem = (size_t)VQ_CH * (D + 1) * sizeof(float);
    hipLaunchKernelGGL(vq_nearest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), shmem, ST, z, codebook, zq, idx, B, D, HW,
                       n_e, z_bstride, q_bstride);
    VD_LAUNCH_CHECK("vd_vq_nearest");
    return 0;
}

// ---- NCSN++ helpers (diffusers upfirdn2d FIR resampling with the (1,3,3,1) kernel, Fourier time embedding) ---------------
// up  : out[2a]   = (x[a-1] + 3 x[a]) / 4,  out[2a+1] = (3 x[a] + x[a+1]) / 4     (per axis; zero outside)  = upsample_2d
// down: out[a]    = (x[2a-1] + 3 x[2a] + 3 x[2a+1] + x[2a+2]) / 8                                           = downsample_2d
// `scale` folds the adjoint factors: d(up)/dx applied to g is 4 * down(g); d(down)/dx applied to g is up(g) / 4.
__global__ __launch_bounds__(256) void fir_up2_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t planes,
                                                      int H, int W, float scale, int accumulate) {
    const int OH = 2 * H, OW = 2 * W;
    const int64_t total = planes * OH * OW;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % OW);
        const int64_t r = i / OW;
        const int oy = (int)(r % OH);
        const int64_t pl = r / OH;
        const float* __restrict__ xp = x + pl * H * W;
        const int ay = oy >> 1, ax = ox >> 1;
        // taps along y: (row, weight) pairs
        const int y0 = (oy & 1) ? ay : ay - 1, y1 = (oy & 1) ? ay + 1 : ay;
        const float wy0 = (oy & 1) ? 0.75f : 0.25f, wy1 = (oy & 1) ? 0.25f : 0.75f;
        const int x0 = (ox & 1) ? ax : ax - 1, x1 = (ox & 1) ? ax + 1 : ax;
        const float wx0 = (ox & 1) ? 0.75f : 0.25f, wx1 = (ox & 1) ? 0.25f : 0.75f;
        auto at = [&](int yy, int xx) -> float {
            return ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) ? xp[yy * W + xx] : 0.f;
        };
        const float v = wy0 * (wx0 * at(y0, x0) + wx1 * at(y0, x1)) + wy1 * (wx0 * at(y1, x0) + wx1 * at(y1, x1));
        out[i] = accumulate ? out[i] + scale * v : scale * v;
    }
}

__global__ __launch_bounds__(256) void fir_down2_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t planes,
                                                        int H, int W, float scale, int accumulate) {
    const int OH = H / 2, OW = W / 2;
    const int64_t total = planes * OH * OW;
    const float k[4] = {0.125f, 0.375f, 0.375f, 0.125f};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % OW);
        const int64_t r = i / OW;
        const int oy = (int)(r % OH);
        const int64_t pl = r / OH;
        const float* __restrict__ xp = x + pl * H * W;
        float v = 0.f;
#pragma unroll
        for (int jy = 0; jy < 4; ++jy) {
            const int yy = 2 * oy + jy - 1;
            if ((unsigned)yy >= (unsigned)H) continue;
            float row = 0.f;
#pragma unroll
            for (int jx = 0; jx < 4; ++jx) {
                const int xx = 2 * ox + jx - 1;
                if ((unsigned)xx < (unsigned)W) row += k[jx] * xp[yy * W + xx];
            }
            v += k[jy] * row;
        }
        out[i] = accumulate ? out[i] + scale * v : scale * v;
    }
}

// emb[b][j] = sin(log(t_b) * W_j * 2pi), emb[b][half + j] = cos(...)   (GaussianFourierProjection, log=True)
__global__ void fourier_embedding_kernel(const float* __restrict__ t, const float* __restrict__ W, float* __restrict__ emb, int B,
                                         int half) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * half) return;
    const int b = i / half, j = i - b * half;
    const float a = (logf(t[b]) * W[j]) * 2.f * 3.14159265358979323846f;
    emb[(int64_t)b * 2 * half + j] = sinf(a);
    emb[(int64_t)b * 2 * half + half + j] = cosf(a);
}

// out[b][i] = x[b][i] * s[b]   or   x[b][i] / s[b]
__global__ __launch_bounds__(256) void rowscale_kernel(const float* __restrict__ x, const float* __restrict__ s, float* __restrict__ out,
                                                       int B, int64_t inner, int divide) {
    const int64_t total = (int64_t)B * inner;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const float sv = s[i / inner];
        out[i] = divide ? x[i] / sv : x[i] * sv;
    }
}

extern "C" int vd_fir_resample2(const float* x, float* out, int64_t planes, int H, int W, int up, float scale, int accumulate,
                                void* stream) {
    VD_REQUIRE(x && out && planes > 0 && H > 0 && W > 0, "vd_fir_resample2: bad args");
    VD_REQUIRE(up || (H % 2 == 0 && W % 2 == 0), "vd_fir_resample2: downsampling needs even dims");
    const int64_t n = up ? planes * 4 * H * W : planes * (H / 2) * (W / 2);
    if (up)
        hipLaunchKernelGGL(fir_up2_kernel, dim3(egrid(n)), dim3(EB), 0, ST, x, out, planes, H, W, scale, accumulate);
    else
        hipLaunchKernelGGL(fir_down2_kernel, dim3(egrid(n)), dim3(EB), 0, ST, x, out, planes, H, W, scale, accumulate);
    VD_LAUNCH_CHECK("vd_fir_resample2");
    return 0;
}

// ---- input-image pyramid of NCSN++: the gradient of one level with respect to its image (ncsnpp.py, record skip_conv_down) -----------------
//   out[b][c][p] = sum_k w[k][c] * g[b][k][p]  +  0.25 * up(coarse)[b][c][p]  (+ out[b][c][p])
// the transposed 1x1 convolution down to C <= 4 image channels fused with the adjoint of the FIR downsampling that made the next level (the up
// kernel above, same taps, zero outside).  HBM-bound on g, read once: an ITEM is four consecutive pixels of one image (one f32x4 load per source
// channel where pixels, stride and pointers allow, else four guarded scalar loads: which elements a thread owns and the order it adds them in
// do not depend on that choice).  A block is 16 items x 16 slices of k: slice s adds k = s, s + 16, ... in increasing order, then the 16 slice
// sums are added in slice order -- a fixed order, no atomics.  w waits in LDS, 512 source channels at a time.
constexpr int PD_KS = 16, PD_IPB = 16, PD_WCHUNK = 512;
template <int C>
__global__ __launch_bounds__(256) void pyramid_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ w, const float* __restrict__ coarse,
                                                            float* __restrict__ out, int B, int K, int H, int W, int64_t g_bstride, int accumulate,
                                                            int vec) {
    __shared__ float ws[PD_WCHUNK * C];
    __shared__ float red[PD_KS][PD_IPB][C * 4];
    const int HW = H * W, ipi = (HW + 3) >> 2;                 // items per image and channel
    const int64_t items = (int64_t)B * ipi;
    const int li = threadIdx.x % PD_IPB, s = threadIdx.x / PD_IPB;
    const int64_t q = (int64_t)blockIdx.x * PD_IPB + li;
    const bool live = q < items;
    const int b = live ? (int)(q / ipi) : 0;
    const int p0 = live ? (int)(q - (int64_t)b * ipi) * 4 : 0;
    float acc[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[c][e] = 0.f;
    const float* __restrict__ gp = g + (int64_t)b * g_bstride + p0;
    for (int k0 = 0; k0 < K; k0 += PD_WCHUNK) {
        const int kn = (K - k0 < PD_WCHUNK) ? K - k0 : PD_WCHUNK;
        __syncthreads();
        for (int i = threadIdx.x; i < kn * C; i += 256) ws[i] = w[(int64_t)k0 * C + i];
        __syncthreads();
        if (live) {
#pragma unroll 4
            for (int k = s; k < kn; k += PD_KS) {
                const float* __restrict__ p = gp + (int64_t)(k0 + k) * HW;
                float v[4];
                if (vec) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = t[e];
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (p0 + e < HW) ? p[e] : 0.f;
                }
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float wv = ws[k * C + c];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[c][e] += wv * v[e];
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[s][li][c * 4 + e] = acc[c][e];
    __syncthreads();
    if ((int)threadIdx.x >= PD_IPB * C) return;
    const int li2 = threadIdx.x / C, c = threadIdx.x - li2 * C;
    const int64_t q2 = (int64_t)blockIdx.x * PD_IPB + li2;
    if (q2 >= items) return;
    const int b2 = (int)(q2 / ipi), pb = (int)(q2 - (int64_t)b2 * ipi) * 4;
    float r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = red[0][li2][c * 4 + e];
    for (int t = 1; t < PD_KS; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] += red[t][li2][c * 4 + e];
    float* __restrict__ op = out + ((int64_t)b2 * C + c) * HW + pb;
    const int CH = H >> 1, CW = W >> 1;
    const float* __restrict__ xp = coarse ? coarse + ((int64_t)b2 * C + c) * CH * CW : nullptr;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int p = pb + e;
        if (p >= HW) break;
        float val = r[e];
        if (xp) {                                             // fir_up2_kernel's value at (oy, ox), scale 1/4
            const int oy = p / W, ox = p - oy * W;
            const int ay = oy >> 1, ax = ox >> 1;
            const int y0 = (oy & 1) ? ay : ay - 1, y1 = (oy & 1) ? ay + 1 : ay;
            const float wy0 = (oy & 1) ? 0.75f : 0.25f, wy1 = (oy & 1) ? 0.25f : 0.75f;
            const int x0 = (ox & 1) ? ax : ax - 1, x1 = (ox & 1) ? ax + 1 : ax;
            const float wx0 = (ox & 1) ? 0.75f : 0.25f, wx1 = (ox & 1) ? 0.25f : 0.75f;
            auto at = [&](int yy, int xx) -> float {
                return ((unsigned)yy < (unsigned)CH && (unsigned)xx < (unsigned)CW) ? xp[yy * CW + xx] : 0.f;
            };
            const float u = wy0 * (wx0 * at(y0, x0) + wx1 * at(y0, x1)) + wy1 * (wx0 * at(y1, x0) + wx1 * at(y1, x1));
            val += 0.25f * u;
        }
        op[e] = accumulate ? op[e] + val : val;
    }
}

extern "C" int vd_pyramid_dgrad(const float* g, const float* w, const float* coarse, float* out, int B, int K, int C, int H, int W,
                                int64_t g_bstride, int accumulate, void* stream) {
    VD_REQUIRE(g && w && out && B > 0 && K > 0 && H > 0 && W > 0, "vd_pyramid_dgrad: bad args");
    VD_REQUIRE(C >= 1 && C <= 4, "vd_pyramid_dgrad: %d image channels not in [1, 4]", C);
    VD_REQUIRE(g_bstride >= (int64_t)K * H * W, "vd_pyramid_dgrad: batch stride %lld < K*H*W %lld", (long long)g_bstride, (long long)K * H * W);
    VD_REQUIRE(!coarse || (H % 2 == 0 && W % 2 == 0), "vd_pyramid_dgrad: a coarser level needs even dims");
    const int HW = H * W;
    const int64_t items = (int64_t)B * ((HW + 3) >> 2);
    const int64_t grid = (items + PD_IPB - 1) / PD_IPB;
    VD_REQUIRE(grid <= 0x7fffffff, "vd_pyramid_dgrad: too many pixels");
    const int vec = (HW % 4 == 0) && (g_bstride % 4 == 0) && ((((uintptr_t)g) & 15) == 0);
#define PD_LAUNCH(CC) \
    hipLaunchKernelGGL(pyramid_dgrad_kernel<CC>, dim3((unsigned)grid), dim3(256), 0, ST, g, w, coarse, out, B, K, H, W, g_bstride, accumulate, vec)
    switch (C) {
        case 1: PD_LAUNCH(1); break;
        case 2: PD_LAUNCH(2); break;
        case 3: PD_LAUNCH(3); break;
        default: PD_LAUNCH(4); break;
    }
#undef PD_LAUNCH
    VD_LAUNCH_CHECK("vd_pyramid_dgrad");
    return 0;
}

extern "C" int vd_fourier_embedding(const float* t, const float* W, float* emb, int B, int half, void* stream) {
    VD_REQUIRE(t && W && emb && B > 0 && half > 0, "vd_fourier_embedding: bad args");
    hipLaunchKernelGGL(fourier_embedding_kernel, dim3((B * half + 255) / 256), dim3(256), 0, ST, t, W, emb, B, half);
    VD_LAUNCH_CHECK("vd_fourier_embedding");
    return 0;
}

extern "C" int vd_rowscale(const float* x, const float* s, float* out, int B, int64_t inner, int divide, void* stream) {
    VD_REQUIRE(x && s && out && B > 0 && inner > 0, "vd_rowscale: bad args");
    hipLaunchKernelGGL(rowscale_kernel, dim3(egrid((int64_t)B * inner)), dim3(EB), 0, ST, x, s, out, B, inner, divide);
    VD_LAUNCH_CHECK("vd_rowscale");
    return 0;
}

extern "C" int vd_poison_batch(const uint8_t* img, const int64_t* idx, const uint8_t* flags, const float* trigger, const float* target,
                               float* pixel_values, float* tgt_out, float* image_out, int B, int C, int H, int W, float vmin,
                               float vmax, int R_trigger_only, void* stream) {
    VD_REQUIRE(img && flags && trigger && target && pixel_values && tgt_out, "vd_poison_batch: null pointer");
    VD_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "vd_poison_batch: bad dims");
    const float denom = (float)(1.0 - 0.0 + 1e-5);  // util.py:147  (max_x - min_x + eps)
    hipLaunchKernelGGL(poison_kernel, dim3(egrid((int64_t)B * C * H * W)), dim3(EB), 0, ST, img, idx, flags, trigger, target,
                       pixel_values, tgt_out, image_out, B, C, H, W, vmin, vmax, denom, R_trigger_only);
    VD_LAUNCH_CHECK("vd_poison_batch");
    return 0;
}

// ---- FID feature extractor (InceptionV3 of pytorch-fid 0.3.0; reference fid_score.py:91-148): pooling and the input resize ----------
namespace {

// 3x3 pooling over NCHW planes: MODE 0 max (F.max_pool2d), 1 average with the zero padding EXCLUDED from the divisor
// (F.avg_pool2d(..., count_include_pad=False) -- the TensorFlow semantics the FID network was trained with).  One thread per output element;
// the input plane of a 8x8 ... 147x147 feature map stays in L2 between the 9 taps.
template <int MODE>
__global__ __launch_bounds__(EB) void pool3_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int C, int H, int W, int OH, int OW,
                                                   int stride, int pad, int64_t x_bstride, int64_t y_bstride) {
    const int64_t total = (int64_t)B * C * OH * OW;
    for (int64_t e = (int64_t)blockIdx.x * EB + threadIdx.x; e < total; e += (int64_t)gridDim.x * EB) {
        const int ox = (int)(e % OW);
        int64_t r = e / OW;
        const int oy = (int)(r % OH);
        r /= OH;
        const int c = (int)(r % C), b = (int)(r / C);
        const float* __restrict__ src = x + b * x_bstride + (int64_t)c * H * W;
        float acc = MODE == 0 ? -INFINITY : 0.f;
        int cnt = 0;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int iy = oy * stride + dy - pad, ix = ox * stride + dx - pad;
                const bool ok = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
                const float v = src[ok ? iy * W + ix : 0];
                if (ok) {
                    acc = MODE == 0 ? fmaxf(acc, v) : acc + v;
                    ++cnt;
                }
            }
        y[b * y_bstride + (int64_t)c * OH * OW + (int64_t)oy * OW + ox] = MODE == 0 ? acc : acc / (float)cnt;
    }
}

// F.interpolate(x, size=(OH, OW), mode="bilinear", align_corners=False) followed by y = mul * v + add (pytorch-fid: 2 x - 1).
// Source index = scale * (dst + 0.5) - 0.5 clamped at 0, scale = in / out, as torch's area_pixel_compute_source_index.
__global__ __launch_bounds__(EB) void resize_bilinear_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t planes, int H, int W, int OH,
                                                             int OW, float sh, float sw, float mul, float add) {
    const int64_t total = planes * OH * OW;
    for (int64_t e = (int64_t)blockIdx.x * EB + threadIdx.x; e < total; e += (int64_t)gridDim.x * EB) {
        const int ox = (int)(e % OW);
        const int64_t r = e / OW;
        const int oy = (int)(r % OH);
        const int64_t pl = r / OH;
        float fy = sh * ((float)oy + 0.5f) - 0.5f, fx = sw * ((float)ox + 0.5f) - 0.5f;
        fy = fy < 0.f ? 0.f : fy;
        fx = fx < 0.f ? 0.f : fx;
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
        const float ly = fy - (float)y0, lx = fx - (float)x0;
        const float* __restrict__ s = x + pl * H * W;
        const float v = (1.f - ly) * ((1.f - lx) * s[y0 * W + x0] + lx * s[y0 * W + x1]) + ly * ((1.f - lx) * s[y1 * W + x0] + lx * s[y1 * W + x1]);
        y[e] = mul * v + add;
    }
}

}  // namespace

extern "C" int vd_pool3(const float* x, float* y, int B, int C, int H, int W, int stride, int pad, int mode, int64_t x_bstride, int64_t y_bstride,
                        void* stream) {
    VD_REQUIRE(x && y && B > 0 && C > 0 && H >= 3 - 2 * pad && W >= 3 - 2 * pad && (stride == 1 || stride == 2) && (pad == 0 || pad == 1) && (mode == 0 || mode == 1),
               "vd_pool3: bad args (3x3 window, stride 1 | 2, pad 0 | 1, mode 0 max | 1 avg without the padding)");
    const int OH = (H + 2 * pad - 3) / stride + 1, OW = (W + 2 * pad - 3) / stride + 1;
    const int64_t n = (int64_t)B * C * OH * OW;
    if (mode == 0)
        hipLaunchKernelGGL(pool3_kernel<0>, dim3(egrid(n)), dim3(EB), 0, ST, x, y, B, C, H, W, OH, OW, stride, pad, x_bstride, y_bstride);
    else
        hipLaunchKernelGGL(pool3_kernel<1>, dim3(egrid(n)), dim3(EB), 0, ST, x, y, B, C, H, W, OH, OW, stride, pad, x_bstride, y_bstride);
    VD_LAUNCH_CHECK("vd_pool3");
    return 0;
}

extern "C" int vd_resize_bilinear(const float* x, float* y, int64_t planes, int H, int W, int OH, int OW, float mul, float add, void* stream) {
    VD_REQUIRE(x && y && planes > 0 && H > 0 && W > 0 && OH > 0 && OW > 0, "vd_resize_bilinear: bad args");
    hipLaunchKernelGGL(resize_bilinear_kernel, dim3(egrid(planes * OH * OW)), dim3(EB), 0, ST, x, y, planes, H, W, OH, OW, (float)H / (float)OH,
                       (float)W / (float)OW, mul, add);
    VD_LAUNCH_CHECK("vd_resize_bilinear");
    return 0;
}

// ---- LPIPS (lpips.LPIPS(net='alex'), reference VillanDiffusion.py:892): the ops around the AlexNet convolutions -----------------------
namespace {

// y[b][c][p] = x[b][c][p] * mul[c] + add[c]   (the ScalingLayer: (x - shift) / scale as x * (1/scale) + (-shift/scale))
__global__ __launch_bounds__(EB) void channel_affine_kernel(const float* __restrict__ x, const float* __restrict__ mul, const float* __restrict__ add,
                                                            float* __restrict__ y, int64_t total, int C, int HW) {
    for (int64_t e = (int64_t)blockIdx.x * EB + threadIdx.x; e < total; e += (int64_t)gridDim.x * EB) {
        const int c = (int)((e / HW) % C);
        y[e] = x[e] * mul[c] + add[c];
    }
}

// One LPIPS tap: out[n] (+)= (1 / HW) * sum_p sum_c w[c] * (f0[n][c][p] / (|f0[n][:, p]| + eps) - f1[n][c][p] / (|f1[n][:, p]| + eps))^2.
// One workgroup per image; a thread owns pixels p, p + 256, ... and walks the channels twice (norms, then the weighted squared
// differences); the per-pixel sums meet in a fixed-order tree.  The feature maps are at most 64 x 55 x 55 floats per image.
__global__ __launch_bounds__(256) void lpips_layer_kernel(const float* __restrict__ f0, const float* __restrict__ f1, const float* __restrict__ w,
                                                          float* __restrict__ out, int C, int HW, int accumulate) {
    const int n = blockIdx.x;
    const float* __restrict__ a = f0 + (int64_t)n * C * HW;
    const float* __restrict__ b = f1 + (int64_t)n * C * HW;
    float acc = 0.f;
    for (int p = threadIdx.x; p < HW; p += 256) {
        float sa = 0.f, sb = 0.f;
        for (int c = 0; c < C; ++c) {
            const float va = a[(int64_t)c * HW + p], vb = b[(int64_t)c * HW + p];
            sa += va * va;
            sb += vb * vb;
        }
        const float ia = 1.f / (sqrtf(sa) + 1e-10f), ib = 1.f / (sqrtf(sb) + 1e-10f);
        float s = 0.f;
        for (int c = 0; c < C; ++c) {
            const float dlt = a[(int64_t)c * HW + p] * ia - b[(int64_t)c * HW + p] * ib;
            s += w[c] * (dlt * dlt);
        }
        acc += s;
    }
    __shared__ float red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[n] = (accumulate ? out[n] : 0.f) + red[0] / (float)HW;
}

}  // namespace

extern "C" int vd_channel_affine(const float* x, const float* mul, const float* add, float* y, int B, int C, int HW, void* stream) {
    VD_REQUIRE(x && mul && add && y && B > 0 && C > 0 && HW > 0, "vd_channel_affine: bad args");
    const int64_t n = (int64_t)B * C * HW;
    hipLaunchKernelGGL(channel_affine_kernel, dim3(egrid(n)), dim3(EB), 0, ST, x, mul, add, y, n, C, HW);
    VD_LAUNCH_CHECK("vd_channel_affine");
    return 0;
}

extern "C" int vd_lpips_layer(const float* f0, const float* f1, const float* w, float* out, int N, int C, int HW, int accumulate, void* stream) {
    VD_REQUIRE(f0 && f1 && w && out && N > 0 && C > 0 && HW > 0, "vd_lpips_layer: bad args");
    hipLaunchKernelGGL(lpips_layer_kernel, dim3(N), dim3(256), 0, ST, f0, f1, w, out, C, HW, accumulate);
    VD_LAUNCH_CHECK("vd_lpips_layer");
    return 0;
}
