// The shaped loss: vd_loss_fwd_bwd's norm with a weight per sample in (explicit, gathered from a timestep table such as min-SNR, and a poison
// weight picked by a flag) and the unweighted loss of every sample out, plus the clean / poisoned split of the batch.
//   stage 1  loss_sample_kernel: every sample is cut into `segments` pieces (a multiple of 4 floats each); one 256-thread workgroup sums one
//            (sample, segment) pair -- no workgroup straddles two samples -- writes dpred on the way and parks its sum in ws[b * segments + s].
//            Beyond the block cap a workgroup walks several pairs.
//   stage 2  loss_sample_finish_kernel, ONE workgroup: a thread adds a sample's partials in index order, divides by chw (sample_loss), and
//            the workgroup reduces the weighted losses, the two class sums and the two counts in a fixed order.
// No atomics: the same bits in every run.  Built with -ffp-contract=off like vd_elem.hip: with every weight 1 the gradient is the one
// mse_kernel writes, bit for bit ((gcoef * 1) * g) * ps.
#include <cmath>

#include "vd_common.h"

namespace {

constexpr int LS_SEG_FLOATS = 2048;     // floats of a sample one workgroup takes before the sample is cut again (8 per thread)
constexpr int LS_MAX_SEGMENTS = 64;     // a 3 x 256 x 256 image: 64 pieces of 3072 floats
constexpr int LS_BLOCK_CAP = 2048;      // 256 CUs x 8 workgroups (cdna guide G11); the pairs beyond are walked

struct LossSamplePlan {
    int segments, blocks;
    int64_t seg_len;                    // floats per piece, a multiple of 4: every piece starts 16-byte aligned relative to its sample
};
// What the launcher does, for the launcher and for vd_loss_sample_plan alike.
inline LossSamplePlan loss_sample_plan(int B, int64_t chw) {
    LossSamplePlan p;
    const int64_t want = (chw + LS_SEG_FLOATS - 1) / LS_SEG_FLOATS;
    p.segments = (int)(want > LS_MAX_SEGMENTS ? LS_MAX_SEGMENTS : want);
    p.seg_len = ((chw + p.segments - 1) / p.segments + 3) & ~(int64_t)3;
    const int64_t pairs = (int64_t)B * p.segments;
    p.blocks = (int)(pairs > LS_BLOCK_CAP ? LS_BLOCK_CAP : pairs);
    return p;
}

// w[b] = weight[b] * wtab[clamp(t[b])] * (flags[b] ? poison_weight : 1), absent factors 1; the same expression in both stages
__device__ __forceinline__ float sample_weight(int b, const float* __restrict__ weight, const float* __restrict__ wtab,
                                               const int64_t* __restrict__ t, int T, const uint8_t* __restrict__ flags, float poison_weight) {
    float w = weight ? weight[b] : 1.0f;
    if (wtab) {
        int64_t tt = t[b];
        tt = tt < 0 ? 0 : (tt > (int64_t)T - 1 ? (int64_t)T - 1 : tt);      // a bad index cannot leave the table
        w = w * wtab[tt];
    }
    return w * ((flags && flags[b]) ? poison_weight : 1.0f);
}

// norm(d) and norm'(d) of mse_kernel<KIND> (vd_elem.hip)
template <int KIND>
__device__ __forceinline__ void loss_norm(float d, float& v, float& g) {
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
}

template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void loss_sample_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                          const float* __restrict__ pscale, const float* __restrict__ weight,
                                                          const float* __restrict__ wtab, const int64_t* __restrict__ t, int T,
                                                          const uint8_t* __restrict__ flags, float poison_weight, float* __restrict__ dpred,
                                                          float* __restrict__ ws, int B, int64_t chw, int segments, int64_t seg_len,
                                                          float gcoef) {
    __shared__ float red[4];
    const int64_t pairs = (int64_t)B * segments;
    for (int64_t w = blockIdx.x; w < pairs; w += gridDim.x) {
        const int b = (int)(w / segments);
        const int s = (int)(w - (int64_t)b * segments);
        const int64_t lo = (int64_t)s * seg_len;
        const int64_t hi = lo + seg_len < chw ? lo + seg_len : chw;
        const float ps = pscale ? pscale[b] : 1.0f;
        const float gw = gcoef * sample_weight(b, weight, wtab, t, T, flags, poison_weight);
        const float* __restrict__ pb = pred + (int64_t)b * chw;
        const float* __restrict__ yb = y + (int64_t)b * chw;
        float* __restrict__ db = dpred ? dpred + (int64_t)b * chw : nullptr;
        float acc = 0.f;
        if (VEC) {                                   // chw % 4 == 0 and 16-byte aligned bases: lo and hi are multiples of 4
            const f32x4* __restrict__ p4 = reinterpret_cast<const f32x4*>(pb);
            const f32x4* __restrict__ y4 = reinterpret_cast<const f32x4*>(yb);
            f32x4* __restrict__ d4 = reinterpret_cast<f32x4*>(db);
            for (int64_t i = (lo >> 2) + threadIdx.x; i < (hi >> 2); i += 256) {
                const f32x4 pv = p4[i], yv = y4[i];
                f32x4 gv;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float d = pv[j] * ps - yv[j];
                    float v, g;
                    loss_norm<KIND>(d, v, g);
                    acc += v;
                    gv[j] = (gw * g) * ps;
                }
                if (db) d4[i] = gv;
            }
        } else {
            for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
                const float d = pb[i] * ps - yb[i];
                float v, g;
                loss_norm<KIND>(d, v, g);
                acc += v;
                if (db) db[i] = (gw * g) * ps;
            }
        }
        acc = block_sum_256(acc, red);
        if (threadIdx.x == 0) ws[w] = acc;
    }
}

__global__ __launch_bounds__(256) void loss_sample_finish_kernel(const float* __restrict__ ws, const float* __restrict__ weight,
                                                                 const float* __restrict__ wtab, const int64_t* __restrict__ t, int T,
                                                                 const uint8_t* __restrict__ flags, float poison_weight,
                                                                 float* __restrict__ loss, float* __restrict__ sample_loss,
                                                                 float* __restrict__ stats, int B, int64_t chw, int segments) {
    __shared__ float red[4];
    float aw = 0.f, ac = 0.f, nc = 0.f, ap = 0.f, np = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float* __restrict__ wb = ws + (int64_t)b * segments;
        float s = wb[0];
        for (int k = 1; k < segments; ++k) s += wb[k];
        const float l = s / (float)chw;
        if (sample_loss) sample_loss[b] = l;
        aw += sample_weight(b, weight, wtab, t, T, flags, poison_weight) * l;
        if (flags && flags[b]) {
            ap += l;
            np += 1.f;
        } else {
            ac += l;
            nc += 1.f;
        }
    }
    aw = block_sum_256(aw, red);
    ac = block_sum_256(ac, red);
    nc = block_sum_256(nc, red);
    ap = block_sum_256(ap, red);
    np = block_sum_256(np, red);
    if (threadIdx.x == 0) {
        *loss = aw / (float)B;
        if (stats) {
            stats[0] = ac;
            stats[1] = nc;
            stats[2] = ap;
            stats[3] = np;
        }
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int64_t vd_loss_sample_ws_floats(int B, int64_t chw) {
    if (B <= 0 || chw <= 0) return 0;
    return (int64_t)B * loss_sample_plan(B, chw).segments;
}

extern "C" int vd_loss_sample_plan(int B, int64_t chw, int* segments, int* blocks) {
    VD_REQUIRE(B > 0 && chw > 0 && segments && blocks, "vd_loss_sample_plan: bad args");
    const LossSamplePlan p = loss_sample_plan(B, chw);
    *segments = p.segments;
    *blocks = p.blocks;
    return 0;
}

#define LS_LAUNCH(KIND, VEC)                                                                                                              \
    hipLaunchKernelGGL((loss_sample_kernel<KIND, VEC>), dim3(p.blocks), dim3(256), 0, ST, pred, y, pscale, weight, wtab, t, T, flags,     \
                       poison_weight, dpred, ws, B, chw, p.segments, p.seg_len, gcoef)

extern "C" int vd_loss_sample_fwd_bwd(const float* pred, const float* y, const float* pscale, const float* weight, const float* wtab,
                                      const int64_t* t, int T, const uint8_t* flags, float poison_weight, float* dpred, float* loss,
                                      float* sample_loss, float* stats, float* ws, int B, int64_t chw, float gscale, int kind, void* stream) {
    VD_REQUIRE(pred && y && loss && ws && B > 0 && chw > 0, "vd_loss_sample_fwd_bwd: bad args");
    VD_REQUIRE(kind >= VD_LOSS_L2 && kind <= VD_LOSS_HUBER, "vd_loss_sample_fwd_bwd: kind %d (0 = l2, 1 = l1, 2 = huber)", kind);
    VD_REQUIRE(!wtab || (t && T > 0), "vd_loss_sample_fwd_bwd: a weight table needs timesteps and T > 0 (T=%d)", T);
    VD_REQUIRE(std::isfinite(poison_weight), "vd_loss_sample_fwd_bwd: poison_weight is not finite");
    const LossSamplePlan p = loss_sample_plan(B, chw);
    const int64_t n = (int64_t)B * chw;
    const float gcoef = (kind == VD_LOSS_L2 ? 2.0f : 1.0f) * gscale / (float)n;
    const bool vec = ((chw & 3) == 0) && (((((uintptr_t)pred) | ((uintptr_t)y) | ((uintptr_t)dpred)) & 15) == 0);
    if (kind == VD_LOSS_L2) {
        if (vec) LS_LAUNCH(0, true); else LS_LAUNCH(0, false);
    } else if (kind == VD_LOSS_L1) {
        if (vec) LS_LAUNCH(1, true); else LS_LAUNCH(1, false);
    } else {
        if (vec) LS_LAUNCH(2, true); else LS_LAUNCH(2, false);
    }
    hipLaunchKernelGGL(loss_sample_finish_kernel, dim3(1), dim3(256), 0, ST, ws, weight, wtab, t, T, flags, poison_weight, loss, sample_loss,
                       stats, B, chw, p.segments);
    VD_LAUNCH_CHECK("vd_loss_sample_fwd_bwd");
    return 0;
}
