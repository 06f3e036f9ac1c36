// Activation-based channel pruning (villandiffusion_amd/actprune.py): per-channel sums of a hidden activation over a whole network in one
// table-driven pass, and the row mask that keeps pruned neurons at zero during a fine-tune.  Both are HBM-bound, plain C++ with 16-byte
// accesses where the data allow, no atomics, every sum in a fixed order: a repeat is bit-identical.  Compiled without FMA contraction; the
// one fused multiply-add of the activation is written out, so the operation order below is the one that runs.
//
// vd_channel_stats.  A channel c of a job is B runs of HW contiguous floats.  It is walked in ITEMS of four consecutive floats of one run:
// run b holds I = ceil(HW / 4) items (the last one partial where HW % 4 != 0), the channel B * I items, item q = b * I + i.  The channel is
// cut into S = segments(B, HW) SEGMENTS of L = ceil(B * I / S) items; one 64-lane wave sums one (channel, segment) UNIT, four units to a
// workgroup, and a job owns ceil(C * S / 4) workgroups.  Lane l takes the items lo + l, lo + l + 64, ... of its segment in that order and keeps
// one f32 partial per position e of an item (four chains), for the sum and for the sum of squares; they are added as (a0 + a1) + (a2 + a3)
// and the 64 lanes by the xor tree of wave_sum.  S == 1: the wave writes out[].  S > 1: it parks its pair in ws[2 * (4 * workgroup + wave)] and
// the finish launch adds a channel's S pairs in index order.  An item is one f32x4 load where x is 16-byte aligned and HW % 4 == 0, four scalar
// loads otherwise: which lane owns an element and the order it is added in do not depend on that choice.
#include "vd_common.h"

namespace {

constexpr int CS_K = 11;                // int64 per job: x, mean, rstd, gamma, beta, B, C, HW, G, first channel, first workgroup
constexpr int CS_SEG_ITEMS = 1024;      // items a wave takes (16 per lane, 4096 floats) before the channel is cut again: short waves balance the levels
constexpr int CS_MAX_SEGMENTS = 256;    // beyond it the segments grow instead

struct ChanPlan {
    int64_t items_per_run, items, seg_items;
    int segments;
};
// What the kernels do, for them, for the launcher and for vd_channel_stats_plan alike.
__host__ __device__ inline ChanPlan chan_plan(int64_t B, int64_t HW) {
    ChanPlan p;
    p.items_per_run = (HW + 3) >> 2;
    p.items = B * p.items_per_run;
    const int64_t want = (p.items + CS_SEG_ITEMS - 1) / CS_SEG_ITEMS;
    p.segments = (int)(want > CS_MAX_SEGMENTS ? CS_MAX_SEGMENTS : (want < 1 ? 1 : want));
    p.seg_items = (p.items + p.segments - 1) / p.segments;
    return p;
}
inline int64_t chan_chain(const ChanPlan& p) { return (p.seg_items + 63) / 64 + 8 + (p.segments - 1); }

__host__ __device__ inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// last job whose entry `col` <= v (block- or thread-uniform binary search; entries ascend)
__device__ __forceinline__ const int64_t* job_of(const int64_t* __restrict__ table, int n_jobs, int stride, int col, int64_t v) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(int64_t)stride * mid + col] <= v) lo = mid; else hi = mid - 1;
    }
    return table + (int64_t)stride * lo;
}

// a = silu(z), z = fma((x - mean) * rstd, gamma[c], beta[c]): the order of the GroupNorm forward's element path (vd_norm.hip, gn_fwd_kernel:
// `(xs[i] - mean) * rstd * gamma[c] + beta[c]`, built with contraction, so the last product and the sum are one FMA), the sigmoid its
// sigmoidf_.  The register, wave and chunk kernels fold the same affine map into z = fma(x, gamma * rstd, beta - mean * gamma * rstd), which
// rounds differently and cancels where |mean| >> 1 / rstd; the subtraction comes first here, so a large mean costs nothing.
template <int ACT>
__device__ __forceinline__ float chan_act(float x, float mean, float rstd, float gam, float bet) {
    if (ACT == 0) return x;
    const float z = __builtin_fmaf((x - mean) * rstd, gam, bet);
    return z * sigmoidf_(z);
}

template <int ACT>
__global__ __launch_bounds__(256) void channel_stats_kernel(const int64_t* __restrict__ table, int n_jobs, float* __restrict__ out,
                                                            float* __restrict__ ws) {
    const int64_t* __restrict__ t = job_of(table, n_jobs, CS_K, 10, (int64_t)blockIdx.x);
    const int64_t B = t[5], C = t[6], HW = t[7], G = t[8];
    const ChanPlan p = chan_plan(B, HW);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t unit = ((int64_t)blockIdx.x - t[10]) * 4 + wave;
    if (unit >= C * p.segments) return;                                  // wave-uniform
    const int64_t c = unit / p.segments;
    const int s = (int)(unit - c * p.segments);
    const float* __restrict__ x = reinterpret_cast<const float*>(t[0]);
    const bool vec = aligned16(x) && (HW & 3) == 0;
    const float* __restrict__ mean = reinterpret_cast<const float*>(t[1]);
    const float* __restrict__ rstd = reinterpret_cast<const float*>(t[2]);
    float gam = 0.f, bet = 0.f;
    int64_t g = 0;
    if (ACT == 1) {
        gam = reinterpret_cast<const float*>(t[3])[c];
        bet = reinterpret_cast<const float*>(t[4])[c];
        g = c / (C / G);
    }
    const int64_t lo = (int64_t)s * p.seg_items;
    const int64_t hi = lo + p.seg_items < p.items ? lo + p.seg_items : p.items;
    float a1[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f};
    int64_t cur_b = -1;
    float m = 0.f, r = 1.f;
    // item q = (run b, item i of the run); a lane's next item is 64 further on: 64 = db * I + di with di < I, so one conditional wrap follows it
    const int64_t I = p.items_per_run;
    int64_t q = lo + lane;
    int64_t b = q / I, i = q - b * I;
    const int64_t db = 64 / I, di = 64 - db * I;
    const float* __restrict__ xc = x + c * HW;
    const int64_t run = C * HW;
#define CS_NEXT()          \
    do {                   \
        q += 64;           \
        b += db;           \
        i += di;           \
        if (i >= I) {      \
            i -= I;        \
            ++b;           \
        }                  \
    } while (0)
#define CS_STATS(bb)                 \
    if (ACT == 1 && (bb) != cur_b) { \
        cur_b = (bb);                \
        m = mean[(bb) * G + g];      \
        r = rstd[(bb) * G + g];      \
    }
    if (vec) {
        while (q < hi) {                                                 // four loads in flight, then their sums in item order
            f32x4 v[4];
            int64_t vb[4];
            int n = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (q < hi) {
                    v[u] = *reinterpret_cast<const f32x4*>(xc + b * run + (i << 2));
                    vb[u] = b;
                    ++n;
                    CS_NEXT();
                }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (u < n) {
                    CS_STATS(vb[u]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float a = chan_act<ACT>(v[u][e], m, r, gam, bet);
                        a1[e] += a;
                        a2[e] += a * a;
                    }
                }
        }
    } else {
        while (q < hi) {
            CS_STATS(b);
            const float* __restrict__ src = xc + b * run + (i << 2);
            const int64_t k0 = i << 2;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (k0 + e < HW) {
                    const float a = chan_act<ACT>(src[e], m, r, gam, bet);
                    a1[e] += a;
                    a2[e] += a * a;
                }
            CS_NEXT();
        }
    }
#undef CS_NEXT
#undef CS_STATS
    const float s1 = wave_sum((a1[0] + a1[1]) + (a1[2] + a1[3]));
    const float s2 = wave_sum((a2[0] + a2[1]) + (a2[2] + a2[3]));
    if (lane == 0) {
        float* __restrict__ dst = p.segments == 1 ? out + 2 * (t[9] + c) : ws + 2 * ((int64_t)blockIdx.x * 4 + wave);
        dst[0] = s1;
        dst[1] = s2;
    }
}

// One thread per output channel: a channel cut into S > 1 segments adds its S parked pairs in index order, one f32 chain each.
__global__ __launch_bounds__(256) void channel_stats_finish_kernel(const int64_t* __restrict__ table, int n_jobs, int64_t n_channels,
                                                                   float* __restrict__ out, const float* __restrict__ ws) {
    const int64_t ch = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ch >= n_channels) return;
    const int64_t* __restrict__ t = job_of(table, n_jobs, CS_K, 9, ch);
    const int64_t c = ch - t[9];
    if (c < 0 || c >= t[6]) return;
    const ChanPlan p = chan_plan(t[5], t[7]);
    if (p.segments == 1) return;
    const float* __restrict__ src = ws + 2 * (t[10] * 4 + c * p.segments);
    float s1 = src[0], s2 = src[1];
    for (int k = 1; k < p.segments; ++k) {
        s1 += src[2 * k];
        s2 += src[2 * k + 1];
    }
    out[2 * ch] = s1;
    out[2 * ch + 1] = s2;
}

// ---- the NEURON TABLE of vd_neuron_scale (vd_defense.hip): {weight offset, rows, row length, bias offset or -1, first neuron, first workgroup}
constexpr int NJ = 6;

// vd_neuron_scale's layout: one wave per row, four rows per workgroup, item q of a row in lane q % 64.  Only dropped rows are touched.
__global__ __launch_bounds__(256) void neuron_keep_rows_kernel(float* __restrict__ buf, const int64_t* __restrict__ table, int n_jobs,
                                                               const float* __restrict__ keep) {
    const int64_t* __restrict__ t = job_of(table, n_jobs, NJ, 5, (int64_t)blockIdx.x);
    const int64_t rows = t[1], len = t[2];
    const int64_t row = ((int64_t)blockIdx.x - t[5]) * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    if (keep[t[4] + row] != 0.0f) return;                                // wave-uniform; NaN keeps
    const int lane = threadIdx.x & 63;
    float* __restrict__ dst = buf + t[0] + row * len;
    const bool vec = aligned16(dst);
    const int64_t items = (len + 3) >> 2;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int64_t q = lane; q < items; q += 64) {
        const int64_t k0 = q << 2;
        if (vec && k0 + 4 <= len) {
            *reinterpret_cast<f32x4*>(dst + k0) = zero;
        } else {
            for (int e = 0; e < 4 && k0 + e < len; ++e) dst[k0 + e] = 0.f;
        }
    }
}

struct ChanTotals {
    int64_t blocks, n_channels;
    bool segmented;
};
// Every rule of the job table, on the host copy; false with the message set.
inline bool chan_table_ok(const int64_t* h, int n_jobs, int act, ChanTotals& tot) {
    int64_t block = 0, chan = 0;
    tot.segmented = false;
    for (int k = 0; k < n_jobs; ++k) {
        const int64_t* t = h + (int64_t)CS_K * k;
        const int64_t B = t[5], C = t[6], HW = t[7], G = t[8];
        if (B < 1 || C < 1 || HW < 1 || G < 1 || B > (1 << 24) || C > (1 << 24) || HW > (1ll << 32)) {
            vd_set_error("vd_channel_stats: job %d has B, C, HW, G = %lld, %lld, %lld, %lld", k, (long long)B, (long long)C, (long long)HW, (long long)G);
            return false;
        }
        if (C % G != 0) {
            vd_set_error("vd_channel_stats: job %d: C = %lld is no multiple of G = %lld", k, (long long)C, (long long)G);
            return false;
        }
        if (t[0] == 0 || (t[0] & 3) != 0) {
            vd_set_error("vd_channel_stats: job %d: x is null or not 4-byte aligned", k);
            return false;
        }
        if (act == 1 && (t[1] == 0 || t[2] == 0 || t[3] == 0 || t[4] == 0 || ((t[1] | t[2] | t[3] | t[4]) & 3) != 0)) {
            vd_set_error("vd_channel_stats: job %d: act = 1 needs mean, rstd, gamma and beta (4-byte aligned)", k);
            return false;
        }
        if (t[9] < chan || t[10] != block) {
            vd_set_error("vd_channel_stats: job %d: first channel %lld (expected >= %lld), first workgroup %lld (expected %lld)", k,
                         (long long)t[9], (long long)chan, (long long)t[10], (long long)block);
            return false;
        }
        const ChanPlan p = chan_plan(B, HW);
        tot.segmented = tot.segmented || p.segments > 1;
        chan = t[9] + C;
        block += (C * p.segments + 3) / 4;
        if (block >= (1ll << 31)) {
            vd_set_error("vd_channel_stats: the table needs %lld workgroups", (long long)block);
            return false;
        }
    }
    tot.blocks = block;
    tot.n_channels = chan;
    return true;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int vd_channel_stats_plan(int B, int C, int64_t HW, int* workgroups, int* segments, int64_t* chain) {
    VD_REQUIRE(B > 0 && C > 0 && HW > 0 && workgroups && segments && chain, "vd_channel_stats_plan: bad args");
    const ChanPlan p = chan_plan(B, HW);
    const int64_t wg = ((int64_t)C * p.segments + 3) / 4;
    VD_REQUIRE(wg < (1ll << 31), "vd_channel_stats_plan: %lld workgroups", (long long)wg);
    *workgroups = (int)wg;
    *segments = p.segments;
    *chain = chan_chain(p);
    return 0;
}

extern "C" int64_t vd_channel_stats_ws_floats(const int64_t* host_table, int n_jobs) {
    if (!host_table || n_jobs < 1) return -1;
    ChanTotals tot;
    if (!chan_table_ok(host_table, n_jobs, 0, tot)) return -1;
    return tot.segmented ? tot.blocks * 8 : 0;
}

extern "C" int vd_channel_stats(const int64_t* host_table, const int64_t* table, int n_jobs, int act, float* out, int64_t out_channels,
                                float* ws, int64_t ws_floats, void* stream) {
    VD_REQUIRE(n_jobs >= 1, "vd_channel_stats: n_jobs = %d", n_jobs);
    VD_REQUIRE(act == 0 || act == 1, "vd_channel_stats: act %d (0 = raw, 1 = silu(groupnorm))", act);
    VD_REQUIRE(host_table && table && out, "vd_channel_stats: null pointer");
    ChanTotals tot;
    if (!chan_table_ok(host_table, n_jobs, act, tot)) return VD_EINVAL;
    VD_REQUIRE(tot.n_channels <= out_channels, "vd_channel_stats: the table writes %lld channels, out holds %lld", (long long)tot.n_channels,
               (long long)out_channels);
    VD_REQUIRE(!tot.segmented || (ws && ws_floats >= tot.blocks * 8), "vd_channel_stats: the workspace holds %lld floats, %lld are needed",
               (long long)ws_floats, (long long)(tot.blocks * 8));
    if (act == 0) hipLaunchKernelGGL((channel_stats_kernel<0>), dim3((unsigned)tot.blocks), dim3(256), 0, ST, table, n_jobs, out, ws);
    else hipLaunchKernelGGL((channel_stats_kernel<1>), dim3((unsigned)tot.blocks), dim3(256), 0, ST, table, n_jobs, out, ws);
    if (tot.segmented)
        hipLaunchKernelGGL(channel_stats_finish_kernel, dim3((unsigned)((tot.n_channels + 255) / 256)), dim3(256), 0, ST, table, n_jobs,
                           tot.n_channels, out, ws);
    VD_LAUNCH_CHECK("vd_channel_stats");
    return 0;
}

extern "C" int vd_neuron_keep_rows(float* buf, const int64_t* table, int n_jobs, int64_t total_blocks, const float* keep, void* stream) {
    VD_REQUIRE(buf && table && keep, "vd_neuron_keep_rows: null pointer");
    VD_REQUIRE((((uintptr_t)buf) & 3) == 0, "vd_neuron_keep_rows: buf not 4-byte aligned");
    VD_REQUIRE(n_jobs > 0 && total_blocks > 0 && total_blocks < (1ll << 31), "vd_neuron_keep_rows: bad args");
    hipLaunchKernelGGL(neuron_keep_rows_kernel, dim3((unsigned)total_blocks), dim3(256), 0, ST, buf, table, n_jobs, keep);
    VD_LAUNCH_CHECK("vd_neuron_keep_rows");
    return 0;
}
