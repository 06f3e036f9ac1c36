// ---- split-precision weight gradient of a 1x1 convolution on WIDE tiles (round 3) ---------------------------------------------
// Included by vd_wgrad_bx3.inc after wgrad1x1_bx3_body (same namespace, same plain [z][M][C] slabs, same job table and reduce grid).
//
// The grouped 1x1 launch on wgrad1x1_bx3_body's 128 x 128 tiles (retired) was the one HBM-bound MFMA kernel of the training step: 6.6 TB/s of FETCH + WRITE traffic, 2.28 x its
// algorithmic bytes (profiles/r02_pmc_traffic.json, r03_pmc_traffic.json) -- a 128 x 128 tile re-reads the dY rows once per 128 channels of
// X and the X rows once per 128 rows of dY, and K (the pixels) is so long that every re-read comes from beyond L2.  A BM x 256 tile
// (BM = 256 when the layer has more than 128 output channels, else 128) loads (BM + 256) rows per BM x 256 outputs: 0.50 x (256 x 256) or
// 0.75 x (128 x 256) of the bytes per FLOP.  Eight waves (2 x 4, wave tile BM/2 x 64), one workgroup per CU; a K-step is 32 pixels (4 octets;
// NP % 8 == 0, an octet never straddles images), the 64 / 48 KB stage is double-buffered: one barrier per K-step.
//     As[buf][part][octet 0..3][BM + 2]     Bs[buf][part][octet 0..3][258]       (octet stride + 2 units: as wgrad1x1_bx3_body)
// ONE (vd_wgrad_desc.math = 3, opt-in bf16 mixed precision): the same (hi, lo) stages, hi fragments only: one bf16 MFMA (ah * bh) per product term.
template <int BM, bool ONE = false>
__device__ __forceinline__ void wgrad1x1_wide_body(const vd_wgrad_desc& d, int ksteps_per_split, int gx, int gy, int lin) {
    constexpr int BC = 256;
    constexpr int LDA_ = BM + 2, LDB_ = BC + 2;
    constexpr int A_U = 2 * 4 * LDA_, B_U = 2 * 4 * LDB_;
    constexpr int WM = BM / 64;                    // 32-row blocks per wave: 2 (BM = 128) or 4 (BM = 256)
    constexpr int AI = BM / 128;                   // dY rows per thread
    extern __shared__ u32x4 wide_lds[];
    u32x4* __restrict__ As = wide_lds;             // [2][A_U]
    u32x4* __restrict__ Bs = wide_lds + 2 * A_U;   // [2][B_U]

    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_m = (d.M + BM - 1) / BM;
    const int bxx = lin % gx, by = lin / gx;
    const int tm = bxx % tiles_m, tc = bxx / tiles_m;
    const int m0 = tm * BM, c0 = tc * BC;
    const int oct_per_img = d.NP >> 3;
    const int oct_total = d.nb * oct_per_img;
    const int ks_total = (oct_total + 3) >> 2;
    const int ks_begin = by * ksteps_per_split;
    const int ks_end = min(ks_total, ks_begin + ksteps_per_split);

    const int so = tid & 3, sr = tid >> 2;         // staging: octet of the K-step, row (m or c) sr + 128 i
    f32x4 ra[2 * AI], rb[4];
    bool oct_ok = false;
    unsigned rowa[AI], rowb[2];
#pragma unroll
    for (int i = 0; i < AI; ++i) rowa[i] = 4u * (unsigned)(min(m0 + sr + 128 * i, d.M - 1) * d.NP);
#pragma unroll
    for (int i = 0; i < 2; ++i) rowb[i] = 4u * (unsigned)(min(c0 + sr + 128 * i, d.C - 1) * d.NP);
    auto load_stage = [&](int ks) {
        const int g = ks * 4 + so;                 // global octet -> (image, pixel)
        oct_ok = g < oct_total;
        const int gg = oct_ok ? g : oct_total - 1;   // (clamped, not 0: an image BEFORE the step's first one would give a negative offset from its descriptor base)
        const int b = gg / oct_per_img, p = (gg - b * oct_per_img) * 8;
        const int b0 = min(ks * 4, oct_total - 1) / oct_per_img;
        const __amdgpu_buffer_rsrc_t dyr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.dY + (int64_t)b0 * d.dy_bstride), 0, 0xFFFFFFF0, 0x00020000);
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.X + (int64_t)b0 * d.x_bstride), 0, 0xFFFFFFF0, 0x00020000);
        const unsigned va = 4u * (unsigned)((b - b0) * d.dy_bstride + p), vb = 4u * (unsigned)((b - b0) * d.x_bstride + p);
#pragma unroll
        for (int i = 0; i < AI; ++i) {
            ra[2 * i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyr, va + rowa[i], 0, 0));
            ra[2 * i + 1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyr, va + rowa[i] + 16u, 0, 0));
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            rb[2 * i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, vb + rowb[i], 0, 0));
            rb[2 * i + 1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, vb + rowb[i] + 16u, 0, 0));
        }
    };
    auto store_stage = [&](int buf) {
        u32x4* __restrict__ as_ = As + buf * A_U;
        u32x4* __restrict__ bs_ = Bs + buf * B_U;
#pragma unroll
        for (int i = 0; i < AI; ++i) {
            const bool aok = oct_ok && (m0 + sr + 128 * i < d.M);
            float va[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                va[j] = aok ? ra[2 * i][j] : 0.f;
                va[4 + j] = aok ? ra[2 * i + 1][j] : 0.f;
            }
            u32x4 hi, lo;
            split_bf16x8(va, hi, lo);
            as_[so * LDA_ + sr + 128 * i] = hi;
            as_[(4 + so) * LDA_ + sr + 128 * i] = lo;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bool bok = oct_ok && (c0 + sr + 128 * i < d.C);
            float vb[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                vb[j] = bok ? rb[2 * i][j] : 0.f;
                vb[4 + j] = bok ? rb[2 * i + 1][j] : 0.f;
            }
            u32x4 hi, lo;
            split_bf16x8(vb, hi, lo);
            bs_[so * LDB_ + sr + 128 * i] = hi;
            bs_[(4 + so) * LDB_ + sr + 128 * i] = lo;
        }
    };

    f32x16 acc[WM][2];
#pragma unroll
    for (int mi = 0; mi < WM; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[mi][ni][v] = 0.f;

    const int wm = wave >> 2, wc = wave & 3;       // 2 x 4 waves: BM/2 rows x 64 channels each
    const int a_rd = h * LDA_ + wm * (BM / 2) + l31, b_rd = h * LDB_ + wc * 64 + l31;

    if (ks_begin < ks_end) {
        load_stage(ks_begin);
        store_stage(0);
        __syncthreads();
        int buf = 0;
        for (int ks = ks_begin; ks < ks_end; ++ks) {
            const bool more = ks + 1 < ks_end;
            if (more) load_stage(ks + 1);
            const u32x4* __restrict__ a_base = As + buf * A_U + a_rd;
            const u32x4* __restrict__ b_base = Bs + buf * B_U + b_rd;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {       // 16 pixels = octets 2kk (lanes 0-31) and 2kk+1 (lanes 32-63)
                bf16x8 ah[WM], al[WM];
#pragma unroll
                for (int mi = 0; mi < WM; ++mi) {
                    ah[mi] = __builtin_bit_cast(bf16x8, a_base[(2 * kk) * LDA_ + mi * 32]);
                    if constexpr (!ONE) al[mi] = __builtin_bit_cast(bf16x8, a_base[(4 + 2 * kk) * LDA_ + mi * 32]);
                }
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    const bf16x8 bh = __builtin_bit_cast(bf16x8, b_base[(2 * kk) * LDB_ + ni * 32]);
                    bf16x8 bl;
                    if constexpr (!ONE) bl = __builtin_bit_cast(bf16x8, b_base[(4 + 2 * kk) * LDB_ + ni * 32]);
#pragma unroll
                    for (int mi = 0; mi < WM; ++mi) {
                        if constexpr (!ONE) {
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mi], bh, acc[mi][ni], 0, 0, 0);
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bl, acc[mi][ni], 0, 0, 0);
                        }
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bh, acc[mi][ni], 0, 0, 0);
                    }
                }
            }
            if (more) store_stage(buf ^ 1);        // the other stage was last read in the previous step, which every wave left at the barrier
            __syncthreads();
            buf ^= 1;
        }
    }
    float* __restrict__ out = (gy > 1) ? (d.ws + (int64_t)by * d.M * d.C) : d.dW;
    const bool accum = (gy == 1) && d.accumulate;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int c = c0 + wc * 64 + ni * 32 + l31;
        if (c >= d.C) continue;
#pragma unroll
        for (int mi = 0; mi < WM; ++mi)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int m = m0 + wm * (BM / 2) + mi * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
                if (m >= d.M) continue;
                const int64_t off = (int64_t)m * d.C + c;
                out[off] = accum ? (out[off] + acc[mi][ni][v]) : acc[mi][ni][v];
            }
    }
}

// BM is a property of the JOB (layers with at most 128 output channels take the 128-row tile), so one launch serves mixed groups.
template <bool ONE = false>
__global__ __launch_bounds__(512, 2) void wgrad1x1_wide_group_kernel(const vd_wgrad_job* __restrict__ jobs, int n_jobs) {
    const vd_wgrad_job* __restrict__ jb = jobs + wgrad_find_job(jobs, n_jobs, blockIdx.x, false);
    const int lin = blockIdx.x - jb->first_block;
    if (lin >= jb->gx * jb->gy) return;
    const vd_wgrad_desc d = jb->d;
    if (d.M > 128) wgrad1x1_wide_body<256, ONE>(d, jb->ks_per, jb->gx, jb->gy, lin);
    else wgrad1x1_wide_body<128, ONE>(d, jb->ks_per, jb->gx, jb->gy, lin);
}

constexpr int W1X1_WIDE_LDS = 2 * (2 * 4 * (256 + 2) + 2 * 4 * (256 + 2)) * 16;      // 132 096 B (BM = 256)

static inline int wgrad1x1_wide_bm(const vd_wgrad_desc& d) { return d.M > 128 ? 256 : 128; }
