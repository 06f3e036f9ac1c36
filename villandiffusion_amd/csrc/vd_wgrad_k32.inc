// ---- split-precision 3x3 weight gradient on v_mfma_f32_16x16x32_bf16 (round 3) -------------------------------------------
// Included by vd_wgrad_bx3.inc (same namespace; same tile geometry, grid, split-K plan, slab layout and job table as wgrad_bx3_body, so
// wgrad_patch_plan / slab_reduce_perm_kernel / wgrad_group_reduce_kernel are shared).
//
// What changes against wgrad_bx3_body (8x8 / 16x16 / 32x32 outputs, plain and upsample-fused):
//  * One MFMA contracts the whole K-step: 32 pixels = the four pixel octets of the step, k-group g = lane >> 4 = octet g.
//    (The chip holds a higher clock on this instruction shape.)
//  * X is written to LDS ONCE, not three times.  The old kernel stored three copies of the X tile shifted by the horizontal tap (24 of
//    its 40 KB of LDS stores per K-step, and 12 of its 20 fragment reads per wave); at three workgroups per CU those stores kept the LDS
//    busier than the MFMAs kept the matrix pipe.  Here a lane reads the aligned octet of its channel and builds the two shifted fragments
//    in registers: the pixel left of the octet is the last bf16 of k-group g - 1's fragment (lane - 16), the pixel right of it the first
//    of k-group g + 1's (lane + 16) -- two ds_bpermute per operand half -- and the shifted octets are v_alignbit re-packings (zero beyond
//    the row ends, as the padding demands).  That VALU work rides in the shadow of the 72 MFMAs of the step.
//  * LDS per stage drops to 24 KB, so the stage is double-buffered: ONE barrier per K-step instead of two.
//  * Units are XOR-swizzled inside their group of eight rows (row ^ 2 * octet): the eight lanes of a ds_write_b128 service group
//    (four octets of two rows) and the 16-lane halves of a ds_read_b128 group (two k-groups of 16 rows) then each hit distinct bank quads
//    with an octet stride that is a multiple of 16 units.
// ONE (vd_wgrad_desc.math = 3, opt-in bf16 mixed precision): the stages are staged as (hi, lo) all the same; the loop reads the hi fragments only and
// issues ah * xh -- one bf16 MFMA per product term.
template <int W, int MODE, bool ONE = false>   // W: 8 | 16 | 32 (output width = pixels per image row); MODE 0: CONV3, 2: CONV3_UP (X is the half-resolution source)
__device__ __forceinline__ void wgrad_k32_body(const vd_wgrad_desc& d, int ksteps_per_split, int gx, int gy, int lin) {
    constexpr int ROWS = 32 / W;                   // image rows per K-step
    constexpr int OPR = W / 8;                     // octets per row
    constexpr int CT = 64;
    constexpr int A_U = 2 * 4 * 128, B_U = 2 * 4 * CT;      // 16-byte units per stage: [part][octet][row]
    __shared__ u32x4 As[2 * A_U];                  // 32 KB
    __shared__ u32x4 Bs[2 * B_U];                  // 16 KB

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, l15 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_m = (d.M + 127) / 128;
    int bx = lin % gx, by = lin / gx;              // XCD-aware remap (see wgrad_patch_kernel)
    {
        const int T = gx * gy;
        if ((T & 7) == 0) {
            const int v = (lin & 7) * (T >> 3) + (lin >> 3);
            bx = v % gx;
            by = v / gx;
        }
    }
    const int r = bx % 3;
    const int rest = bx / 3;
    const int tm = rest % tiles_m, tc = rest / tiles_m;
    const int m0 = tm * 128, c0 = tc * CT;
    const int steps_per_img = d.OH / ROWS;
    const int ks_total = d.nb * steps_per_img;
    const int ks_begin = by * ksteps_per_split;
    const int ks_end = min(ks_total, ks_begin + ksteps_per_split);
    const int HWs = d.H * d.W;

    // staging roles: lanes run along the 4 octets of the K-step (128 contiguous bytes of a dY row), then along rows m / channels c
    const int so = tid & 3;
    const int s_rr = so / OPR, s_xo = so - s_rr * OPR;
    const int am = tid >> 2;                       // A: rows am and am + 64;  B: channel am
    const bool a_ok0 = m0 + am < d.M, a_ok1 = m0 + am + 64 < d.M;
    const bool b_ok = c0 + am < d.C;
    const unsigned a_voff0 = 4u * (unsigned)((int64_t)min(m0 + am, d.M - 1) * d.NP + 8 * so);
    const unsigned a_voff1 = 4u * (unsigned)((int64_t)min(m0 + am + 64, d.M - 1) * d.NP + 8 * so);
    const unsigned b_voff = 4u * (unsigned)((int64_t)min(c0 + am, d.C - 1) * HWs + (MODE == 2 ? 4 : 8) * s_xo);
    const int a_dst0 = so * 128 + (am ^ (2 * so)), a_dst1 = so * 128 + ((am + 64) ^ (2 * so));
    const int b_dst = so * CT + (am ^ (2 * so));

    // TWO register sets (round 4): the loads of step ks + 2 are issued at the top of step ks, so a store never waits for memory.  In-kernel stamps of
    // the one-set kernels (profiles/r04_wgrad_stamps.txt) put 2150 of a step's 4750 cycles into convert + store, most of it the wait for loads
    // issued only one MFMA phase earlier.
    f32x4 ra0[4], rb0[2], ra1[4], rb1[2];
    bool row_ok0 = false, row_ok1 = false;
    auto load_stage = [&](int ks, f32x4 (&ra)[4], f32x4 (&rb)[2], bool& row_ok) {
        const int b = ks / steps_per_img;
        const int y0 = (ks - b * steps_per_img) * ROWS;
        const __amdgpu_buffer_rsrc_t dyr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.dY + (int64_t)b * d.dy_bstride + y0 * W), 0, 0xFFFFFFF0, 0x00020000);
        ra[0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyr, a_voff0, 0, 0));
        ra[1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyr, a_voff0 + 16u, 0, 0));
        ra[2] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyr, a_voff1, 0, 0));
        ra[3] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyr, a_voff1 + 16u, 0, 0));
        int iy = y0 + s_rr + r - 1;
        if (MODE == 2) {                           // row of the (virtual) upsampled image -> source row
            row_ok = (unsigned)iy < (unsigned)(2 * d.H);
            iy >>= 1;
        } else {
            row_ok = (unsigned)iy < (unsigned)d.H;
        }
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.X + (int64_t)b * d.x_bstride), 0, 0xFFFFFFF0, 0x00020000);
        const unsigned xv = row_ok ? b_voff + 4u * (unsigned)(iy * d.W) : 0xFFFFFFFFu;      // a row outside the image is out of range: reads 0
        rb[0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, xv, 0, 0));
        if (MODE != 2) rb[1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, xv + 16u, 0, 0));
    };
    auto store_stage = [&](int buf, const f32x4 (&ra)[4], const f32x4 (&rb)[2], bool row_ok) {
        u32x4* __restrict__ as_ = As + buf * A_U;
        u32x4* __restrict__ bs_ = Bs + buf * B_U;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bool ok = i ? a_ok1 : a_ok0;
            float v[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = ok ? ra[2 * i][j] : 0.f;
                v[4 + j] = ok ? ra[2 * i + 1][j] : 0.f;
            }
            u32x4 hi, lo;
            split_bf16x8(v, hi, lo);
            as_[i ? a_dst1 : a_dst0] = hi;
            as_[4 * 128 + (i ? a_dst1 : a_dst0)] = lo;
        }
        const bool ok = b_ok && row_ok;
        float e[8];
        if (MODE == 2) {                           // 8 upsampled pixels = 4 source pixels, each twice
#pragma unroll
            for (int j = 0; j < 4; ++j) e[2 * j] = e[2 * j + 1] = ok ? rb[0][j] : 0.f;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                e[j] = ok ? rb[0][j] : 0.f;
                e[4 + j] = ok ? rb[1][j] : 0.f;
            }
        }
        u32x4 hi, lo;
        split_bf16x8(e, hi, lo);
        bs_[b_dst] = hi;
        bs_[4 * CT + b_dst] = lo;
    };

    f32x4 acc[4][2][3];                            // [m tile][c tile][tap s]
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int sx = 0; sx < 3; ++sx) acc[mt][ct][sx] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int wm = wave >> 1, wc = wave & 1;       // 2 x 2 waves: 64 m x 32 c each
    const int a_rd = g * 128 + wm * 64 + (l15 ^ (2 * g));
    const int b_rd = g * CT + wc * 32 + (l15 ^ (2 * g));
    const bool left_ok = (g % OPR) != 0, right_ok = (g % OPR) != OPR - 1;     // the octet's neighbours inside its image row (else: zero padding)

    // fragments of taps s = 0 (pixels x - 1) and s = 2 (pixels x + 1) from the aligned octet c = (p0 p1 | p2 p3 | p4 p5 | p6 p7)
    auto shifted = [&](const u32x4& c, u32x4& fl, u32x4& fr) {
        unsigned L = (unsigned)__shfl_up((int)c[3], 16, 64);      // k-group g - 1: (p-2 p-1)
        unsigned R = (unsigned)__shfl_down((int)c[0], 16, 64);    // k-group g + 1: (p8 p9)
        L = left_ok ? L : 0u;
        R = right_ok ? R : 0u;
        const unsigned m01 = __builtin_amdgcn_alignbit(c[1], c[0], 16), m12 = __builtin_amdgcn_alignbit(c[2], c[1], 16),
                       m23 = __builtin_amdgcn_alignbit(c[3], c[2], 16);
        fl = u32x4{__builtin_amdgcn_alignbit(c[0], L, 16), m01, m12, m23};
        fr = u32x4{m01, m12, m23, __builtin_amdgcn_alignbit(R, c[3], 16)};
    };

    auto compute = [&](int buf) {
            const u32x4* __restrict__ as_ = As + buf * A_U + a_rd;
            const u32x4* __restrict__ bs_ = Bs + buf * B_U + b_rd;
            bf16x8 ah[4], al[4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                ah[mt] = __builtin_bit_cast(bf16x8, as_[mt * 16]);
                if constexpr (!ONE) al[mt] = __builtin_bit_cast(bf16x8, as_[4 * 128 + mt * 16]);
            }
            // both channel tiles' fragments and their neighbour exchanges are issued up front; the centre tap (which needs no exchange)
            // multiplies first, so the ds_bpermute round trips of the shifted fragments hide under 24 MFMAs
            u32x4 fh[2][3], fl[2][3];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                fh[ct][1] = bs_[ct * 16];
                if constexpr (!ONE) fl[ct][1] = bs_[4 * CT + ct * 16];
            }
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                shifted(fh[ct][1], fh[ct][0], fh[ct][2]);
                if constexpr (!ONE) shifted(fl[ct][1], fl[ct][0], fl[ct][2]);
            }
#pragma unroll
            for (int o = 0; o < 3; ++o) {
                const int sx = o == 0 ? 1 : (o == 1 ? 0 : 2);
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const bf16x8 xh = __builtin_bit_cast(bf16x8, fh[ct][sx]);
                    // the three products of a tile are a dependency chain on its accumulator: walk the four m tiles inside each product, so that
                    // an MFMA's accumulator was written four issues (64 cycles) earlier, not by the instruction in front of it
                    if constexpr (!ONE) {
                        const bf16x8 xl = __builtin_bit_cast(bf16x8, fl[ct][sx]);
#pragma unroll
                        for (int mt = 0; mt < 4; ++mt) acc[mt][ct][sx] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[mt], xh, acc[mt][ct][sx], 0, 0, 0);
#pragma unroll
                        for (int mt = 0; mt < 4; ++mt) acc[mt][ct][sx] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mt], xl, acc[mt][ct][sx], 0, 0, 0);
                    }
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) acc[mt][ct][sx] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mt], xh, acc[mt][ct][sx], 0, 0, 0);
                }
                if (o == 0) __builtin_amdgcn_sched_barrier(0);
            }
    };
#ifdef VD_WG_PRIO         // experiment: the two workgroups of a CU in anti-phase by static priority (wave slot parity from HW_ID)
    if ((__builtin_amdgcn_s_getreg((31 << 11) | 4) & 1u) == 0u) __builtin_amdgcn_s_setprio(3);
#endif
#ifdef VD_WG_STAMPS
    const unsigned long long rt_begin = __builtin_amdgcn_s_memrealtime();
    WG_STAMP(cy_begin);
    unsigned long long sL = 0, sM = 0, sS = 0, sB2 = 0;
#endif
    if (ks_begin < ks_end) {
        // steps in pairs (straight-line body, no exit in the middle): buffer 0 / set 0 hold the even steps of the range, buffer 1 / set 1 the odd ones
        // every load is issued UNCONDITIONALLY (past the end: the last step again, never stored): a load under a branch makes the compiler wait
        // for vmcnt(0) at the next store, i.e. for the set that was issued a moment ago as well
        const int ks_last = ks_end - 1;
        load_stage(ks_begin, ra0, rb0, row_ok0);
        load_stage(min(ks_begin + 1, ks_last), ra1, rb1, row_ok1);
        store_stage(0, ra0, rb0, row_ok0);
        __syncthreads();
        int ks = ks_begin;
        while (ks + 1 < ks_end) {
#ifdef VD_WG_STAMPS
            WG_STAMP(t0);
#endif
            load_stage(min(ks + 2, ks_last), ra0, rb0, row_ok0);
            __builtin_amdgcn_sched_barrier(0);
#ifdef VD_WG_STAMPS
            WG_STAMP(t1);
#endif
            compute(0);
            __builtin_amdgcn_sched_barrier(0);
#ifdef VD_WG_STAMPS
            WG_STAMP(t2);
#endif
            store_stage(1, ra1, rb1, row_ok1);                     // the other stage was last read in the previous step, which every wave left at the barrier
#ifdef VD_WG_STAMPS
            WG_STAMP(t3);
#endif
            __syncthreads();
#ifdef VD_WG_STAMPS
            WG_STAMP(t4);
            sL += t1 - t0, sM += t2 - t1, sS += t3 - t2, sB2 += t4 - t3;
#endif
            load_stage(min(ks + 3, ks_last), ra1, rb1, row_ok1);
            __builtin_amdgcn_sched_barrier(0);
            compute(1);
            __builtin_amdgcn_sched_barrier(0);
            store_stage(0, ra0, rb0, row_ok0);                     // (beyond the range: a copy nobody reads)
            __syncthreads();
            ks += 2;
        }
        if (ks < ks_end) compute(0);                               // odd count: the last step sits in buffer 0
    }

#ifdef VD_WG_STAMPS
    WG_STAMP(cy_loop);
    if (g_wg_stamps && lane == 0) {      // (only the even half-steps are stamped: sums over (ks_end - ks_begin) / 2 steps)
        unsigned long long* __restrict__ o = g_wg_stamps + ((int64_t)blockIdx.x * 4 + wave) * 12;
        o[0] = rt_begin, o[1] = __builtin_amdgcn_s_memrealtime(), o[2] = cy_begin, o[3] = cy_loop, o[4] = cy_loop;
        o[5] = sL, o[6] = sM, o[7] = 0, o[8] = sS, o[9] = sB2, o[10] = (unsigned long long)((ks_end - ks_begin) / 2), o[11] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4);
    }
#endif
    // ---- store: lane (g, l15) holds rows m = 4 g + {0..3} of column c = l15 of every 16 x 16 tile ----
    const int Ncols = d.C * 9;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int c = c0 + wc * 32 + ct * 16 + l15;
        if (c >= d.C) continue;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int m = m0 + wm * 64 + mt * 16 + 4 * g + v;
                if (m >= d.M) continue;
                if (gy > 1) {                      // split-K slab ws[z][r][m][c][3] (slab_reduce_perm_kernel / wgrad_group_reduce_kernel un-permute)
                    float* __restrict__ o = d.ws + (int64_t)by * d.M * Ncols + (int64_t)r * d.M * d.C * 3 + ((int64_t)m * d.C + c) * 3;
#pragma unroll
                    for (int sx = 0; sx < 3; ++sx) o[sx] = acc[mt][ct][sx][v];
                } else {
                    float* __restrict__ o = d.dW + (int64_t)m * Ncols + c * 9 + r * 3;
#pragma unroll
                    for (int sx = 0; sx < 3; ++sx) o[sx] = d.accumulate ? (o[sx] + acc[mt][ct][sx][v]) : acc[mt][ct][sx][v];
                }
            }
    }
}

template <int W, int MODE>
__global__ __launch_bounds__(NT, 2) void wgrad_k32_kernel(const vd_wgrad_desc d, int ksteps_per_split) {
    wgrad_k32_body<W, MODE>(d, ksteps_per_split, gridDim.x, gridDim.y, blockIdx.x + gridDim.x * blockIdx.y);
}

template <int W, int MODE, bool ONE = false>
__global__ __launch_bounds__(NT, 2) void wgrad_k32_group_kernel(const vd_wgrad_job* __restrict__ jobs, int n_jobs) {
    const vd_wgrad_job* __restrict__ jb = jobs + wgrad_find_job(jobs, n_jobs, blockIdx.x, false);
    const int lin = blockIdx.x - jb->first_block;
    if (lin >= jb->gx * jb->gy) return;            // padding blocks between jobs
    const vd_wgrad_desc d = jb->d;
    wgrad_k32_body<W, MODE, ONE>(d, jb->ks_per, jb->gx, jb->gy, lin);
}

// Round 3 (one register set, loads one step ahead): 0.93-0.97 x of wgrad_bx3_body on seven of the eight layer shapes of config #2 -- the halved LDS
// traffic and the single barrier did not pay for dropping from three workgroups per CU to two.  Round 4 (two register sets, loads two steps ahead,
// every load unconditional so that the stores wait with vmcnt(6), 234 VGPRs): 1.02 x (1.45 / 1.23 ms against 1.48 / 1.26 for the grouped 32x32 /
// 16x16 launches, training step -0.5 % on three same-box pairs) -- the only kernel of the classes it takes since then (the three-copy kernel's
// instantiations for them are retired).  In-kernel stamps (profiles/r04_wgrad_stamps.txt): both kernels sit on the same ~1.4 ms for config #2's ten 32x32 layers at a matrix-pipe
// utilisation of 64 % (1.9 GHz) vs 73 % (1.65 GHz) -- util x clock is the invariant, i.e. the launch is power-limited; static priorities that put
// the two workgroups of a CU in anti-phase and re-ordered MFMA dependency chains moved single workgroups but not the launch.
