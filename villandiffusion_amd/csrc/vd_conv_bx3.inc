// ---- split-precision ("bf16x3") 3x3 convolution on the bf16 matrix cores -------------------------------------------------
// Included by vd_gemm.hip inside its anonymous namespace (shares gemm_epilogue / splitk_epilogue_kernel / NT).
//
// The f32-input MFMA runs at 1/16 of the bf16 MFMA rate (157 vs 2500 TFLOP/s).  An f32 value is the sum of two bf16 values
// to 16 significant bits:  x = hi + lo + O(2^-17 |x|),  hi = bf16(x), lo = bf16(x - hi).  A product a*b is then
//     a_hi*b_hi + a_hi*b_lo + a_lo*b_hi        (the dropped a_lo*b_lo term is O(2^-16 |ab|))
// i.e. THREE v_mfma_f32_32x32x16_bf16 per 16-deep k-slab, accumulated in f32: 96 cycles where the f32 MFMA needs 512.  The
// result agrees with the exact-f32 kernel to ~1e-5 relative (the path's tolerance is 1e-3, north_star; the reference itself
// trains this configuration under fp16 autocast, VillanDiffusion.py:261-262).  Opt-in per call: the caller passes the
// pre-split weights (vd_conv3_pack_weights) in vd_gemm_desc.a_packed; without it vd_gemm stays on the exact-f32 kernels.
//
// Packed weights (global, 16-byte units of 8 bf16 = the k-octet of one lane of the MFMA A operand):
//     unit index = ((((cc*9 + t)*2 + part)*2 + q)*Mpad + m)      cc: 16-channel chunk, t: tap, part: hi/lo, q: k-octet
//     element j of the unit = channel cc*16 + q*8 + j            (Mpad = M rounded up to 128, zero rows beyond M)
// LDS per workgroup (128 output channels x 64*WN pixels of one image / IMGS whole small images):
//     As[buf][s][part][q][128 m]   one tap ROW (3 taps) of the current chunk, 24 KB (x2: double-buffered), a straight copy of 12 runs of 2 KB
//     Ps[part][q][PLANE pix]  the zero-padded halo patch of the chunk's 16 channels, split once when it is written
// Both images are read with ONE conflict-free ds_read_b128 per fragment: 32 lanes = 32 consecutive rows (A) or 32
// consecutive pixels of an image row (B), 16 bytes each; tap shifts move the B address by whole 16-byte units.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int XC = 16;                                           // channels per chunk = K of one MFMA

__device__ __forceinline__ void split_bf16x8(const float (&v)[8], u32x4& hi, u32x4& lo) {
    bf16x8 h, l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const __bf16 t = (__bf16)v[j];
        h[j] = t;
        l[j] = (__bf16)(v[j] - (float)t);
    }
    hi = __builtin_bit_cast(u32x4, h);
    lo = __builtin_bit_cast(u32x4, l);
}

// element (m, c, t) of the logical [M][C][9] operand sits at src[m*rs + c*cs + t]  (plain: rs = lda, cs = 9; the transposed
// operand of the stride-1 dgrad, A'[c_in][m_out] = W[m_out][c_in]: rs = 9, cs = lda).  One thread owns (m, chunk, k-octet): it
// reads the 9 taps of its 8 channels (plain layout: 288 contiguous bytes per thread; transposed: 36 contiguous bytes per channel,
// consecutive across lanes) and writes 9 x (hi, lo) 16-byte units, lanes along m (coalesced).
template <int T>   // T = 9 (3x3) or 1 (1x1 convolution / linear layer: the [M][C] matrix itself)
__device__ __forceinline__ void conv3_pack_one(const float* __restrict__ src, u32x4* __restrict__ dst, int M, int C, int Mpad, int64_t rs,
                                               int64_t cs, int local) {
    if (local >= Mpad * (C / XC) * 2) return;
    const int m = local % Mpad;
    const int rest = local / Mpad;
    const int q = rest & 1, cc = rest >> 1;
    float v[8][T];
    const float* __restrict__ s0 = src + (int64_t)(m < M ? m : 0) * rs + (int64_t)(cc * XC + q * 8) * cs;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int t = 0; t < T; ++t) v[j][t] = s0[(int64_t)j * cs + t];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        float w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = (m < M) ? v[j][t] : 0.f;
        u32x4 hi, lo;
        split_bf16x8(w, hi, lo);
        const int64_t base = ((int64_t)(cc * T + t) * 4 + q) * Mpad + m;
        dst[base] = hi;
        dst[base + 2 * (int64_t)Mpad] = lo;
    }
}

__global__ __launch_bounds__(256) void conv3_pack_kernel(const float* __restrict__ src, u32x4* __restrict__ dst, int M, int C, int Mpad,
                                                         int64_t rs, int64_t cs, int T) {
    if (T == 9) conv3_pack_one<9>(src, dst, M, C, Mpad, rs, cs, blockIdx.x * 256 + threadIdx.x);
    else conv3_pack_one<1>(src, dst, M, C, Mpad, rs, cs, blockIdx.x * 256 + threadIdx.x);
}

// All convolutions of a network in one launch: table[j] = {src, dst, M, C, row_stride, chan_stride, first block of job j, taps};
// a workgroup belongs to exactly one job (each job's thread count is rounded up to whole workgroups by the caller).
__global__ __launch_bounds__(256) void conv3_pack_multi_kernel(const int64_t* __restrict__ table, int n_jobs) {
    int lo = 0, hi = n_jobs - 1;
    const int64_t blk = blockIdx.x;
    while (lo < hi) {                                            // last job whose first block <= blk (block-uniform)
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid * 8 + 6] <= blk) lo = mid;
        else hi = mid - 1;
    }
    const int64_t* __restrict__ jb = table + lo * 8;
    const int M = (int)jb[2], C = (int)jb[3];
    const int local = (int)(blk - jb[6]) * 256 + threadIdx.x;
    if (jb[7] == 1)
        conv3_pack_one<1>(reinterpret_cast<const float*>(jb[0]), reinterpret_cast<u32x4*>(jb[1]), M, C, (M + 127) / 128 * 128, jb[4], jb[5], local);
    else
        conv3_pack_one<9>(reinterpret_cast<const float*>(jb[0]), reinterpret_cast<u32x4*>(jb[1]), M, C, (M + 127) / 128 * 128, jb[4], jb[5], local);
}

// Wave layouts: (NTH 256, WM 2) four waves of 64 x 64 -> 128 x 128 tile, 2 workgroups per CU; (512, 1) eight waves of 32 x 64, same tile, 4 waves per
// SIMD; (512, 2) eight waves of 64 x 64 -> 128 x 256 tile, one workgroup per CU: the weight operand is fetched (L2) and stored (LDS) once per 256 pixels.
// MODE 4 (stride 2, round 3): output pixel (y, x) reads input (2y + r - pad, 2x + s - pad).  The patch keeps the even and the odd input columns in
// separate halves of a row -- unit [row][parity][column >> 1] -- so that the 32 consecutive output pixels of a fragment still read 32 consecutive
// 16-byte units for every tap: tap (r, s) is the lane-uniform offset r * PW + (s & 1) * (W + 1) + (s >> 1) from the pixel's base unit (2 ty) * PW + x.
template <int W, int MODE, int WN, int NTH = NT, int WM = (NTH == 512 ? 1 : 2)>   // MODE 0: CONV3, 1: CONV3_T (flipped taps), 2: CONV3_UP (source at half resolution), 3: CONV3 of silu(GroupNorm(x)) (d.gn_ss), 4: CONV3_S2
__global__ __launch_bounds__(NTH, WM == 2 ? 2 : 4) void conv3_bx3_kernel(const vd_gemm_desc d, int chunks_per_split) {
    constexpr int BM = 128;
    constexpr int WAVES_N = (NTH / 64) / (BM / (32 * WM));
    constexpr int NPIX = WAVES_N * 32 * WN;
    constexpr int IMGS = (W * W >= NPIX) ? 1 : NPIX / (W * W);
    constexpr int TR = (IMGS == 1) ? NPIX / W : W;
    constexpr int PWH = W + 1;                                    // MODE 4: units per column parity
    constexpr int PW = (MODE == 4) ? 2 * PWH : W + 2, PR = (MODE == 4) ? 2 * TR + 1 : TR + 2, PIMG = PR * PW, PLANE = IMGS * PIMG;
    constexpr int A_UNITS = 3 * 2 * 2 * BM;                      // 1536 16-byte units per tap row
    constexpr int A_IT = A_UNITS / NTH;                           // 6
    constexpr int P_ITEMS = 2 * PLANE;                           // (k-octet, pixel) items per chunk
    constexpr int P_IT = (P_ITEMS + NTH - 1) / NTH;
    __shared__ u32x4 As[2 * A_UNITS];                             // double-buffered: one barrier per tap-row step
    __shared__ u32x4 Ps[4 * PLANE];
    __shared__ float Sab[(MODE == 3) ? 2 * 1024 : 2];            // MODE 3: (scale, shift) per input channel of this tile's image

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
    const int tiles_m = (d.M + BM - 1) / BM;
    int bid = blockIdx.x;
    {
        const int nwg = gridDim.x;
        if ((nwg & 7) == 0) bid = (bid & 7) * (nwg >> 3) + (bid >> 3);
    }
    const int tm = bid % tiles_m, tn = bid / tiles_m;
    const int m0 = tm * BM, n0 = tn * NPIX;
    int b0, y0, x0 = 0;
    if (IMGS == 1) {
        // W is the TILE width: for images wider than 32 px a tile is two full 64-pixel rows (W = 64) or one 128-pixel row
        // segment starting at column x0 (W = 128, OW % 128 == 0) -- NPIX consecutive pixels in row-major order either way.
        const int tiles_per_img = d.NP / NPIX;
        b0 = tn / tiles_per_img;
        const int pix0 = (tn - b0 * tiles_per_img) * NPIX;
        y0 = pix0 / d.OW;
        x0 = pix0 - y0 * d.OW;
    } else {
        b0 = tn * IMGS;
        y0 = 0;
    }
    const u32x4* __restrict__ Apk = reinterpret_cast<const u32x4*>(d.a_packed);
    const int Mpad = d.a_packed_mpad;
    const float* __restrict__ Xb = d.B + (int64_t)b0 * d.b_bstride;
    const int HWs = d.H * d.W;
    const int nb_total = d.N / d.NP;

    // Both operands are fetched with buffer loads: a 32-bit per-lane byte offset that is fixed for the whole tile (VGPR) + a wave-uniform byte
    // offset per (chunk, channel) / (chunk, tap row) in the instruction's SGPR operand -- no 64-bit address per load stream to keep and to
    // advance (18 VGPR pairs in the flat-load version), and a masked patch item is simply out of range (offset 0xFFFFFFFF reads 0).
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Xb), 0, 0xFFFFFFF0, 0x00020000);
    const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(Apk), 0, 0xFFFFFFF0, 0x00020000);
    // patch item -> source offset of its first channel (channel cc*16 + q*8 of image b0 + img), fixed for the tile
    unsigned poff[P_IT];
    unsigned pmask = 0;
#pragma unroll
    for (int i = 0; i < P_IT; ++i) {
        const int e = tid + i * NTH;
        const int q = e / PLANE, rem = e - q * PLANE;
        const int img = rem / PIMG, rem2 = rem - img * PIMG;
        const int py = rem2 / PW, px = rem2 - py * PW;
        int iy = y0 + py - 1, ix = x0 + px - 1;
        bool ok = e < P_ITEMS && (b0 + img) < nb_total;
        if (MODE == 4) {
            const int par = px / PWH, pxh = px - par * PWH;
            iy = 2 * y0 + py - d.pad;
            ix = 2 * (x0 + pxh) + par - d.pad;
            ok = ok && (unsigned)iy < (unsigned)d.H && (unsigned)ix < (unsigned)d.W;
        } else if (MODE == 2) {
            ok = ok && (unsigned)iy < (unsigned)(2 * d.H) && (unsigned)ix < (unsigned)(2 * d.W);
            iy >>= 1;
            ix >>= 1;
        } else {
            ok = ok && (unsigned)iy < (unsigned)d.H && (unsigned)ix < (unsigned)d.W;
        }
        poff[i] = ok ? 4u * (unsigned)((int)(img * d.b_bstride) + q * 8 * HWs + iy * d.W + ix) : 0xFFFFFFFFu;
        pmask |= (ok ? 1u : 0u) << i;
    }

    u32x4 ra[A_IT];
    float rp[P_IT][8];
    unsigned aoff[A_IT];
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
        const int u = tid + i * NTH;
        aoff[i] = 16u * (unsigned)((u >> 7) * Mpad + (u & 127));
    }
    auto load_a = [&](int cc, int r) {
        const unsigned so = 16u * (unsigned)((cc * 36 + r * 12) * Mpad + m0);           // wave-uniform
#pragma unroll
        for (int i = 0; i < A_IT; ++i) ra[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(ars, aoff[i], so, 0));
    };
    auto store_a = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_IT; ++i) As[buf * A_UNITS + tid + i * NTH] = ra[i];
    };
    auto load_p = [&](int cc) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned so = 4u * (unsigned)((cc * XC + j) * HWs);                        // wave-uniform
#pragma unroll
            for (int i = 0; i < P_IT; ++i) rp[i][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, poff[i], so, 0));
        }
    };
    auto store_p = [&](int cc) {
#pragma unroll
        for (int i = 0; i < P_IT; ++i) {
            const int e = tid + i * NTH;
            if (e < P_ITEMS) {
                float v[8];
                const bool ok = (pmask >> i) & 1u;
                if (MODE == 3) {                                  // same expression as gn_fwd_reg_kernel: z = x*ga + be ; z*sigmoid(z)
                    const float* __restrict__ ss = Sab + 2 * (cc * XC + (e / PLANE) * 8);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float z = rp[i][j] * ss[2 * j] + ss[2 * j + 1];
                        rp[i][j] = z * sigmoidf_(z);
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = (MODE != 3 || ok) ? rp[i][j] : 0.f;   // MODE 3: zero padding applies to the NORMALISED activation; otherwise a masked item was out of range and already read 0
                u32x4 hi, lo;
                split_bf16x8(v, hi, lo);
                Ps[e] = hi;
                Ps[2 * PLANE + e] = lo;
            }
        }
    };

    f32x16 acc[WM][WN];
#pragma unroll
    for (int mi = 0; mi < WM; ++mi)
#pragma unroll
        for (int ni = 0; ni < WN; ++ni)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[mi][ni][v] = 0.f;

    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const u32x4* __restrict__ a_base = As + h * BM + wm * 32 * WM + l31;
    const u32x4* __restrict__ p_base[WN];
#pragma unroll
    for (int ni = 0; ni < WN; ++ni) {
        const int qx = (wn * WN + ni) * 32 + l31;
        const int img = qx / (TR * W), r2 = qx - img * (TR * W);
        const int ty = r2 / W, x = r2 - ty * W;
        p_base[ni] = Ps + h * PLANE + img * PIMG + (MODE == 4 ? 2 * ty : ty) * PW + x;
    }

    const int nchunks = d.C / XC;
    const int c_begin = blockIdx.y * chunks_per_split;
    const int c_end = min(nchunks, c_begin + chunks_per_split);
    load_a(c_begin, 0);
    load_p(c_begin);
    if (MODE == 3) {
        const float* __restrict__ ssb = d.gn_ss + (int64_t)b0 * 2 * d.C;
        for (int i = tid; i < 2 * d.C; i += NTH) Sab[i] = ssb[i];
        __syncthreads();
    }
    store_a(0);
    store_p(c_begin);
    __syncthreads();
    int buf = 0;
    for (int cc = c_begin; cc < c_end; ++cc) {
        const bool more = cc + 1 < c_end;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            if (r < 2) load_a(cc, r + 1);
            else if (more) load_a(cc + 1, 0);
            if (r == 1 && more) load_p(cc + 1);       // (issuing it a tap row earlier measured the same)
            // the loads stay AHEAD of the tap row's MFMAs (hipcc otherwise sinks the r = 0 weight loads next to their LDS stores, 8 MFMAs
            // before the data is needed; measured: neutral at 16x16 / 32x32, 3-5 % at 4x4 / 8x8)
            __builtin_amdgcn_sched_barrier(0);
            const int pr = (MODE == 1) ? 2 - r : r;
            const u32x4* __restrict__ a_cur = a_base + buf * A_UNITS;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int ps = (MODE == 1) ? 2 - s : s;
                bf16x8 ah[WM], al[WM];
#pragma unroll
                for (int mi = 0; mi < WM; ++mi) {
                    ah[mi] = __builtin_bit_cast(bf16x8, a_cur[(s * 4 + 0) * BM + mi * 32]);
                    al[mi] = __builtin_bit_cast(bf16x8, a_cur[(s * 4 + 2) * BM + mi * 32]);
                }
#pragma unroll
                for (int ni = 0; ni < WN; ++ni) {
                    const int tap_off = (MODE == 4) ? pr * PW + (ps & 1) * PWH + (ps >> 1) : pr * PW + ps;
                    const bf16x8 bh = __builtin_bit_cast(bf16x8, p_base[ni][tap_off]);
                    const bf16x8 bl = __builtin_bit_cast(bf16x8, p_base[ni][2 * PLANE + tap_off]);
#pragma unroll
                    for (int mi = 0; mi < WM; ++mi) {
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mi], bh, acc[mi][ni], 0, 0, 0);
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bl, acc[mi][ni], 0, 0, 0);
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bh, acc[mi][ni], 0, 0, 0);
                    }
                }
                if (WN == 4) __builtin_amdgcn_sched_barrier(0);      // 128 accumulator registers: keep ONE tap's fragments live (hipcc otherwise hoists three and spills)
            }
            // the other A buffer was last read in the previous step (which ended with a barrier): fill it without waiting;
            // the single patch buffer is overwritten only after every wave has finished this step's reads.  (Reading the
            // fragments a tap ahead into a second register set, fenced with sched_barriers, measured the same: stripped of all staging and
            // barriers this loop runs at 1.55 PFLOP/s executed, 66 % of the 2.36 the matrix pipe sustains from registers.)
            if (r < 2 || more) store_a(buf ^ 1);
            if (r == 2 && more) {
                __syncthreads();
                store_p(cc + 1);
            }
            __syncthreads();
            buf ^= 1;
        }
    }
    if (gridDim.y == 1) {
        if (MODE == 1 && (W == 16 || W == 32) && WN == 2 && d.pool2) {
            // Input gradient of the upsample convolution: dx[y][x] = sum of the 2x2 block of dU it was replicated into.  The tile holds whole
            // row pairs (W = 32: the wave's two 32-pixel rows sit in acc[.][0] / acc[.][1] of the same lane; W = 16: rows 2k, 2k+1 are lanes
            // l31 and l31 ^ 16 of one accumulator), horizontal neighbours are lanes l31, l31 ^ 1: the full-resolution dU never exists.
            const int OW2 = W / 2;
            float* __restrict__ Db = d.D + (int64_t)b0 * d.d_bstride;
#pragma unroll
            for (int mi = 0; mi < WM; ++mi) {
#pragma unroll
                for (int ni = 0; ni < (W == 32 ? 1 : WN); ++ni) {
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        float sv = (W == 32) ? acc[mi][0][v] + acc[mi][1][v] : acc[mi][ni][v] + __shfl_xor(acc[mi][ni][v], 16, 64);
                        sv += __shfl_xor(sv, 1, 64);
                        const int m = m0 + wm * 32 * WM + mi * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
                        const int oy = (W == 32) ? (y0 >> 1) + wn : (y0 >> 1) + wn * 2 + ni;
                        const int ox = (W == 32) ? (l31 >> 1) : ((l31 & 15) >> 1);
                        const bool writer = (W == 32) ? ((l31 & 1) == 0) : ((l31 & 17) == 0);
                        if (writer && m < d.M) Db[(int64_t)m * d.ldd + oy * OW2 + ox] = d.alpha * sv;
                    }
                }
            }
            return;
        }
        gemm_epilogue<WM, WN>(d, acc, m0, n0, wm, wn, lane, h);
        return;
    }
    float* __restrict__ slab = d.ws + (int64_t)blockIdx.y * d.M * d.N;
#pragma unroll
    for (int ni = 0; ni < WN; ++ni) {
        const int n = n0 + wn * 32 * WN + ni * 32 + l31;
        if (n >= d.N) continue;
#pragma unroll
        for (int mi = 0; mi < WM; ++mi)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int m = m0 + wm * 32 * WM + mi * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
                if (m < d.M) slab[(int64_t)m * d.N + n] = acc[mi][ni][v];
            }
    }
}

// ---- split-precision 1x1 convolution / plain GEMM:  D[b][m][p] = sum_k A[m][k] * B[b][k][p]  (VD_B_PLAIN, weights pre-packed) ----
// The packed operand is the 3x3 layout with one tap: unit ((cc*2 + part)*2 + q)*Mpad + m.  A transposed weight matrix (the 1x1
// input gradient W^T dY) is just packed with swapped strides, so this kernel never sees a_mode.  A stage is NSUB = 4 chunks of
// 16 channels: As[sub][part][q][128 m] (32 KB, straight copy) and Bs[sub][part][q][128 pixels] (32 KB; a thread loads 8 channels x
// 4 consecutive pixels with 8 float4, transposes in registers and writes 4 x (hi, lo) units): 48 MFMAs per wave and stage.
constexpr int GS = 4;                                             // 16-channel chunks per stage

// Position of pixel n (0..127) inside a 128-unit B plane.  The stager writes, per instruction, pixel 4 a + b of eight consecutive
// quads a (fixed b): plain order puts those eight 16-byte units 64 bytes apart = 4-way bank conflict on every ds_write_b128 (the
// B writes alone then keep the LDS busier than the MFMAs keep the matrix pipe).  Within each block of 32 pixels (a = quad 0..7,
// b = 0..3) the unit goes to ((a + 2 b) & 7) + 8 (a >> 2) + 16 ((a >> 1) & 1): the eight lanes of a write hit eight different bank
// quads, and the 16-lane groups of the fragment reads ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} of 32 consecutive pixels) hit 16.
__device__ __forceinline__ int bswz(int n) {
    const int a = (n >> 2) & 7, b = n & 3;
    return (n & ~31) | (((a + 2 * b) & 7) + 8 * (a >> 2) + 16 * ((a >> 1) & 1));
}

// NTH = 512: 128 x 256 tile, eight waves, one workgroup per CU (the weight stage is fetched from L2 and stored to LDS once per 256 pixels).
// Split K (round 4; blockIdx.y = split, st_per stages each): problems with fewer than one round of tiles and a long K -- the 1x1 convolutions of
// the 8x8 / 16x16 levels at small batches (BASELINE config #5: M = 896, K = 2688, N = 512 is 28 tiles of 42 stages) -- write their partial
// sums to the slab d.ws[z][m][n]; splitk_epilogue4_kernel adds them in fixed order and applies bias / residual.
template <int NTH>
__global__ __launch_bounds__(NTH, 2) void gemm_bx3_kernel(const vd_gemm_desc d, int st_per) {
    constexpr int WM = 2, WN = 2, BM = 128, BN = NTH / 2, WAVES_N = NTH / 128;
    constexpr int A_IT = GS * 4 * BM / NTH;                       // 8 (4) units per thread
    // B staging: one (4-pixel quad, k-octet, chunk) item per thread = 8 float4 loads along the pixels (512 contiguous bytes per
    // channel row and half-wave), transposed in registers into 4 pixel units.
    // K is short (2 - 8 stages per tile) and the kernel streams its B operand from HBM: what limits it is the bytes it keeps in flight,
    // so the loads run TWO stages ahead of the MFMAs (two register sets of 64 registers, stages unrolled by two; the LDS image stays single:
    // a second one would cost the second workgroup per CU).
    __shared__ u32x4 As[GS * 4 * BM];
    __shared__ u32x4 Bs[GS * 4 * BN];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
    const int tiles_m = (d.M + BM - 1) / BM;
    int bid = blockIdx.x;
    {
        const int nwg = gridDim.x;
        if ((nwg & 7) == 0) bid = (bid & 7) * (nwg >> 3) + (bid >> 3);
    }
    const int tm = bid % tiles_m, tn = bid / tiles_m;
    const int m0 = tm * BM, n0 = tn * BN;
    const u32x4* __restrict__ Apk = reinterpret_cast<const u32x4*>(d.a_packed);
    const int Mpad = d.a_packed_mpad;
    const int nchunks = d.K / XC;
    const int nst = (nchunks + GS - 1) / GS;
    // BN | NP (a tile inside one image) or NP | BN (8x8 / 4x4 layers: whole images per tile): only the batch offset differs per quad
    const int pg = tid & (BN / 4 - 1), pq = (tid / (BN / 4)) & 1, psub = tid / (BN / 2);  // quad of the tile, k-octet, chunk of the stage
    // buffer loads (see conv3_bx3_kernel): descriptor bases are the packed weights and the tile's first image, lane offsets are 32-bit
    const int b_first = n0 / d.NP;
    const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.B + (int64_t)b_first * d.b_bstride), 0, 0xFFFFFFF0, 0x00020000);
    const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(Apk), 0, 0xFFFFFFF0, 0x00020000);
    unsigned bpix;                                                // byte offset of this thread's quad, k-octet pq, relative to the tile's first image
    {
        const int n = n0 + 4 * pg;                                // NP % 4 == 0: a quad never straddles images
        const int b = n / d.NP;
        bpix = 4u * (unsigned)((b - b_first) * d.b_bstride + (n - b * d.NP) + (int64_t)pq * 8 * d.ldb);
    }
    const unsigned ldb4 = 4u * (unsigned)d.ldb;
    const unsigned a_lane = 16u * (unsigned)((tid >> 7) * Mpad + m0 + (tid & 127));       // the lane part of every A unit this thread loads

    u32x4 ra0[A_IT], ra1[A_IT];
    f32x4 rp0[8], rp1[8];
    // A unit u = tid + i*NT of the stage: run = u >> 7 = sub*4 + part*2 + q, m = u & 127; global unit ((cc0+sub)*4 + part*2+q)*Mpad + m0 + m
    auto load_stage = [&](int st, u32x4 (&ra)[A_IT], f32x4 (&rp)[8]) {
        const int cc0 = min(st, nst - 1) * GS;                    // past the end: reload the last stage (its copy is never read)
#pragma unroll
        for (int i = 0; i < A_IT; ++i) {
            // unit u = tid + i*NTH: run = u >> 7 = i * (NTH / 128) + (tid >> 7); chunk of the stage (run >> 2) and the i-dependent part of the
            // (part, q) index (run & 3) are compile-time per i, so everything but a_lane is a scalar offset
            constexpr int RPI = NTH / 128;                            // runs per i: 2 (256 threads) or 4 (512)
            const int sub = (i * RPI) >> 2, pqi = (i * RPI) & 3;
            const int cc = min(cc0 + sub, nchunks - 1);             // clamped: a tail stage computes only its valid chunks
            ra[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(ars, a_lane, 16u * (unsigned)((cc * 4 + pqi) * Mpad), 0));
        }
        {
            const int cc = min(cc0 + psub, nchunks - 1);
            const unsigned vo = bpix + (unsigned)(cc * XC) * ldb4;
#pragma unroll
            for (int j = 0; j < 8; ++j) rp[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(brs, vo, j * ldb4, 0));
        }
    };
    auto store_stage = [&](const u32x4 (&ra)[A_IT], const f32x4 (&rp)[8]) {
#pragma unroll
        for (int i = 0; i < A_IT; ++i) As[tid + i * NTH] = ra[i];
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            float w[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] = rp[j][px];
            u32x4 hi, lo;
            split_bf16x8(w, hi, lo);
            Bs[((psub * 2 + 0) * 2 + pq) * BN + bswz(4 * pg + px)] = hi;
            Bs[((psub * 2 + 1) * 2 + pq) * BN + bswz(4 * pg + px)] = lo;
        }
    };

    f32x16 acc[WM][WN];
#pragma unroll
    for (int mi = 0; mi < WM; ++mi)
#pragma unroll
        for (int ni = 0; ni < WN; ++ni)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[mi][ni][v] = 0.f;

    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const u32x4* __restrict__ a_base = As + h * BM + wm * 64 + l31;
    const u32x4* __restrict__ b_base = Bs + h * BN + wn * 64 + bswz(l31);
    auto mfma_stage = [&](int st) {
#pragma unroll
        for (int sub = 0; sub < GS; ++sub) {
            if (st * GS + sub < nchunks) {                        // block-uniform
                bf16x8 ah[WM], al[WM];
#pragma unroll
                for (int mi = 0; mi < WM; ++mi) {
                    ah[mi] = __builtin_bit_cast(bf16x8, a_base[(sub * 4 + 0) * BM + mi * 32]);
                    al[mi] = __builtin_bit_cast(bf16x8, a_base[(sub * 4 + 2) * BM + mi * 32]);
                }
#pragma unroll
                for (int ni = 0; ni < WN; ++ni) {
                    const bf16x8 bh = __builtin_bit_cast(bf16x8, b_base[(sub * 4 + 0) * BN + ni * 32]);
                    const bf16x8 bl = __builtin_bit_cast(bf16x8, b_base[(sub * 4 + 2) * BN + ni * 32]);
#pragma unroll
                    for (int mi = 0; mi < WM; ++mi) {
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mi], bh, acc[mi][ni], 0, 0, 0);
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bl, acc[mi][ni], 0, 0, 0);
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bh, acc[mi][ni], 0, 0, 0);
                    }
                }
            }
        }
    };

    const int s_begin = blockIdx.y * st_per, s_end = min(nst, s_begin + st_per);
    load_stage(s_begin, ra0, rp0);
    load_stage(s_begin + 1, ra1, rp1);
    store_stage(ra0, rp0);
    __syncthreads();
    for (int st = s_begin; st < s_end; st += 2) {
        load_stage(st + 2, ra0, rp0);
        mfma_stage(st);
        __syncthreads();
        store_stage(ra1, rp1);                                    // stage st + 1 (issued two stages ago)
        __syncthreads();
        if (st + 1 >= s_end) break;
        load_stage(st + 3, ra1, rp1);
        mfma_stage(st + 1);
        __syncthreads();
        store_stage(ra0, rp0);
        __syncthreads();
    }
    if (gridDim.y == 1) {
        gemm_epilogue<WM, WN>(d, acc, m0, n0, wm, wn, lane, h);
        return;
    }
    float* __restrict__ slab = d.ws + (int64_t)blockIdx.y * d.M * d.N;
#pragma unroll
    for (int ni = 0; ni < WN; ++ni) {
        const int n = n0 + wn * 32 * WN + ni * 32 + l31;
#pragma unroll
        for (int mi = 0; mi < WM; ++mi)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int m = m0 + wm * 32 * WM + mi * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
                if (m < d.M) slab[(int64_t)m * d.N + n] = acc[mi][ni][v];
            }
    }
}

// Persistent variant for grids of more than two workgroups per CU: K is short here (2 - 8 stages per 128 x 128 tile), so a tile's
// prologue (first stage load: a full HBM round trip with nothing to overlap) and epilogue (64 KB of stores) cost as much as its
// steady state.  Each workgroup walks tiles bid, bid + grid, ... and treats (tile, stage) as ONE stream: the loads of the next
// tile's first stage are issued before the MFMAs of the current tile's last stage and stay in flight across its epilogue.
__global__ __launch_bounds__(NT, 2) void gemm_bx3_persist_kernel(const vd_gemm_desc d, int ntiles) {
    constexpr int WM = 2, WN = 2, BM = 128, BN = 128;
    constexpr int A_IT = GS * 4 * BM / NT;
    __shared__ u32x4 As[GS * 4 * BM];
    __shared__ u32x4 Bs[GS * 4 * BN];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
    const int tiles_m = (d.M + BM - 1) / BM;
    const u32x4* __restrict__ Apk = reinterpret_cast<const u32x4*>(d.a_packed);
    const int Mpad = d.a_packed_mpad;
    const int nchunks = d.K / XC;
    const int nst = (nchunks + GS - 1) / GS;
    const int pg = tid & 31, pq = (tid >> 5) & 1, psub = tid >> 6;
    const bool remap = (ntiles & 7) == 0;

    u32x4 ra[A_IT];
    f32x4 rp[8];
    auto tile_origin = [&](int t, int& m0, int& n0) {
        const int r = remap ? (t & 7) * (ntiles >> 3) + (t >> 3) : t;          // gridDim.x is a multiple of 8: t & 7 == blockIdx.x & 7
        m0 = (r % tiles_m) * BM;
        n0 = (r / tiles_m) * BN;
    };
    const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(Apk), 0, 0xFFFFFFF0, 0x00020000);
    const unsigned ldb4 = 4u * (unsigned)d.ldb;
    auto load_a = [&](int m0, int cc0) {
        const unsigned a_lane = 16u * (unsigned)((tid >> 7) * Mpad + m0 + (tid & 127));
#pragma unroll
        for (int i = 0; i < A_IT; ++i) {
            const int sub = (i * 2) >> 2, pqi = (i * 2) & 3;           // run = 2 i + (tid >> 7): see gemm_bx3_kernel
            const int cc = min(cc0 + sub, nchunks - 1);
            ra[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(ars, a_lane, 16u * (unsigned)((cc * 4 + pqi) * Mpad), 0));
        }
    };
    auto load_b = [&](int n0, int cc0) {
        {
            const int b_first = n0 / d.NP;                            // wave-uniform: the descriptor is rebuilt per tile with scalar instructions
            const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.B + (int64_t)b_first * d.b_bstride), 0, 0xFFFFFFF0, 0x00020000);
            const int n = n0 + 4 * pg;
            const int b = n / d.NP;
            const int cc = min(cc0 + psub, nchunks - 1);
            const unsigned vo = 4u * (unsigned)((b - b_first) * d.b_bstride + (n - b * d.NP)) + (unsigned)(cc * XC + pq * 8) * ldb4;
#pragma unroll
            for (int j = 0; j < 8; ++j) rp[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(brs, vo, j * ldb4, 0));
        }
    };
    auto store_stage = [&]() {
#pragma unroll
        for (int i = 0; i < A_IT; ++i) As[tid + i * NT] = ra[i];
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            float w[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] = rp[j][px];
            u32x4 hi, lo;
            split_bf16x8(w, hi, lo);
            Bs[((psub * 2 + 0) * 2 + pq) * BN + bswz(4 * pg + px)] = hi;
            Bs[((psub * 2 + 1) * 2 + pq) * BN + bswz(4 * pg + px)] = lo;
        }
    };

    const int wm = wave >> 1, wn = wave & 1;
    const u32x4* __restrict__ a_base = As + h * BM + wm * 64 + l31;
    const u32x4* __restrict__ b_base = Bs + h * BN + wn * 64 + bswz(l31);

    int t = blockIdx.x;
    if (t >= ntiles) return;
    int m0, n0;
    tile_origin(t, m0, n0);
    load_a(m0, 0);
    load_b(n0, 0);
    store_stage();
    __syncthreads();
    while (true) {
        f32x16 acc[WM][WN];
#pragma unroll
        for (int mi = 0; mi < WM; ++mi)
#pragma unroll
            for (int ni = 0; ni < WN; ++ni)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[mi][ni][v] = 0.f;
        const int tn = t + gridDim.x;
        int m1 = 0, n1 = 0;
        const bool next_tile = tn < ntiles;
        if (next_tile) tile_origin(tn, m1, n1);
        for (int st = 0; st < nst; ++st) {
            const int cc0 = st * GS;
            const bool last = st + 1 == nst;
            if (!last) {
                load_a(m0, cc0 + GS);
                load_b(n0, cc0 + GS);
            } else if (next_tile) {
                load_b(n1, 0);                                    // the activations (HBM) only: the weights are an L2 hit, fetched after the epilogue
            }
#pragma unroll
            for (int sub = 0; sub < GS; ++sub) {
                if (cc0 + sub < nchunks) {                        // block-uniform
                    bf16x8 ah[WM], al[WM];
#pragma unroll
                    for (int mi = 0; mi < WM; ++mi) {
                        ah[mi] = __builtin_bit_cast(bf16x8, a_base[(sub * 4 + 0) * BM + mi * 32]);
                        al[mi] = __builtin_bit_cast(bf16x8, a_base[(sub * 4 + 2) * BM + mi * 32]);
                    }
#pragma unroll
                    for (int ni = 0; ni < WN; ++ni) {
                        const bf16x8 bh = __builtin_bit_cast(bf16x8, b_base[(sub * 4 + 0) * BN + ni * 32]);
                        const bf16x8 bl = __builtin_bit_cast(bf16x8, b_base[(sub * 4 + 2) * BN + ni * 32]);
#pragma unroll
                        for (int mi = 0; mi < WM; ++mi) {
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mi], bh, acc[mi][ni], 0, 0, 0);
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bl, acc[mi][ni], 0, 0, 0);
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bh, acc[mi][ni], 0, 0, 0);
                        }
                    }
                }
            }
            if (!last) {
                __syncthreads();
                store_stage();
                __syncthreads();
            }
        }
        gemm_epilogue<WM, WN>(d, acc, m0, n0, wm, wn, lane, h);               // the next tile's first stage is in flight meanwhile
        if (!next_tile) break;
        load_a(m1, 0);
        __syncthreads();
        store_stage();
        __syncthreads();
        t = tn;
        m0 = m1;
        n0 = n1;
    }
}

// ---- split-precision product of two ACTIVATION matrices (attention: scores, values and their gradients) ---------------------
// D[b][m][n] = alpha * sum_k A_b[m][k] * B_b[k][n] with per-batch A (a_bstride != 0): nothing can be pre-packed, both operands
// are split where they are written to LDS.  ADIR / BDIR = the operand is k-contiguous (VD_A_ROW / VD_B_KCONTIG): a thread loads
// the 8 consecutive k of its fragment octet with two float4; otherwise (VD_A_COL / VD_B_PLAIN: m / n contiguous) it gathers 8
// k-rows with 8 loads coalesced along m / n.  LDS: [plane = sub*4 + part*2 + q][130] units for each operand (the odd-ish plane
// stride keeps the 8 octet-lanes of the k-contiguous writers on distinct banks), GS = 4 chunks of 16 k per stage.
template <bool ADIR, bool BDIR>
__global__ __launch_bounds__(NT, 2) void gemm_bx3_act_kernel(const vd_gemm_desc d) {
    constexpr int WM = 2, WN = 2, BM = 128, BN = 128, LD_ = 130;
    constexpr int IT = GS * 2 * BM / NT;                          // 4 (row, k-octet) items per thread and operand
    __shared__ u32x4 As[GS * 4 * LD_];
    __shared__ u32x4 Bs[GS * 4 * LD_];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
    const int tiles_m = (d.M + BM - 1) / BM;
    int bid = blockIdx.x;
    {
        const int nwg = gridDim.x;
        if ((nwg & 7) == 0) bid = (bid & 7) * (nwg >> 3) + (bid >> 3);
    }
    const int tm = bid % tiles_m, tn = bid / tiles_m;
    const int m0 = tm * BM, n0 = tn * BN;
    const int b = n0 / d.NP, p0 = n0 - b * d.NP;                  // BN | NP
    const float* __restrict__ Ap = d.A + batch_off(d, b, d.a_bstride, d.a_b2stride);
    const float* __restrict__ Bp = d.B + batch_off(d, b, d.b_bstride, d.b_b2stride);
    const int nchunks = d.K / XC;

    float ra[IT][8], rb[IT][8];
    // item e = tid + i*NT.  k-contiguous operand: octet o = e & 7 (of the 8 in a 64-k stage), row x = e >> 3 (0..127);
    // gathered operand: row x = e & 127, q = (e >> 7) & 1, sub = e >> 8.
    auto load_stage = [&](int cc0) {
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int e = tid + i * NT;
            if (ADIR) {
                const int o = e & 7, x = e >> 3;
                const int kk = min(cc0 * XC + o * 8, d.K - 8);
                const float* __restrict__ src = Ap + (int64_t)min(m0 + x, d.M - 1) * d.lda + kk;
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    ra[i][j] = v0[j];
                    ra[i][4 + j] = v1[j];
                }
            } else {
                const int x = e & 127, cc = min(cc0 + (e >> 8), nchunks - 1);
                const float* __restrict__ src = Ap + (int64_t)(cc * XC + ((e >> 7) & 1) * 8) * d.lda + min(m0 + x, d.M - 1);
#pragma unroll
                for (int j = 0; j < 8; ++j) ra[i][j] = src[(int64_t)j * d.lda];
            }
            if (BDIR) {
                const int o = e & 7, x = e >> 3;
                const int kk = min(cc0 * XC + o * 8, d.K - 8);
                const float* __restrict__ src = Bp + (int64_t)(p0 + x) * d.ldb + kk;
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    rb[i][j] = v0[j];
                    rb[i][4 + j] = v1[j];
                }
            } else {
                const int x = e & 127, cc = min(cc0 + (e >> 8), nchunks - 1);
                const float* __restrict__ src = Bp + (int64_t)(cc * XC + ((e >> 7) & 1) * 8) * d.ldb + p0 + x;
#pragma unroll
                for (int j = 0; j < 8; ++j) rb[i][j] = src[(int64_t)j * d.ldb];
            }
        }
    };
    auto store_stage = [&]() {
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int e = tid + i * NT;
            u32x4 hi, lo;
            {
                const int x = ADIR ? (e >> 3) : (e & 127);
                const int plane = ADIR ? ((e & 7) >> 1) * 4 + ((e & 7) & 1) : (e >> 8) * 4 + ((e >> 7) & 1);   // sub*4 + q (part 0)
                float v[8];
                const bool ok = m0 + x < d.M;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = ok ? ra[i][j] : 0.f;
                split_bf16x8(v, hi, lo);
                As[plane * LD_ + x] = hi;
                As[(plane + 2) * LD_ + x] = lo;
            }
            {
                const int x = BDIR ? (e >> 3) : (e & 127);
                const int plane = BDIR ? ((e & 7) >> 1) * 4 + ((e & 7) & 1) : (e >> 8) * 4 + ((e >> 7) & 1);
                split_bf16x8(rb[i], hi, lo);
                Bs[plane * LD_ + x] = hi;
                Bs[(plane + 2) * LD_ + x] = lo;
            }
        }
    };

    f32x16 acc[WM][WN];
#pragma unroll
    for (int mi = 0; mi < WM; ++mi)
#pragma unroll
        for (int ni = 0; ni < WN; ++ni)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[mi][ni][v] = 0.f;

    const int wm = wave >> 1, wn = wave & 1;
    const u32x4* __restrict__ a_base = As + h * LD_ + wm * 64 + l31;
    const u32x4* __restrict__ b_base = Bs + h * LD_ + wn * 64 + l31;

    load_stage(0);
    store_stage();
    __syncthreads();
    for (int cc0 = 0; cc0 < nchunks; cc0 += GS) {
        const bool more = cc0 + GS < nchunks;
        if (more) load_stage(cc0 + GS);
#pragma unroll
        for (int sub = 0; sub < GS; ++sub) {
            if (cc0 + sub < nchunks) {                            // block-uniform
                bf16x8 ah[WM], al[WM];
#pragma unroll
                for (int mi = 0; mi < WM; ++mi) {
                    ah[mi] = __builtin_bit_cast(bf16x8, a_base[(sub * 4 + 0) * LD_ + mi * 32]);
                    al[mi] = __builtin_bit_cast(bf16x8, a_base[(sub * 4 + 2) * LD_ + mi * 32]);
                }
#pragma unroll
                for (int ni = 0; ni < WN; ++ni) {
                    const bf16x8 bh = __builtin_bit_cast(bf16x8, b_base[(sub * 4 + 0) * LD_ + ni * 32]);
                    const bf16x8 bl = __builtin_bit_cast(bf16x8, b_base[(sub * 4 + 2) * LD_ + ni * 32]);
#pragma unroll
                    for (int mi = 0; mi < WM; ++mi) {
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mi], bh, acc[mi][ni], 0, 0, 0);
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bl, acc[mi][ni], 0, 0, 0);
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bh, acc[mi][ni], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
        if (more) store_stage();
        __syncthreads();
    }
    gemm_epilogue<WM, WN>(d, acc, m0, n0, wm, wn, lane, h);
}

// d.math == 1: both operands are activations (per-batch A), split in the kernel
static bool gemm_bx3_act_eligible(const vd_gemm_desc& d) {
    if (d.math != 1 || d.a_packed || d.a_bstride == 0 || d.d_trans || d.debug || d.tile || d.gn_ss) return false;
    if (d.b_mode != VD_B_PLAIN && d.b_mode != VD_B_KCONTIG) return false;
    if (d.NP % 128 != 0 || d.N % 128 != 0 || d.K % XC != 0 || d.K < 32 || d.M < 64) return false;
    if ((d.lda & 3) || (d.ldb & 3) || (d.a_bstride & 3) || (d.b_bstride & 3) || (d.a_b2stride & 3) || (d.b_b2stride & 3)) return false;
    if (((((uintptr_t)d.A) | ((uintptr_t)d.B)) & 15) != 0) return false;
    if (d.a_mode == VD_A_COL && d.M % 4 != 0) return false;
    return true;
}

static void launch_gemm_bx3_act(const vd_gemm_desc& d, hipStream_t st, char* name) {
    const dim3 grid(vd_cdiv(d.M, 128) * (d.N / 128));
    const bool adir = d.a_mode == VD_A_ROW, bdir = d.b_mode == VD_B_KCONTIG;
    // (<ADIR, BDIR> spelled 1 / 0: the recorded names have always carried them as numbers)
    if (adir && bdir) VD_LAUNCH_OR_NAME(name, (gemm_bx3_act_kernel<1, 1>), grid, dim3(NT), 0, st, d);
    else if (adir) VD_LAUNCH_OR_NAME(name, (gemm_bx3_act_kernel<1, 0>), grid, dim3(NT), 0, st, d);
    else if (bdir) VD_LAUNCH_OR_NAME(name, (gemm_bx3_act_kernel<0, 1>), grid, dim3(NT), 0, st, d);
    else VD_LAUNCH_OR_NAME(name, (gemm_bx3_act_kernel<0, 0>), grid, dim3(NT), 0, st, d);
}

static bool gemm_bx3_eligible(const vd_gemm_desc& d) {
    if (!d.a_packed || d.a_packed_mpad < d.M || (d.a_packed_mpad & 127) != 0 || (((uintptr_t)d.a_packed) & 15) != 0) return false;
    if (d.b_mode != VD_B_PLAIN || d.d_trans || d.debug || d.tile || d.nb2 > 1 || d.a_bstride != 0 || d.gn_ss) return false;
    if ((d.ldb & 3) || (d.b_bstride & 3) || (((uintptr_t)d.B) & 15) || (d.NP & 3)) return false;      // float4 loads along the pixels
    return (d.NP % 128 == 0 || 128 % d.NP == 0) && d.N % 128 == 0 && d.K % XC == 0 && d.M >= 64;
}

// Split-K plan of the 128 x 128-tile 1x1 kernel (vd_gemm_tile 9): under three quarters of a round of tiles and at least four 64-channel
// stages -> enough splits for ~two rounds, at least two stages each.  splits == 1: the direct epilogue.
static void gemm_bx3_plan(const vd_gemm_desc& d, int& splits, int& st_per) {
    const int base = vd_cdiv(d.M, 128) * (d.N / 128);
    const int nst = vd_cdiv(d.K / XC, GS);
    splits = 1, st_per = nst;
    if (base >= 192 || nst < 4 || d.pool2 || d.act || d.gn_part) return;
    splits = vd_cdiv(512, base);
    if (splits > nst / 2) splits = nst / 2;
    st_per = vd_cdiv(nst, splits);
    splits = vd_cdiv(nst, st_per);
}

// 128 x 256 tiles for the 1x1 family: whole rounds of 256 workgroups (see bx3_big_tile) AND a long K -- measured 3-9 % faster for
// K >= 384 at 16x16, but 10-17 % slower for K = 128 / 256 at 32x32 (one workgroup per CU: nothing overlaps a tile's prologue and epilogue)
static bool gemm_bx3_big_tile(const vd_gemm_desc& d) {
    if (d.K < 384 || d.N % 256 != 0 || !(d.NP % 256 == 0 || 256 % d.NP == 0)) return false;
    const int nb = vd_cdiv(d.M, 128) * (d.N / 256);
    return nb >= 256 && (nb % 256 == 0 || nb % 256 >= 192);
}

static bool bx3_eligible(const vd_gemm_desc& d) {
    if (!d.a_packed || d.a_packed_mpad < d.M || (d.a_packed_mpad & 127) != 0) return false;
    if (d.b_mode == VD_B_CONV3_S2) {                              // stride 2 (round 3): 4x4 .. 32x32 outputs of an input twice as large
        if (d.d_trans || d.debug || d.tile || d.nb2 > 1 || d.gn_ss || d.pool2) return false;
        const bool wide2 = d.OW == 64 || (d.OW >= 128 && d.OW % 128 == 0);    // round 4: 64 / 128-pixel row-segment tiles (the 128x128 / 64x64 outputs of config #4)
        if ((d.OW != 4 && d.OW != 8 && d.OW != 16 && d.OW != 32 && !wide2) || d.OH != d.OW || d.H != 2 * d.OH || d.W != 2 * d.OW) return false;
        if (wide2 && ((d.OH * d.OW) % 128 != 0 || d.b_bstride >= (1ll << 29))) return false;
        if (d.pad != 0 && d.pad != 1) return false;
        return d.OH * d.OW == d.NP && d.C % XC == 0 && d.K == d.C * 9 && d.M >= 64 && (((uintptr_t)d.a_packed) & 15) == 0;
    }
    if (d.b_mode != VD_B_CONV3 && d.b_mode != VD_B_CONV3_T && d.b_mode != VD_B_CONV3_UP) return false;
    if (d.d_trans || d.debug || d.tile || d.nb2 > 1) return false;
    if (d.gn_ss && (d.b_mode != VD_B_CONV3 || (d.OW != 16 && d.OW != 32) || d.C > 1024)) return false;
    const bool wide = d.OW == 64 || (d.OW >= 128 && d.OW % 128 == 0);       // row-segment tiles
    if (d.OW != 4 && d.OW != 8 && d.OW != 16 && d.OW != 32 && !wide) return false;
    if (d.b_mode == VD_B_CONV3_UP && d.OW == 4) return false;
    if ((!wide && d.OH != d.OW) || d.OH * d.OW != d.NP || d.C % XC != 0 || d.K != d.C * 9 || d.M < 64) return false;
    if (wide && (d.NP % 128 != 0 || d.b_bstride >= (1ll << 31))) return false;
    if ((((uintptr_t)d.a_packed) & 15) != 0) return false;
    return true;
}

// 8x8 layers: the channel loop is split over workgroups either way (too few tiles); with 128 x 256 tiles (four images, eight waves) every chunk of the
// weight operand is fetched by half as many workgroups -- these layers re-read the weights once per pixel tile (64 tiles of 128 pixels at B = 128)
static bool bx3_big_split(const vd_gemm_desc& d) {
    if (d.OW != 8 || d.OH != 8 || d.pool2 || d.gn_ss || d.N % 256 != 0) return false;
    if (d.b_mode != VD_B_CONV3 && d.b_mode != VD_B_CONV3_T) return false;
    const int base = vd_cdiv(d.M, 128) * (d.N / 256);
    return base >= 32 && base < 256 && d.C / XC >= 8;
}

static void bx3_plan(const vd_gemm_desc& d, int& splits, int& c_per) {
    const int base = vd_cdiv(d.M, 128) * vd_cdiv(d.N, 128);
    const int nchunks = d.C / XC;
    splits = 1;
    if (bx3_big_split(d)) {
        const int bb = vd_cdiv(d.M, 128) * (d.N / 256);
        static const int tgt = getenv("VD_BX3_BIGSPLIT_TARGET") ? atoi(getenv("VD_BX3_BIGSPLIT_TARGET")) : 256;
        splits = vd_cdiv(tgt, bb);
        if (splits > nchunks / 2) splits = nchunks / 2;
        c_per = vd_cdiv(nchunks, splits);
        splits = vd_cdiv(nchunks, c_per);
        return;
    }
    static const int target = getenv("VD_BX3_SPLIT_TARGET") ? atoi(getenv("VD_BX3_SPLIT_TARGET")) : 512;
    if (base < 256) {
        splits = vd_cdiv(d.OW == 4 ? target / 2 : target, base);      // 4x4 layers: 8 splits of 4 chunks beat 16 of 2 (25.8 vs 28.3 us at 512 channels)
        const int max_splits = nchunks / 2 > 0 ? nchunks / 2 : 1;
        if (splits > max_splits) splits = max_splits;
    }
    c_per = vd_cdiv(nchunks, splits);
    splits = vd_cdiv(nchunks, c_per);
}

// 0: 128 x 128 tiles; 1: 128 x 256 (eight waves of 64 x 64); 2: 128 x 512 (eight waves of 64 x 128, 32x32 layers: whole rounds of 256 workgroups again,
// and the weight operand is fetched and stored once per 512 pixels)
static int bx3_big_tile(const vd_gemm_desc& d, int splits) {
    if (splits != 1 || (d.OW != 16 && d.OW != 32) || d.N % 256 != 0) return 0;
    // ... for the FORWARD kinds (plain, upsample-fused, GroupNorm-folding loader): +8-11 % per kernel in isolation, 1.4 % of a sampler step, 0.6 % of a
    // training step.  Not for the flipped-tap input gradient: it runs beside the weight gradients of the side stream, and at 212 VGPRs and 87 KB of
    // LDS a 128 x 512 workgroup leaves no room on its CU for those workgroups, which is what fills the 128 x 256 kernels' bubbles (measured neutral).
    if (d.b_mode != VD_B_CONV3_T && !d.pool2 && d.OW == 32 && d.N % 512 == 0) {
        const int nh = vd_cdiv(d.M, 128) * (d.N / 512);
        if (nh >= 256 && (nh % 256 == 0 || nh % 256 >= 192)) return 2;
    }
    const int nb = vd_cdiv(d.M, 128) * (d.N / 256);
    return (nb >= 256 && (nb % 256 == 0 || nb % 256 >= 192)) ? 1 : 0;
}

// The persistent 16x16x32 kernel (vd_conv_k32p.hip) takes a stride-1 / upsample-fused convolution when its 256-pixel tiles fill the chip's 256
// workgroup slots to >= 75 % in every round (a 128 x 256 tile per CU: 300 tiles would cost two rounds for 1.17 rounds of work; the 128 x 128
// tiles below pack such grids two per CU).
static bool k32p_pick(const vd_gemm_desc& d) {
    if (d.b_mode != VD_B_CONV3 && d.b_mode != VD_B_CONV3_T && d.b_mode != VD_B_CONV3_UP) return false;
    if (!vd_conv3_k32p_eligible(d) || d.N % 256 != 0) return false;
    const int nt = vd_cdiv(d.M, 128) * (d.N / 256);
    const int rounds = vd_cdiv(nt, 256);
    return nt >= 192 && 4 * nt >= 3 * rounds * 256;
}

// vd_gemm_desc.pool2 (2x2 block sums in the epilogue): the flipped-tap 3x3 convolution on a packed operand with a bare epilogue, on the persistent kernel
// (any image it takes) or at 16x16 / 32x32 outputs on a grid that no planner splits (>= 256 tiles of 128 x 128).  Asked by vd_gemm_tile before anything
// else: a refused problem answers -1 there and VD_EINVAL at vd_gemm, before any launch.
static bool pool2_ok(const vd_gemm_desc& d) {
    if (!d.a_packed || d.b_mode != VD_B_CONV3_T || d.bias || d.rowadd || d.residual || d.accumulate) return false;
    if (k32p_pick(d)) return true;
    return d.OH == d.OW && (d.OW == 16 || d.OW == 32) && vd_cdiv(d.M, 128) * vd_cdiv(d.N, 128) >= 256;
}

// tile: vd_gemm_tile() of the problem -- 18 the persistent 16x16x32 kernel, 16 the 8x8 layers' 128 x 256 tiles with the channel loop split,
// 15 / 12 the 128 x 512 / 128 x 256 tiles (eight waves, one workgroup per CU, unsplit), 8 the 128 x 128 tiles
static int launch_bx3(const vd_gemm_desc& d, int tile, hipStream_t st, char* name) {
    const int mode = d.b_mode == VD_B_CONV3 ? (d.gn_ss ? 3 : 0) : (d.b_mode == VD_B_CONV3_T ? 1 : (d.b_mode == VD_B_CONV3_S2 ? 4 : 2));
    if (tile == 18) {
        if (vd_launch_conv3_k32p(d, mode, st, name) != 0) return VD_EINVAL;
        if (name && d.OW > 32) {                                  // one instantiation walks 8 x 32 segments of any wider image: the image width beside it
            char at[16];
            snprintf(at, sizeof(at), "@%d", d.OW);
            vd_name_append(name, at);
        }
        return 0;
    }
    int splits, c_per;
    bx3_plan(d, splits, c_per);
    if (!name && splits > 1 && d.ws == nullptr) {
        vd_set_error("vd_gemm: split-K workspace required (%d splits): query vd_gemm_ws_floats()", splits);
        return VD_EINVAL;
    }
    if (tile == 16) {
        dim3 grids(vd_cdiv(d.M, 128) * (d.N / 256), splits);
        if (mode == 0) VD_LAUNCH_OR_NAME(name, (conv3_bx3_kernel<8, 0, 2, 512, 2>), grids, dim3(512), 0, st, d, c_per);
        else VD_LAUNCH_OR_NAME(name, (conv3_bx3_kernel<8, 1, 2, 512, 2>), grids, dim3(512), 0, st, d, c_per);
        if (!name && splits > 1) launch_splitk_epilogue(d, splits, st);
        return 0;
    }
    // 128 x 256 / 128 x 512 tiles where whole rounds of 256 workgroups come out (bx3_big_tile): the weight operand is then fetched from L2 and
    // stored to LDS once per 256 / 512 pixels (measured +5-10 % each step at 16x16 / 32x32; a partly filled last round packs better with the
    // 128 x 128 tiles, two per CU)
    if (tile == 15) {
        dim3 gridh(vd_cdiv(d.M, 128) * (d.N / 512), 1);
        switch (mode) {
        case 0: VD_LAUNCH_OR_NAME(name, (conv3_bx3_kernel<32, 0, 4, 512, 2>), gridh, dim3(512), 0, st, d, c_per); break;
        case 1: VD_LAUNCH_OR_NAME(name, (conv3_bx3_kernel<32, 1, 4, 512, 2>), gridh, dim3(512), 0, st, d, c_per); break;
        case 2: VD_LAUNCH_OR_NAME(name, (conv3_bx3_kernel<32, 2, 4, 512, 2>), gridh, dim3(512), 0, st, d, c_per); break;
        default: VD_LAUNCH_OR_NAME(name, (conv3_bx3_kernel<32, 3, 4, 512, 2>), gridh, dim3(512), 0, st, d, c_per); break;
        }
        return 0;
    }
    bool done = false;
    if (tile == 12) {
        dim3 gridb(vd_cdiv(d.M, 128) * (d.N / 256), 1);
#define BX3_BIG(WW, MD)                                                                                   \
    if (!done && d.OW == WW && mode == MD) {                                                              \
        VD_LAUNCH_OR_NAME(name, (conv3_bx3_kernel<WW, MD, 2, 512, 2>), gridb, dim3(512), 0, st, d, c_per); \
        done = true;                                                                                      \
    }
        BX3_BIG(32, 0) BX3_BIG(32, 1) BX3_BIG(32, 2) BX3_BIG(32, 3)
        BX3_BIG(16, 0) BX3_BIG(16, 1) BX3_BIG(16, 2) BX3_BIG(16, 3)
#undef BX3_BIG
        return done ? 0 : VD_EINVAL;
    }
    dim3 grid(vd_cdiv(d.M, 128) * vd_cdiv(d.N, 128), splits);
    const int tw = d.OW >= 128 && d.OW % 128 == 0 ? 128 : d.OW;      // tile width: the image's, or 128-pixel row segments of wider ones
#define BX3_CASE(WW, MD)                                                                      \
    if (!done && tw == WW && mode == MD) {                                                    \
        VD_LAUNCH_OR_NAME(name, (conv3_bx3_kernel<WW, MD, 2, 256, 2>), grid, dim3(NT), 0, st, d, c_per); \
        done = true;                                                                          \
    }
    BX3_CASE(32, 0) BX3_CASE(32, 1) BX3_CASE(32, 2) BX3_CASE(32, 3)
    BX3_CASE(16, 0) BX3_CASE(16, 1) BX3_CASE(16, 2) BX3_CASE(16, 3)
    BX3_CASE(8, 0) BX3_CASE(8, 1) BX3_CASE(8, 2)
    BX3_CASE(4, 0) BX3_CASE(4, 1)
    BX3_CASE(32, 4) BX3_CASE(16, 4) BX3_CASE(8, 4) BX3_CASE(4, 4)
    BX3_CASE(64, 0) BX3_CASE(64, 1) BX3_CASE(64, 2)
    BX3_CASE(128, 0) BX3_CASE(128, 1) BX3_CASE(128, 2)
    BX3_CASE(64, 4) BX3_CASE(128, 4)
#undef BX3_CASE
    if (!done) return VD_EINVAL;
    if (!name && splits > 1) launch_splitk_epilogue(d, splits, st);
    return 0;
}
