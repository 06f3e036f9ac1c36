// Included by vd_gemm.hip after wgrad_patch_store (anonymous namespace); types from vd_conv_bx3.inc.
// ---- split-precision weight gradient of the stride-1 3x3 convolution ----------------------------------------------------
// dW[m][c][r][s] = sum_{b,y,x} dY[b][m][y][x] * X[b][c][y+r-1][x+s-1]: the reduction index is the PIXEL, and a lane's 8-deep
// k-fragment is 8 consecutive pixels of one row -- contiguous in NCHW for dY, and for X as well once the horizontal tap shift
// is taken out of the address: the X tile is written to LDS THREE times, shifted by s-1 pixels (zero beyond the row ends), each
// copy 16-byte aligned.  The shifted copies cost no extra split work: x = hi + lo is computed once for the 10 pixels
// [8o-1, 8o+8] of an octet (the two neighbours arrive by lane shuffles), and the copies are re-packings of those 16-bit halves.
// Same tile geometry, grid, split-K plan and epilogue as wgrad_patch_kernel (128 m x 64 c x 3 taps of one tap row r per
// workgroup, K-step = 32 output pixels), so wgrad_patch_plan / wgrad_patch_store / slab_reduce_perm_kernel are shared.
//     As[part][octet 0..3][m]       (octet stride LDA_ = 130 units: the 4 octets of a row land 8 banks apart on the write side)
//     Bs[s][part][octet 0..3][c]    (octet stride LDB_ = 66 units)
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void split_pair(float a, float b, unsigned& hi, unsigned& lo) {
    bf16x2 h, l;
    h[0] = (__bf16)a;
    h[1] = (__bf16)b;
    l[0] = (__bf16)(a - (float)h[0]);
    l[1] = (__bf16)(b - (float)h[1]);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
}

// WIDE (W == 32 only): the image is wider than 32 px (OW % 32 == 0); a K-step is one 32-pixel SEGMENT of a row starting at column
// x0, and the two halo pixels of an octet are read from memory (a segment's neighbours are real pixels, not padding).
#include "vd_wgrad_job.h"

#ifdef VD_WG_STAMPS            // diagnostic build only (tools/wg_stamps.py): where a K-step's time goes, per wave; never in the shipped library
__device__ unsigned long long* g_wg_stamps = nullptr;
#define WG_STAMP(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#endif

template <int W, int MODE, bool WIDE = false>   // MODE 0: CONV3, 2: CONV3_UP (X is the half-resolution source of the nearest-2x upsample),
                                                // 4: CONV3_S2 (round 4: X is the 2 OH x 2 OW input of the stride-2 Downsample2D convolution, d.pad = 0 | 1)
__device__ __forceinline__ void wgrad_bx3_body(const vd_wgrad_desc& d, int ksteps_per_split, int gx, int gy, int lin) {
    constexpr int ROWS = 32 / W;                   // image rows per K-step
    constexpr int OPR = W >= 8 ? W / 8 : 1;        // octets per row (W == 4: an octet is TWO rows of one image, see below)
    constexpr bool W4 = (W == 4);                  // 4x4 outputs: K-step = two whole images, octet so = rows 2(so&1), 2(so&1)+1 of image so>>1
    constexpr int CT = 64;
    constexpr int LDA_ = 130, LDB_ = 66;
    __shared__ u32x4 As[2 * 4 * LDA_];
    __shared__ u32x4 Bs[3 * 2 * 4 * LDB_];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
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
    const int segs = WIDE ? d.OW / 32 : 1;         // K-steps per image row (WIDE) ...
    const int steps_per_img = WIDE ? d.OH * segs : (W4 ? 1 : d.OH / ROWS);
    const int ks_total = W4 ? (d.nb + 1) / 2 : d.nb * steps_per_img;
    const int ks_begin = by * ksteps_per_split;
    const int ks_end = min(ks_total, ks_begin + ksteps_per_split);
    const int HWs = d.H * d.W;

    // staging roles: lanes run along the 4 octets of the K-step (128 contiguous bytes), then along rows m / channels c
    const int so = tid & 3;                        // octet of the K-step
    const int s_rr = so / OPR, s_xo = so - s_rr * OPR;
    const int am = tid >> 2;                       // A: rows am and am + 64
    const int bc = tid >> 2;                       // B: channel
    const bool a_ok0 = m0 + am < d.M, a_ok1 = m0 + am + 64 < d.M;
    const bool b_ok = c0 + bc < d.C;
    const int64_t a_off0 = (int64_t)min(m0 + am, d.M - 1) * d.NP + 8 * (W4 ? (so & 1) : so);
    const int64_t a_off1 = (int64_t)min(m0 + am + 64, d.M - 1) * d.NP + 8 * (W4 ? (so & 1) : so);
    const int64_t b_off = (int64_t)min(c0 + bc, d.C - 1) * HWs + (MODE == 2 ? 4 : (MODE == 4 ? 16 : 8)) * s_xo;
    const unsigned a_voff0 = 4u * (unsigned)a_off0, a_voff1 = 4u * (unsigned)a_off1, b_voff = 4u * (unsigned)b_off;   // byte offsets inside one image

    f32x4 ra[4], rb[4];                            // (rb[2], rb[3]: stride 2 only.  A template-dependent array size captured by the lambdas keeps their closure in scratch memory)
    float rl = 0.f, rr_ = 0.f;                     // WIDE: the pixels left / right of this thread's octet
    bool row_ok = false, row_ok2 = false, img_ok = true;
    auto load_stage = [&](int ks) {
        if (W4) {
            const int bi = 2 * ks + (so >> 1);
            img_ok = bi < d.nb;
            const int bb = img_ok ? bi : 0;
            const float* __restrict__ dyb = d.dY + (int64_t)bb * d.dy_bstride;
            ra[0] = *reinterpret_cast<const f32x4*>(dyb + a_off0);
            ra[1] = *reinterpret_cast<const f32x4*>(dyb + a_off0 + 4);
            ra[2] = *reinterpret_cast<const f32x4*>(dyb + a_off1);
            ra[3] = *reinterpret_cast<const f32x4*>(dyb + a_off1 + 4);
            const int iyt = 2 * (so & 1) + r - 1, iyb = iyt + 1;
            row_ok = img_ok && (unsigned)iyt < 4u;
            row_ok2 = img_ok && (unsigned)iyb < 4u;
            const float* __restrict__ xb = d.X + (int64_t)bb * d.x_bstride + (int64_t)min(c0 + bc, d.C - 1) * HWs;
            rb[0] = *reinterpret_cast<const f32x4*>(xb + (row_ok ? iyt : 0) * 4);
            rb[1] = *reinterpret_cast<const f32x4*>(xb + (row_ok2 ? iyb : 0) * 4);
            return;
        }
        const int b = ks / steps_per_img;
        int y0, x0 = 0;
        if (WIDE) {
            const int rem = ks - b * steps_per_img;
            y0 = rem / segs;
            x0 = (rem - y0 * segs) * 32;
        } else {
            y0 = (ks - b * steps_per_img) * ROWS;
        }
        // Buffer loads: the descriptor's base is the K-step's image (wave-uniform, rebuilt per step with scalar instructions), the lane part is a
        // 32-bit byte offset -- fixed for the tile on the dY side, two integer operations per step on the X side (a row outside the image is simply out
        // of range and reads 0) -- instead of a 64-bit address per load.
        const __amdgpu_buffer_rsrc_t dyr = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(d.dY + (int64_t)b * d.dy_bstride + (WIDE ? y0 * d.OW + x0 : y0 * W)), 0, 0xFFFFFFF0, 0x00020000);
        ra[0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyr, a_voff0, 0, 0));
        ra[1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyr, a_voff0 + 16u, 0, 0));
        ra[2] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyr, a_voff1, 0, 0));
        ra[3] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyr, a_voff1 + 16u, 0, 0));
        int iy = (MODE == 4) ? 2 * (y0 + s_rr) + r - d.pad : y0 + s_rr + r - 1;
        if (MODE == 2) {                           // row of the (virtual) upsampled image -> source row
            row_ok = (unsigned)iy < (unsigned)(2 * d.H);
            iy >>= 1;
        } else {
            row_ok = (unsigned)iy < (unsigned)d.H;
        }
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.X + (int64_t)b * d.x_bstride), 0, 0xFFFFFFF0, 0x00020000);
        const unsigned xv = row_ok ? b_voff + 4u * (unsigned)(iy * d.W + (MODE == 2 ? x0 / 2 : (MODE == 4 ? 2 * x0 : x0))) : 0xFFFFFFFFu;
        rb[0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, xv, 0, 0));
        if (MODE != 2) rb[1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, xv + 16u, 0, 0));
        if constexpr (MODE == 4) {
            // stride 2: the octet's 8 output columns read input columns 16 xo - pad ... 16 xo + 16 - pad: the 16 aligned ones plus ONE neighbour
            // (right of them for pad 0, left for pad 1; outside the row it is the zero padding)
            rb[2] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, xv + 32u, 0, 0));
            rb[3] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, xv + 48u, 0, 0));
            const int ix0 = 2 * x0 + 16 * s_xo;     // (x0: the segment's first OUTPUT column, wide images)
            // ONE load with a selected offset, then both neighbours assigned unconditionally: "if (pad) rl = ...; else rr_ = ...;" becomes a store through
            // a selected pointer, which pins the lambdas' closure (operands, descriptors, flags) in scratch memory and turns the buffer loads into
            // waterfall loops (496 bytes of private segment, 40 TF/s)
            const bool p1 = d.pad != 0;
            const bool hok = row_ok && (p1 ? ix0 > 0 : ix0 + 16 < d.W);
            const float hv = hok ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, p1 ? xv - 4u : xv + 64u, 0, 0)) : 0.f;
            rl = p1 ? hv : 0.f;
            rr_ = p1 ? 0.f : hv;
        }
        if (WIDE && MODE != 4) {
            const int ix = x0 + 8 * s_xo;          // first pixel of the octet (MODE 2: in the upsampled image, whose width is OW)
            const unsigned nsrc = (MODE == 2) ? 4u : 8u;  // source pixels under the octet
            rl = (ix > 0 && row_ok) ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, xv - 4u, 0, 0)) : 0.f;
            rr_ = (ix + 8 < d.OW && row_ok) ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, xv + 4u * nsrc, 0, 0)) : 0.f;
        }
    };
    auto store_stage = [&]() {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bool ok = (i ? a_ok1 : a_ok0) && img_ok;
            float v[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = ok ? ra[2 * i][j] : 0.f;
                v[4 + j] = ok ? ra[2 * i + 1][j] : 0.f;
            }
            u32x4 hi, lo;
            split_bf16x8(v, hi, lo);
            As[so * LDA_ + am + 64 * i] = hi;
            As[(4 + so) * LDA_ + am + 64 * i] = lo;
        }
        if (W4) {                                  // two 4-pixel rows per octet, each with its own zero halo: (0, t0..t3, 0), (0, b0..b3, 0)
            const bool okt = b_ok && row_ok, okb = b_ok && row_ok2;
            unsigned T[3], TL[3], U[3], UL[3];
            split_pair(0.f, okt ? rb[0][0] : 0.f, T[0], TL[0]);
            split_pair(okt ? rb[0][1] : 0.f, okt ? rb[0][2] : 0.f, T[1], TL[1]);
            split_pair(okt ? rb[0][3] : 0.f, 0.f, T[2], TL[2]);
            split_pair(0.f, okb ? rb[1][0] : 0.f, U[0], UL[0]);
            split_pair(okb ? rb[1][1] : 0.f, okb ? rb[1][2] : 0.f, U[1], UL[1]);
            split_pair(okb ? rb[1][3] : 0.f, 0.f, U[2], UL[2]);
            u32x4* __restrict__ bs4 = Bs + so * LDB_ + bc;
            bs4[(0 * 2 + 0) * 4 * LDB_] = u32x4{T[0], T[1], U[0], U[1]};
            bs4[(0 * 2 + 1) * 4 * LDB_] = u32x4{TL[0], TL[1], UL[0], UL[1]};
            bs4[(1 * 2 + 0) * 4 * LDB_] = u32x4{__builtin_amdgcn_alignbit(T[1], T[0], 16), __builtin_amdgcn_alignbit(T[2], T[1], 16),
                                                __builtin_amdgcn_alignbit(U[1], U[0], 16), __builtin_amdgcn_alignbit(U[2], U[1], 16)};
            bs4[(1 * 2 + 1) * 4 * LDB_] = u32x4{__builtin_amdgcn_alignbit(TL[1], TL[0], 16), __builtin_amdgcn_alignbit(TL[2], TL[1], 16),
                                                __builtin_amdgcn_alignbit(UL[1], UL[0], 16), __builtin_amdgcn_alignbit(UL[2], UL[1], 16)};
            bs4[(2 * 2 + 0) * 4 * LDB_] = u32x4{T[1], T[2], U[1], U[2]};
            bs4[(2 * 2 + 1) * 4 * LDB_] = u32x4{TL[1], TL[2], UL[1], UL[2]};
            return;
        }
        const bool ok = b_ok && row_ok;
        if constexpr (MODE == 4) {
            // e[j] = input column 16 xo - pad + j, j = 0..16; tap s of output column k reads e[2 k + s].  Taps 0 and 2 share their even elements
            // (tap 2 = tap 0 shifted by one output column), tap 1 takes the odd ones.
            // (both paddings with compile-time indices and a select: a branch per padding made the compiler put e[] into scratch memory -- 496 bytes of
            // private segment, 40 TF/s)
            float e[18];
            const bool p1 = d.pad != 0;
#pragma unroll
            for (int j = 0; j < 17; ++j) {
                const float v0 = (j < 16) ? rb[(j < 16 ? j : 0) >> 2][j & 3] : rr_;                    // pad 0: input column 16 xo + j
                const float v1 = (j == 0) ? rl : rb[((j > 0 ? j : 1) - 1) >> 2][((j > 0 ? j : 1) - 1) & 3];     // pad 1: input column 16 xo + j - 1
                e[j] = ok ? (p1 ? v1 : v0) : 0.f;
            }
            e[17] = 0.f;
            unsigned D[5], Lw[5], O[4], Ol[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) split_pair(e[4 * k], e[4 * k + 2], D[k], Lw[k]);          // even elements: (e0,e2) (e4,e6) (e8,e10) (e12,e14)
            split_pair(e[16], 0.f, D[4], Lw[4]);
#pragma unroll
            for (int k = 0; k < 4; ++k) split_pair(e[4 * k + 1], e[4 * k + 3], O[k], Ol[k]);      // odd elements:  (e1,e3) (e5,e7) (e9,e11) (e13,e15)
            u32x4* __restrict__ bs = Bs + so * LDB_ + bc;
            bs[(0 * 2 + 0) * 4 * LDB_] = u32x4{D[0], D[1], D[2], D[3]};
            bs[(0 * 2 + 1) * 4 * LDB_] = u32x4{Lw[0], Lw[1], Lw[2], Lw[3]};
            bs[(1 * 2 + 0) * 4 * LDB_] = u32x4{O[0], O[1], O[2], O[3]};
            bs[(1 * 2 + 1) * 4 * LDB_] = u32x4{Ol[0], Ol[1], Ol[2], Ol[3]};
            bs[(2 * 2 + 0) * 4 * LDB_] = u32x4{__builtin_amdgcn_alignbit(D[1], D[0], 16), __builtin_amdgcn_alignbit(D[2], D[1], 16),
                                               __builtin_amdgcn_alignbit(D[3], D[2], 16), __builtin_amdgcn_alignbit(D[4], D[3], 16)};
            bs[(2 * 2 + 1) * 4 * LDB_] = u32x4{__builtin_amdgcn_alignbit(Lw[1], Lw[0], 16), __builtin_amdgcn_alignbit(Lw[2], Lw[1], 16),
                                               __builtin_amdgcn_alignbit(Lw[3], Lw[2], 16), __builtin_amdgcn_alignbit(Lw[4], Lw[3], 16)};
            return;
        }
        float e[10];
        if (MODE == 2) {                           // 8 upsampled pixels = 4 source pixels, each twice
#pragma unroll
            for (int j = 0; j < 4; ++j) e[1 + 2 * j] = e[2 + 2 * j] = ok ? rb[0][j] : 0.f;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                e[1 + j] = ok ? rb[0][j] : 0.f;
                e[5 + j] = ok ? rb[1][j] : 0.f;
            }
        }
        // horizontal neighbours: the octets of one row sit in adjacent lanes
        // (DPP row shifts, not __shfl_up / __shfl_down: those compile to ds_bpermute_b32, an LDS-crossbar round trip inside the store window; the
        // octets of a row are 2 or 4 adjacent lanes, never across a 16-lane row)
        const float lft = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, e[8]), 0x111, 0xF, 0xF, true));   // row_shr:1: from lane - 1
        const float rgt = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, e[1]), 0x101, 0xF, 0xF, true));   // row_shl:1: from lane + 1
        e[0] = (s_xo > 0) ? lft : 0.f;
        e[9] = (s_xo < OPR - 1) ? rgt : 0.f;
        if (WIDE) {                                // segment edges: the neighbour is a pixel of the adjacent segment
            e[0] = ok ? rl : 0.f;
            e[9] = ok ? rr_ : 0.f;
        }
        unsigned D[5], Lw[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) split_pair(e[2 * k], e[2 * k + 1], D[k], Lw[k]);
        u32x4* __restrict__ bs = Bs + so * LDB_ + bc;
        bs[(0 * 2 + 0) * 4 * LDB_] = u32x4{D[0], D[1], D[2], D[3]};
        bs[(0 * 2 + 1) * 4 * LDB_] = u32x4{Lw[0], Lw[1], Lw[2], Lw[3]};
        bs[(1 * 2 + 0) * 4 * LDB_] = u32x4{__builtin_amdgcn_alignbit(D[1], D[0], 16), __builtin_amdgcn_alignbit(D[2], D[1], 16),
                                           __builtin_amdgcn_alignbit(D[3], D[2], 16), __builtin_amdgcn_alignbit(D[4], D[3], 16)};
        bs[(1 * 2 + 1) * 4 * LDB_] = u32x4{__builtin_amdgcn_alignbit(Lw[1], Lw[0], 16), __builtin_amdgcn_alignbit(Lw[2], Lw[1], 16),
                                           __builtin_amdgcn_alignbit(Lw[3], Lw[2], 16), __builtin_amdgcn_alignbit(Lw[4], Lw[3], 16)};
        bs[(2 * 2 + 0) * 4 * LDB_] = u32x4{D[1], D[2], D[3], D[4]};
        bs[(2 * 2 + 1) * 4 * LDB_] = u32x4{Lw[1], Lw[2], Lw[3], Lw[4]};
    };

    f32x16 acc[2][3];                              // [m group][tap s]
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int sx = 0; sx < 3; ++sx)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[mi][sx][v] = 0.f;

    const int wm = wave >> 1, wc = wave & 1;       // 2 x 2 waves: 64 m x 32 c each
    const u32x4* __restrict__ a_base = As + h * LDA_ + wm * 64 + l31;
    const u32x4* __restrict__ b_base = Bs + h * LDB_ + wc * 32 + l31;

#ifdef VD_WG_STAMPS
    const unsigned long long rt_begin = __builtin_amdgcn_s_memrealtime();
    WG_STAMP(cy_begin);
    unsigned long long sL = 0, sM = 0, sB1 = 0, sS = 0, sB2 = 0;
#endif
    if (ks_begin < ks_end) {
        load_stage(ks_begin);
        store_stage();
        __syncthreads();
        for (int ks = ks_begin; ks < ks_end; ++ks) {
            const bool more = ks + 1 < ks_end;
#ifdef VD_WG_STAMPS
            WG_STAMP(t0);
#endif
            if (more) load_stage(ks + 1);
#ifdef VD_WG_STAMPS
            WG_STAMP(t1);
#endif
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {       // 16 pixels = octets 2kk (lanes 0-31) and 2kk+1 (lanes 32-63)
                bf16x8 ah[2], al[2];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    ah[mi] = __builtin_bit_cast(bf16x8, a_base[(2 * kk) * LDA_ + mi * 32]);
                    al[mi] = __builtin_bit_cast(bf16x8, a_base[(4 + 2 * kk) * LDA_ + mi * 32]);
                }
#pragma unroll
                for (int sx = 0; sx < 3; ++sx) {
                    const bf16x8 bh = __builtin_bit_cast(bf16x8, b_base[((sx * 2 + 0) * 4 + 2 * kk) * LDB_]);
                    const bf16x8 bl = __builtin_bit_cast(bf16x8, b_base[((sx * 2 + 1) * 4 + 2 * kk) * LDB_]);
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi) {
                        acc[mi][sx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mi], bh, acc[mi][sx], 0, 0, 0);
                        acc[mi][sx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bl, acc[mi][sx], 0, 0, 0);
                        acc[mi][sx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bh, acc[mi][sx], 0, 0, 0);
                    }
                }
            }
#ifdef VD_WG_STAMPS
            WG_STAMP(t2);
            __syncthreads();
            WG_STAMP(t3);
            if (more) store_stage();
            WG_STAMP(t4);
            __syncthreads();
            WG_STAMP(t5);
            sL += t1 - t0, sM += t2 - t1, sB1 += t3 - t2, sS += t4 - t3, sB2 += t5 - t4;
#else
            __syncthreads();
            if (more) store_stage();
            __syncthreads();
#endif
        }
    }
#ifdef VD_WG_STAMPS
    WG_STAMP(cy_loop);
#endif
    wgrad_patch_store(d, acc, r, m0, c0, wm, wc, lane, h, by, gy);
#ifdef VD_WG_STAMPS
    if (g_wg_stamps && lane == 0) {
        unsigned long long* __restrict__ o = g_wg_stamps + ((int64_t)blockIdx.x * 4 + wave) * 12;
        o[0] = rt_begin, o[1] = __builtin_amdgcn_s_memrealtime(), o[2] = cy_begin, o[3] = cy_loop, o[4] = __builtin_amdgcn_s_memtime();
        o[5] = sL, o[6] = sM, o[7] = sB1, o[8] = sS, o[9] = sB2, o[10] = (unsigned long long)(ks_end - ks_begin), o[11] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) /* HW_ID */;
    }
#endif
}

template <int W, int MODE, bool WIDE = false>
__global__ __launch_bounds__(NT, 3) void wgrad_bx3_kernel(const vd_wgrad_desc d, int ksteps_per_split) {
    wgrad_bx3_body<W, MODE, WIDE>(d, ksteps_per_split, gridDim.x, gridDim.y, blockIdx.x + gridDim.x * blockIdx.y);
}

template <int W, int MODE, bool WIDE = false>
__global__ __launch_bounds__(NT, 3) void wgrad_bx3_group_kernel(const vd_wgrad_job* __restrict__ jobs, int n_jobs) {
    const vd_wgrad_job* __restrict__ jb = jobs + wgrad_find_job(jobs, n_jobs, blockIdx.x, false);
    const int lin = blockIdx.x - jb->first_block;
    if (lin >= jb->gx * jb->gy) return;            // padding blocks between jobs
    const vd_wgrad_desc d = jb->d;
    wgrad_bx3_body<W, MODE, WIDE>(d, jb->ks_per, jb->gx, jb->gy, lin);
}

#include "vd_wgrad_k32.inc"

// ---- split-precision weight gradient of a 1x1 convolution:  dW[m][c] = sum_{b,p} dY[b][m][p] * X[b][c][p]  ------------------
// Both operands are pixel-contiguous, so a lane's 8-deep k-fragment is one aligned 32-byte read of each.  A workgroup owns a
// 128 (m) x 128 (c) tile and a contiguous range of K-steps of 64 pixels (8 octets; NP % 8 == 0, so an octet never straddles images;
// octets beyond the last pixel are zero).  LDS: As[part][octet 0..7][m], Bs[part][octet][c], octet stride 130 units.
// Split-K slabs are plain [M][C] images reduced in fixed order by slab_reduce_kernel.
__device__ __forceinline__ void wgrad1x1_bx3_body(const vd_wgrad_desc& d, int ksteps_per_split, int gx, int gy, int lin) {
    constexpr int LD_ = 130;
    __shared__ u32x4 As[2 * 8 * LD_];
    __shared__ u32x4 Bs[2 * 8 * LD_];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
    const int tiles_m = (d.M + 127) / 128;
    const int bxx = lin % gx, by = lin / gx;
    const int tm = bxx % tiles_m, tc = bxx / tiles_m;
    const int m0 = tm * 128, c0 = tc * 128;
    const int oct_per_img = d.NP >> 3;
    const int oct_total = d.nb * oct_per_img;
    const int ks_total = (oct_total + 7) >> 3;
    const int ks_begin = by * ksteps_per_split;
    const int ks_end = min(ks_total, ks_begin + ksteps_per_split);

    const int so = tid & 7, sr = tid >> 3;         // staging: octet of the K-step, row (m or c) sr + 32*i
    f32x4 ra[8], rb[8];
    bool oct_ok = false;
    // buffer loads: descriptor base = the K-step's first image (wave-uniform), 32-bit lane offsets; the row offsets are fixed for the tile
    unsigned rowa[4], rowb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        rowa[i] = 4u * (unsigned)(min(m0 + sr + 32 * i, d.M - 1) * d.NP);
        rowb[i] = 4u * (unsigned)(min(c0 + sr + 32 * i, d.C - 1) * d.NP);
    }
    auto load_stage = [&](int ks) {
        const int g = ks * 8 + so;                 // global octet -> (image, pixel)
        oct_ok = g < oct_total;
        const int gg = oct_ok ? g : oct_total - 1;   // (clamped, not 0: an image BEFORE the step's first one would give a negative offset from its descriptor base)
        const int b = gg / oct_per_img, p = (gg - b * oct_per_img) * 8;
        const int b0 = min(ks * 8, oct_total - 1) / oct_per_img;
        const __amdgpu_buffer_rsrc_t dyr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.dY + (int64_t)b0 * d.dy_bstride), 0, 0xFFFFFFF0, 0x00020000);
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(d.X + (int64_t)b0 * d.x_bstride), 0, 0xFFFFFFF0, 0x00020000);
        const unsigned va = 4u * (unsigned)((b - b0) * d.dy_bstride + p), vb = 4u * (unsigned)((b - b0) * d.x_bstride + p);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ra[2 * i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyr, va + rowa[i], 0, 0));
            ra[2 * i + 1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyr, va + rowa[i] + 16u, 0, 0));
            rb[2 * i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, vb + rowb[i], 0, 0));
            rb[2 * i + 1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, vb + rowb[i] + 16u, 0, 0));
        }
    };
    auto store_stage = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool aok = oct_ok && (m0 + sr + 32 * i < d.M), bok = oct_ok && (c0 + sr + 32 * i < d.C);
            float va[8], vb[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                va[j] = aok ? ra[2 * i][j] : 0.f;
                va[4 + j] = aok ? ra[2 * i + 1][j] : 0.f;
                vb[j] = bok ? rb[2 * i][j] : 0.f;
                vb[4 + j] = bok ? rb[2 * i + 1][j] : 0.f;
            }
            u32x4 hi, lo;
            split_bf16x8(va, hi, lo);
            As[so * LD_ + sr + 32 * i] = hi;
            As[(8 + so) * LD_ + sr + 32 * i] = lo;
            split_bf16x8(vb, hi, lo);
            Bs[so * LD_ + sr + 32 * i] = hi;
            Bs[(8 + so) * LD_ + sr + 32 * i] = lo;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[mi][ni][v] = 0.f;

    const int wm = wave >> 1, wc = wave & 1;       // 2 x 2 waves: 64 m x 64 c each
    const u32x4* __restrict__ a_base = As + h * LD_ + wm * 64 + l31;
    const u32x4* __restrict__ b_base = Bs + h * LD_ + wc * 64 + l31;

    if (ks_begin < ks_end) {
        load_stage(ks_begin);
        store_stage();
        __syncthreads();
        for (int ks = ks_begin; ks < ks_end; ++ks) {
            const bool more = ks + 1 < ks_end;
            if (more) load_stage(ks + 1);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {       // 16 pixels = octets 2kk (lanes 0-31) and 2kk+1 (lanes 32-63)
                bf16x8 ah[2], al[2];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    ah[mi] = __builtin_bit_cast(bf16x8, a_base[(2 * kk) * LD_ + mi * 32]);
                    al[mi] = __builtin_bit_cast(bf16x8, a_base[(8 + 2 * kk) * LD_ + mi * 32]);
                }
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    const bf16x8 bh = __builtin_bit_cast(bf16x8, b_base[(2 * kk) * LD_ + ni * 32]);
                    const bf16x8 bl = __builtin_bit_cast(bf16x8, b_base[(8 + 2 * kk) * LD_ + ni * 32]);
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi) {
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mi], bh, acc[mi][ni], 0, 0, 0);
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bl, acc[mi][ni], 0, 0, 0);
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mi], bh, acc[mi][ni], 0, 0, 0);
                    }
                }
            }
            __syncthreads();
            if (more) store_stage();
            __syncthreads();
        }
    }
    float* __restrict__ out = (gy > 1) ? (d.ws + (int64_t)by * d.M * d.C) : d.dW;
    const bool accum = (gy == 1) && d.accumulate;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int c = c0 + wc * 64 + ni * 32 + l31;
        if (c >= d.C) continue;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int m = m0 + wm * 64 + mi * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
                if (m >= d.M) continue;
                const int64_t off = (int64_t)m * d.C + c;
                out[off] = accum ? (out[off] + acc[mi][ni][v]) : acc[mi][ni][v];
            }
    }
}

__global__ __launch_bounds__(NT, 2) void wgrad1x1_bx3_kernel(const vd_wgrad_desc d, int ksteps_per_split) {
    wgrad1x1_bx3_body(d, ksteps_per_split, gridDim.x, gridDim.y, blockIdx.x + gridDim.x * blockIdx.y);
}

#include "vd_wgrad1x1_wide.inc"

// Fixed-order reduction of every split job's slabs in one launch: 3x3 jobs keep the permuted slab layout ws[z][r][m][c][3]
// (slab_reduce_perm_kernel), 1x1 jobs plain [M][C] images.
__global__ __launch_bounds__(256) void wgrad_group_reduce_kernel(const vd_wgrad_job* __restrict__ jobs, int n_jobs) {
    const vd_wgrad_job* __restrict__ jb = jobs + wgrad_find_job(jobs, n_jobs, blockIdx.x, true);
    const int lb = blockIdx.x - jb->first_rblock;
    if (lb >= jb->rblocks || jb->gy <= 1) return;
    const int M = jb->d.M, C = jb->d.C, T = jb->d.T, splits = jb->gy, accumulate = jb->d.accumulate;
    const float* __restrict__ ws = jb->d.ws;
    float* __restrict__ out = jb->d.dW;
    const int64_t n = (int64_t)M * C * T;
    if ((n & 3) == 0 && ((((uintptr_t)ws) & 15) == 0)) {
        // float4 form (round 4): 16 bytes per lane and four slabs in flight per thread, the SAME summation order (bit-identical results).  The scalar loop
        // below moved config #4's 128 slabs per layer at ~1.5 TB/s (1.5 ms per step).
        const int64_t n4 = n >> 2;
        const f32x4* __restrict__ ws4 = reinterpret_cast<const f32x4*>(ws);
        for (int64_t i4 = lb * 256 + threadIdx.x; i4 < n4; i4 += (int64_t)jb->rblocks * 256) {
            const f32x4* __restrict__ p = ws4 + i4;
            f32x4 s = p[0];
            int z = 1;
            for (; z + 4 <= splits; z += 4) {
                const f32x4 a = p[(int64_t)z * n4], b = p[(int64_t)(z + 1) * n4], c = p[(int64_t)(z + 2) * n4], e = p[(int64_t)(z + 3) * n4];
#pragma unroll
                for (int j = 0; j < 4; ++j) s[j] = (((s[j] + a[j]) + b[j]) + c[j]) + e[j];
            }
            for (; z < splits; ++z) {
                const f32x4 a = p[(int64_t)z * n4];
#pragma unroll
                for (int j = 0; j < 4; ++j) s[j] += a[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t i = 4 * i4 + j;
                int64_t o = i;
                if (T == 9) {
                    const int sx = (int)(i % 3);
                    const int64_t t = i / 3;
                    const int c = (int)(t % C);
                    const int64_t t2 = t / C;
                    const int m = (int)(t2 % M), r = (int)(t2 / M);
                    o = ((int64_t)m * C + c) * 9 + r * 3 + sx;
                }
                out[o] = accumulate ? (out[o] + s[j]) : s[j];
            }
        }
        return;
    }
    for (int64_t i = lb * 256 + threadIdx.x; i < n; i += (int64_t)jb->rblocks * 256) {
        float s = ws[i];
        for (int z = 1; z < splits; ++z) s += ws[(int64_t)z * n + i];
        int64_t o = i;
        if (T == 9) {
            const int sx = (int)(i % 3);
            const int64_t t = i / 3;
            const int c = (int)(t % C);
            const int64_t t2 = t / C;
            const int m = (int)(t2 % M), r = (int)(t2 / M);
            o = ((int64_t)m * C + c) * 9 + r * 3 + sx;
        }
        out[o] = accumulate ? (out[o] + s) : s;
    }
}

static bool wgrad1x1_bx3_eligible(const vd_wgrad_desc& d) {
    return d.math == 1 && d.T == 1 && d.mode == VD_B_PLAIN && d.NP % 8 == 0 && d.M >= 64 && d.C >= 64 && d.tile == 0 &&
           (d.x_bstride & 3) == 0 && (d.dy_bstride & 3) == 0 && ((((uintptr_t)d.X) | ((uintptr_t)d.dY)) & 15) == 0;
}

static void wgrad1x1_bx3_plan(const vd_wgrad_desc& d, int& splits, int& ks_per) {
    const int ks_total = (int)(((int64_t)d.nb * (d.NP >> 3) + 7) >> 3);
    const int base = vd_cdiv(d.M, 128) * vd_cdiv(d.C, 128);
    splits = d.splits;
    if (splits <= 0) {                             // one workgroup per CU (measured: 256 beats 192 / 384 / 512 -- every extra split is a 128 x 128 slab), >= 4 K-steps per split
        constexpr int target = 256;
        splits = vd_cdiv(target, base);
        const int max_splits = ks_total / 4 > 0 ? ks_total / 4 : 1;
        if (splits > max_splits) splits = max_splits;
        if (splits < 1) splits = 1;
    }
    ks_per = vd_cdiv(ks_total, splits);
    splits = vd_cdiv(ks_total, ks_per);
}
