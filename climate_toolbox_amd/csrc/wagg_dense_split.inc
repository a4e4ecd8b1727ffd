// Split form of the full-form fp32 contraction (included by wagg_dense.hip): the same work items, LDS image, DMA pieces,
// swizzle, double buffer and fragment offsets as dense_mfma_kernel<float, 0, false, MT>, but the products run on the f16
// matrix pipe.  Each operand is an f16 high part plus an f16 low part of a power-of-two scaled copy:
//   X row t:     x 2^ex[t] = xh + xl   (dense_pack_x_split_kernel; ex[t] puts the row's largest |x| in [2^14, 2^15))
//   W column r:  w 2^ew[r] = wh + wl   (here, in registers, from the fp32 W tile; ew[r] from the plan's column maxima)
// and a 16 x 16 x 32 block is xh.wl + xl.wh + xh.wh: three v_mfma_f32_16x16x32_f16 (16 cycles each) against eight
// v_mfma_f32_16x16x4_f32 (32 cycles each).  The f32 accumulators hold the scaled sums; dense_reduce_split_kernel undoes
// the scales (exact: powers of two) before the division by den[r].
//
// k order: lane group kq's W fragments are pieces kq (k = 4 kq + c) and kq + 4 (k = 16 + 4 kq + c), c = 0..3; they are
// converted into one 8 x f16 operand in that order.  The X packer writes the same k set in the same order: the high
// parts into piece kq, the low parts into piece kq + 4, so the two fragment reads of the fp32 kernel (frag0, frag1)
// fetch xh and xl.  A and B agree on k; which k an MFMA lane slot stands for does not matter otherwise.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// exponent that brings a maximum m > 0 into [2^14, 2^15) (0 for m = 0): f16 keeps the scaled value and its remainder
__host__ __device__ __forceinline__ int split_exp(float m) {
    int e = 0;
    if (!(m > 0.0f)) return 0;
    (void)frexpf(m, &e);                               // m = f 2^e, f in [0.5, 1)
    return 15 - e;
}

// four fp32 W values of piece kq and four of piece kq + 4 -> scaled f16 high and low parts, in k order
__device__ __forceinline__ void split_w8(f32x4 a, f32x4 b, int e, f16x8 &hi, f16x8 &lo) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float va = __builtin_amdgcn_ldexpf(a[c], e), vb = __builtin_amdgcn_ldexpf(b[c], e);
        const _Float16 ha = (_Float16)va, hb = (_Float16)vb;
        hi[c] = ha; hi[4 + c] = hb;
        lo[c] = (_Float16)(va - (float)ha); lo[4 + c] = (_Float16)(vb - (float)hb);
    }
}

template <int MT>
__global__ __launch_bounds__(D_THREADS, 2) void dense_split_kernel(
    const f16x8 *__restrict__ Xp, const float *__restrict__ Wp, const float *__restrict__ wmax, int n_kt, int n_nt, int n_mb,
    int S, int kt_per_slice, float *__restrict__ slabs) {
    static_assert(MT <= D_MT, "accumulators of MT row blocks must fit the register file");
    extern __shared__ __attribute__((aligned(16))) char lds[];   // [2][BUF_BYTES]
    constexpr int XT4 = d_xt_bytes(MT);
    constexpr int BUF_BYTES = d_buf_bytes(MT);
    constexpr int XPIECES = XT4 / 1024;
    constexpr int NXP = (XPIECES + 7) / 8;
    constexpr int NP = 4 + NXP;
    constexpr int DPB = (NP + MT - 1) / MT;
    static_assert(DPB <= 5, "at most five DMA pieces per row block");
    static_assert(NP <= 10, "prologue issues at most ten pieces");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, kq = lane >> 4;

    // work item as in dense_mfma_kernel (blocks with equal blockIdx % 8 share a k-slice)
    int j = (int)(blockIdx.x >> 3);
    const int nt = j % n_nt; j /= n_nt;
    const int mb = j % n_mb;
    const int ks = (int)(blockIdx.x & 7) + 8 * (j / n_mb);
    const int kt0 = ks * kt_per_slice;
    const int kt1 = kt0 + kt_per_slice < n_kt ? kt0 + kt_per_slice : n_kt;
    const int ntiles = kt1 > kt0 ? kt1 - kt0 : 0;
    const int64_t w_first = (int64_t)nt * n_kt + kt0;
    // scales of this lane's two columns (the plan pads wmax to whole column tiles with zeros)
    const int ew0 = split_exp(wmax[nt * D_BN + wave * 32 + lr]);
    const int ew1 = split_exp(wmax[nt * D_BN + wave * 32 + 16 + lr]);

    const char *xsrc = reinterpret_cast<const char *>(Xp) + ((int64_t)mb * n_kt + kt0) * XT4 + lane * 16;
    const char *wsrc = reinterpret_cast<const char *>(Wp) + w_first * D_WTB + lane * 16;
#define WAGG_DMA_X(q, tile, buf)                                                                  \
    __builtin_amdgcn_global_load_lds((gptr_t)(xsrc + (int64_t)(tile) * XT4 + (q) * 1024),      \
                                     (lptr_t)(lds + (buf) * BUF_BYTES + (q) * 1024), 16, 0, 0)
#define WAGG_DMA_W(q, tile, buf)                                                                  \
    __builtin_amdgcn_global_load_lds((gptr_t)(wsrc + (int64_t)(tile) * D_WTB + (q) * 1024),   \
                                     (lptr_t)(lds + (buf) * BUF_BYTES + XT4 + (q) * 1024), 16, 0, 0)
#define WAGG_DMA_PIECE(i, tile, buf)                                                              \
    do {                                                                                          \
        constexpr int i_ = (i);                                                                   \
        if constexpr (i_ < 4) WAGG_DMA_W(wave + 8 * i_, tile, buf);                               \
        else if constexpr (8 * (i_ - 4) + 7 < XPIECES) WAGG_DMA_X(wave + 8 * (i_ - 4), tile, buf); \
        else { if (wave + 8 * (i_ - 4) < XPIECES) WAGG_DMA_X(wave + 8 * (i_ - 4), tile, buf); }   \
    } while (0)
#define WAGG_DMA_BLOCK(RB, tile, buf)                                                             \
    do {                                                                                          \
        if constexpr (DPB * (RB) + 0 < NP && 0 < DPB) WAGG_DMA_PIECE(DPB * (RB) + 0 < NP ? DPB * (RB) + 0 : 0, tile, buf); \
        if constexpr (DPB * (RB) + 1 < NP && 1 < DPB) WAGG_DMA_PIECE(DPB * (RB) + 1 < NP ? DPB * (RB) + 1 : 0, tile, buf); \
        if constexpr (DPB * (RB) + 2 < NP && 2 < DPB) WAGG_DMA_PIECE(DPB * (RB) + 2 < NP ? DPB * (RB) + 2 : 0, tile, buf); \
        if constexpr (DPB * (RB) + 3 < NP && 3 < DPB) WAGG_DMA_PIECE(DPB * (RB) + 3 < NP ? DPB * (RB) + 3 : 0, tile, buf); \
        if constexpr (DPB * (RB) + 4 < NP && 4 < DPB) WAGG_DMA_PIECE(DPB * (RB) + 4 < NP ? DPB * (RB) + 4 : 0, tile, buf); \
    } while (0)

    f32x4 acc[MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m][0] = acc[m][1] = f32x4{0, 0, 0, 0};

    if (ntiles > 0) {
        WAGG_DMA_PIECE(0, 0, 0); WAGG_DMA_PIECE(1, 0, 0); WAGG_DMA_PIECE(2, 0, 0); WAGG_DMA_PIECE(3, 0, 0);
        WAGG_DMA_PIECE(4, 0, 0);
        if constexpr (NP > 5) WAGG_DMA_PIECE(NP > 5 ? 5 : 0, 0, 0);
        if constexpr (NP > 6) WAGG_DMA_PIECE(NP > 6 ? 6 : 0, 0, 0);
        if constexpr (NP > 7) WAGG_DMA_PIECE(NP > 7 ? 7 : 0, 0, 0);
        if constexpr (NP > 8) WAGG_DMA_PIECE(NP > 8 ? 8 : 0, 0, 0);
        if constexpr (NP > 9) WAGG_DMA_PIECE(NP > 9 ? 9 : 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    const int f = lr >> 1;
    const int frag0 = (lr * 8 + (kq ^ f)) * 16;            // piece kq: W k = 4 kq + c, X high parts
    const int frag1 = (lr * 8 + ((kq ^ f) ^ 4)) * 16;      // piece kq + 4: W k = 16 + 4 kq + c, X low parts
    const int boff = XT4 + wave * (32 * 128);

#define WAGG_MFMA16(RB, CB, A, B) acc[RB][CB] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A, B, acc[RB][CB], 0, 0, 0)
#define WAGG_READ_A(H, L, RB)                                                                     \
    do {                                                                                          \
        H = *reinterpret_cast<const f16x8 *>(img + frag0 + (RB) * 2048);                          \
        L = *reinterpret_cast<const f16x8 *>(img + frag1 + (RB) * 2048);                          \
    } while (0)
    // Row block RB: six MFMAs, cross terms first, xh.wh last (the largest term is added to the smallest partial sums
    // last).  The next block's fragment reads go right behind the first MFMA; the next tile's DMA pieces go after the
    // third (waves 0-3) or the sixth (waves 4-7), so that one wave of a SIMD always has MFMAs to issue.
#define WAGG_BLOCK_(RB, H, L, NH, NL)                                                             \
    do {                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        WAGG_MFMA16(RB, 0, H, wl0);                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        if constexpr ((RB) + 1 < MT) WAGG_READ_A(NH, NL, (RB) + 1 < MT ? (RB) + 1 : 0);           \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        WAGG_MFMA16(RB, 1, H, wl1);                                                               \
        WAGG_MFMA16(RB, 0, L, wh0);                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        if (early_dma) WAGG_DMA_BLOCK(RB, tnext, nbuf);                                           \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        WAGG_MFMA16(RB, 1, L, wh1);                                                               \
        WAGG_MFMA16(RB, 0, H, wh0);                                                               \
        WAGG_MFMA16(RB, 1, H, wh1);                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        if (!early_dma) WAGG_DMA_BLOCK(RB, tnext, nbuf);                                          \
    } while (0)
#define WAGG_BLOCK(RB)                                                                            \
    do {                                                                                          \
        if constexpr ((RB) < MT) {                                                                \
            constexpr int rb_ = (RB) < MT ? (RB) : 0;                                             \
            if constexpr ((RB) & 1) WAGG_BLOCK_(rb_, aBh, aBl, aAh, aAl);                         \
            else WAGG_BLOCK_(rb_, aAh, aAl, aBh, aBl);                                            \
        }                                                                                         \
    } while (0)

    const bool early_dma = wave < 4;
    for (int tile = 0; tile < ntiles; ++tile) {
        const char *img = lds + (tile & 1) * BUF_BYTES;
        const int nbuf = (tile & 1) ^ 1;
        const int tnext = tile + 1 < ntiles ? tile + 1 : tile;     // last tile: harmless re-load
        f16x8 wh0, wl0, wh1, wl1, aAh, aAl, aBh, aBl;
        {
            const f32x4 b00 = *reinterpret_cast<const f32x4 *>(img + boff + frag0);
            const f32x4 b01 = *reinterpret_cast<const f32x4 *>(img + boff + frag1);
            const f32x4 b10 = *reinterpret_cast<const f32x4 *>(img + boff + 2048 + frag0);
            const f32x4 b11 = *reinterpret_cast<const f32x4 *>(img + boff + 2048 + frag1);
            WAGG_READ_A(aAh, aAl, 0);
            split_w8(b00, b01, ew0, wh0, wl0);
            split_w8(b10, b11, ew1, wh1, wl1);
        }
        WAGG_BLOCK(0); WAGG_BLOCK(1); WAGG_BLOCK(2); WAGG_BLOCK(3); WAGG_BLOCK(4); WAGG_BLOCK(5);
        WAGG_BLOCK(6); WAGG_BLOCK(7); WAGG_BLOCK(8); WAGG_BLOCK(9); WAGG_BLOCK(10); WAGG_BLOCK(11);
        WAGG_BLOCK(12); WAGG_BLOCK(13); WAGG_BLOCK(14); WAGG_BLOCK(15); WAGG_BLOCK(16); WAGG_BLOCK(17);
        WAGG_BLOCK(18); WAGG_BLOCK(19); WAGG_BLOCK(20); WAGG_BLOCK(21); WAGG_BLOCK(22);
        static_assert(MT <= 23, "row blocks are written out up to 22");
        __builtin_amdgcn_sched_barrier(0);
        // this wave's DMA pieces of tile+1 have landed; every wave is done reading this buffer
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    // C/D map of the f16 form: col = lane & 15, row = 4 (lane >> 4) + reg (as v_mfma_f32_16x16x4_f32)
    float *slab = slabs + ((((int64_t)mb * n_nt + nt) * S + ks) * (MT * 16)) * D_BN;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                slab[(m * 16 + kq * 4 + r) * D_BN + wave * 32 + cb * 16 + lr] = acc[m][cb][r];
#undef WAGG_DMA_X
#undef WAGG_DMA_W
#undef WAGG_DMA_PIECE
#undef WAGG_DMA_BLOCK
#undef WAGG_MFMA16
#undef WAGG_READ_A
#undef WAGG_BLOCK_
#undef WAGG_BLOCK
}

// row maxima of the transformed X (NaN counts as 0, +-inf is left out): rowmax[t] (zeroed by the caller) as float bits,
// combined with an unsigned atomic max (non-negative floats order like their bits: the same result in any order)
__global__ void dense_rowmax_kernel(const float *__restrict__ X, int64_t ldx, int64_t G, PackXfT<float> xf,
                                    unsigned *__restrict__ rowmax) {
    const int64_t t = blockIdx.y;
    const float *src = X + t * ldx;
    const float *src2 = xf.mode == XF_EDD ? xf.X2 + t * ldx : src;
    bool inf_seen = false;
    float m = 0.0f;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (int64_t)gridDim.x * blockDim.x) {
        const float y = pack_xf<float>(xf, src[g], src2[g], inf_seen);
        const float a = fabsf(y);
        m = a <= FLT_MAX && a > m ? a : m;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __shared__ float wm[16];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fmaxf(m, wm[w]);
        if (m > 0.0f) atomicMax(rowmax + t, __float_as_uint(m));
    }
}

// X (T x G) -> packed split tiles: the slot layout of dense_pack_x_kernel<float>, but piece p < 4 of a row holds the f16
// high parts and piece p + 4 the low parts of k = 32 kt + {4 p + c, 16 + 4 p + c}, c = 0..3, scaled by 2^ex[t].  Same
// transforms, NaN -> 0 (S6), zero rows >= T and cells >= G; +-inf: high part +-inf, low part 0, and the caller is told.
__global__ void dense_pack_x_split_kernel(const float *__restrict__ X, int64_t Tn, int64_t ldx, int64_t G, int n_kt, int bm,
                                          int64_t n_slots, int aligned, const unsigned *__restrict__ rowmax,
                                          f16x8 *__restrict__ Xp, PackXfT<float> xf, int *__restrict__ inf_flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int tile_slots = bm * 8;
    bool inf_seen = false;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n_slots; s += stride) {
        const int slot = (int)(s % tile_slots);
        const int64_t tk = s / tile_slots;
        const int kt = (int)(tk % n_kt);
        const int64_t mb = tk / n_kt;
        const int row = slot >> 3, p = (slot & 7) ^ ((row >> 1) & 7);
        const bool low = p >= 4;
        const int64_t t = mb * bm + row, k0 = (int64_t)kt * 32 + 4 * (p & 3);
        f16x8 o;
#pragma unroll
        for (int c = 0; c < 8; ++c) o[c] = (_Float16)0.0f;
        if (t < Tn) {
            const int ex = split_exp(__uint_as_float(rowmax[t]));
            const float *src = X + t * ldx;
            const float *src2 = xf.mode == XF_EDD ? xf.X2 + t * ldx : src;
            float v[8], h[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) { v[c] = 0.0f; h[c] = 0.0f; }
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int64_t kk = k0 + 16 * half;
                if (aligned && kk + 4 <= G) {
                    const f32x4 a = *reinterpret_cast<const f32x4 *>(src + kk);
                    const f32x4 b = xf.mode == XF_EDD ? *reinterpret_cast<const f32x4 *>(src2 + kk) : a;
#pragma unroll
                    for (int c = 0; c < 4; ++c) { v[4 * half + c] = a[c]; h[4 * half + c] = b[c]; }
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) if (kk + c < G) { v[4 * half + c] = src[kk + c]; h[4 * half + c] = src2[kk + c]; }
                }
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int64_t k = k0 + 16 * (c >> 2) + (c & 3);
                if (k >= G) continue;
                const float y = __builtin_amdgcn_ldexpf(pack_xf<float>(xf, v[c], h[c], inf_seen), ex);
                const _Float16 hi = (_Float16)y;
                o[c] = low ? (__builtin_isinf(y) ? (_Float16)0.0f : (_Float16)(y - (float)hi)) : hi;
            }
        }
        Xp[s] = o;
    }
    if (inf_seen) __hip_atomic_store(inf_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// out[t, r] = 2^-(ex[t] + ew[r]) sum_s slab[mb][nt][s][t_local][c] / den[r]: the scales come off (exactly) before the
// division, the sum is added in the order of dense_reduce_kernel
__global__ void dense_reduce_split_kernel(const float *__restrict__ slabs, int n_nt, int S, int bm, int32_t R,
                                          const float *__restrict__ den, const unsigned *__restrict__ rowmax,
                                          const float *__restrict__ wmax, float *__restrict__ out, int64_t ldo) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t t = blockIdx.y;
    if (r >= R) return;
    const int mb = (int)(t / bm), tl = (int)(t % bm);
    const int nt = (int)(r / D_BN), c = (int)(r % D_BN);
    const float *p = slabs + ((((int64_t)mb * n_nt + nt) * S) * bm + tl) * D_BN + c;
    float s = 0.0f;
    for (int k = 0; k < S; ++k) s += p[(int64_t)k * bm * D_BN];
    const int e = split_exp(__uint_as_float(rowmax[t])) + split_exp(wmax[r]);
    out[t * ldo + r] = __builtin_amdgcn_ldexpf(s, -e) / den[r];
}

// column maxima of a full-form fp32 W (plan time; the grid of dense_colsum_kernel): max |w| per column with +-inf and NaN
// left out, into wmax[n_nt * 256] (zeroed by the caller; float bits, unsigned atomic max -- order-free)
__global__ void dense_colmax_kernel(const f32x4 *__restrict__ Wp, int n_kt, int kt_per_block, unsigned *__restrict__ wmax) {
    const int nt = blockIdx.x;
    const int ktb = blockIdx.y * kt_per_block;
    const int kte = ktb + kt_per_block < n_kt ? ktb + kt_per_block : n_kt;
    for (int slot = threadIdx.x; slot < D_WSLOTS; slot += blockDim.x) {
        float m = 0.0f;
        for (int kt = ktb; kt < kte; ++kt) {
            const f32x4 v = Wp[((int64_t)nt * n_kt + kt) * D_WSLOTS + slot];
#pragma unroll
            for (int c = 0; c < 4; ++c) { const float a = fabsf(v[c]); m = a <= FLT_MAX && a > m ? a : m; }
        }
        // the 8 slots of a column are 8 neighbouring lanes
        m = fmaxf(m, __shfl_xor(m, 1, 64));
        m = fmaxf(m, __shfl_xor(m, 2, 64));
        m = fmaxf(m, __shfl_xor(m, 4, 64));
        if ((slot & 7) == 0 && m > 0.0f) atomicMax(wmax + nt * D_BN + (slot >> 3), __float_as_uint(m));
    }
}
