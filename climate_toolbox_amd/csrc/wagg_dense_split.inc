// Split form of the full-form fp32 contraction (included by wagg_dense.hip): the same work items, packed tile images,
// swizzle and fragment offsets as dense_mfma_kernel<float, 0, false, MT>, but the products run on the f16 matrix pipe
// (and the pipeline is its own, see dense_split_kernel).  Each operand is an f16 high part plus an f16 low part of a
// power-of-two scaled copy:
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

// four fp32 W values of piece kq and four of piece kq + 4 -> scaled f16 high and low parts, in k order, a pair of values
// at a time: v = w 2^e, h = f16(v) (one v_cvt_pk_f16_f32 a pair), l = f16(v - (float)h).  v - (float)h is exact in fp32
// (h is v rounded to eleven bits), and so is (float)h x -1, so one fused multiply-add that reads the f16 half and rounds its
// fp32 result to f16 gives the bits of conversion back, subtraction and conversion: v_fma_mixlo_f16 / v_fma_mixhi_f16,
// two instructions a pair where the plain form takes five (the whole split is 40 vector instructions a tile and wave where
// the plain form compiled to 62).  The compiler folds the multiplier -1 into a subtraction again (or packs the pair into
// v_pk_fma_f32), so the two are written out; the closing s_nop covers the matrix instruction that reads the result next.
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void split_w8(f32x4 a, f32x4 b, int e, f16x8 &hi, f16x8 &lo) {
    u32x4 H, L;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const float v0 = __builtin_amdgcn_ldexpf(p < 2 ? a[2 * p] : b[2 * p - 4], e);
        const float v1 = __builtin_amdgcn_ldexpf(p < 2 ? a[2 * p + 1] : b[2 * p - 3], e);
        const unsigned h = __builtin_bit_cast(unsigned, f16x2{(_Float16)v0, (_Float16)v1});
        unsigned l;
        asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]\n\t"
            "v_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
            "s_nop 1"
            : "=&v"(l) : "v"(h), "v"(v0), "v"(v1));
        H[p] = h;
        L[p] = l;
    }
    hi = __builtin_bit_cast(f16x8, H);
    lo = __builtin_bit_cast(f16x8, L);
}

// Pipeline (the fp32 kernel's double buffer left the f16 tile -- 3 x 16 cycles a row-block column -- about half a tile for
// its DMA to land, a vmcnt(0) drain and a barrier every tile):
//   * W goes straight to registers: lane (lr, kq) of wave w needs exactly the four 16-byte pieces b00 b01 b10 b11 of rows
//     32 w + lr (+ 16) of the packed W tile, so it loads them with buffer_load_dwordx4 (the packed layout is the LDS image:
//     the same offsets).  The loads of tile t + 1 are issued right after tile t's pieces have been split, into the same
//     registers, and have a whole tile to land.
//   * LDS holds X tiles only, in a ring of three: the DMA pieces of tile t + 2 are issued inside tile t, into the buffer
//     that tile t - 1 read (every wave passed the barrier behind it).  At the end of tile t a wave waits for its pieces of
//     tile t + 1 only -- vmcnt(4 + NXP) leaves the W loads of t + 1 and the pieces of t + 2 in flight (vector-memory loads,
//     LDS-DMA included, retire in issue order) -- and the workgroup takes its one barrier.
//   * Every wave issues the same number of vector-memory ops on every path (a wave without an i-th X piece fetches piece
//     (wave + 8 i) mod XPIECES again: the same bytes to the same place, never read before the barrier), so the compiler's
//     own wait before the split counts exactly: vmcnt(NXP), the pieces of t + 2 stay in flight.
//   * The split of column block 1's W operands runs between the first six MFMAs (row blocks 0 and 1, column block 0).
// Per accumulator the three MFMAs keep their order (xh.wl, xl.wh, xh.wh) and k order: the result is the double-buffered
// kernel's, bit for bit.
//
// DBG is a diagnostic knob (WAGG_SPLIT_DBG env, read by the -DWAGG_DIAG build only; tools/split_ablate.sh): bit0 = no W loads
// and no X DMA in the k-loop, bit2 = no per-tile wait or barrier, bit3 = no split arithmetic (the raw register pairs go to
// the MFMAs as they are: same loads, same waits).  Results are wrong with any bit set.
//
// IMG: Wp is the plan's f16 image of W (dense_split_image_kernel below): the tile layout of the packed fp32 W, but the four
// 16-byte slots a lane loads hold wh0, wl0, wh1, wl1 -- the bits split_w8 makes of them -- so the loaded registers ARE the
// operands and the split (and the column scales) leave the k-loop.  The operands are then live for the whole tile while
// the loads of tile t + 1 are in flight, so the loads go into a second set of four registers and the tile loop is written
// out twice with the sets exchanged (no copies).  Same loads at the same place, same waits, same MFMA order: the result is
// that of the IMG = false kernel, bit for bit.

// buffer descriptor of `bytes` bytes at a wave-uniform address (read back from lane 0, so that the compiler keeps the
// descriptor in SGPRs instead of looping over the lanes' copies)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t split_tile_rsrc(const char *base, int bytes) {
    const uint64_t a = reinterpret_cast<uint64_t>(base);
    // (readfirstlane returns int: each half goes through uint32_t, or bit 31 of the low half would spread into the high one)
    const uint64_t u = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((unsigned)a) |
                       (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((unsigned)(a >> 32)) << 32;
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(u), (short)0, bytes, 0x00020000);
}

// byte offsets of lane (lr, kq)'s two fragments inside a 2-KiB block of sixteen tile rows
__device__ __forceinline__ unsigned split_frag0(int lr, int kq) { return (lr * 8 + (kq ^ (lr >> 1))) * 16; }        // piece kq
__device__ __forceinline__ unsigned split_frag1(int lr, int kq) { return (lr * 8 + ((kq ^ (lr >> 1)) ^ 4)) * 16; }  // piece kq + 4

template <int MT, int DBG = 0, bool IMG = false>
__global__ __launch_bounds__(D_THREADS, 2) void dense_split_kernel(
    const f16x8 *__restrict__ Xp, const float *__restrict__ Wp, const float *__restrict__ wmax, int n_kt, int n_nt, int n_mb,
    int S, int kt_per_slice, float *__restrict__ slabs) {
    static_assert(MT <= D_MT, "accumulators of MT row blocks must fit the register file");
    extern __shared__ __attribute__((aligned(16))) char lds[];   // [3][XT4]
    constexpr int XT4 = d_xt_bytes(MT);
    constexpr int XPIECES = XT4 / 1024;
    constexpr int NXP = (XPIECES + 7) / 8;                // X pieces per wave and tile
    static_assert(NXP <= 6, "at most six X pieces per wave");
    // the end-of-tile wait: this wave's pieces of tile t + 1 have landed; W of t + 1 (4) and X of t + 2 (NXP) may not have
    constexpr int VM_KEEP = 4 + NXP;
    constexpr int WAIT_TILE = (VM_KEEP & 15) | (7 << 4) | (0 << 8) | ((VM_KEEP >> 4) << 14);   // vmcnt(VM_KEEP) lgkmcnt(0)

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
    // scales of this lane's two columns (the plan pads wmax to whole column tiles with zeros); the image holds scaled parts
    const int ew0 = IMG ? 0 : split_exp(wmax[nt * D_BN + wave * 32 + lr]);
    const int ew1 = IMG ? 0 : split_exp(wmax[nt * D_BN + wave * 32 + 16 + lr]);

    const unsigned frag0 = split_frag0(lr, kq);            // piece kq: W k = 4 kq + c, X high parts
    const unsigned frag1 = split_frag1(lr, kq);            // piece kq + 4: W k = 16 + 4 kq + c, X low parts
    // buffer descriptors of one tile (wave-uniform: the tile's X image, the tile's W image) and 32-bit per-lane offsets; the
    // range check holds every W load (and the lane part of every X piece) inside its tile
    const char *xslice = reinterpret_cast<const char *>(Xp) + ((int64_t)mb * n_kt + kt0) * XT4;
    const char *wslice = reinterpret_cast<const char *>(Wp) + w_first * D_WTB;
    const unsigned lane16 = lane * 16;
    const unsigned wfrag0 = wave * 4096 + frag0, wfrag1 = wave * 4096 + frag1;   // this wave's rows 32 w ... 32 w + 31
#define WAGG_RSRC(base, bytes) split_tile_rsrc(base, bytes)
#define WAGG_DMA_X(i, xr, buf)                                                                    \
    do {                                                                                          \
        constexpr int i_ = (i);                                                                   \
        const int q_ = (wave + 8 * i_) % XPIECES;                                                 \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lptr_t)(lds + (buf) * XT4 + q_ * 1024), 16, lane16, q_ * 1024, 0, 0); \
    } while (0)
#define WAGG_DMA_XALL(tile, buf)                                                                  \
    do {                                                                                          \
        const auto xr_ = WAGG_RSRC(xslice + (int64_t)(tile) * XT4, XT4);                          \
        WAGG_DMA_X(0, xr_, buf);                                                                  \
        if constexpr (NXP > 1) WAGG_DMA_X(NXP > 1 ? 1 : 0, xr_, buf);                             \
        if constexpr (NXP > 2) WAGG_DMA_X(NXP > 2 ? 2 : 0, xr_, buf);                             \
        if constexpr (NXP > 3) WAGG_DMA_X(NXP > 3 ? 3 : 0, xr_, buf);                             \
        if constexpr (NXP > 4) WAGG_DMA_X(NXP > 4 ? 4 : 0, xr_, buf);                             \
        if constexpr (NXP > 5) WAGG_DMA_X(NXP > 5 ? 5 : 0, xr_, buf);                             \
    } while (0)
#define WAGG_LOAD_W(tile, D00, D01, D10, D11)                                                     \
    do {                                                                                          \
        const auto wr_ = WAGG_RSRC(wslice + (int64_t)(tile) * D_WTB, D_WTB);                      \
        D00 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wr_, wfrag0, 0, 0));        \
        D01 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wr_, wfrag1, 0, 0));        \
        D10 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wr_, wfrag0 + 2048, 0, 0)); \
        D11 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wr_, wfrag1 + 2048, 0, 0)); \
    } while (0)

    f32x4 acc[MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m][0] = acc[m][1] = f32x4{0, 0, 0, 0};

    f32x4 b00, b01, b10, b11;
    if (ntiles > 0) {
        const int t1 = ntiles > 1 ? 1 : 0;
        WAGG_LOAD_W(0, b00, b01, b10, b11);
        WAGG_DMA_XALL(0, 0);
        WAGG_DMA_XALL(t1, 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    // DBG bit3: no split arithmetic, the raw register pairs go to the MFMAs as they are (same loads, same waits); IMG: the
    // registers hold the parts already
#define WAGG_SPLIT(A, B, E, HI, LO)                                                               \
    do {                                                                                          \
        if constexpr (IMG || (DBG & 8)) { HI = __builtin_bit_cast(f16x8, A); LO = __builtin_bit_cast(f16x8, B); } \
        else split_w8(A, B, E, HI, LO);                                                           \
    } while (0)
#define WAGG_MFMA16(RB, CB, A, B) acc[RB][CB] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A, B, acc[RB][CB], 0, 0, 0)
#define WAGG_READ_A(H, L, RB)                                                                     \
    do {                                                                                          \
        H = *reinterpret_cast<const f16x8 *>(img + frag0 + (RB) * 2048);                          \
        L = *reinterpret_cast<const f16x8 *>(img + frag1 + (RB) * 2048);                          \
    } while (0)
    // X piece i of tile t + 2 goes behind row block xdma_block(i): spread over the tile, none in the first two blocks
    constexpr auto xdma_block = [](int i) { return MT <= 2 ? MT - 1 : 2 + i * (MT - 2) / NXP; };
#define WAGG_DMA_AT(RB, i)                                                                        \
    do {                                                                                          \
        if constexpr (!(DBG & 1) && (i) < NXP && xdma_block(i) == (RB)) WAGG_DMA_X((i) < NXP ? (i) : 0, xfar, bfar); \
    } while (0)
#define WAGG_DMA_BLOCK(RB)                                                                        \
    do {                                                                                          \
        WAGG_DMA_AT(RB, 0); WAGG_DMA_AT(RB, 1); WAGG_DMA_AT(RB, 2);                               \
        WAGG_DMA_AT(RB, 3); WAGG_DMA_AT(RB, 4); WAGG_DMA_AT(RB, 5);                               \
    } while (0)
    // Row block RB >= 2: six MFMAs, cross terms first, xh.wh last (the largest term is added to the smallest partial sums
    // last); the next block's fragment reads go right behind the first MFMA, this block's X pieces behind the last
#define WAGG_BLOCK_(RB, H, L, NH, NL)                                                             \
    do {                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        WAGG_MFMA16(RB, 0, H, wl0);                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        if constexpr ((RB) + 1 < MT) WAGG_READ_A(NH, NL, (RB) + 1 < MT ? (RB) + 1 : 0);           \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        WAGG_MFMA16(RB, 1, H, wl1);                                                               \
        WAGG_MFMA16(RB, 0, L, wh0);                                                               \
        WAGG_MFMA16(RB, 1, L, wh1);                                                               \
        WAGG_MFMA16(RB, 0, H, wh0);                                                               \
        WAGG_MFMA16(RB, 1, H, wh1);                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        WAGG_DMA_BLOCK(RB);                                                                       \
    } while (0)
#define WAGG_BLOCK(RB)                                                                            \
    do {                                                                                          \
        if constexpr ((RB) < MT) {                                                                \
            constexpr int rb_ = (RB) < MT ? (RB) : 0;                                             \
            if constexpr ((RB) & 1) WAGG_BLOCK_(rb_, aBh, aBl, aAh, aAl);                         \
            else WAGG_BLOCK_(rb_, aAh, aAl, aBh, aBl);                                            \
        }                                                                                         \
    } while (0)

    // One tile: C00 C01 C10 C11 hold its W pieces (IMG: its operands), N00 ... N11 take those of tile t + 1 (IMG = false: the
    // same registers, free once the pieces have been split)
#define WAGG_TILE(tile, C00, C01, C10, C11, N00, N01, N10, N11)                                                               \
    do {                                                                                                                      \
        const char *img = lds + bcur * XT4;                                                                                   \
        const int bfar = bcur == 0 ? 2 : bcur - 1; /* buffer of tile t + 2 (read by tile t - 1) */                            \
        const int tnext = (tile) + 1 < ntiles ? (tile) + 1 : ntiles - 1; /* last tiles: harmless re-loads inside the slice */ \
        const int tfar = (tile) + 2 < ntiles ? (tile) + 2 : ntiles - 1;                                                       \
        const auto xfar = WAGG_RSRC(xslice + (int64_t)tfar * XT4, XT4);                                                       \
        f16x8 wh0, wl0, wh1, wl1, aAh, aAl, aBh, aBl;                                                                         \
        /* row blocks 0 and 1, column block 0, with column block 1's split between the MFMAs; then W of tile t + 1 */         \
        WAGG_READ_A(aAh, aAl, 0);                                                                                             \
        WAGG_SPLIT(C00, C01, ew0, wh0, wl0);                                                                                  \
        if constexpr (MT > 1) WAGG_READ_A(aBh, aBl, MT > 1 ? 1 : 0);                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                                                    \
        WAGG_MFMA16(0, 0, aAh, wl0);                                                                                          \
        WAGG_MFMA16(0, 0, aAl, wh0);                                                                                          \
        WAGG_MFMA16(0, 0, aAh, wh0);                                                                                          \
        if constexpr (MT > 1) {                                                                                               \
            WAGG_MFMA16(MT > 1 ? 1 : 0, 0, aBh, wl0);                                                                         \
            WAGG_MFMA16(MT > 1 ? 1 : 0, 0, aBl, wh0);                                                                         \
            WAGG_MFMA16(MT > 1 ? 1 : 0, 0, aBh, wh0);                                                                         \
        }                                                                                                                     \
        WAGG_SPLIT(C10, C11, ew1, wh1, wl1);                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                                    \
        if constexpr (!(DBG & 1)) WAGG_LOAD_W(tnext, N00, N01, N10, N11);                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                                    \
        WAGG_MFMA16(0, 1, aAh, wl1);                                                                                          \
        WAGG_MFMA16(0, 1, aAl, wh1);                                                                                          \
        WAGG_MFMA16(0, 1, aAh, wh1);                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                                                    \
        if constexpr (MT > 2) WAGG_READ_A(aAh, aAl, MT > 2 ? 2 : 0);                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                                                    \
        if constexpr (MT > 1) {                                                                                               \
            WAGG_MFMA16(MT > 1 ? 1 : 0, 1, aBh, wl1);                                                                         \
            WAGG_MFMA16(MT > 1 ? 1 : 0, 1, aBl, wh1);                                                                         \
            WAGG_MFMA16(MT > 1 ? 1 : 0, 1, aBh, wh1);                                                                         \
        }                                                                                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                                    \
        WAGG_DMA_BLOCK(0); WAGG_DMA_BLOCK(1);                                                                                 \
        WAGG_BLOCK(2); WAGG_BLOCK(3); WAGG_BLOCK(4); WAGG_BLOCK(5);                                                           \
        WAGG_BLOCK(6); WAGG_BLOCK(7); WAGG_BLOCK(8); WAGG_BLOCK(9); WAGG_BLOCK(10); WAGG_BLOCK(11);                           \
        WAGG_BLOCK(12); WAGG_BLOCK(13); WAGG_BLOCK(14); WAGG_BLOCK(15); WAGG_BLOCK(16); WAGG_BLOCK(17);                       \
        WAGG_BLOCK(18); WAGG_BLOCK(19); WAGG_BLOCK(20); WAGG_BLOCK(21); WAGG_BLOCK(22);                                       \
        static_assert(MT <= 23, "row blocks are written out up to 22");                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                                    \
        if constexpr (!(DBG & 4)) {                                                                                           \
            __builtin_amdgcn_s_waitcnt(WAIT_TILE);                                                                            \
            __builtin_amdgcn_s_barrier();                                                                                     \
        }                                                                                                                     \
        bcur = bcur == 2 ? 0 : bcur + 1;                                                                                      \
    } while (0)
    int bcur = 0;                                              // ring buffer of tile t
    if constexpr (IMG) {
        f32x4 d00, d01, d10, d11;                                 // the second operand set
        for (int tile = 0; tile < ntiles; tile += 2) {
            WAGG_TILE(tile, b00, b01, b10, b11, d00, d01, d10, d11);
            if (tile + 1 < ntiles) WAGG_TILE(tile + 1, d00, d01, d10, d11, b00, b01, b10, b11);
        }
    } else {
        for (int tile = 0; tile < ntiles; ++tile) WAGG_TILE(tile, b00, b01, b10, b11, b00, b01, b10, b11);
    }
    // the re-loads behind the last tile land before the wave ends
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // C/D map of the f16 form: col = lane & 15, row = 4 (lane >> 4) + reg (as v_mfma_f32_16x16x4_f32)
    float *slab = slabs + ((((int64_t)mb * n_nt + nt) * S + ks) * (MT * 16)) * D_BN;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                slab[(m * 16 + kq * 4 + r) * D_BN + wave * 32 + cb * 16 + lr] = acc[m][cb][r];
#undef WAGG_RSRC
#undef WAGG_DMA_X
#undef WAGG_DMA_XALL
#undef WAGG_LOAD_W
#undef WAGG_DMA_AT
#undef WAGG_DMA_BLOCK
#undef WAGG_SPLIT
#undef WAGG_MFMA16
#undef WAGG_READ_A
#undef WAGG_BLOCK_
#undef WAGG_BLOCK
#undef WAGG_TILE
}

// The f16 image of a packed fp32 W (plan time; what dense_split_kernel<MT, DBG, true> loads): a workgroup takes a tile as
// the split kernel's does -- lane (lr, kq) of wave w reads its four pieces at the kernel's offsets, splits them with
// split_w8 at the scales of its two columns and stores wh0, wl0, wh1, wl1 at the same four offsets of the image tile.  The
// eight waves' offsets cover every 16-byte slot of a tile once.
__global__ __launch_bounds__(D_THREADS) void dense_split_image_kernel(const float *__restrict__ Wp, const float *__restrict__ wmax,
                                                                      int n_kt, int64_t n_tiles, float *__restrict__ image) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, kq = lane >> 4;
    const unsigned wfrag0 = wave * 4096 + split_frag0(lr, kq), wfrag1 = wave * 4096 + split_frag1(lr, kq);
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t nt = t / n_kt;
        const int ew0 = split_exp(wmax[nt * D_BN + wave * 32 + lr]);
        const int ew1 = split_exp(wmax[nt * D_BN + wave * 32 + 16 + lr]);
        const char *src = reinterpret_cast<const char *>(Wp) + t * D_WTB;
        char *dst = reinterpret_cast<char *>(image) + t * D_WTB;
        const f32x4 b00 = *reinterpret_cast<const f32x4 *>(src + wfrag0), b01 = *reinterpret_cast<const f32x4 *>(src + wfrag1);
        const f32x4 b10 = *reinterpret_cast<const f32x4 *>(src + wfrag0 + 2048), b11 = *reinterpret_cast<const f32x4 *>(src + wfrag1 + 2048);
        f16x8 wh0, wl0, wh1, wl1;
        split_w8(b00, b01, ew0, wh0, wl0);
        split_w8(b10, b11, ew1, wh1, wl1);
        *reinterpret_cast<f16x8 *>(dst + wfrag0) = wh0;
        *reinterpret_cast<f16x8 *>(dst + wfrag1) = wl0;
        *reinterpret_cast<f16x8 *>(dst + wfrag0 + 2048) = wh1;
        *reinterpret_cast<f16x8 *>(dst + wfrag1 + 2048) = wl1;
    }
}

// Row maxima of the transformed X (NaN counts as 0, +-inf is left out), in two steps without a buffer to clear: a row is cut
// into SPLIT_NS strips of whole 4-cell quads (the last one takes the G % 4 cells behind them), workgroup (j, t) writes the
// maximum of strip j of row t -- 0 for a strip without cells -- as float bits into part[t][j], and the pack kernel below
// takes the maximum of a row's SPLIT_NS words.  Every word is written on every apply, and the maximum of non-negative floats
// is the same in any order.  aligned: X (and the EDD second field) and ldx are multiples of 16 bytes, the quads are loaded whole.
constexpr int SPLIT_NS = 64;
constexpr int SPLIT_PREP_THREADS = 256;
__global__ __launch_bounds__(SPLIT_PREP_THREADS) void dense_rowmax_kernel(const float *__restrict__ X, int64_t ldx, int64_t G, int aligned,
                                                                          PackXfT<float> xf, unsigned *__restrict__ part) {
    const int64_t t = blockIdx.y;
    const float *src = X + t * ldx;
    const float *src2 = xf.mode == XF_EDD ? xf.X2 + t * ldx : src;
    const bool edd = xf.mode == XF_EDD;
    const int64_t nq = (G + 3) >> 2, per = (nq + SPLIT_NS - 1) / SPLIT_NS;
    const int64_t q0 = (int64_t)blockIdx.x * per < nq ? (int64_t)blockIdx.x * per : nq;
    const int64_t q1 = q0 + per < nq ? q0 + per : nq;
    bool inf_seen = false;
    float m = 0.0f;
    auto take = [&](float x, float x2) {
        const float a = fabsf(pack_xf<float>(xf, x, x2, inf_seen));
        m = a <= FLT_MAX && a > m ? a : m;
    };
    if (aligned) {
        const int64_t qf = q1 < (G >> 2) ? q1 : (G >> 2);          // the quads that lie inside the row as a whole
        const f32x4 *s4 = reinterpret_cast<const f32x4 *>(src), *s42 = reinterpret_cast<const f32x4 *>(src2);
        int64_t q = q0 + threadIdx.x;
        for (; q + 3 * SPLIT_PREP_THREADS < qf; q += 4 * SPLIT_PREP_THREADS) {   // four loads (EDD: eight) in flight
            f32x4 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = s4[q + i * SPLIT_PREP_THREADS];
#pragma unroll
            for (int i = 0; i < 4; ++i) b[i] = edd ? s42[q + i * SPLIT_PREP_THREADS] : a[i];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 4; ++c) take(a[i][c], b[i][c]);
        }
        for (; q < qf; q += SPLIT_PREP_THREADS) {
            const f32x4 a = s4[q];
            const f32x4 b = edd ? s42[q] : a;
#pragma unroll
            for (int c = 0; c < 4; ++c) take(a[c], b[c]);
        }
        if (q0 <= qf && qf < q1 && threadIdx.x == 0)                // this strip ends in the ragged quad: the last G % 4 cells
            for (int64_t g = 4 * qf; g < G; ++g) take(src[g], src2[g]);
    } else {
        const int64_t g1 = 4 * q1 < G ? 4 * q1 : G;
        for (int64_t g = 4 * q0 + threadIdx.x; g < g1; g += SPLIT_PREP_THREADS) take(src[g], src2[g]);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __shared__ float wm[SPLIT_PREP_THREADS / 64];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SPLIT_PREP_THREADS / 64; ++w) m = fmaxf(m, wm[w]);
        part[t * SPLIT_NS + blockIdx.x] = __float_as_uint(m);
    }
}

// X (T x G) -> packed split tiles: the slot layout of dense_pack_x_kernel<float>, but piece p < 4 of a row holds the f16
// high parts and piece p + 4 the low parts of k = 32 kt + {4 p + c, 16 + 4 p + c}, c = 0..3, scaled by 2^ex[t].  Same
// transforms, NaN -> 0 (S6), zero rows >= T and cells >= G; +-inf: high part +-inf, low part 0, and the caller is told.
//
// Workgroup (m, mb, cb) of a grid (MT, n_mb, n_cb) keeps the sixteen rows of row block mb's 16-row group m and walks the k tiles
// 4 (cb + i n_cb) + wave, i = 0, 1, ...: no division anywhere.  It first takes the rows' maxima from the SPLIT_NS partial words
// of dense_rowmax_kernel (sixteen lanes a row, one 16-byte load each) -- and, as the workgroup that owns the rows' first slots
// (cb = 0), writes them to rowmax[t] for the reduce kernel.  Lane (lr, p) of a wave then owns the pair of pieces p and p + 4 of
// row 16 m + lr: it loads the row's cells 4 p + c and 16 + 4 p + c once, transforms and scales each value once and stores the
// high parts at slot p ^ swz and the low parts at slot (p + 4) ^ swz = (p ^ swz) ^ 4 of the row, swz = (row >> 1) & 7 (the
// swizzle of the tile image).  A wave reads 128 bytes of each of sixteen rows and its two stores cover the sixteen 128-byte tile
// rows whole: 2 KiB of the image, end to end.
__global__ __launch_bounds__(SPLIT_PREP_THREADS) void dense_pack_x_split_kernel(
    const float *__restrict__ X, int64_t Tn, int64_t ldx, int64_t G, int n_kt, int aligned, const unsigned *__restrict__ part,
    unsigned *__restrict__ rowmax, f16x8 *__restrict__ Xp, PackXfT<float> xf, int *__restrict__ inf_flag) {
    const int m = blockIdx.x, cb = blockIdx.z, n_cb = gridDim.z, bm = (int)gridDim.x * 16;
    const int64_t mb = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __shared__ int ex_s[16];
    {
        const int r = threadIdx.x >> 4, q = threadIdx.x & 15;
        const int64_t t = mb * bm + m * 16 + r;
        unsigned mx = 0;                                           // (non-negative floats order like their bits)
        if (t < Tn) {
            const u32x4 v = *reinterpret_cast<const u32x4 *>(part + t * SPLIT_NS + 4 * q);
            mx = max(max(v[0], v[1]), max(v[2], v[3]));
        }
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o, 64));
        if (q == 0) {
            ex_s[r] = split_exp(__uint_as_float(mx));
            if (cb == 0 && t < Tn) rowmax[t] = mx;
        }
    }
    __syncthreads();
    const int lr = lane >> 2, p = lane & 3;
    const int row = m * 16 + lr;
    const int64_t t = mb * bm + row;
    const int ex = ex_s[lr];
    const int s_hi = p ^ ((lr >> 1) & 7), s_lo = s_hi ^ 4;         // (row >> 1) & 7 = (lr >> 1) & 7: row = 16 m + lr
    const float *src = X + (t < Tn ? t : 0) * ldx;
    const float *src2 = xf.mode == XF_EDD ? xf.X2 + (t < Tn ? t : 0) * ldx : src;
    f16x8 *dst = Xp + (mb * n_kt * bm + row) * 8;                 // the row's eight slots in k tile 0 of row block mb
    bool inf_seen = false;
    for (int kt = 4 * cb + wave; kt < n_kt; kt += 4 * n_cb) {
        const int64_t k0 = (int64_t)kt * 32 + 4 * p;
        f16x8 hi, lo;
#pragma unroll
        for (int c = 0; c < 8; ++c) hi[c] = lo[c] = (_Float16)0.0f;
        if (t < Tn) {
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
                hi[c] = (_Float16)y;
                lo[c] = __builtin_isinf(y) ? (_Float16)0.0f : (_Float16)(y - (float)hi[c]);
            }
        }
        f16x8 *o = dst + (int64_t)kt * bm * 8;
        o[s_hi] = hi;
        o[s_lo] = lo;
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
