
constexpr int kWaves = 8;                 // waves per workgroup
constexpr int kThreads = kWaves * 64;     // 512
constexpr int kLdsWords = PRV_LDS_WORDS;  // 16384 words = 64 KiB
constexpr int kSetB = 128;                // byte offset of set B inside an LDS row
constexpr int kFoldSets = 7;              // G = 1,2,4,...,64

__shared__ __attribute__((aligned(16))) uint32_t s_tab[kLdsWords];

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------
struct LaneConst {
    uint32_t c;                  // byte i = 16k + 4t_i  (LDS column of instruction i)
    uint32_t s0, s1, s2, s3;     // v_perm selectors of instruction i
};

__device__ __forceinline__ LaneConst lane_const(int lane)
{
    LaneConst L;
    const uint32_t k = (lane >> 2) & 7;
    uint32_t c = 0, s[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t t = (i + lane) & 3;
        c |= (16u * k + 4u * t) << (8 * i);
        // result byte0 <- c byte i (S1 bytes 0-3), byte1 <- x byte t (S0 bytes
        // 4-7), bytes 2,3 <- 0x00 (selector 0x0c)
        s[i] = 0x0c0c0000u | ((4u + t) << 8) | (uint32_t)i;
    }
    L.c = c;
    L.s0 = s[0];
    L.s1 = s[1];
    L.s2 = s[2];
    L.s3 = s[3];
    return L;
}

template <int SETOFF>
__device__ __forceinline__ void zlookup(uint32_t x, const LaneConst &L, uint32_t &r0, uint32_t &r1, uint32_t &r2,
                                        uint32_t &r3)
{
    const uint32_t a0 = __builtin_amdgcn_perm(x, L.c, L.s0);
    const uint32_t a1 = __builtin_amdgcn_perm(x, L.c, L.s1);
    const uint32_t a2 = __builtin_amdgcn_perm(x, L.c, L.s2);
    const uint32_t a3 = __builtin_amdgcn_perm(x, L.c, L.s3);
    const char *t = reinterpret_cast<const char *>(s_tab) + SETOFF;
    r0 = *reinterpret_cast<const uint32_t *>(t + a0);
    r1 = *reinterpret_cast<const uint32_t *>(t + a1);
    r2 = *reinterpret_cast<const uint32_t *>(t + a2);
    r3 = *reinterpret_cast<const uint32_t *>(t + a3);
}

// x -> Z(x) through the four byte tables of set SETOFF
template <int SETOFF>
__device__ __forceinline__ uint32_t zstep(uint32_t x, const LaneConst &L)
{
    uint32_t r0, r1, r2, r3;
    zlookup<SETOFF>(x, L, r0, r1, r2, r3);
    return r0 ^ r1 ^ r2 ^ r3;
}

// x -> Z(x) ^ w with two 3-input XORs (v_bitop3_b32 0x96)
template <int SETOFF>
__device__ __forceinline__ uint32_t zstep_xor(uint32_t x, uint32_t w, const LaneConst &L)
{
    uint32_t r0, r1, r2, r3;
    zlookup<SETOFF>(x, L, r0, r1, r2, r3);
    return __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_bitop3_b32(r0, r1, r2, 0x96), r3, w, 0x96);
}

// one 16-byte piece; LAST = this piece ends the lane's part of the block.
// FUSE3: merge the lookup XORs with the next data word in v_bitop3 (6 VALU
// per word instead of 8).
template <bool LAST, bool FUSE3 = false>
__device__ __forceinline__ uint32_t piece(uint32_t u, const v4u &d, const LaneConst &L)
{
    if (FUSE3) {
        uint32_t x = u ^ d.x;
        x = zstep_xor<0>(x, d.y, L);
        x = zstep_xor<0>(x, d.z, L);
        x = zstep_xor<0>(x, d.w, L);
        return LAST ? zstep<0>(x, L) : zstep<kSetB>(x, L);
    }
    u = zstep<0>(u ^ d.x, L);
    u = zstep<0>(u ^ d.y, L);
    u = zstep<0>(u ^ d.z, L);
    return LAST ? zstep<0>(u ^ d.w, L) : zstep<kSetB>(u ^ d.w, L);
}

// v -> sum_i bit_i(v) * col[i]   (per-lane GF(2) matrix-vector).
// Per bit one v_bfe_i32 (bit -> 0 / ~0 mask) and one v_bitop3 computing
// f ^ (mask & col) (truth table 0x78 = S0 ^ (S1 & S2)); four independent
// accumulators keep the XOR chain 8 deep instead of 32.
__device__ __forceinline__ uint32_t bitmat(uint32_t v, const uint32_t (&col)[32])
{
    uint32_t f[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 32; i++) {
        const uint32_t m = (uint32_t)(((int32_t)(v << (31 - i))) >> 31);
        f[i & 3] = __builtin_amdgcn_bitop3_b32(f[i & 3], m, col[i], 0x78);
    }
    return __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_bitop3_b32(f[0], f[1], f[2], 0x96), f[3], 0u, 0x96);
}

// one 16-byte piece that ENDS a block, stopping before the last table step:
// returns x = register ^ last word, so that the caller's fold applies
// Z_(4 + fold distance) to x in one go (nib_fold)
template <bool FUSE3 = false>
__device__ __forceinline__ uint32_t piece_pre(uint32_t u, const v4u &d, const LaneConst &L)
{
    if (FUSE3) {
        uint32_t x = u ^ d.x;
        x = zstep_xor<0>(x, d.y, L);
        x = zstep_xor<0>(x, d.z, L);
        return zstep_xor<0>(x, d.w, L);
    }
    u = zstep<0>(u ^ d.x, L);
    u = zstep<0>(u ^ d.y, L);
    u = zstep<0>(u ^ d.z, L);
    return u ^ d.w;
}

// Nibble-table fold.  Lane column c of a G-lane block must advance its
// pre-step register x by Z_(4 + 16(G-1-c)) (the block's last table step plus
// the distance to the block end).  That map is linear, so it is the XOR of 8
// lookups, one per nibble n of x, in per-slot tables of width TW (a multiple
// of G; slot s holds column c = s % G)
//     T[n][v][s] = Z_(4 + 16(G-1-s%G))(v << 4n)    (word (16n + v)·TW + s)
// 8·16·TW words (16 KiB at TW = 32).  With TW = 32 (G <= 32) or 64 and slot
// s = lane % TW, the 32 lanes of a ds_read half sit in 32 distinct banks, so
// every lookup is conflict-free whatever G.  8 LDS reads + 20 VALU, against
// 4 LDS reads + 8 VALU (last step) plus 64 VALU (bitmat) for the column fold.
__shared__ __attribute__((aligned(16))) uint32_t s_nib16[8 * 16 * 16];
__shared__ __attribute__((aligned(16))) uint32_t s_nib32[8 * 16 * 32];
__shared__ __attribute__((aligned(16))) uint32_t s_nib64[8 * 16 * 64];

template <int TW>
__device__ __forceinline__ uint32_t *nib_tab()
{
    static_assert(TW == 16 || TW == 32 || TW == 64, "nibble table width");
    if constexpr (TW == 64)
        return s_nib64;
    else if constexpr (TW == 32)
        return s_nib32;
    else
        return s_nib16;
}

// table width of the rows / small kernels for G lanes per block
template <int G>
constexpr int nib_width() { return G > 32 ? G : 32; }

// nq 16-B pieces of src to dst (LDS, 16-B aligned: the DMA targets are
// declared aligned(16)) by the workgroup.  With
// PRISKV_TABLE_DMA, straight to LDS (global_load_lds_dwordx4: lane l of a
// wave writes 16 B at the wave's LDS base + 16 l; no VGPR staging and no
// ds_write); the caller's __syncthreads waits for them (vmcnt 0).  Every
// wave's trip count is uniform: nq and blockDim.x are multiples of 64.
#ifndef PRISKV_TABLE_DMA
#define PRISKV_TABLE_DMA 1
#endif
// before the barrier that publishes tables copied by copy_to_lds: the DMA
// writes land with vmcnt, which a workgroup barrier need not wait for
__device__ __forceinline__ void lds_dma_landed()
{
#if PRISKV_TABLE_DMA
    __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt 0
#endif
}

__device__ __forceinline__ void copy_to_lds(const uint32_t *__restrict__ src, uint32_t *dst, int nq)
{
#if PRISKV_TABLE_DMA
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < nq; i += blockDim.x)
        __builtin_amdgcn_global_load_lds(src + 4 * i, dst + 4 * (i - lane), 16, 0, 0);
#else
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
    for (int i = threadIdx.x; i < nq; i += blockDim.x)
        d4[i] = s4[i];
#endif
}

template <int TW>
__device__ __forceinline__ void load_nib_image(const uint32_t *__restrict__ img)
{
    copy_to_lds(img, nib_tab<TW>(), 8 * 16 * TW / 4);
}

// cb = 4·s: the lane's byte offset inside one table row (s = lane % TW)
template <int TW>
__device__ __forceinline__ uint32_t nib_fold(uint32_t x, uint32_t cb)
{
    const char *t = reinterpret_cast<const char *>(nib_tab<TW>());
    uint32_t r[8];
#pragma unroll
    for (int n = 0; n < 8; n++) {
        const uint32_t a = ((x >> (4 * n)) & 15u) * (4u * TW) + cb;
        r[n] = *reinterpret_cast<const uint32_t *>(t + n * 64 * TW + a);
    }
    const uint32_t p = __builtin_amdgcn_bitop3_b32(r[0], r[1], r[2], 0x96);
    const uint32_t q = __builtin_amdgcn_bitop3_b32(r[3], r[4], r[5], 0x96);
    return __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_bitop3_b32(p, q, r[6], 0x96), r[7], 0u, 0x96);
}

__device__ __forceinline__ uint32_t dpp_xor(uint32_t v, int ctrl_sel)
{
    // ctrl is a compile-time constant at every call site
    switch (ctrl_sel) {
    case 0: return v ^ (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);   // quad [1,0,3,2]
    case 1: return v ^ (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false);   // quad [2,3,0,1]
    case 2: return v ^ (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x124, 0xF, 0xF, false);  // row_ror:4
    default: return v ^ (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, false); // row_ror:8
    }
}

// XOR over all 64 lanes; result is wave-uniform
__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
    v = dpp_xor(v, 0);
    v = dpp_xor(v, 1);
    v = dpp_xor(v, 2);
    v = dpp_xor(v, 3);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) ^ (uint32_t)__builtin_amdgcn_readlane((int)v, 16) ^
           (uint32_t)__builtin_amdgcn_readlane((int)v, 32) ^ (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

// XOR within aligned groups of G lanes (G power of two <= 64); every lane of
// a group ends with the group total
template <int G>
__device__ __forceinline__ uint32_t group_xor(uint32_t v)
{
#pragma unroll
    for (int m = 1; m < G; m <<= 1)
        v ^= (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}

__device__ __forceinline__ void load_lds_image(const uint32_t *__restrict__ img)
{
    copy_to_lds(img, s_tab, kLdsWords / 4);
}

// Wave-uniform buffer descriptor from a pointer: readfirstlane the halves so
// hipcc can prove uniformity (else it wraps every buffer op in a
// readfirstlane waterfall loop, CDNA HIP guide T20).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const uint8_t *p, uint32_t bytes)
{
    const uint64_t a = (uint64_t)(uintptr_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void *)(uintptr_t)(((uint64_t)hi << 32) | lo), 0, bytes,
                                             0x00020000);
}

// readfirstlane returns int: go through uint32_t so the low half is never
// sign-extended into the high half (bit 31 set = offsets >= 2 GiB)
__device__ __forceinline__ uint64_t uniform64(uint64_t v)
{
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
    return ((uint64_t)hi << 32) | lo;
}

// One chunk = CH rows.  Descriptor base = the chunk's row in the wave's
// first block (SGPRs), voffset = lane's block offset + 16*column (VGPR),
// row k's offset = k*RB (12-bit immediate).  AUX = cache policy (2 = nt).
template <int CH, int RB, int AUX>
__device__ __forceinline__ void load_chunk(v4u (&X)[CH], const uint8_t *cp, uint32_t span, uint32_t voff)
{
    const __amdgpu_buffer_rsrc_t r = uniform_rsrc(cp, span);
#pragma unroll
    for (int k = 0; k < CH; k++) {
        X[k] = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(r, (int)(voff + k * RB), 0, AUX));
        // keep the loads in row order: vmcnt retires in issue order, so row k
        // must not be issued behind rows the hash needs later
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---------------------------------------------------------------------------
// hot kernel: G lanes per block (G = 16, 32 or 64), so a wave hashes NB = 64/G
// consecutive blocks at once.  A block is R rows of RB = 16G bytes; lane l
// owns column c = l % G (bytes [16c, 16c+16) of every row) of block l / G.
// One row step is one global_load_dwordx4 per lane covering NB runs of RB
// contiguous bytes.  The last word of every row but the block's last uses
// set B (Z_(4 + RB - 16)), which lands the lane on its piece of the next row;
// after the last row lane l folds its partial over Z_(16(G-1-c)) (per-lane
// columns) and the G lanes of a block XOR-reduce (DPP within 16-lane rows,
// readlane across rows).
//
// Each wave owns a contiguous range of block groups (NB blocks each); CRCs
// are collected one per lane in a VGPR and flushed as one 256-B store per 64
// blocks.  Chunks of CH rows are pipelined NBUF deep in registers: chunk
// q+NBUF-1's loads are issued (pinned by a scheduling barrier) before chunk q
// is hashed, and no loop exit sits inside a group of NBUF chunks, so the
// waitcnt state at the loop head is path-independent (only prefetches in
// flight).
// ---------------------------------------------------------------------------
struct RowsOut {
    uint32_t res, nres;
    uint64_t res_base;
};

// XOR over the 16 lanes of each DPP row, then read the four row totals
__device__ __forceinline__ void row_totals(uint32_t f, uint32_t (&s)[4])
{
    f = dpp_xor(f, 0);
    f = dpp_xor(f, 1);
    f = dpp_xor(f, 2);
    f = dpp_xor(f, 3);
    s[0] = (uint32_t)__builtin_amdgcn_readlane((int)f, 0);
    s[1] = (uint32_t)__builtin_amdgcn_readlane((int)f, 16);
    s[2] = (uint32_t)__builtin_amdgcn_readlane((int)f, 32);
    s[3] = (uint32_t)__builtin_amdgcn_readlane((int)f, 48);
}

// record the NB = 64/G block CRCs of one wave group (row totals s) in the
// per-lane result buffer; flush 64 results as one coalesced store
template <int G>
__device__ __forceinline__ void record_group(const uint32_t (&s)[4], RowsOut &o, uint32_t *__restrict__ out,
                                             int lane)
{
    if (G == 64) {
        o.res = (lane == (int)o.nres) ? (s[0] ^ s[1] ^ s[2] ^ s[3]) : o.res;
    } else if (G == 32) {
        o.res = (lane == (int)o.nres) ? (s[0] ^ s[1]) : o.res;
        o.res = (lane == (int)o.nres + 1) ? (s[2] ^ s[3]) : o.res;
    } else {
        o.res = (lane == (int)o.nres) ? s[0] : o.res;
        o.res = (lane == (int)o.nres + 1) ? s[1] : o.res;
        o.res = (lane == (int)o.nres + 2) ? s[2] : o.res;
        o.res = (lane == (int)o.nres + 3) ? s[3] : o.res;
    }
    o.nres += 64 / G;
    if (o.nres == 64) {
        out[o.res_base + lane] = o.res;
        o.res_base += 64;
        o.nres = 0;
    }
}

template <int G>
__device__ __forceinline__ void emit_group(uint32_t f, RowsOut &o, uint32_t *__restrict__ out, int lane)
{
    uint32_t s[4];
    row_totals(f, s);
    record_group<G>(s, o, out, lane);
}

// fold of a block-ending register: NIB = nibble tables on the pre-step
// register, else the column bit-matrix on the stepped one
template <int G, bool NIB>
__device__ __forceinline__ uint32_t fold_lane(uint32_t u, const uint32_t (&col)[32], uint32_t cb)
{
    if constexpr (NIB)
        return nib_fold<nib_width<G>()>(u, cb);
    else
        return bitmat(u, col);
}

template <bool NIB, bool FUSE3>
__device__ __forceinline__ uint32_t piece_end(uint32_t u, const v4u &d, const LaneConst &L)
{
    if constexpr (NIB)
        return piece_pre<FUSE3>(u, d, L);
    else
        return piece<true, FUSE3>(u, d, L);
}

template <int G, int CH, bool FUSE3, bool NIB>
__device__ __forceinline__ uint32_t hash_chunk(uint32_t u, const v4u (&X)[CH], bool blk_end, const LaneConst &L,
                                               const uint32_t (&col)[32], uint32_t cb, RowsOut &o,
                                               uint32_t *__restrict__ out, int lane)
{
#pragma unroll
    for (int k = 0; k < CH - 1; k++)
        u = piece<false, FUSE3>(u, X[k], L);
    if (!blk_end)
        return piece<false, FUSE3>(u, X[CH - 1], L);
    u = piece_end<NIB, FUSE3>(u, X[CH - 1], L);
    emit_group<G>(fold_lane<G, NIB>(u, col, cb), o, out, lane);
    return 0;
}

// Product OPT bits of crc_rows_kernel (the explorer's crc_rows_x_kernel,
// tools/crc_rows_explore.inc, adds the measurement-only ones):
// OPT bit 1: pipelined fold -- only valid when one chunk is one block group
//            (block_size == CH * 16 * G)
// OPT bit 5: nibble-table fold (nib_fold; foldG then points at the 8*16*TW
//            word nibble image, TW = nib_width<G>, instead of the bit-matrix
//            columns)
// OPT bits 8-9: progress-priority mode (set_priority): every NBUF chunks
//            each wave posts its chunk count and ranks itself among the
//            workgroup's waves; the laggards raise their issue priority
//            (s_setprio), so a CU's waves finish closer together
// [g0, g0 + ng) = wave wid's contiguous share of n units among W waves:
// equal shares, or XCD-weighted (xw = (we << 16) | wo: waves of even
// workgroups -- even XCDs under round-robin dispatch -- weigh we, odd wo)
// (NW waves per workgroup)
#ifdef PRISKV_CRC_COVERAGE
__device__ unsigned long long g_cov[2]; // groups hashed, sum of their indices (test-only build)
// per-wave timing of the last rows-kernel launch (test-only build, tools/wave_times.py):
// {XCC id | wave id << 8, groups, start, end} (s_memrealtime, 100 MHz)
constexpr int kCovWaves = 8192;
__device__ unsigned long long g_wave_t[kCovWaves][4];
#endif
template <int NW = kWaves>
__device__ __forceinline__ void wave_range(uint64_t n, uint64_t W, uint64_t wid, uint32_t xw, uint64_t &g0,
                                           uint64_t &ng)
{
    if (!xw) {
        g0 = uniform64(n * wid / W);
        ng = n * (wid + 1) / W - g0;
    } else {
        // Workgroup b runs on XCD (b + k) % 8, k = the XCD the launch's
        // hardware queue dispatches first (round 5: 0, 5, 6 or 7 by queue on
        // one box, tools/xcd_offset_probe.hip): xw's first weight belongs to
        // even XCDs, so it goes to the odd workgroups when k is odd.  k's
        // parity is the same for every workgroup of the launch (round-robin
        // dispatch), so every wave computes the same split.
        uint32_t xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
        const bool kodd = ((xcc ^ (uint32_t)blockIdx.x) & 1u) != 0;
        const uint64_t we = kodd ? xw & 0xFFFF : xw >> 16, wo = kodd ? xw >> 16 : xw & 0xFFFF;
        auto prefix = [&](uint64_t w) { // weighted share of waves [0, w)
            const uint64_t b = w / NW, k = w % NW;
            return ((b + 1) / 2) * NW * we + (b / 2) * NW * wo + k * ((b & 1) ? wo : we);
        };
        const uint64_t tot = prefix(W);
        g0 = uniform64(n * prefix(wid) / tot);
        ng = n * prefix(wid + 1) / tot - g0;
    }
#ifdef PRISKV_CRC_COVERAGE
    // test-only build (make cov): every wave's range into g_cov, so the host
    // can check that the launch's ranges tile [0, n) (priskv_crc_cov_take)
    if (__lane_id() == 0 && ng) {
        atomicAdd(&g_cov[0], (unsigned long long)ng);
        atomicAdd(&g_cov[1], (unsigned long long)(ng * g0 + ng * (ng - 1) / 2));
    }
#endif
}

// Progress priority (rows kernel OPT bits 8-9, extents kernel the same):
// each wave posts its progress count in LDS and reads the workgroup's (stale
// values are fine); after its next NBUF chunks it sets its issue priority
// from how many of the workgroup's waves are ahead.  MODE 1: the two last
// waves 3, the back half 1; MODE 2: the back half 3; MODE 3: graded,
// (waves ahead) / 2.  MODE 0: nothing.
// NW = waves per workgroup.
__shared__ uint32_t s_prog[16];

template <int MODE, int NW = kWaves>
__device__ __forceinline__ void init_progress()
{
    if (MODE && threadIdx.x < NW)
        s_prog[threadIdx.x] = 0;
}

template <int MODE, int NW = kWaves>
__device__ __forceinline__ uint32_t post_progress(uint32_t q, int wave, int lane)
{
    if constexpr (MODE == 0)
        return 0u;
    if (lane == 0)
        s_prog[wave] = q;
    return s_prog[lane & (NW - 1)];
}

template <int MODE, int NW = kWaves>
__device__ __forceinline__ void set_priority(uint32_t peer, uint32_t q, int lane)
{
    if constexpr (MODE == 0)
        return;
    // waves ahead, scaled to eighths of the workgroup
    const uint32_t ahead = (uint32_t)__builtin_popcountll(__ballot(lane < NW && peer > q)) * 8 / NW;
    if constexpr (MODE == 1) {
        if (ahead >= 6)
            __builtin_amdgcn_s_setprio(3);
        else if (ahead >= 4)
            __builtin_amdgcn_s_setprio(1);
        else
            __builtin_amdgcn_s_setprio(0);
    } else if constexpr (MODE == 2) {
        if (ahead >= 4)
            __builtin_amdgcn_s_setprio(3);
        else
            __builtin_amdgcn_s_setprio(0);
    } else {
        if (ahead >= 6)
            __builtin_amdgcn_s_setprio(3);
        else if (ahead >= 4)
            __builtin_amdgcn_s_setprio(2);
        else if (ahead >= 2)
            __builtin_amdgcn_s_setprio(1);
        else
            __builtin_amdgcn_s_setprio(0);
    }
}

// OPT bit 10 (extents and sub-KiB kernels): one 16-wave workgroup per CU
// instead of two of 8 (the tables are filled once per CU, and the 32 B of
// progress slots fit: two 8-wave workgroups already use 2 x 80 KiB of the
// 160 KiB LDS)
constexpr int ext_waves(int OPT) { return (OPT & 1024) ? 16 : kWaves; }

// ---------------------------------------------------------------------------
// Byte-balanced split of the extents kernel (OPT bit 11).  Each extent costs
// ext_cost(len) = ceil(len / 2 KiB) + 1 (its chunks plus one for the fold);
// crc_ext_cost_kernel sums the costs of each tile of kExtTile extents.  Wave
// w of W then owns [e(total w / W), e(total (w+1) / W)) with
// e(t) = min{ i : P(i) >= t }, P(i) = cost of the extents before i: a
// partition of [0, n) (costs are >= 1, so P is strictly increasing, e(0) = 0
// and e(total) = n).  A wave finds e(t) from the tile sums (kExtTileLanes
// per lane, at most 64 * 8 tiles: host-checked) and then the lengths of one
// tile, with ballots over the monotone predicate P < t.
// ---------------------------------------------------------------------------
constexpr uint32_t kExtTile = 256;
constexpr int kExtTileLanes = 8;

__device__ __forceinline__ uint32_t ext_cost(uint32_t len) { return (len + 2047u) / 2048u + 1u; }

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d)
{
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64);
    const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

// inclusive prefix sum over the wave's lanes
__device__ __forceinline__ uint64_t wave_incl_scan64(uint64_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t u = shfl_up64(v, d);
        if (lane >= d)
            v += u;
    }
    return v;
}

// one wave per tile: tile_cost[t] = sum of ext_cost over extents [t kExtTile, ...)
__global__ __launch_bounds__(256) void crc_ext_cost_kernel(const uint32_t *__restrict__ lengths, uint64_t n,
                                                           uint32_t *__restrict__ tile_cost, uint64_t ntiles)
{
    const uint64_t t = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= ntiles)
        return;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < (int)kExtTile / 64; k++) {
        const uint64_t i = t * kExtTile + (uint64_t)k * 64 + lane;
        if (i < n)
            c += ext_cost(lengths[i]);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
        c += (uint32_t)__shfl_xor((int)c, m, 64);
    if (lane == 0)
        tile_cost[t] = c;
}

// the wave's tile prefix: lane l holds tiles [l K, l K + K) (K = kExtTileLanes)
struct ExtTiles {
    uint64_t excl[kExtTileLanes]; // exclusive prefix of each of the lane's tiles (~0: no tile)
    uint64_t total;
};

__device__ __forceinline__ ExtTiles ext_tiles(const uint32_t *__restrict__ tile_cost, uint64_t ntiles, int lane)
{
    ExtTiles T;
    uint32_t c[kExtTileLanes];
    uint64_t sum = 0;
#pragma unroll
    for (int j = 0; j < kExtTileLanes; j++) {
        const uint64_t t = (uint64_t)lane * kExtTileLanes + j;
        c[j] = t < ntiles ? tile_cost[t] : 0u;
        sum += c[j];
    }
    const uint64_t incl = wave_incl_scan64(sum, lane);
    T.total = readlane64(incl, 63);
    uint64_t run = incl - sum;
#pragma unroll
    for (int j = 0; j < kExtTileLanes; j++) {
        const uint64_t t = (uint64_t)lane * kExtTileLanes + j;
        T.excl[j] = t < ntiles ? run : ~0ull;
        run += c[j];
    }
    return T;
}

// e(target) = min{ i : P(i) >= target } (wave-uniform)
__device__ __forceinline__ uint64_t ext_boundary(const ExtTiles &T, const uint32_t *__restrict__ lengths, uint64_t n,
                                                 uint64_t target, int lane)
{
    if (target == 0)
        return 0;
    // t* = last tile whose prefix is below the target (tile 0's is 0)
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < kExtTileLanes; j++)
        cnt += (uint32_t)__builtin_popcountll(__ballot(T.excl[j] < target));
    const uint32_t ts = cnt - 1;
    const uint32_t jl = ts % kExtTileLanes;
    uint64_t mine = 0;
#pragma unroll
    for (int j = 0; j < kExtTileLanes; j++)
        mine = (uint32_t)j == jl ? T.excl[j] : mine;
    const uint64_t tp = readlane64(mine, (int)(ts / kExtTileLanes));
    // inside tile t*: lane l holds extents b + 4l .. b + 4l + 3
    const uint64_t b = (uint64_t)ts * kExtTile;
    uint32_t c[4];
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint64_t i = b + 4u * (uint32_t)lane + k;
        c[k] = i < n ? ext_cost(lengths[i]) : 0u;
        sum += c[k];
    }
    uint64_t run = tp + wave_incl_scan64(sum, lane) - sum;
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint64_t i = b + 4u * (uint32_t)lane + k;
        run += c[k]; // P(i + 1)
        m += (uint32_t)__builtin_popcountll(__ballot(i < n && run < target));
    }
    const uint64_t e = b + m + 1;
    return uniform64(e < n ? e : n);
}

// sum over the 64 lanes, every lane gets it (DPP butterfly within rows of
// 16, then the four row totals)
__device__ __forceinline__ uint32_t wave_sum32(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);  // quad [1,0,3,2]
    v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false);  // quad [2,3,0,1]
    v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x124, 0xF, 0xF, false); // row_ror:4
    v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, false); // row_ror:8
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

// ---------------------------------------------------------------------------
// Shifted partial CRCs (the rows kernel's split mode and the fused kernel).
// A part of a block or extent contributes its CRC moved to the end,
// Z_d(crc) with d the bytes after the part (linear, no affine term: SURVEY
// §0.2); Z_d is applied as one 32x32 GF(2) matrix per set bit of d, from the
// columns of Z_(2^b) in LDS.
// ---------------------------------------------------------------------------
constexpr int kFusedZRows = 48;                  // = crc_gpu.hip kZpowRows
__shared__ __attribute__((aligned(16))) uint32_t s_zpow[kFusedZRows * 32];    // columns of Z_(2^b), b < 48

// v -> Z(v) for the matrix whose 32 columns are at cols (LDS): lane l < 32
// contributes column l when bit l of the wave-uniform v is set
__device__ __forceinline__ uint32_t zapply_lds(uint32_t v, const uint32_t *cols, int lane)
{
    return wave_xor((lane < 32 && ((v >> (lane & 31)) & 1u)) ? cols[lane & 31] : 0u);
}

// XOR over lanes 0-31 when lanes 32-63 hold 0 (DPP within the two rows,
// then two readlanes: half of wave_xor's cross-row step)
__device__ __forceinline__ uint32_t xor_lo32(uint32_t v)
{
    v = dpp_xor(v, 0);
    v = dpp_xor(v, 1);
    v = dpp_xor(v, 2);
    v = dpp_xor(v, 3);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) ^ (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
}

// Z_r(v): one apply per set bit of r (r < 2^48).  The columns of the next
// four set bits' matrices are read from LDS together (their addresses do not
// depend on v), so the serial chain per bit is one select and one 32-lane
// XOR reduction rather than an LDS round trip and a 64-lane one: the shift
// sits at the end of a part, on its wave's last path
#ifndef PRISKV_ZSHIFT_BATCH
#define PRISKV_ZSHIFT_BATCH 1
#endif
__device__ __forceinline__ uint32_t zshift_lds(uint32_t v, uint64_t r, int lane)
{
#if PRISKV_ZSHIFT_BATCH
    const uint32_t l = (uint32_t)lane & 31;
    const bool lo = lane < 32;
#pragma unroll 1
    while (r) {
        uint32_t c[4];
        uint64_t rr = r;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            c[j] = s_zpow[(rr ? __builtin_ctzll(rr) : 0) * 32 + l];
            rr &= rr - 1;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (r) {
                v = xor_lo32((lo && ((v >> l) & 1u)) ? c[j] : 0u);
                r &= r - 1;
            }
        }
    }
    return v;
#else
#pragma unroll 1
    while (r) {
        const int b = __builtin_ctzll(r);
        v = zapply_lds(v, s_zpow + b * 32, lane);
        r &= r - 1;
    }
    return v;
#endif
}

// Cross-workgroup finish of a block / extent with parts in several
// workgroups, through ONE zero-at-rest 64-bit word per item, acc[x] = (units
// counted << 32) | XOR of the shares.  A share g covering c of the item's m
// units goes in as two atomics on that word: XOR g into the low half, then
// add c << 32 (neither disturbs the other half); the add that makes the
// count m returns the word as it was just before it, whose low half is the
// XOR of every share, and the word is put back to 0.  All of an item's
// atomics are on one location, so they are totally ordered there, and each
// thread's XOR precedes its add (two read-modify-writes of one atomic object
// by one thread keep program order): every share's XOR precedes the
// completing add.  Nothing relies on two addresses' atomics becoming visible in
// issue order.  (Rounds 1-5 kept count and XOR in two words, relying on an
// add whose operand depended on the XOR's return; in graphs with
// memory-node scratch 6-16 of 1900 split-mode blocks came out as exactly the
// block minus its first-finished part -- the count seen without that part's
// XOR (tools/classify_graph_race.py, 60 of 60 records, DESIGN.md §5) -- and
// where the compiler knew c != 0 it dropped the dependency, issuing a
// no-return XOR beside the add.  A compare-and-swap loop on one word, tried
// first in round 6, was exact but serialised a lone block's 256 workgroups:
// 1 x 256 MiB 51 -> 302 us.)  Any lane may call it, for its own x.
__device__ __forceinline__ void finish_shared(uint64_t *__restrict__ acc, uint32_t *__restrict__ out, uint64_t x,
                                              uint32_t g, uint32_t c, uint32_t m)
{
    if (c == m) {
        out[x] = g;
        return;
    }
    __hip_atomic_fetch_xor(&acc[x], (uint64_t)g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t old = __hip_atomic_fetch_add(&acc[x], (uint64_t)c << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((uint32_t)(old >> 32) + c == m) {
        // the completing add returned every share (all XORs precede it), so
        // no exchange round trip: the word goes back to 0 with a
        // write-through store nobody waits for
        out[x] = (uint32_t)old;
        __hip_atomic_store(&acc[x], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// workgroups per CU a rows-kernel instance must fit (sets its VGPR budget):
// pipelines holding more than 64 VGPRs of row data get the whole 256-VGPR
// file at one 8-wave workgroup per CU
constexpr int rows_min_wg(int CH, int NBUF) { return CH * NBUF * 4 > 64 ? 1 : 2; }

//
// xw: XCD weights (DESIGN §5).  Workgroup b runs on XCD (b + k) % 8 (round-robin
// dispatch from the queue's first XCD k, checked once per context by a probe
// kernel; wave_range reads k's parity); with xw = (we << 16)
// | wo, waves of even-XCD workgroups take we parts of the batch and odd ones
// wo (waves on odd XCDs finish ~10 % later under an equal split on every
// MI355X measured).  xw = 0: equal shares.
//
// stride: block i starts at base + i * stride (stride >= block_size; the
// head-split path hashes the 1 KiB-multiple bodies of longer blocks, 4-byte
// aligned, which the buffer loads read at full rate).
//
// tile: 0 = each wave owns one contiguous range of block groups (the split
// above).  tile > 0 = block-cyclic order: wave w takes tiles w, w + W, w + 2W,
// ... of `tile` groups each (the last tile may be short), so at any moment
// the chip reads a window of about W tiles instead of W ranges spread over
// the whole batch.  For batches of tens of GiB that is faster (page-walk
// locality, DESIGN §5); the host picks it by batch size.
//
// split (OPT bit 6, G = 64, not PIPE, stride == block_size, no tiles): the
// batch is cut into units of block_size / split bytes, ngroups counts units,
// and each wave owns a contiguous, XCD-weighted range of units -- so the
// weights apply at sub-block granularity when there are few blocks per wave
// (1 MiB blocks: 2 per wave).  A wave hashes its range as one contiguous
// stream; a block it holds whole is stored as usual, a part of a block (its
// first and last only) contributes its CRC moved to the block end (Z_d from
// s_zpow, d = bytes after the part) through finish_shared's zero-at-rest
// word per block (acc: the caller's zeroed scratch of nblocks 64-bit words)
// -- one launch, no combine kernel.
// split mode with OPT bit 7 (few large blocks): each wave's (at most two)
// parts of blocks -- block, shifted CRC, units -- merged per workgroup before
// the cross-workgroup finish
// OPT bit 10: one 16-wave workgroup per CU (the tables loaded once for 16
// waves; rows_waves)
constexpr uint32_t kPartNone = 0xFFFFFFFFu;
__shared__ uint32_t s_part[kWaves][2][3];
constexpr int rows_waves(int OPT) { return (OPT & 1024) ? 16 : kWaves; }

// Window mode (OPT bit 13, odd sizes or bases near a multiple W of 1 KiB,
// W - 15 <= B <= W + 48; the host picks which, crc_gpu.hip window_bytes):
// block b = [s, e = s + B) is hashed as its window [w0, eh) -- eh the 16-B
// boundary at or after e, w0 = eh - W -- at the plan's full rate: aligned
// rows (with G < 64, lane group j reads block j of its group at its own
// offset), nothing added to the per-block chain but the last lane of each
// block's group writing the window's last granule G_b (its piece of the
// last row) to an LDS slot.  Every 64 blocks, when the wave stores their
// CRCs, lane i
// corrects block b's window CRC c (linear, init 0, no xorout) from G_b and
// G_(b-1) (the previous block's; across groups a carried one):
//   - tail: c ^= crc(G_b's bytes from e on) (leading zeros are free);
//   - front (w0 < s: the window starts at s & ~15 = G_(b-1)'s granule):
//     c ^= Z_(W - 16)(crc(G_(b-1)'s bytes below s, then zeros));
//   - head (w0 > s: the block's bytes before the window): c ^=
//     Z_W(crc(G_(b-1)'s bytes from s on || the granules from the 16-B
//     boundary after s up to w0)); those "gap" granules exist only for B > W
//     (4097 B: one block in 16) and are loaded there;
//   - c is now Z_p(crc(block)), p = eh - e: out = Z_-p(c).
// The wave's first block takes G_(g0-1) from one load before its loop.
// Image (per W, kWinImgWords): slice-by-4 tables, then nibble tables
// (8 nibbles x 16 values) of Z_W, Z_(W - 16) and Z_-p for p = 0..15.
constexpr int kWinNib = 8 * 16;
constexpr int kWinImgWords = 4 * 256 + 18 * kWinNib;
__shared__ __attribute__((aligned(16))) uint32_t s_winimg[kWinImgWords];
__shared__ v4u s_wing[kWaves][64]; // G_b of the wave's current 64 blocks

// reflected slice-by-4 step over one little-endian word, and over a granule
__device__ __forceinline__ uint32_t win_word(uint32_t c, uint32_t w)
{
    c ^= w;
    return s_winimg[3 * 256 + (c & 0xff)] ^ s_winimg[2 * 256 + ((c >> 8) & 0xff)] ^
           s_winimg[256 + ((c >> 16) & 0xff)] ^ s_winimg[c >> 24];
}

__device__ __forceinline__ uint32_t win_gran(uint32_t c, v4u g)
{
    return win_word(win_word(win_word(win_word(c, g[0]), g[1]), g[2]), g[3]);
}

// the granule's bytes from byte a (0..16) on (FROM), or below it
template <bool FROM>
__device__ __forceinline__ v4u win_keep(v4u g, uint32_t a)
{
    v4u r;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int lo = (int)a - 4 * j;
        const uint32_t m = lo <= 0 ? ~0u : (lo >= 4 ? 0u : ~0u << (8 * lo));
        r[j] = g[j] & (FROM ? m : ~m);
    }
    return r;
}

// v through nibble table t (s_winimg + 4 * 256 + k * kWinNib)
__device__ __forceinline__ uint32_t win_apply(const uint32_t *t, uint32_t v)
{
    uint32_t r = 0;
#pragma unroll
    for (int n = 0; n < 8; n++)
        r ^= t[n * 16 + ((v >> (4 * n)) & 15u)];
    return r;
}

template <int G, int CH, int NBUF, int AUX, int OPT = 0>
__global__ __launch_bounds__(64 * rows_waves(OPT), rows_waves(OPT) == 16 ? 1 : rows_min_wg(CH, NBUF)) void crc_rows_kernel(
    const uint8_t *__restrict__ base, uint64_t ngroups, uint32_t block_size,
    const uint32_t *__restrict__ lds_image, const uint32_t *__restrict__ foldG,
    uint32_t *__restrict__ out, uint32_t xw, uint32_t tile, uint32_t stride, uint32_t split,
    const uint32_t *__restrict__ zpow, uint64_t *__restrict__ acc)
{
    constexpr int NB = 64 / G;          // blocks per wave group
    constexpr int RB = 16 * G;          // bytes per row of one block
    constexpr bool PIPE = (OPT & 2) != 0;
    constexpr bool NIB = (OPT & 32) != 0;
    constexpr int PRIO_MODE = (OPT >> 8) & 3;
    constexpr bool EARLY = (OPT & 16) != 0;
    constexpr bool SPLIT = (OPT & 64) != 0;
    constexpr bool MERGE = SPLIT && (OPT & 128) != 0; // parts merged per workgroup (few large blocks)
    constexpr int NW = rows_waves(OPT);
    constexpr bool WIN = (OPT & 8192) != 0; // window mode (s_winimg above; DESIGN §4)
    static_assert(!WIN || !SPLIT, "window mode: whole blocks");
    static_assert((OPT & ~(2 | 16 | 32 | 64 | 128 | 1024 | 8192 | (3 << 8))) == 0,
                  "product rows-kernel options only (see crc_rows_x_kernel)");
    static_assert(!MERGE || NW == kWaves, "the workgroup merge holds 8 waves' parts");
    static_assert(!SPLIT || (G == 64 && !PIPE), "split mode: one block per wave group, unpipelined fold");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const LaneConst L = lane_const(lane);
    const uint32_t cb = 4u * (uint32_t)(lane % nib_width<G>());
    uint32_t col[32];
    // the LDS tables (every wave of the workgroup loads its share, so this
    // runs before any wave may leave)
    auto tables = [&]() __attribute__((always_inline)) {
        load_lds_image(lds_image);
        if constexpr (NIB) {
            load_nib_image<nib_width<G>()>(foldG);
        } else {
#pragma unroll
            for (int i = 0; i < 32; i++)
                col[i] = foldG[i * 64 + lane];
        }
        static_assert(kWinImgWords % 256 == 0 && kFusedZRows * 32 % 256 == 0, "whole waves of 16-B pieces");
        if constexpr (WIN)
            copy_to_lds(zpow, s_winimg, kWinImgWords / 4);
        if constexpr (SPLIT) {
            copy_to_lds(zpow, s_zpow, kFusedZRows * 32 / 4);
            if (MERGE && threadIdx.x < kWaves * 2)
                s_part[threadIdx.x >> 1][threadIdx.x & 1][0] = kPartNone;
        }
        init_progress<PRIO_MODE, NW>();
        lds_dma_landed();
        __syncthreads();
    };
    if constexpr (!EARLY)
        tables();

#ifdef PRISKV_CRC_COVERAGE
    const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
#endif
    const uint64_t W = (uint64_t)gridDim.x * NW;
    const uint64_t wid = (uint64_t)blockIdx.x * NW + wave;
    const uint32_t T = SPLIT ? 0u : __builtin_amdgcn_readfirstlane(tile);
    uint64_t g0, ng;
    if (T) {
        const uint64_t ntiles = (ngroups + T - 1) / T;
        const uint64_t mine = ntiles > wid ? (ntiles - 1 - wid) / W + 1 : 0;
        const uint64_t last = wid + (mine - 1) * W; // this wave's last tile
        g0 = uniform64(wid * T);
        ng = mine ? (mine - 1) * T + (last + 1 == ntiles ? ngroups - last * T : T) : 0;
    } else {
        wave_range<NW>(ngroups, W, wid, xw, g0, ng);
    }
    if (!EARLY && !MERGE && ng == 0) // (MERGE: every wave reaches the workgroup merge)
        return;
    // stride: bytes from one block to the next (block_size, or more when the
    // blocks are the bodies of longer ones: the head-split path)
    const uint32_t S = SPLIT ? __builtin_amdgcn_readfirstlane(split) : 1u; // units per block
    const uint32_t cpb = block_size / (CH * RB);                          // chunks per block
    const uint32_t cps = cpb / S;                                          // ... per wave unit (block or part)
    const uint32_t nq = __builtin_amdgcn_readfirstlane((uint32_t)ng * cps); // < 2^31: host-checked
    // (WIN: block j of a group starts its window within 15 bytes of j stride)
    const uint32_t span = (NB - 1) * stride + (WIN && NB > 1 ? 16u : 0u) + CH * RB; // bytes one chunk spans
    uint32_t voff = (uint32_t)(lane / G) * (WIN ? 0u : stride) + (uint32_t)(lane % G) * 16;
    const uint64_t gstride = SPLIT ? (uint64_t)cps * CH * RB : (uint64_t)NB * stride; // bytes per unit
    const uint32_t cstride = CH * RB;                                     // bytes per chunk in a block
    const uint64_t tjump = T ? (W - 1) * (uint64_t)T * gstride : 0;       // tile end -> this wave's next tile

    // prefetch cursor: (pp, pc) = address / chunk-in-block of the next chunk
    // to load; it stops at the wave's last chunk (re-loads are harmless)
    // WIN: block b's window is the block_size bytes ending at the first 16-B
    // boundary at or after its end, base + (b + 1) stride (stride = the odd
    // block size); consecutive windows overlap or leave gaps of a few bytes
    // (corrected when the CRCs are stored: s_winimg's comment)
    // With NB > 1 blocks per group (G < 64), lane group j reads block j's
    // window at its own offset from block 0's (voff; uniform per group)
    uint64_t wend = (uint64_t)(uintptr_t)base + (g0 * NB + 1) * (uint64_t)stride; // WIN: end of the group's first block
    auto win = [&]() {
        if constexpr (WIN && NB > 1) {
            const uint64_t e0 = (wend + 15) & ~(uint64_t)15;
            uint32_t d = 0;
#pragma unroll
            for (int j = 1; j < NB; j++) {
                const uint32_t dj = (uint32_t)(((wend + (uint64_t)j * stride + 15) & ~(uint64_t)15) - e0);
                d = lane / G == j ? dj : d;
            }
            voff = (uint32_t)(lane % G) * 16 + d;
        }
        return reinterpret_cast<const uint8_t *>((uintptr_t)uniform64(((wend + 15) & ~(uint64_t)15) - block_size));
    };
    const uint8_t *pp = WIN ? win() : base + g0 * gstride;
    uint32_t pc = 0, pq = 0, pg = 0;
    auto advance = [&]() {
        if (pq + 1 < nq) {
            pq++;
            if (++pc == cps) {
                pc = 0;
                if constexpr (WIN) {
                    wend += (uint64_t)NB * stride;
                    pp = win();
                } else
                    pp += gstride - (uint64_t)(cps - 1) * cstride;
                if (T && ++pg == T) {
                    pg = 0;
                    pp += tjump;
                }
            } else {
                pp += cstride;
            }
        }
    };

    v4u buf[NBUF][CH];
    // WIN: G_(g0-1), the granule before the wave's first block, requested
    // before the chunks: it is read into SGPRs before the main loop, and
    // being the oldest load it costs no wait beyond the first chunk's (with
    // EARLY, the tables' wait covers it)
    v4u cload = {0, 0, 0, 0};
    if constexpr (WIN) {
        const uint64_t s0 = (uint64_t)(uintptr_t)base + g0 * NB * stride;
        const uint32_t a0 = (uint32_t)(s0 & 15);
        const uint8_t *gp = reinterpret_cast<const uint8_t *>((uintptr_t)(a0 ? s0 & ~(uint64_t)15 : s0));
        const __amdgpu_buffer_rsrc_t r = uniform_rsrc(gp, a0 ? 16u : 0u); // (none: s aligned, G unused)
        cload = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(r, 0, 0, AUX));
        __builtin_amdgcn_sched_barrier(0);
    }
    // EARLY (OPT bit 4): the first NBUF - 1 chunks are requested before the
    // tables, so their HBM latency overlaps the table loads instead of
    // following them; the workgroup barrier then waits for both
    if ((!EARLY && !MERGE) || ng) {
#pragma unroll
        for (int j = 0; j < NBUF - 1; j++) {
            load_chunk<CH, RB, AUX>(buf[j], pp, span, voff);
            advance();
        }
    }
    if constexpr (EARLY) {
        tables();
        if (!MERGE && ng == 0)
            return;
    }
    // SPLIT: cq = the hash's chunk within its block, pu = the chunk where
    // the current part of it started (> 0: the block began in another
    // wave), hb = that block; whole blocks are recorded from the first one
    // the range holds entirely
    uint32_t u = 0, q = 0;
    uint32_t cq = SPLIT ? (uint32_t)(g0 % S) * cps : 0u, pu = cq, nparts = 0;
    uint64_t hb = SPLIT ? g0 / S : 0;
    RowsOut o{0u, 0u, SPLIT ? (g0 + S - 1) / S : g0 * NB};
    // record one finished group's CRCs (row totals s); with tiles, a group
    // that starts a new tile first flushes the previous tile's results
    uint32_t hrec = 0;
    uint64_t htile = wid;
    auto rec = [&](const uint32_t (&s)[4]) {
        if (T && hrec == T) {
            if (o.nres && lane < (int)o.nres)
                out[o.res_base + lane] = o.res;
            o.nres = 0;
            htile += W;
            o.res_base = htile * T * NB;
            hrec = 0;
        }
        record_group<G>(s, o, out, lane);
        hrec++;
    };
    // WIN: carry = G_(b-1) of the group's first block (in SGPRs: a register
    // the loop's loads may still be writing would make the store step wait
    // for every load in flight)
    uint32_t carry[4] = {0, 0, 0, 0};
    auto win_flush = [&](uint32_t n) __attribute__((always_inline)) {
        if constexpr (WIN) {
            const v4u og = s_wing[wave][lane];
            v4u gp = s_wing[wave][lane > 0 ? lane - 1 : 0];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                gp[k] = lane == 0 ? carry[k] : gp[k];
                carry[k] = (uint32_t)__builtin_amdgcn_readlane((int)og[k], (int)n - 1);
            }
            if (lane < (int)n) {
                const uint64_t b = o.res_base + (uint64_t)lane;
                const uint64_t s0 = (uint64_t)(uintptr_t)base + b * stride, e = s0 + stride;
                const uint64_t eh = (e + 15) & ~(uint64_t)15, w0 = eh - block_size;
                const uint32_t p = (uint32_t)(eh - e), a = (uint32_t)(s0 & 15);
                // front: G_(b-1) below s, through Z_(W - 16); head: from s on
                // (none if s is aligned), through Z_W; neither: nothing
                const bool front = w0 < s0;
                const v4u m = front ? win_keep<false>(gp, a) : win_keep<true>(gp, (w0 > s0 && a) ? a : 16u);
                uint32_t h = win_gran(0, m);
                if (stride > block_size) { // gap granules [ceil16(s), w0)
                    for (uint64_t c = (s0 + 15) & ~(uint64_t)15; c < w0; c += 16)
                        h = win_gran(h, *reinterpret_cast<const v4u *>((uintptr_t)c));
                }
                const uint32_t x = o.res ^ win_gran(0, win_keep<true>(og, 16 - p)) ^
                                   win_apply(s_winimg + 4 * 256 + (front ? kWinNib : 0), h);
                out[b] = win_apply(s_winimg + 4 * 256 + (2 + p) * kWinNib, x);
            }
            o.res_base += n;
            o.nres = 0;
        }
    };
    auto win_rec = [&](const uint32_t (&s)[4]) __attribute__((always_inline)) {
        if constexpr (WIN) {
            const int r = lane - (int)o.nres; // the group's blocks go to lanes nres .. nres + NB - 1
            if constexpr (G == 64)
                o.res = r == 0 ? (s[0] ^ s[1] ^ s[2] ^ s[3]) : o.res;
            else if constexpr (G == 32)
                o.res = r == 0 ? (s[0] ^ s[1]) : (r == 1 ? (s[2] ^ s[3]) : o.res);
            else
                o.res = r == 0 ? s[0] : (r == 1 ? s[1] : (r == 2 ? s[2] : (r == 3 ? s[3] : o.res)));
            o.nres += NB;
            if (o.nres == 64)
                win_flush(64);
        } else {
            rec(s);
        }
    };
    // each block's last granule G (the last lane of its group's piece of the
    // last row) into the slots of the blocks recorded next
    auto keep_last = [&](const v4u &x) __attribute__((always_inline)) {
        if constexpr (WIN) {
            if (lane % G == G - 1)
                s_wing[wave][o.nres + lane / G] = x;
        }
    };
    if constexpr (WIN) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            carry[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)cload[k]);
    }
    if (PIPE) {
        // one chunk == one block group (host-checked cps == 1): the fold and
        // row reduction of group q-1 are computed in the same straight-line
        // block as the hash of group q (independent chains the scheduler can
        // interleave); only the result bookkeeping waits behind a branch
        bool have = false;
        auto step = [&](const v4u (&X)[CH]) {
            uint32_t s[4];
            row_totals(fold_lane<G, NIB>(u, col, cb), s);
            uint32_t un = 0;
#pragma unroll
            for (int k = 0; k < CH - 1; k++)
                un = piece<false>(un, X[k], L);
            un = piece_end<NIB, false>(un, X[CH - 1], L);
            if constexpr (WIN) {
                // one block group per chunk (cps == 1): record the previous
                // group (which may store 64 CRCs), then keep this one's granules
                if (have)
                    win_rec(s);
                keep_last(X[CH - 1]);
            } else {
                if (have)
                    rec(s);
            }
            have = true;
            u = un;
        };
        for (; q + NBUF <= nq; q += NBUF) {
            const uint32_t peer = post_progress<PRIO_MODE, NW>(q, wave, lane);
#pragma unroll
            for (int j = 0; j < NBUF; j++) {
                load_chunk<CH, RB, AUX>(buf[(j + NBUF - 1) % NBUF], pp, span, voff);
                advance();
                __builtin_amdgcn_sched_barrier(0);
                step(buf[j]);
            }
            set_priority<PRIO_MODE, NW>(peer, q, lane);
        }
#pragma unroll
        for (int j = 0; j < NBUF - 1; j++) {
            if (q + j >= nq)
                break;
            step(buf[j]);
        }
        uint32_t s[4];
        row_totals(fold_lane<G, NIB>(u, col, cb), s);
        win_rec(s);
    } else {
        // hq: the chunk's index in the wave's stream (SPLIT: its last chunk
        // may end a part of a block)
        auto hash = [&](const v4u (&X)[CH], uint32_t hq) {
            const bool bend = cq + 1 == cpb;
#pragma unroll
            for (int k = 0; k < CH - 1; k++)
                u = piece<false>(u, X[k], L);
            if (!bend && !(SPLIT && hq + 1 == nq)) {
                u = piece<false>(u, X[CH - 1], L);
                cq++;
                return;
            }
            u = piece_end<NIB, false>(u, X[CH - 1], L);
            uint32_t s[4];
            row_totals(fold_lane<G, NIB>(u, col, cb), s);
            if constexpr (WIN) {
                keep_last(X[CH - 1]);
                win_rec(s);
            } else if (!SPLIT || (bend && pu == 0)) {
                rec(s);
            } else {
                // a part: chunks [pu, cq] of block hb, moved to the block end;
                // MERGE: into the wave's slot (first part 0, last part 1)
                const uint32_t d = (cpb - 1 - cq) * (uint32_t)(CH * RB);
                const uint32_t v = zshift_lds(s[0] ^ s[1] ^ s[2] ^ s[3], d, lane);
                if (lane == 0) {
                    if constexpr (MERGE) {
                        uint32_t *sl = s_part[wave][nparts];
                        sl[0] = (uint32_t)hb;
                        sl[1] = v;
                        sl[2] = (cq + 1 - pu) / cps;
                    } else {
                        finish_shared(acc, out, hb, v, (cq + 1 - pu) / cps, S);
                    }
                }
                nparts++;
            }
            u = 0;
            cq = 0;
            pu = 0;
            hb++;
        };
        for (; q + NBUF <= nq; q += NBUF) {
            const uint32_t peer = post_progress<PRIO_MODE, NW>(q, wave, lane);
#pragma unroll
            for (int j = 0; j < NBUF; j++) {
                load_chunk<CH, RB, AUX>(buf[(j + NBUF - 1) % NBUF], pp, span, voff);
                advance();
                __builtin_amdgcn_sched_barrier(0);
                hash(buf[j], q + j);
            }
            set_priority<PRIO_MODE, NW>(peer, q, lane);
        }
        // tail: the remaining nq - q < NBUF chunks are already in buf[0..]
#pragma unroll
        for (int j = 0; j < NBUF - 1; j++) {
            if (q + j >= nq)
                break;
            hash(buf[j], q + j);
        }
    }
    if constexpr (WIN) {
        if (o.nres)
            win_flush(o.nres);
    } else if (o.nres && lane < (int)o.nres) {
        out[o.res_base + lane] = o.res;
    }
#ifdef PRISKV_CRC_COVERAGE
    if (lane == 0 && wid < (uint64_t)kCovWaves) {
        uint32_t xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
        g_wave_t[wid][0] = (unsigned long long)xcc | (wid << 8);
        g_wave_t[wid][1] = ng;
        g_wave_t[wid][2] = t_start;
        g_wave_t[wid][3] = __builtin_amdgcn_s_memrealtime();
    }
#endif
    if constexpr (MERGE) {
        // the workgroup's parts (lane 2w + k of wave 0: wave w's slot k),
        // grouped by block; the first lane of each group sends the group's
        // share through finish_shared, all groups' atomics in parallel --
        // one atomic pair per block and workgroup instead of one per wave (a
        // lone large block has a part in every wave), and no serial chain
        // when a workgroup's parts belong to several blocks
        __syncthreads();
        if (wave != 0)
            return;
        const uint32_t bx = lane < 2 * kWaves ? s_part[lane >> 1][lane & 1][0] : kPartNone;
        const uint32_t bv = lane < 2 * kWaves ? s_part[lane >> 1][lane & 1][1] : 0u;
        const uint32_t bn = lane < 2 * kWaves ? s_part[lane >> 1][lane & 1][2] : 0u;
        uint32_t gv = 0, gn = 0;
        bool lead = bx != kPartNone;
#pragma unroll
        for (int m = 0; m < 2 * kWaves; m++) {
            const uint32_t xm = (uint32_t)__builtin_amdgcn_readlane((int)bx, m);
            const uint32_t vm = (uint32_t)__builtin_amdgcn_readlane((int)bv, m);
            const uint32_t nm = (uint32_t)__builtin_amdgcn_readlane((int)bn, m);
            if (xm == bx) {
                gv ^= vm;
                gn += nm;
                lead = lead && m >= lane;
            }
        }
        if (lead)
            finish_shared(acc, out, bx, gv, gn, S);
    }
}

// ---------------------------------------------------------------------------
// Read roof of the rows kernel's access pattern (priskv_crc_read_roof_dev, a
// diagnostic): G = 64, the same per-wave ranges (wave_range, XCD weights),
// chunk loads (load_chunk: CH rows of 1 KiB, nt) and loop shape as
// crc_rows_kernel, but no LDS tables and no hashing: each chunk is XORed into
// a register.  The host launches it in the CRC plan's own pipeline depth and
// occupancy (variant 0) or in other depths and occupancies (variants 1-6) and
// with the CRC kernels' progress priority (PRIO, variants 7-8), so
// that the best of them is what HBM gives this pattern on this box and this
// allocation: the measured roof the CRC kernel is compared with (bench.py
// roofline.measured_peak).  Wave w stores the XOR of all its words in
// out[w] (plain stores, one slot per wave: no atomics), so the loads cannot
// be dropped and the XOR of the sink is the XOR of the batch's words.  The
// CRC kernel's split mode is mirrored by passing units as blocks, and its
// block-cyclic tiles of `tile` blocks (batches of >= 64 GiB) by the same
// tile order.  stride > 0: the window mode's pattern (odd block sizes): block
// b's reads are the block_size-byte window ending at the first 16-B boundary
// at or after base + (b + 1) stride, as crc_rows_kernel's WIN reads them
// (no tiles there).
// ---------------------------------------------------------------------------
template <int CH, int NBUF, int AUX, int PRIO = 0>
__global__ __launch_bounds__(kThreads, rows_min_wg(CH, NBUF)) void crc_read_roof_kernel(
    const uint8_t *__restrict__ base, uint64_t nblocks, uint32_t block_size, uint32_t *__restrict__ out, uint32_t xw,
    uint32_t tile, uint32_t stride)
{
    constexpr int RB = 1024;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if constexpr (PRIO != 0) {
        init_progress<PRIO>();
        __syncthreads();
    }
    const uint64_t W = (uint64_t)gridDim.x * kWaves;
    const uint64_t wid = (uint64_t)blockIdx.x * kWaves + wave;
    const uint32_t T = __builtin_amdgcn_readfirstlane(tile); // block-cyclic tiles, as crc_rows_kernel's
    uint64_t g0, ng;
    if (T) {
        const uint64_t ntiles = (nblocks + T - 1) / T;
        const uint64_t mine = ntiles > wid ? (ntiles - 1 - wid) / W + 1 : 0;
        const uint64_t last = wid + (mine - 1) * W;
        g0 = uniform64(wid * T);
        ng = mine ? (mine - 1) * T + (last + 1 == ntiles ? nblocks - last * T : T) : 0;
    } else {
        wave_range(nblocks, W, wid, xw, g0, ng);
    }
    const uint32_t cps = block_size / (CH * RB);
    const uint32_t nq = __builtin_amdgcn_readfirstlane((uint32_t)ng * cps); // < 2^31: host-checked
    const uint32_t voff = (uint32_t)lane * 16;
    const uint32_t St = __builtin_amdgcn_readfirstlane(stride);
    uint64_t gb = g0; // (St: the block of the chunk at pp)
    auto winp = [&](uint64_t b) { // St: block b's window
        return reinterpret_cast<const uint8_t *>(
            (uintptr_t)uniform64((((uint64_t)(uintptr_t)base + (b + 1) * St + 15) & ~(uint64_t)15) - block_size));
    };
    const uint8_t *pp = St ? winp(g0) : base + g0 * (uint64_t)block_size;
    const uint64_t tjump = T ? (W - 1) * (uint64_t)T * block_size : 0; // tile end -> this wave's next tile
    uint32_t pq = 0, pc = 0, pg = 0;
    auto advance = [&]() { // consecutive chunks inside a tile (or the wave's range)
        if (pq + 1 < nq) {
            pq++;
            if (St) {
                if (++pc == cps) {
                    pc = 0;
                    pp = winp(++gb);
                } else {
                    pp += CH * RB;
                }
                return;
            }
            pp += CH * RB;
            if (T && ++pc == cps) {
                pc = 0;
                if (++pg == T) {
                    pg = 0;
                    pp += tjump;
                }
            }
        }
    };
    uint32_t acc = 0, q = 0;
    if (nq) {
        v4u buf[NBUF][CH];
#pragma unroll
        for (int j = 0; j < NBUF - 1; j++) {
            load_chunk<CH, RB, AUX>(buf[j], pp, CH * RB, voff);
            advance();
        }
        for (; q + NBUF <= nq; q += NBUF) {
            const uint32_t peer = post_progress<PRIO>(q, wave, lane);
#pragma unroll
            for (int j = 0; j < NBUF; j++) {
                load_chunk<CH, RB, AUX>(buf[(j + NBUF - 1) % NBUF], pp, CH * RB, voff);
                advance();
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < CH; k++)
                    acc ^= buf[j][k].x ^ buf[j][k].y ^ buf[j][k].z ^ buf[j][k].w;
            }
            set_priority<PRIO>(peer, q, lane);
        }
#pragma unroll
        for (int j = 0; j < NBUF - 1; j++) {
            if (q + j >= nq)
                break;
#pragma unroll
            for (int k = 0; k < CH; k++)
                acc ^= buf[j][k].x ^ buf[j][k].y ^ buf[j][k].z ^ buf[j][k].w;
        }
    }
    acc = wave_xor(acc);
    if (lane == 0) // every launched wave writes its slot (0 when it read nothing)
        out[wid] = acc;
}

// ---------------------------------------------------------------------------
// sub-KiB power-of-two blocks (16..512 B): G = block/16 lanes per block, so a
// 1 KiB row holds 64/G whole blocks and row r is simply base + r*1024.  No
// row gap; per-lane fold over Z_(16(G-1-l%G)); XOR within G-lane groups (DPP
// quad steps for G <= 4, then shuffles).  Waves own contiguous row ranges and
// pipeline chunks of CH rows NBUF deep like the rows kernel.  The host
// launches it on whole rows only (nblocks a multiple of 64/G); a ragged tail
// goes to the generic kernel.
// ---------------------------------------------------------------------------
template <int G>
__device__ __forceinline__ uint32_t group_total(uint32_t v)
{
    if (G >= 2)
        v = dpp_xor(v, 0);
    if (G >= 4)
        v = dpp_xor(v, 1);
#pragma unroll
    for (int m = 4; m < G; m <<= 1)
        v ^= (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}

// Byte-table fold of the sub-KiB kernel (OPT bit 1, G = 2..16).  Every lane's
// piece ends its block, so every piece pays a fold: Z_(4 + 16(G-1-c)) applied
// to the pre-step register x.  That map is linear, so it is four lookups, one
// per byte j of x, in per-column byte tables F_j[b][c] = Z_(4+16(G-1-c))(b <<
// 8j) -- the same form as a main table step (one v_perm address + one
// ds_read_b32 per byte), against eight nibble lookups with shift/mask/add
// addressing.  The tables sit in the free B half of the 64 KiB main image
// (the sub-KiB kernel never uses set B: one row per block), 32 words per byte
// value b, laid out so the 32 lanes of a ds_read half hit 32 distinct banks
// in every lookup whatever the data:
//   G <= 8: h = (lane & 31) / G, lookup i reads byte j = (i + h) & 3 from
//           copy h >> 2 (8/G copies): word b*64 + 32 + (h>>2)*4G + j*G + c;
//   G = 16: the two lanes per column in a half (h = 0, 1) read bytes of
//           opposite parity: lookup i reads byte j = 2(i>>1) + ((i+h) & 1),
//           tables j < 2 at b*64 + 32 + 16(j&1) + c, tables j >= 2 the same
//           in a second 64 KiB region (v_perm puts 1 into address byte 2).
// 64 KiB of LDS for G <= 8 (the image goes into s_tab, as the main image),
// 128 KiB for G = 16 (s_small, referenced only by the G = 16 kernels, so the
// G <= 8 kernels reserve 64 KiB and two 8-wave workgroups fit a CU).
__shared__ __attribute__((aligned(16))) uint32_t s_small[2 * kLdsWords];

template <int G>
__device__ __forceinline__ uint32_t *small_lds()
{
    if constexpr (G == 16)
        return s_small;
    else
        return s_tab;
}

struct FoldConst {
    uint32_t c;              // byte i: column byte of lookup i (G = 16: bytes 0, 1 + 0x01 in byte 2)
    uint32_t s0, s1, s2, s3; // v_perm selectors of lookup i
};

template <int G>
__device__ __forceinline__ FoldConst fold_const(int lane)
{
    static_assert(G >= 2 && G <= 16, "byte fold: G = 2..16");
    FoldConst F;
    const uint32_t h = (uint32_t)(lane & 31) / G, cc = (uint32_t)lane % G;
    uint32_t c = 0, s[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (G == 16) {
            const uint32_t j = 2u * (i >> 1) + ((i + h) & 1u);
            const uint32_t e = 16u * (j & 1u) + cc;
            c |= (128u + 4u * e) << (8 * (i & 1));
            // byte0 <- c byte (i & 1), byte1 <- x byte j, byte2 <- c byte 2 (= 1) for j >= 2, byte3 <- 0
            s[i] = 0x0c000000u | ((i >= 2 ? 2u : 0x0cu) << 16) | ((4u + j) << 8) | (uint32_t)(i & 1);
        } else {
            const uint32_t j = (i + h) & 3u;
            const uint32_t e = (h >> 2) * 4u * G + j * G + cc;
            c |= (128u + 4u * e) << (8 * i);
            s[i] = 0x0c0c0000u | ((4u + j) << 8) | (uint32_t)i;
        }
    }
    if (G == 16)
        c |= 1u << 16;
    F.c = c;
    F.s0 = s[0];
    F.s1 = s[1];
    F.s2 = s[2];
    F.s3 = s[3];
    return F;
}

// the main table step on the sub-KiB image (set A only)
template <int G>
__device__ __forceinline__ uint32_t zstep_small(uint32_t x, const LaneConst &L)
{
    const char *t = reinterpret_cast<const char *>(small_lds<G>());
    const uint32_t r0 = *reinterpret_cast<const uint32_t *>(t + __builtin_amdgcn_perm(x, L.c, L.s0));
    const uint32_t r1 = *reinterpret_cast<const uint32_t *>(t + __builtin_amdgcn_perm(x, L.c, L.s1));
    const uint32_t r2 = *reinterpret_cast<const uint32_t *>(t + __builtin_amdgcn_perm(x, L.c, L.s2));
    const uint32_t r3 = *reinterpret_cast<const uint32_t *>(t + __builtin_amdgcn_perm(x, L.c, L.s3));
    return __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_bitop3_b32(r0, r1, r2, 0x96), r3, 0u, 0x96);
}

// x -> Z_(4 + 16(G-1-c))(x) through the byte fold tables (in the B half of
// s_tab for G <= 8, in s_small for G = 16)
template <int G>
__device__ __forceinline__ uint32_t byte_fold(uint32_t x, const FoldConst &F)
{
    const char *t = reinterpret_cast<const char *>(small_lds<G>());
    const uint32_t r0 = *reinterpret_cast<const uint32_t *>(t + __builtin_amdgcn_perm(x, F.c, F.s0));
    const uint32_t r1 = *reinterpret_cast<const uint32_t *>(t + __builtin_amdgcn_perm(x, F.c, F.s1));
    const uint32_t r2 = *reinterpret_cast<const uint32_t *>(t + __builtin_amdgcn_perm(x, F.c, F.s2));
    const uint32_t r3 = *reinterpret_cast<const uint32_t *>(t + __builtin_amdgcn_perm(x, F.c, F.s3));
    return __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_bitop3_b32(r0, r1, r2, 0x96), r3, 0u, 0x96);
}

// XOR of a G-lane group, correct in the group's FIRST lane only (the lane
// that stores): quad DPP steps, then row rotations (no ds_bpermute).  G = 8:
// row_ror:12 brings lane l + 4 to lane l, so lanes 0 and 8 add the other
// quad of their group (other lanes mix in the next group's quad); G = 16:
// rotations by 4 and 8 give every lane the row total.
template <int G>
__device__ __forceinline__ uint32_t group_total_first(uint32_t v)
{
    if (G >= 2)
        v = dpp_xor(v, 0);
    if (G >= 4)
        v = dpp_xor(v, 1);
    if (G == 8)
        v ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x12C, 0xF, 0xF, false); // row_ror:12
    if (G >= 16) {
        v = dpp_xor(v, 2);
        v = dpp_xor(v, 3);
    }
    return v;
}

// OPT bit 0: nibble-table fold (G >= 2; foldG = the 8*16*32-word image)
// OPT bit 1: byte-table fold (G = 2..16; lds_image = the sub-KiB image of
//            prv_small_image, foldG unused)
// OPT bit 2: the first chunks are requested before the LDS tables are loaded
// bits 8-9: progress-priority mode; bit 10: 16 waves
template <int G, int OPT = 0, int CH = 4, int NBUF = 2>
__global__ __launch_bounds__(64 * ext_waves(OPT), 16 / ext_waves(OPT)) void crc_small_kernel(
    const uint8_t *__restrict__ base, uint64_t nrows, const uint32_t *__restrict__ lds_image,
    const uint32_t *__restrict__ foldG, uint32_t *__restrict__ out)
{
    constexpr uint32_t kPerRow = 64 / G;
    constexpr bool BF = (OPT & 2) != 0 && G >= 2 && G <= 16;
    constexpr bool NIB = (OPT & 1) != 0 && G > 1 && !BF;
    constexpr int PRIO_MODE = (OPT >> 8) & 3;
    constexpr int NW = ext_waves(OPT);
    constexpr bool EARLY = (OPT & 4) != 0;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const LaneConst L = lane_const(lane);
    uint32_t col[32];
    // the LDS tables: every wave loads its share, before any may leave
    auto tables = [&]() __attribute__((always_inline)) {
        if constexpr (BF) {
            copy_to_lds(lds_image, small_lds<G>(), (G == 16 ? 2 : 1) * kLdsWords / 4);
        } else {
            load_lds_image(lds_image);
        }
        if constexpr (BF) {
        } else if constexpr (NIB) {
            load_nib_image<32>(foldG);
        } else {
#pragma unroll
            for (int i = 0; i < 32; i++)
                col[i] = foldG[i * 64 + lane];
        }
        init_progress<PRIO_MODE, NW>();
        lds_dma_landed();
        __syncthreads();
    };
    if constexpr (!EARLY)
        tables();

    const uint64_t W = (uint64_t)gridDim.x * NW;
    const uint64_t wid = (uint64_t)blockIdx.x * NW + wave;
    const uint64_t r0 = uniform64(nrows * wid / W);
    const uint64_t nr = nrows * (wid + 1) / W - r0;
    if (!EARLY && nr == 0)
        return;
    const uint32_t nq = __builtin_amdgcn_readfirstlane((uint32_t)((nr + CH - 1) / CH)); // chunks
    const uint32_t rows_last = __builtin_amdgcn_readfirstlane((uint32_t)(nr - (uint64_t)(nq - 1) * CH));
    const uint32_t voff = (uint32_t)lane * 16;
    const uint8_t *wp = base + r0 * PRV_ROW_BYTES;
    // the last chunk may hold fewer than CH rows: its loads are clamped to
    // the wave's last row (re-reads), and only real rows are stored
    auto load = [&](v4u (&X)[CH], uint32_t q) {
        q = q < nq ? q : nq - 1;
        const uint32_t rows = (q + 1 == nq) ? rows_last : CH;
        const __amdgpu_buffer_rsrc_t r = uniform_rsrc(wp + (uint64_t)q * CH * PRV_ROW_BYTES, rows * PRV_ROW_BYTES);
#pragma unroll
        for (int k = 0; k < CH; k++) {
            const uint32_t kk = (uint32_t)k < rows ? (uint32_t)k : rows - 1;
            X[k] = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(r, (int)(voff + kk * PRV_ROW_BYTES),
                                                                                 0, 2));
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    [[maybe_unused]] FoldConst F;
    if constexpr (BF)
        F = fold_const<G>(lane);
    auto hash = [&](const v4u (&X)[CH], uint32_t q) {
        const uint32_t rows = (q + 1 == nq) ? rows_last : CH;
        uint32_t c[CH];
#pragma unroll
        for (int k = 0; k < CH; k++) {
            if constexpr (BF) {
                uint32_t u = zstep_small<G>(X[k].x, L);
                u = zstep_small<G>(u ^ X[k].y, L);
                u = zstep_small<G>(u ^ X[k].z, L);
                c[k] = group_total_first<G>(byte_fold<G>(u ^ X[k].w, F));
            } else {
                c[k] = group_total<G>(G == 1 ? piece<true>(0u, X[k], L)
                                             : (NIB ? nib_fold<32>(piece_pre(0u, X[k], L), 4u * (uint32_t)(lane & 31))
                                                    : bitmat(piece<true>(0u, X[k], L), col)));
            }
        }
        uint32_t *o = out + (r0 + (uint64_t)q * CH) * kPerRow + lane / G;
#pragma unroll
        for (int k = 0; k < CH; k++)
            if ((uint32_t)k < rows && (lane % G) == 0)
                o[k * kPerRow] = c[k];
    };
    v4u buf[NBUF][CH];
    // EARLY (OPT bit 2): the first chunks are requested before the tables
    if (!EARLY || nr) {
#pragma unroll
        for (int j = 0; j < NBUF - 1; j++)
            load(buf[j], j);
    }
    if constexpr (EARLY) {
        tables();
        if (nr == 0)
            return;
    }
    uint32_t q = 0;
    for (; q + NBUF <= nq; q += NBUF) {
        const uint32_t peer = post_progress<PRIO_MODE, NW>(q, wave, lane);
#pragma unroll
        for (int j = 0; j < NBUF; j++) {
            load(buf[(j + NBUF - 1) % NBUF], q + j + NBUF - 1);
            __builtin_amdgcn_sched_barrier(0);
            hash(buf[j], q + j);
        }
        set_priority<PRIO_MODE, NW>(peer, q, lane);
    }
#pragma unroll
    for (int j = 0; j < NBUF - 1; j++) {
        if (q + j >= nq)
            break;
        hash(buf[j], q + j);
    }
}

// ---------------------------------------------------------------------------
// uniform-stride blocks of any size B >= 16 at any base alignment
// (crc_stride_kernel): block i = [base + i*B, base + (i+1)*B).  PrisKV's -v
// accepts any value-block size up to 1 MiB (server/server.c:236-244; only a
// memfile insists on a power of two, server/memory.c:413), so sizes such as
// 4100 or 1000 B are legal server configurations.
//
// The rows kernel's scheme with the block grid shifted to each block's END:
// G lanes per block, rows of RB = 16G bytes, R = ceil(B / RB) rows per block,
// and row r of a block covers its bytes [r*RB - F, (r+1)*RB - F), F = R*RB - B
// < RB.  Lane c's 16-B window in row r starts at r*RB + 16c - F, so the last
// lane of the last row ends exactly at the block end: the fold is the rows
// kernel's (Z_(4 + 16(G-1-c)) per lane, then the group XOR), with no trailing
// pad to undo.  Only row 0 reaches in front of the block, by F bytes: zero
// bytes in front do not change the CRC (init 0), so lanes whose window lies
// wholly in front load nothing (voffset 0x80000000: out of range, returns 0,
// no memory access), and the one lane whose window holds the block's first
// byte (c* = F / 16, d = F % 16 > 0) loads the block's first 16 bytes and
// shifts them up by d bytes in registers.  The geometry is the same for every
// block, so all of this is per-lane constants.  Windows start at any byte:
// raw buffer loads at unaligned offsets return the bytes at that offset
// (tools/unaligned_probe: full rate at 4-byte alignment, 5.3 of 7.0 TB/s at
// odd bytes), and block sizes or bases that are not multiples of 4 take the
// ODD variant (aligned loads + funnel shifts, below).  Every load stays inside
// its block (ODD: inside the dwords that hold it), and the wave's descriptor
// ends at the end of its range, so lane groups past it read zeros; their CRCs
// are not stored.
//
// A wave owns a contiguous range of blocks.  For G >= 16 each of its NB =
// 64/G lane groups walks one contiguous run of it, block after block; for G <
// 16 the groups take adjacent blocks side by side.  The wave's rows form one
// stream -- (block g of every lane group, row r) -- loaded CH rows at a time,
// NBUF chunks deep; a chunk may cross from one block into the next, the hash
// side keeps its own (block, row) cursor.  G < 16 only with R = 1 (the set-B
// row jump is built for gaps of 16G - 16 with G = 16, 32, 64).
// Reference semantics: server/crc.c:90-109 per block.
// ---------------------------------------------------------------------------

// x as a 128-bit little-endian value shifted up by d bytes (d wave-uniform,
// 0..15): byte k of the result = byte k - d of x, zeros below d
__device__ __forceinline__ v4u shift_up_bytes(v4u x, uint32_t d)
{
    const uint32_t q = d >> 2, r = 8u * (d & 3u);
    const uint32_t s0 = q == 0 ? x.x : 0u;
    const uint32_t s1 = q == 0 ? x.y : (q == 1 ? x.x : 0u);
    const uint32_t s2 = q == 0 ? x.z : (q == 1 ? x.y : (q == 2 ? x.x : 0u));
    const uint32_t s3 = q == 0 ? x.w : (q == 1 ? x.z : (q == 2 ? x.y : x.x));
    auto fsh = [r](uint32_t hi, uint32_t lo) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (32u - r)); };
    v4u o;
    o.x = s0 << r;
    o.y = fsh(s1, s0);
    o.z = fsh(s2, s1);
    o.w = fsh(s3, s2);
    return o;
}

// BF (G <= 8, so R = 1 and set B is never used): lds_image is the sub-KiB
// byte-fold image (prv_small_image) and the fold takes byte_fold's four
// lookups instead of nib_fold's eight; nib is unused.
// PRIO (progress-priority mode, 0 = off): the kernel runs as one 16-wave
// workgroup per CU instead of two of 8 (the same waves per CU; the LDS tables
// are loaded once per CU and the progress slots fit), and every NBUF chunks
// each wave posts its progress and sets its issue priority (set_priority).
// EARLY: the first chunks are requested before the LDS tables are loaded.
template <int G, int CH, int NBUF, int AUX, bool ODD = false, bool BF = false, int PRIO = 0, bool EARLY = false>
__global__ __launch_bounds__(64 * (PRIO ? 16 : kWaves), PRIO ? 1 : rows_min_wg(CH, NBUF)) void crc_stride_kernel(
    const uint8_t *__restrict__ base, uint64_t nblocks, uint32_t B, uint32_t R,
    const uint32_t *__restrict__ lds_image, const uint32_t *__restrict__ nib, uint32_t *__restrict__ out)
{
    static_assert(!BF || G <= 8, "byte fold in the stride kernel: G <= 8");
    constexpr int NB = 64 / G;     // blocks per group
    constexpr uint32_t RB = 16 * G; // bytes per row of one block
    constexpr int TW = nib_width<G>();
    constexpr int NW = PRIO ? 16 : kWaves;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const LaneConst L = lane_const(lane);
    const uint32_t cb = 4u * (uint32_t)(lane % TW);
    [[maybe_unused]] FoldConst FC;
    if constexpr (BF)
        FC = fold_const<(BF ? G : 2)>(lane);
    // the LDS tables: every wave loads its share, before any may leave
    auto tables = [&]() __attribute__((always_inline)) {
        load_lds_image(lds_image);
        if constexpr (!BF)
            load_nib_image<TW>(nib);
        init_progress<PRIO, NW>();
        lds_dma_landed();
        __syncthreads();
    };
    if constexpr (!EARLY)
        tables();

    const uint64_t W = (uint64_t)gridDim.x * NW;
    const uint64_t wid = (uint64_t)blockIdx.x * NW + wave;
    uint64_t b0, nbw; // the wave's blocks
    wave_range<NW>(nblocks, W, wid, 0u, b0, nbw);
    if (!EARLY && nbw == 0)
        return;
    // Lane group j takes block g*NB + j of the wave's range in step g:
    // adjacent blocks side by side, and the CRC stores stay contiguous.
    // (Lane groups walking runs of consecutive blocks instead re-read fewer
    // shared 16-B lines but measured 1.5-6 % slower: tools/, DESIGN App. A.)
    const uint32_t H = __builtin_amdgcn_readfirstlane((uint32_t)((nbw + NB - 1) / NB));
    const uint32_t nrows = H * R; // < 2^31: host-checked
    const uint32_t nq = (nrows + CH - 1) / CH;

    // per-lane geometry, the same in every block
    const uint32_t c = (uint32_t)lane % G, j = (uint32_t)lane / G;
    const uint32_t F = R * RB - B;      // bytes row 0 reaches in front of the block (< RB)
    const uint32_t cs = F >> 4, d = F & 15u;
    const uint32_t jb = j * B; // lane group j's first block, from the wave's first
    const uint32_t vbase = jb + 16u * c - F; // + srow: row r's window (r >= 1; mod 2^32)
    const uint32_t v0 = c < cs ? 0x80000000u : (c == cs ? jb : vbase);
    const bool part = c == cs && d != 0;

    // One descriptor for the wave's whole range (< 2 GiB: host-checked); the
    // lane groups past the range's end (H*NB > nbw) read zeros and store
    // nothing.  Loader cursor: srow = byte offset of the row's grid line
    // (block g of every lane group: g*B + r*RB), lr = row in block, lleft =
    // rows after it; branch-free, it stays on the wave's last row (re-loads
    // are never hashed).  Row 0 lanes: 0x80000000 + srow stays out of range.
    // ODD (a block size or base that is not a multiple of 4): windows start
    // at odd bytes, and such loads stream at 5.3 instead of 7.0 TB/s
    // (tools/unaligned_probe).  The descriptor then starts at the 4-byte
    // boundary below the range (dl bytes lower) and ends at the one above its
    // end (the dword holding the last byte is mapped: same page), each lane
    // loads its window's aligned dwordx4 and funnel-shifts in the dword after
    // it: the next lane's first dword (DPP wave_shl:1; its window starts 16 B
    // later), or, for a group's last lane and row 0's partial lane, an extra
    // masked dword load.
    const uint8_t *wa = base + b0 * B;
    const uint32_t dl = ODD ? (uint32_t)((uintptr_t)wa & 3u) : 0u;
    const __amdgpu_buffer_rsrc_t rs =
        uniform_rsrc(wa - dl, ODD ? ((uint32_t)(nbw * B) + dl + 3u) & ~3u : (uint32_t)(nbw * B));
    const uint32_t gadv = (uint32_t)NB * B; // grid line step from one block of a lane group to its next
    uint32_t srow = 0, lgo = 0, lr = 0, lleft = nrows - 1;
    // clamp = false where the caller knows the next row exists (the main
    // loop with NBUF = 2): no end test in the row loop
    auto advance = [&](bool clamp) __attribute__((always_inline)) {
        const bool more = !clamp || lleft != 0;
        const bool wrap = more && lr + 1 == R;
        lleft -= more ? 1u : 0u;
        lr = wrap ? 0u : (more ? lr + 1 : lr);
        lgo += wrap ? gadv : 0u;
        srow = wrap ? lgo : (more ? srow + RB : srow);
    };
    // ODD: lanes that take the dword after their window from a load of
    // their own: a group's last lane, and row 0's partial lane (its window
    // starts at the block, 16 - d bytes before the next lane's)
    const bool xlast = ODD && c == G - 1;
    uint32_t E[ODD ? NBUF : 1][ODD ? CH : 1]; // those dwords, per row in flight
    auto load_rows = [&](v4u (&X)[CH], uint32_t (&Ex)[ODD ? CH : 1], bool clamp) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < CH; k++) {
            const uint32_t vo = (lr ? vbase : v0) + srow;
            if constexpr (ODD) {
                const uint32_t va = vo + dl, al = va & ~3u; // out-of-range lanes stay >= 2^31
                X[k] = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)al, 0, AUX));
                const bool xe = xlast || (lr == 0 && part);
                Ex[k] = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(xe ? al + 16u : 0x80000000u), 0, AUX);
            } else {
                X[k] = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)vo, 0, AUX));
            }
            __builtin_amdgcn_sched_barrier(0);
            advance(clamp);
        }
    };

    // hash cursor (block hg of every lane group, row hr) and results: lane t
    // < NB stores lane group t's CRC (G >= 16: from the row totals), lane c
    // = 0 of each group for G < 16.  32-bit indices from the wave's first
    // output (nbw < 2^31).
    uint32_t u = 0, hr = 0, hq = 0, hg = 0;
    // stores through a descriptor over the wave's outputs: lanes that store
    // nothing, and runs past the range's end, get an out-of-range offset
    // (dropped) -- no divergent branch in the row loop
    const __amdgpu_buffer_rsrc_t ro = uniform_rsrc(reinterpret_cast<const uint8_t *>(out + b0), (uint32_t)nbw * 4u);
    const bool sl = G >= 16 ? lane < NB : c == 0;
    // byte offset of the storing lane's first block: G >= 16, lane t < NB
    // stores lane group t's CRC; G < 16, lane c = 0 of group j stores group j's
    const uint32_t kst = sl ? 4u * (G >= 16 ? (uint32_t)lane : j) : 0x80000000u;
    const uint32_t kstep = 4u * NB; // ... and per block of it
    auto emit = [&](uint32_t f) __attribute__((always_inline)) {
        uint32_t v;
        if constexpr (G >= 16) {
            f = dpp_xor(dpp_xor(dpp_xor(dpp_xor(f, 0), 1), 2), 3); // 16-lane row totals
            const uint32_t t0 = (uint32_t)__builtin_amdgcn_readlane((int)f, 0);
            const uint32_t t1 = (uint32_t)__builtin_amdgcn_readlane((int)f, 16);
            const uint32_t t2 = (uint32_t)__builtin_amdgcn_readlane((int)f, 32);
            const uint32_t t3 = (uint32_t)__builtin_amdgcn_readlane((int)f, 48);
            if (G == 64)
                v = t0 ^ t1 ^ t2 ^ t3;
            else if (G == 32)
                v = lane == 0 ? (t0 ^ t1) : (t2 ^ t3);
            else
                v = lane == 0 ? t0 : (lane == 1 ? t1 : (lane == 2 ? t2 : t3));
        } else {
            v = group_total<G>(f);
        }
        __builtin_amdgcn_raw_buffer_store_b32(v, ro, (int)(kst + kstep * hg), 0, 0);
    };
    // one row; GUARD: past the wave's last row (the final chunk's re-loads)
    // nothing happens
    uint32_t hs = 0, hgo = 0; // ODD: the hash side's copy of srow / lgo
    const uint32_t mb = vbase + dl;   // ODD: window start - descriptor start, less the grid offset
    auto hash_row = [&](const v4u &X, uint32_t Ex, bool live) __attribute__((always_inline)) {
        if (live) {
            v4u x = X;
            if constexpr (ODD) {
                // the 16 bytes from the window start: the aligned dwords and
                // the next one, shifted down by m = start mod 4 (lanes whose
                // window lies wholly in front of the block are zeroed below)
                const uint32_t m = ((hr ? mb : (c == cs ? jb + dl : mb)) + hs) & 3u;
                const uint32_t nx = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x.x, 0x130, 0xF, 0xF, false);
                const uint32_t n4 = (xlast || (hr == 0 && part)) ? Ex : nx;
                v4u y;
                y.x = __builtin_amdgcn_alignbyte(x.y, x.x, m);
                y.y = __builtin_amdgcn_alignbyte(x.z, x.y, m);
                y.z = __builtin_amdgcn_alignbyte(x.w, x.z, m);
                y.w = __builtin_amdgcn_alignbyte(n4, x.w, m);
                const bool front = hr == 0 && c < cs;
                x.x = front ? 0u : y.x;
                x.y = front ? 0u : y.y;
                x.z = front ? 0u : y.z;
                x.w = front ? 0u : y.w;
            }
            if (hr == 0 && d != 0) {
                const v4u sx = shift_up_bytes(x, d);
                x = part ? sx : x;
            }
            // hr / hg are wave-uniform: updated without branches (and
            // readfirstlane'd), else hipcc promotes them to per-lane
            // scratch behind a divergent branch
            const bool last = hr + 1 >= R;
            if (!last) {
                u = piece<false>(u, x, L);
            } else {
                if constexpr (BF)
                    emit(byte_fold<G>(piece_pre(u, x, L), FC));
                else
                    emit(nib_fold<TW>(piece_pre(u, x, L), cb));
                u = 0;
            }
            hg = __builtin_amdgcn_readfirstlane(hg + (last ? 1u : 0u));
            hr = __builtin_amdgcn_readfirstlane(last ? 0u : hr + 1);
            if constexpr (ODD) {
                hgo = __builtin_amdgcn_readfirstlane(hgo + (last ? gadv : 0u));
                hs = __builtin_amdgcn_readfirstlane(last ? hgo : hs + RB);
            }
            hq++;
        }
    };

    v4u buf[NBUF][CH];
    if (!EARLY || nbw) {
#pragma unroll
        for (int t = 0; t < NBUF - 1; t++)
            load_rows(buf[t], E[ODD ? t : 0], true);
    }
    if constexpr (EARLY) {
        tables();
        if (nbw == 0)
            return;
    }
    uint32_t q = 0;
    // every chunk of the main loop is whole (the last, possibly partial chunk
    // is always left to the tail)
    for (; q + NBUF < nq; q += NBUF) {
        const uint32_t peer = post_progress<PRIO, NW>(q, wave, lane);
#pragma unroll
        for (int t = 0; t < NBUF; t++) {
            // chunks q + NBUF - 1 + t <= q + 2 NBUF - 2 < nq when NBUF = 2
            load_rows(buf[(t + NBUF - 1) % NBUF], E[ODD ? (t + NBUF - 1) % NBUF : 0], NBUF > 2);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < CH; k++)
                hash_row(buf[t][k], E[ODD ? t : 0][ODD ? k : 0], true);
        }
        set_priority<PRIO, NW>(peer, q, lane);
    }
    // tail: chunks q .. nq - 1 (at most NBUF); q .. q + NBUF - 2 are loaded
#pragma unroll
    for (int t = 0; t < NBUF; t++) {
        if (q + t >= nq)
            break;
        load_rows(buf[(t + NBUF - 1) % NBUF], E[ODD ? (t + NBUF - 1) % NBUF : 0], true); // past nq: re-loads
#pragma unroll
        for (int k = 0; k < CH; k++)
            hash_row(buf[t][k], E[ODD ? t : 0][ODD ? k : 0], hq < nrows);
    }
}

// ---------------------------------------------------------------------------
// per-value extents (priskv_crc32_ranges_dev, unaligned / odd-size blocks,
// the host scrub): one wave per (offset, length), each wave owning a
// contiguous run of extents.
//
// Geometry.  Because init = 0, zero bytes in FRONT of a message do not change
// its CRC; zero bytes AFTER it do, but only by an invertible shift:
// crc(M | 0^p) = Z_p(crc M).  So an extent [off, end) is hashed as the
// 16-B-aligned span [A0, Eu) = [off & ~15, ceil16(end)) with the bytes before
// off and after end zeroed, right-aligned onto NC chunks of CH whole 1 KiB
// rows that END at Eu (leading rows before A0 are virtual zeros), and the
// result is shifted back by p = Eu - end < 16 bytes (Z_-p, 16 x 32 columns
// in LDS).  Every chunk is the same CH-row step as the rows kernel (set B row
// jumps, G = 64 fold), with no per-row branches and no byte-serial tail.
//
// Loads.  Each chunk is one buffer descriptor [rowbase, min(rowbase + CH KiB,
// Eu)); lanes whose 16-B window starts before A0 get voffset 0x80000000.
// Out-of-range buffer loads return 0 without touching memory, so a chunk is
// always exactly CH full-exec loads (a fixed vmcnt per chunk) and no byte
// outside the 16-B windows overlapping the extent is ever read.
//
// Pipeline.  The wave's extents form one flat stream of chunks, loaded NBUF
// deep exactly like the rows kernel (the loader runs NBUF-1 chunks ahead and
// crosses extent boundaries; the next extent's (offset, length) is fetched
// one extent early).  Reference semantics: server/crc.c:90-109 per extent.
// ---------------------------------------------------------------------------
__shared__ __attribute__((aligned(16))) uint32_t s_unshift[16 * 32];
// OPT bit 0 (nibble fold): columns of Z_-p o Z_(256(3-k)), word (4p + k)*32 + j
__shared__ __attribute__((aligned(16))) uint32_t s_rowshift[16 * 4 * 32];

template <int V>
struct IntC { // a compile-time int for generic lambdas
    static constexpr int value = V;
};

struct Ext {
    uint64_t i;        // item index (extent, or segment in the segmented mode)
    uint64_t off, end; // bytes [off, end), relative to the (aligned) base
    uint64_t A0, hi;   // first window; end of loadable bytes (Eu, or A0 if empty)
    int64_t VS;        // start of the first (virtual) row
    uint32_t NC;       // chunks, >= 1
    // segmented mode: extent xi; d whole 2^s-byte segments lie between this
    // segment and the extent's last one (0 for the last itself); split = the
    // extent has more than one segment
    uint64_t xi;
    uint32_t d, s, split;
    uint32_t last; // fused mode: the extent's last segment
};

template <int CH>
__device__ __forceinline__ Ext make_ext(uint64_t i, uint64_t off, uint32_t len)
{
    Ext x;
    x.i = i;
    x.off = off;
    x.end = off + len;
    x.A0 = off & ~(uint64_t)15;
    const uint64_t Eu = (x.end + 15) & ~(uint64_t)15;
    x.hi = len ? Eu : x.A0;
    const uint64_t R = (Eu - x.A0 + PRV_ROW_BYTES - 1) / PRV_ROW_BYTES;
    const uint64_t nc = (R + CH - 1) / CH;
    x.NC = nc ? (uint32_t)nc : 1u;
    x.VS = (int64_t)Eu - (int64_t)x.NC * CH * PRV_ROW_BYTES;
    return x;
}

// zero the bytes of a 16-B window before byte `lo` and from byte `hi` on
// (window-relative; lo <= 0 / hi >= 16 keep everything)
__device__ __forceinline__ v4u mask_window(v4u d, int32_t lo, int32_t hi)
{
    uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int32_t a = lo - 4 * j; // bytes of dword j to clear at its bottom
        const int32_t b = hi - 4 * j; // bytes of dword j to keep
        uint32_t m = a >= 4 ? 0u : (a <= 0 ? ~0u : (0xFFFFFFFFu << (8 * a)));
        m &= b >= 4 ? ~0u : (b <= 0 ? 0u : (0xFFFFFFFFu >> (32 - 8 * b)));
        w[j] &= m;
    }
    return v4u{w[0], w[1], w[2], w[3]};
}

template <int CH, int AUX>
__device__ __forceinline__ void load_ext_chunk(v4u (&X)[CH], const uint8_t *base, const Ext &x, uint32_t c,
                                               int lane)
{
    const int64_t rowbase = x.VS + (int64_t)c * CH * PRV_ROW_BYTES;
    const int64_t room = (int64_t)x.hi - rowbase;
    const uint32_t bytes = room <= 0 ? 0u : (room >= CH * (int64_t)PRV_ROW_BYTES ? CH * PRV_ROW_BYTES : (uint32_t)room);
    const int32_t low = c == 0 ? (int32_t)((int64_t)x.A0 - rowbase) : 0; // first in-range offset
    const __amdgpu_buffer_rsrc_t r = uniform_rsrc(base + rowbase, bytes);
#pragma unroll
    for (int k = 0; k < CH; k++) {
        const int32_t o = k * (int32_t)PRV_ROW_BYTES + 16 * lane;
        const int32_t vo = o >= low ? o : (int32_t)0x80000000;
        X[k] = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(r, vo, 0, AUX));
        __builtin_amdgcn_sched_barrier(0);
    }
}

//
// OPT bit 0: nibble fold.  Lane l's pre-step register is advanced by
// Z_(4 + 16(15 - l%16)) through the G = 16 nibble tables (fold64 then points
// at that 8 KiB image), the four 16-lane rows are XOR-reduced, and row k's
// total still needs Z_(256(3-k)) and the whole CRC Z_-p: both are one
// distributed matrix apply (lane l owns bit l%32 of rows 2(l/32) and
// 2(l/32)+1; unshift then points at the 8 KiB s_rowshift image) and one
// wave XOR -- in place of the 64-VALU bit-matrix, a wave XOR, and a second
// apply + wave XOR for p != 0.
// OPT bit 1: mask only where it can change a byte: the first chunk when the
// extent start is not 16-B aligned, the last chunk when its end is not
// (windows before the start already load as zeros).
// OPT bits 8-9: progress-priority mode (set_priority); progress = items
// the wave's loader has passed (every wave holds the same item count).
// OPT bit 11: byte-balanced split (ext_boundary): seg_prefix then holds the
// per-tile costs of crc_ext_cost_kernel instead of segment prefixes.
// OPT bit 14: per-wave chunk size (many-extents shape).  Before its walk a
// wave sizes its chunks from its own extents (a sample of the first 256):
// the chunks are right-aligned to each extent's end, so an extent of R rows
// hashes ceil(R / C) * C rows, the rest zeros in front.  Bigger chunks keep
// more bytes in flight per wave -- worth 5-8 % on scattered values of 2-4
// blocks -- but hash more zero rows on short extents.  The wave takes C = 8
// when at most 30 % of its hashed rows would be such zero rows, else C = 4
// under the same rule, else the template's CH (tools/ranges_explore,
// profiles/r03/ranges/).
// OPT bit 12 (tools/ranges_explore only): read roof -- the same loads and
// loop, the hash replaced by an XOR of the loaded words.
// OPT bit 2: segmented.  The items are the segments that crc_seg_plan_kernel
// laid out (extent i = m = seg_prefix[i+1] - seg_prefix[i] segments of
// 1 << seg_shift[i] bytes counted from its start, the last one ending at
// the extent's end and r <= 2^s bytes long).  Counted from the start, every
// segment of a 16-B-aligned value is 16-B aligned at both ends except the
// last one's end: no masks and no extra chunk for the alignment window.
// Segment k < m-1 is shifted to the start of the last segment,
// crc -> Z_((m-2-k) << s)(crc), in at most 16 binary steps (distributed
// applies of zpow's columns of Z_(2^k), one wave XOR each) and stored to
// sub[segment]; crc_seg_reduce_kernel finishes the split extents,
// out = Z_r(XOR of the shifted segments) ^ crc(last) (the CRC is linear with
// no affine term).  An extent of one segment is stored to out[] directly.  (Atomic XORs into out[] instead cost up to 2.4x: all segments
// of an extent finish together and serialize on one address.)
template <int CH, int NBUF, int AUX, int OPT = 0>
__global__ __launch_bounds__(64 * ext_waves(OPT), 16 / ext_waves(OPT)) void crc_ranges_kernel(
    const uint8_t *__restrict__ base, uint64_t n, const uint64_t *__restrict__ offsets,
    const uint32_t *__restrict__ lengths, uint64_t shift, uint64_t stride, uint32_t len_const,
    const uint32_t *__restrict__ lds_image, const uint32_t *__restrict__ fold64,
    const uint32_t *__restrict__ unshift, uint32_t *__restrict__ out,
    const uint32_t *__restrict__ seg_prefix, const uint8_t *__restrict__ seg_shift,
    const uint32_t *__restrict__ zpow, uint32_t *__restrict__ sub)
{
    constexpr bool NIB = (OPT & 1) != 0;
    constexpr bool MASK_SKIP = (OPT & 2) != 0;
    constexpr bool SEG = (OPT & 4) != 0;
    constexpr int PRIO_MODE = (OPT >> 8) & 3;
    constexpr int NW = ext_waves(OPT);
    constexpr bool BAL = (OPT & 2048) != 0;
    constexpr bool ROOF = (OPT & 4096) != 0;
    constexpr bool ADAPT = (OPT & 16384) != 0;
    static_assert(!(BAL && SEG), "balanced split: extents, not segments");
    if constexpr (SEG) {
        // the grid is sized for the most segments the plan can produce:
        // workgroups with no segment leave before filling LDS
        const uint64_t nt = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(seg_prefix[n]);
        const uint64_t w = (uint64_t)gridDim.x * NW;
        if (nt * ((uint64_t)blockIdx.x * NW) / w == nt * ((uint64_t)blockIdx.x * NW + NW) / w)
            return;
    }
    load_lds_image(lds_image);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const LaneConst L = lane_const(lane);
    uint32_t col[32];
    if constexpr (NIB) {
        load_nib_image<16>(fold64);
        copy_to_lds(unshift, s_rowshift, 16 * 4 * 32 / 4);
    } else {
        copy_to_lds(unshift, s_unshift, 16 * 32 / 4);
#pragma unroll
        for (int i = 0; i < 32; i++)
            col[i] = fold64[i * 64 + lane];
    }
    init_progress<PRIO_MODE, NW>();
    lds_dma_landed();
    __syncthreads();

    const uint64_t W = (uint64_t)gridDim.x * NW;
    const uint64_t wid = (uint64_t)blockIdx.x * NW + wave;
    const uint64_t NT = SEG ? (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(seg_prefix[n]) : n; // items
    uint64_t e0, e1;
    if constexpr (BAL) { // seg_prefix = the per-tile costs of crc_ext_cost_kernel
        const ExtTiles T = ext_tiles(seg_prefix, (n + kExtTile - 1) / kExtTile, lane);
        e0 = ext_boundary(T, lengths, n, T.total * wid / W, lane);
        e1 = ext_boundary(T, lengths, n, T.total * (wid + 1) / W, lane);
    } else {
        e0 = uniform64(NT * wid / W);
        e1 = uniform64(NT * (wid + 1) / W);
    }
    if (e0 >= e1)
        return;
    auto meta_off = [&](uint64_t i) {
        return uniform64((offsets ? offsets[i] : i * stride) + shift);
    };
    auto meta_len = [&](uint64_t i) {
        return offsets ? (uint32_t)__builtin_amdgcn_readfirstlane(lengths[i]) : len_const;
    };
    // SEG: cursor on segment ck of extent ci (cm segments of 1 << cs bytes
    // counted from coff; the last one ends at cend and may be shorter)
    uint64_t ci = 0, coff = 0, cend = 0;
    uint32_t ck = 0, cm = 1, cs = 0;
    auto seg_load = [&](uint64_t i) {
        ci = i;
        const uint32_t p0 = (uint32_t)__builtin_amdgcn_readfirstlane(seg_prefix[i]);
        cm = (uint32_t)__builtin_amdgcn_readfirstlane(seg_prefix[i + 1]) - p0;
        cs = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)seg_shift[i]);
        coff = meta_off(i);
        cend = coff + meta_len(i);
    };
    auto seg_item = [&](uint64_t &o, uint32_t &l) {
        const uint64_t st = coff + ((uint64_t)ck << cs);
        const uint64_t en = ck + 1 == cm ? cend : st + (1ull << cs);
        o = st;
        l = (uint32_t)(en - st);
    };
    auto seg_step = [&]() {
        if (++ck == cm) {
            ck = 0;
            if (ci + 1 < n)
                seg_load(ci + 1);
        }
    };
    // the item after the one the loader is on: (noff, nlen) and, segmented,
    // its extent / distance / size (nseg)
    Ext nseg{};
    auto seg_tag = [&](Ext &x) {
        x.xi = ci;
        x.d = ck + 1 < cm ? cm - 2 - ck : 0u; // whole segments between it and the last one
        x.s = cs;
        x.split = cm > 1;
    };
    auto next_meta = [&](uint64_t i, uint64_t &o, uint32_t &l) {
        if constexpr (SEG) {
            seg_step();
            seg_item(o, l);
            seg_tag(nseg);
        } else {
            o = meta_off(i);
            l = meta_len(i);
        }
    };

    auto walk = [&](auto chunk_rows) {
        constexpr int C = decltype(chunk_rows)::value;
        uint64_t o0;
        uint32_t l0;
        if constexpr (SEG) {
            // the extent holding segment e0: last i with seg_prefix[i] <= e0.
            // 64-way search: each round the lanes read 64 evenly spaced prefix
            // entries (the prefix is strictly increasing) and the ballot's count
            // narrows [lo, hi) 64x -- 3 rounds for 16384 extents instead of 14
            // dependent scalar loads
            uint64_t lo = 0, hi = n;
            while (hi - lo > 1) {
                const uint64_t step = (hi - lo + 63) / 64;
                const uint64_t idx = lo + (uint64_t)lane * step;
                const bool le = idx < hi && (uint64_t)seg_prefix[idx] <= e0;
                const uint64_t k = (uint64_t)__builtin_popcountll(__ballot(le)); // >= 1: prefix[lo] <= e0
                lo = uniform64(lo + (k - 1) * step);
                const uint64_t nh = lo + step;
                hi = uniform64(nh < hi ? nh : hi);
            }
            seg_load(lo);
            ck = (uint32_t)(e0 - (uint32_t)__builtin_amdgcn_readfirstlane(seg_prefix[lo]));
            seg_item(o0, l0);
        } else {
            o0 = meta_off(e0);
            l0 = meta_len(e0);
        }
        // loader cursor: chunk lc of item lx; (noff, nlen) = item lx.i + 1
        Ext lx = make_ext<C>(e0, o0, l0);
        if constexpr (SEG)
            seg_tag(lx);
        uint32_t lc = 0;
        uint64_t noff = 0;
        uint32_t nlen = 0;
        if (e0 + 1 < e1)
            next_meta(e0 + 1, noff, nlen);
        auto advance = [&]() {
            if (lc + 1 < lx.NC) {
                lc++;
            } else if (lx.i + 1 < e1) { // else: stay on the last chunk (re-loads are harmless)
                lx = make_ext<C>(lx.i + 1, noff, nlen);
                if constexpr (SEG) {
                    lx.xi = nseg.xi;
                    lx.d = nseg.d;
                    lx.s = nseg.s;
                    lx.split = nseg.split;
                }
                lc = 0;
                if (lx.i + 1 < e1)
                    next_meta(lx.i + 1, noff, nlen);
            }
        };

        uint32_t u = 0;
        // hash chunk c of extent x; true after the wave's final chunk
        auto hash = [&](v4u (&X)[C], const Ext &x, uint32_t c) -> bool {
            const bool last = c + 1 == x.NC;
            const int64_t rowbase = x.VS + (int64_t)c * C * PRV_ROW_BYTES;
            if constexpr (ROOF) {
    #pragma unroll
                for (int k = 0; k < C; k++)
                    u ^= X[k].x ^ X[k].y ^ X[k].z ^ X[k].w;
                if (!last)
                    return false;
                const uint32_t v = wave_xor(u);
                u = 0;
                if (lane == 0)
                    out[x.i] = v;
                return x.i + 1 == e1;
            }
            if (c == 0 && (!MASK_SKIP || (x.off & 15))) {
                const int32_t lo = (int32_t)((int64_t)x.off - rowbase) - 16 * lane;
    #pragma unroll
                for (int k = 0; k < C; k++)
                    X[k] = mask_window(X[k], lo - k * (int32_t)PRV_ROW_BYTES, 16);
            }
            const int32_t p = (int32_t)(((x.end + 15) & ~(uint64_t)15) - x.end); // pad bytes after end
            if (last && (!MASK_SKIP || p))
                X[C - 1] = mask_window(X[C - 1], 0, lane == 63 ? 16 - p : 16);
    #pragma unroll
            for (int k = 0; k < C - 1; k++)
                u = piece<false>(u, X[k], L);
            if (!last) {
                u = piece<false>(u, X[C - 1], L);
                return false;
            }
            uint32_t crc;
            if constexpr (NIB) {
                u = piece_pre(u, X[C - 1], L);
                uint32_t s4[4];
                row_totals(nib_fold<16>(u, 4u * (uint32_t)(lane & 15)), s4);
                const uint32_t sa = lane < 32 ? s4[0] : s4[2];
                const uint32_t sb = lane < 32 ? s4[1] : s4[3];
                const uint32_t j = (uint32_t)lane & 31;
                const uint32_t *t = s_rowshift + (uint32_t)p * 128 + (lane < 32 ? 0 : 64) + j;
                const uint32_t va = ((sa >> j) & 1u) ? t[0] : 0u;
                const uint32_t vb = ((sb >> j) & 1u) ? t[32] : 0u;
                crc = wave_xor(va ^ vb);
            } else {
                u = piece<true>(u, X[C - 1], L);
                crc = wave_xor(bitmat(u, col));
                if (p) {
                    const uint32_t v = (lane < 32 && ((crc >> lane) & 1u)) ? s_unshift[p * 32 + lane] : 0u;
                    crc = wave_xor(v);
                }
            }
            u = 0;
            if constexpr (SEG) {
                if (x.split) {
                    uint32_t zc[16]; // d < 2^16 (the plan's target_segments bound)
    #pragma unroll
                    for (int b = 0; b < 16; b++) // independent loads first, then the dependent applies
                        zc[b] = ((x.d >> b) & 1u) ? zpow[(x.s + b) * 32 + (lane & 31)] : 0u;
    #pragma unroll
                    for (int b = 0; b < 16; b++)
                        if ((x.d >> b) & 1u)
                            crc = wave_xor((lane < 32 && ((crc >> lane) & 1u)) ? zc[b] : 0u);
                    if (lane == 0)
                        sub[x.i] = crc;
                } else if (lane == 0) {
                    out[x.xi] = crc;
                }
            } else if (lane == 0) {
                out[x.i] = crc;
            }
            return x.i + 1 == e1;
        };

        v4u buf[NBUF][C];
        Ext hx[NBUF];
        uint32_t hc[NBUF];
    #pragma unroll
        for (int j = 0; j < NBUF - 1; j++) {
            load_ext_chunk<C, AUX>(buf[j], base, lx, lc, lane);
            hx[j] = lx;
            hc[j] = lc;
            advance();
        }
        // the exit test sits after each full group of NBUF chunks (an exit
        // inside the unrolled group turns the slot rotation into register copies
        // that wait for every load in flight); chunks after the final one are
        // clamped re-loads and are not hashed
        bool fin = false;
        while (!fin) {
            const uint32_t qp = (uint32_t)(lx.i - e0); // items the loader has passed
            const uint32_t peer = post_progress<PRIO_MODE, NW>(qp, wave, lane);
    #pragma unroll
            for (int j = 0; j < NBUF; j++) {
                const int nj = (j + NBUF - 1) % NBUF;
                load_ext_chunk<C, AUX>(buf[nj], base, lx, lc, lane);
                hx[nj] = lx;
                hc[nj] = lc;
                advance();
                __builtin_amdgcn_sched_barrier(0);
                if (!fin)
                    fin = hash(buf[j], hx[j], hc[j]);
            }
            set_priority<PRIO_MODE, NW>(peer, qp, lane);
        }
    };
    if constexpr (ADAPT && !SEG && !BAL) {
        // rows the wave's extents span (R) and would hash at C = 8 / 4
        // (whole chunks), over a sample of its first 256 extents
        const uint64_t cnt = e1 - e0 < 256 ? e1 - e0 : 256;
        uint32_t r_all = 0, r8 = 0, r4 = 0;
        for (uint64_t i = e0 + (uint64_t)lane; i < e0 + cnt; i += 64) {
            const uint64_t o = (offsets ? offsets[i] : i * stride) + shift;
            const uint32_t l = offsets ? lengths[i] : len_const;
            const uint64_t a0 = o & ~(uint64_t)15, eu = (o + l + 15) & ~(uint64_t)15;
            const uint64_t R = l ? (eu - a0 + PRV_ROW_BYTES - 1) / PRV_ROW_BYTES : 0;
            const uint64_t R8 = R > 8 ? (R + 7) & ~(uint64_t)7 : 8, R4 = R > 4 ? (R + 3) & ~(uint64_t)3 : 4;
            // saturated at 2^22 rows (4 GiB) per extent: four per lane and
            // 64 lanes stay below 2^30, and only the ratios matter
            r_all += (uint32_t)(R < (1u << 22) ? R : (1u << 22));
            r8 += (uint32_t)(R8 < (1u << 22) ? R8 : (1u << 22));
            r4 += (uint32_t)(R4 < (1u << 22) ? R4 : (1u << 22));
        }
        const uint64_t ra = wave_sum32(r_all), h8 = wave_sum32(r8), h4 = wave_sum32(r4);
        if (10 * (h8 - ra) <= 3 * h8)
            walk(IntC<8>{});
        else if (10 * (h4 - ra) <= 3 * h4)
            walk(IntC<4>{});
        else
            walk(IntC<CH>{});
    } else {
        walk(IntC<CH>{});
    }
}

// ---------------------------------------------------------------------------
// Segmented extents (few large values: fewer items than resident waves).
//
// crc_seg_plan_kernel (one workgroup of 1024): extent i of length len gets
// m = ceil(len / 2^s) segments (m = 1 for an empty extent), 2^s one size for
// the call, the smallest power of two >= 16 KiB with total / 2^s <=
// target_segments (so at most n + target_segments segments); seg_shift[i] = s and
// seg_prefix = exclusive prefix sum of m (n + 1 entries, total last).  Segments are
// counted from the extent's start, so every segment but the last is exactly
// 2^s bytes and sits a whole number of them before the last one.
// Thread t takes the contiguous extents [t·per, (t+1)·per): its lengths load
// together, then a wave scan of the thread sums and a scan of the 16 wave
// totals through LDS.
// ---------------------------------------------------------------------------
constexpr uint32_t kSegMinShift = 14;    // 16 KiB
constexpr int kSegPlanThreads = 1024;
constexpr int kSegPlanPerThread = 16;    // extents per thread: n <= 16384

__global__ __launch_bounds__(kSegPlanThreads) void crc_seg_plan_kernel(const uint32_t *__restrict__ lengths,
                                                                     uint32_t len_const, uint64_t n,
                                                                     uint32_t target_segments,
                                                                     uint32_t *__restrict__ seg_prefix,
                                                                     uint8_t *__restrict__ seg_shift)
{
    __shared__ uint32_t s_wave[kSegPlanThreads / 64];
    __shared__ uint64_t s_bytes[kSegPlanThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t per = (uint32_t)((n + kSegPlanThreads - 1) / kSegPlanThreads);
    const uint64_t i0 = (uint64_t)tid * per;
    uint64_t len[kSegPlanPerThread];
    uint64_t bytes = 0;
#pragma unroll
    for (int j = 0; j < kSegPlanPerThread; j++) {
        const uint64_t i = i0 + j;
        len[j] = ((uint32_t)j < per && i < n) ? (lengths ? lengths[i] : len_const) : 0u;
        bytes += len[j];
    }
    // one segment size for the whole call: the smallest power of two >= 16 KiB
    // that cuts the total into at most target_segments full segments, so the
    // count split of segments over the waves is a byte split
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)bytes, d, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(bytes >> 32), d, 64);
        bytes += ((uint64_t)hi << 32) | lo;
    }
    if (lane == 0)
        s_bytes[w] = bytes;
    __syncthreads();
    uint64_t total_bytes = 0;
    for (uint32_t k = 0; k < kSegPlanThreads / 64; k++)
        total_bytes += s_bytes[k];
    const uint64_t q = (total_bytes + target_segments - 1) / target_segments; // bytes per segment
    const uint32_t lq = q > 1 ? 64u - (uint32_t)__builtin_clzll(q - 1) : 0u;  // ceil(log2 q)
    const uint32_t sh = lq > kSegMinShift ? lq : kSegMinShift;
    uint32_t m[kSegPlanPerThread];
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < kSegPlanPerThread; j++) {
        const uint64_t i = i0 + j;
        m[j] = 0;
        if ((uint32_t)j < per && i < n) {
            m[j] = len[j] ? (uint32_t)((len[j] + (1ull << sh) - 1) >> sh) : 1u;
            sum += m[j];
        }
    }
    uint32_t x = sum; // inclusive wave scan
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64);
        x += lane >= (uint32_t)d ? y : 0u;
    }
    if (lane == 63)
        s_wave[w] = x;
    __syncthreads();
    uint32_t before = 0, total = 0; // exclusive prefix of the wave totals
    for (uint32_t k = 0; k < kSegPlanThreads / 64; k++) {
        before += k < w ? s_wave[k] : 0u;
        total += s_wave[k];
    }
    uint32_t run = before + x - sum;
#pragma unroll
    for (int j = 0; j < kSegPlanPerThread; j++) {
        const uint64_t i = i0 + j;
        if ((uint32_t)j < per && i < n) {
            seg_prefix[i] = run;
            seg_shift[i] = (uint8_t)sh;
            run += m[j];
        }
    }
    if (tid == 0)
        seg_prefix[n] = total;
}

// one 256-thread workgroup per split extent: out = Z_r(XOR of segments
// 0..m-2) ^ sub[last], r = the last segment's length (zpow: columns of
// Z_(2^k)).  The XOR is spread over the workgroup with 8 loads in flight per
// thread: a lone 256 MiB value has 16384 segments, and one wave walking them
// took 33 us (profiles/r01/segments/huge_value_*).
constexpr int kSegReduceThreads = 256;

__global__ __launch_bounds__(kSegReduceThreads) void crc_seg_reduce_kernel(
    const uint32_t *__restrict__ sub, const uint32_t *__restrict__ seg_prefix, const uint8_t *__restrict__ seg_shift,
    const uint32_t *__restrict__ lengths, uint32_t len_const, const uint32_t *__restrict__ zpow, uint64_t n,
    uint32_t *__restrict__ out)
{
    __shared__ uint32_t s_part[kSegReduceThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint32_t p0 = seg_prefix[i], p1 = seg_prefix[i + 1];
        if (p1 - p0 < 2)
            continue; // stored directly by the extents kernel (uniform per workgroup)
        uint32_t acc = 0;
        for (uint32_t t = p0 + threadIdx.x; t + 1 < p1; t += 8 * kSegReduceThreads) {
            uint32_t v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint32_t u = t + (uint32_t)k * kSegReduceThreads;
                v[k] = u + 1 < p1 ? sub[u] : 0u;
            }
#pragma unroll
            for (int k = 0; k < 8; k++)
                acc ^= v[k];
        }
        acc = wave_xor(acc);
        if (lane == 0)
            s_part[wave] = acc;
        __syncthreads();
        if (wave == 0) {
            acc = 0;
#pragma unroll
            for (int w = 0; w < kSegReduceThreads / 64; w++)
                acc ^= s_part[w];
            const uint64_t len = lengths ? lengths[i] : len_const;
            const uint32_t sh = seg_shift[i];
            const uint64_t r = len - ((uint64_t)(p1 - p0 - 1) << sh); // 1 .. 2^sh
#pragma unroll 1
            for (uint32_t b = 0; b <= sh; b++)
                if ((r >> b) & 1u)
                    acc = wave_xor((lane < 32 && ((acc >> lane) & 1u)) ? zpow[b * 32 + (lane & 31)] : 0u);
            if (lane == 0)
                out[i] = acc ^ sub[p1 - 1];
        }
        __syncthreads(); // s_part is reused by the next extent
    }
}

// ---------------------------------------------------------------------------
// Few extents in ONE launch (crc_ranges_fused_kernel): the segmented path of
// plan kernel -> extents kernel -> reduce kernel above, in one kernel with
// one workgroup per CU (DESIGN.md §4).
//
// Plan, redone by every workgroup: the call's one segment size 2^s exactly
// as crc_seg_plan_kernel picks it, and the exclusive prefix of segments per
// extent, m_i = ceil(len_i / 2^s) (1 if empty).  Up to kFusedWavePlan
// extents every wave plans alone (lane i holds extent i: one load, a wave
// sum and a wave scan, no barrier); above that the workgroup plans into LDS
// (s_segp).  Extents stay whole -- no prefix at all -- when none is longer
// than 2^s or when the count split is already balanced by bytes.
//
// Speculation: the tables go to LDS by DMA first, and before the plan every
// wave assumes the whole-extent outcome and issues its first chunk loads;
// the plan's barriers wait only for LDS, so those loads stay in flight.  If
// the plan cuts an extent the wave restarts on the real cut.
//
// Walk: segments only place the cuts.  They split evenly over the waves
// (one size: a byte split), and a wave hashes its segments of one extent as
// ONE contiguous range -- one fold per range, not per segment, so a lone
// 256 MiB value costs each wave one fold.  Whole extents are stored straight
// to out[].  The loader keeps the range geometry in scalars and tags each
// chunk it issues for the hash side of the register pipeline.
//
// Combine (linear, no affine term: SURVEY §0.2): a part of an extent
// contributes its CRC moved to the extent's end, Z_d(crc) with d the bytes
// after the part, and the extent's CRC is the XOR of the contributions.
// Only a wave's first and last ranges can be parts: they go to two LDS
// slots (extent, contribution, segments), or with the wave plan XOR and
// count into per-extent LDS accumulators, and after a barrier wave 0 merges
// them.  An extent shared with other workgroups (only the workgroup's first
// and last can be) is finished through finish_shared's zero-at-rest word
// acc[extent] (segment count and XOR of the shares: an XOR and an add per
// share; the add that completes the count exchanges the word for 0 and
// stores the CRC): one atomic location per extent, so no cache writeback or
// invalidate is needed (a release/acquire pair cost 4 us of a 60 us call).
// ---------------------------------------------------------------------------
constexpr int kFusedWaves = 16;
constexpr uint32_t kFusedMaxExtents = 16384;
constexpr uint32_t kFusedWavePlan = 64;
constexpr uint32_t kFusedNone = 0xFFFFFFFFu;
__shared__ uint32_t s_segp[kFusedMaxExtents + 1];
__shared__ uint64_t s_fsum[kFusedWaves];
__shared__ uint32_t s_fcnt[kFusedWaves];
__shared__ uint32_t s_fmax[kFusedWaves];
__shared__ uint32_t s_dacc[kFusedWavePlan], s_dcnt[kFusedWavePlan]; // wave plan: shares of split extents
__shared__ uint32_t s_fslot[kFusedWaves][2][4]; // extent, contribution, segments, (pad)

// maximum over the 64 lanes, every lane gets it
__device__ __forceinline__ uint32_t wave_max32(uint32_t v)
{
    v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false));
    v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false));
    v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x124, 0xF, 0xF, false));
    v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, false));
    return max(max((uint32_t)__builtin_amdgcn_readlane((int)v, 0), (uint32_t)__builtin_amdgcn_readlane((int)v, 16)),
               max((uint32_t)__builtin_amdgcn_readlane((int)v, 32), (uint32_t)__builtin_amdgcn_readlane((int)v, 48)));
}

// inclusive prefix sum over the 64 lanes (row_shr steps inside rows of 16,
// then the totals of the rows below)
__device__ __forceinline__ uint32_t wave_scan32(uint32_t x, int lane)
{
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false); // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false); // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false); // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false); // row_shr:8
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)x, 15);
    const uint32_t r1 = (uint32_t)__builtin_amdgcn_readlane((int)x, 31);
    const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)x, 47);
    return x + (lane >= 16 ? r0 : 0u) + (lane >= 32 ? r1 : 0u) + (lane >= 48 ? r2 : 0u);
}

// Workgroup barrier for LDS only: this wave's LDS stores are complete
// (lgkmcnt 0) but its vector memory loads stay in flight -- __syncthreads()
// also waits for those (vmcnt 0), which would stall the speculative chunk
// loads issued before the plan.  The empty asm statements keep the compiler
// from moving memory accesses across it.
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0xC07F); // vmcnt 63, expcnt 7, lgkmcnt 0
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// chunk tag flags: pad bytes after the range end (bits 0-4) | flags
constexpr uint32_t kFLastChunk = 1u << 5, kFWhole = 1u << 6, kFFinal = 1u << 8;
constexpr int32_t kFNoMask = -(1 << 30);

// xw: XCD weights of the split of units (segments, or whole extents) over
// the waves, as crc_rows_kernel's (wave_range), applied when there are at
// least 32 units per wave.
template <int CH, int NBUF, int AUX, int PRIO_MODE, int NW = kFusedWaves>
__global__ __launch_bounds__(64 * NW, 1) void crc_ranges_fused_kernel(
    const uint8_t *__restrict__ base, uint64_t n, const uint64_t *__restrict__ offsets,
    const uint32_t *__restrict__ lengths, uint64_t shift, uint64_t stride, uint32_t len_const,
    const uint32_t *__restrict__ lds_image, const uint32_t *__restrict__ nib16,
    const uint32_t *__restrict__ rowshift, uint32_t *__restrict__ out, const uint32_t *__restrict__ zpow,
    uint32_t target_segments, uint32_t min_shift, uint64_t *__restrict__ acc, uint32_t xw)
{
    static_assert(NW <= kFusedWaves, "LDS slots");
    static_assert((NBUF - 1) * CH < 16, "the prologue's loads fit one vmcnt immediate");
    constexpr int PER = kFusedMaxExtents / (64 * NW); // workgroup plan: extents per thread
    constexpr int64_t CB = (int64_t)CH * PRV_ROW_BYTES; // bytes per chunk
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool wplan = n <= kFusedWavePlan;
    const uint64_t W = (uint64_t)gridDim.x * NW;
    const uint64_t wid = (uint64_t)blockIdx.x * NW + wave;
    // The tables go straight to LDS (global_load_lds_dwordx4: lane l of a
    // wave writes 16 B at the wave's LDS base + 16 l).  Workgroup plan: they
    // are the first loads, and every wave waits for them (vmcnt 0) before it
    // issues its first chunk loads, so the LDS-only barriers below leave just
    // those in flight.  Wave plan: below, after the first chunk loads.
    constexpr int NT4 = 64 * NW;
    static_assert((PRV_LDS_WORDS / 4) % NT4 == 0 && 16 * 4 * 32 / 4 <= NT4 && 8 * 16 * 16 / 4 <= NT4 &&
                      kFusedZRows * 32 / 4 <= NT4 && (kFusedZRows * 32 / 4) % 64 == 0,
                  "whole waves per table");
    auto to_lds = [&](const uint32_t *src, uint32_t *dst, int piece) { // piece: 16-B index, wave-aligned
        __builtin_amdgcn_global_load_lds(src + 4 * piece, dst + 4 * (piece - lane), 16, 0, 0);
    };
    auto tables = [&]() {
#pragma unroll
        for (int j = 0; j < PRV_LDS_WORDS / 4 / NT4; j++)
            to_lds(lds_image, s_tab, (int)threadIdx.x + j * NT4);
        if (threadIdx.x < 8 * 16 * 16 / 4)
            to_lds(nib16, s_nib16, (int)threadIdx.x);
        if (threadIdx.x < 16 * 4 * 32 / 4)
            to_lds(rowshift, s_rowshift, (int)threadIdx.x);
        if (threadIdx.x < kFusedZRows * 32 / 4)
            to_lds(zpow, s_zpow, (int)threadIdx.x);
    };
    // The wave plan (n <= kFusedWavePlan): lane i holds extent i's length and
    // offset.  They are all the plan needs, so they are loaded (and waited
    // for) first; the plan, the wave's first chunk loads and then the tables
    // follow, and the tables' latency overlaps the chunks' instead of coming
    // before it.  (A lone large value's waves start streaming ~1-2 us
    // sooner; and nothing is speculated.)
    uint32_t wlen = 0;
    uint64_t woff = 0;
    if (wplan) {
        if ((uint64_t)lane < n) {
            wlen = lengths ? lengths[lane] : len_const;
            woff = (offsets ? offsets[lane] : (uint64_t)lane * stride) + shift;
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);
    } else {
        tables();
    }
    // Then the workgroup plan's lengths, so that their latencies overlap the
    // tables' and the speculative start below.
    const uint32_t per = wplan ? 0u : (uint32_t)((n + 64 * NW - 1) / (64 * NW)); // workgroup plan, <= PER
    const uint64_t i0 = (uint64_t)threadIdx.x * per;
    uint32_t len[PER];
#pragma unroll
    for (int j = 0; j < PER; j++)
        len[j] = ((uint32_t)j < per && i0 + j < n) ? (lengths ? lengths[i0 + j] : len_const) : 0u;
    // ---- the wave's work and the loader cursor ----
    // Speculation: until the plan says otherwise every extent is one segment
    // (segp(i) = i, the count split).  That is the plan's answer whenever no
    // extent is longer than 2^s -- every call of small values -- and then the
    // first chunks are already in flight when the plan ends.
    bool spec = true;
    // an extent's length and offset: the wave plan's lanes, else memory
    auto ext_len = [&](uint64_t i) -> uint32_t {
        if (wplan)
            return (uint32_t)__builtin_amdgcn_readlane((int)wlen, (int)i);
        return lengths ? (uint32_t)__builtin_amdgcn_readfirstlane(lengths[i]) : len_const;
    };
    auto ext_off = [&](uint64_t i) -> uint64_t {
        if (wplan)
            return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)woff, (int)i)) |
                   ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(woff >> 32), (int)i) << 32);
        return uniform64((offsets ? offsets[i] : i * stride) + shift);
    };
    uint32_t sh = min_shift, NTs = (uint32_t)n, wexcl = 0;
    auto segp = [&](uint64_t i) -> uint32_t { // segments before extent i (i <= n)
        if (spec)
            return (uint32_t)i;
        if (wplan)
            return i < n ? (uint32_t)__builtin_amdgcn_readlane((int)wexcl, (int)i) : NTs;
        return (uint32_t)__builtin_amdgcn_readfirstlane(s_segp[i]);
    };
    uint64_t e0 = 0, e1 = 0; // the wave's segments
    auto split = [&](uint64_t units) {
        uint64_t ng;
        wave_range<NW>(units, W, wid, units >= 32 * W ? xw : 0u, e0, ng);
        e1 = uniform64(e0 + ng);
    };
    split(n);
    // the wave's range of extent ci (its segments in [e0, e1), contiguous
    // bytes [st, en) of the extent [coff, cend)); extent ci + 1 starts at
    // noff (loaded one extent ahead).  The range's chunks: NC chunks of CB
    // bytes from VS (the first one starting at or below A0 = the range start
    // rounded down to 16 B), loadable bytes up to hi; chunk lc next.  Tag
    // words of the range's last chunk: fl (pad | flags), xi, td = bytes of
    // the extent after the range, tn = the range's segments.
    uint64_t ci = 0, coff = 0, cend = 0, noff = 0;
    uint32_t p0 = 0, p1 = 0, nlen = 0;
    int64_t VS = 0;
    uint64_t A0 = 0, hi = 0;
    uint32_t NC = 1, lc = 0, fl = 0, xi = 0, td = 0, tn = 0;
    int32_t lo0 = kFNoMask;
    auto start_range = [&]() {
        const uint64_t ks = (e0 > p0 ? e0 : p0) - p0, ke = (e1 < p1 ? e1 : p1) - p0;
        const uint64_t st = coff + (ks << sh);
        const uint64_t en = ke == p1 - p0 ? cend : coff + (ke << sh);
        A0 = st & ~(uint64_t)15;
        const uint64_t Eu = (en + 15) & ~(uint64_t)15;
        hi = en > st ? Eu : A0;
        const uint64_t nc = (Eu - A0 + CB - 1) / CB;
        NC = nc ? (uint32_t)nc : 1u;
        VS = (int64_t)Eu - (int64_t)NC * CB;
        lo0 = (st & 15) ? (int32_t)((int64_t)st - VS) : kFNoMask;
        const bool whole = ks == 0 && ke == p1 - p0;
        fl = (uint32_t)(Eu - en) | (whole ? kFWhole : 0u);
        xi = (uint32_t)ci;
        td = (uint32_t)(cend - en);
        tn = (uint32_t)(ke - ks);
        lc = 0;
    };
    auto begin = [&]() { // the cursor at segment e0 (e0 < e1)
        if (spec) {
            ci = e0;
        } else if (wplan) { // last i with segp(i) <= e0 (strictly increasing)
            ci = (uint64_t)__builtin_popcountll(__ballot((uint64_t)lane < n && wexcl <= e0)) - 1;
        } else { // 64-way ballot search over LDS, as crc_ranges_kernel's
            uint64_t lo = 0, hi2 = n;
            while (hi2 - lo > 1) {
                const uint64_t step = (hi2 - lo + 63) / 64;
                const uint64_t idx = lo + (uint64_t)lane * step;
                const bool le = idx < hi2 && (uint64_t)s_segp[idx] <= e0;
                const uint64_t k = (uint64_t)__builtin_popcountll(__ballot(le));
                lo = uniform64(lo + (k - 1) * step);
                const uint64_t nh = lo + step;
                hi2 = uniform64(nh < hi2 ? nh : hi2);
            }
            ci = lo;
        }
        coff = ext_off(ci);
        cend = coff + ext_len(ci);
        p0 = segp(ci);
        p1 = segp(ci + 1);
        if (ci + 1 < n && e1 > p1) {
            noff = ext_off(ci + 1);
            nlen = ext_len(ci + 1);
        }
        start_range();
    };
    uint32_t nck = 0; // chunks the loader has passed (progress priority)
    auto advance = [&]() {
        nck++;
        if (lc + 1 < NC) {
            lc++;
        } else if (p1 < e1) { // else: stay on the final chunk (re-loads are never hashed)
            ci++;
            coff = noff;
            cend = noff + nlen;
            p0 = p1;
            p1 = segp(ci + 1);
            if (ci + 1 < n && e1 > p1) {
                noff = ext_off(ci + 1);
                nlen = ext_len(ci + 1);
            }
            start_range();
        }
    };
    struct Tag {
        int32_t lo;
        uint32_t fl, xi, td, tn;
    };
    auto load = [&](v4u (&X)[CH], Tag &tg) {
        const int64_t rowbase = VS + (int64_t)lc * CB;
        const int64_t room = (int64_t)hi - rowbase;
        const uint32_t bytes = room <= 0 ? 0u : (room >= CB ? (uint32_t)CB : (uint32_t)room);
        const int32_t low = lc == 0 ? (int32_t)((int64_t)A0 - rowbase) : 0; // first in-range offset
        const __amdgpu_buffer_rsrc_t rs = uniform_rsrc(base + rowbase, bytes);
#pragma unroll
        for (int k = 0; k < CH; k++) {
            const int32_t o = k * (int32_t)PRV_ROW_BYTES + 16 * lane;
            X[k] = __builtin_bit_cast(
                v4u, __builtin_amdgcn_raw_buffer_load_b128(rs, o >= low ? o : (int32_t)0x80000000, 0, AUX));
            __builtin_amdgcn_sched_barrier(0);
        }
        tg.lo = lc == 0 ? lo0 : kFNoMask;
        tg.fl = lc + 1 == NC ? (fl | kFLastChunk | (p1 >= e1 ? kFFinal : 0u)) : 0u;
        tg.xi = xi;
        tg.td = td;
        tg.tn = tn;
    };
    v4u buf[NBUF][CH];
    Tag tag[NBUF];
    auto prologue = [&]() {
#pragma unroll
        for (int j = 0; j < NBUF - 1; j++) {
            load(buf[j], tag[j]);
            advance();
        }
    };
    // ---- plan (host-checked n <= kFusedMaxExtents) ----
    // one segment size 2^s for the call: the smallest s >= min_shift with
    // ceil(total / 2^s) <= target (target a power of two, host-checked)
    const uint32_t tlog = (uint32_t)__builtin_ctz(target_segments);
    auto seg_shift = [&](uint64_t total) {
        const uint32_t cl = total > 1 ? 64u - (uint32_t)__builtin_clzll(total - 1) : 0u; // ceil(log2 total)
        const uint32_t lq = cl > tlog ? cl - tlog : 0u;
        return (uint32_t)__builtin_amdgcn_readfirstlane(lq > min_shift ? lq : min_shift);
    };
    auto segs = [&](uint32_t l) { return l ? (uint32_t)(((uint64_t)l + (1ull << sh) - 1) >> sh) : 1u; };
    // Extents stay whole -- the speculation is the plan, NT = n and segp(i) =
    // i, no prefix needed -- when none is longer than 2^s, or when the count
    // split is byte-balanced already: the ceil(n / W) longest extents a wave
    // can get hold at most 1.5x the mean bytes per wave.  (3000 x 64 KiB
    // values: 37.5 us whole against 48 us split.)
    // (Extents up to 2^kSegMinShift stay whole whatever the segment size:
    // finer segments only place the cuts of long extents, and cutting a
    // 4 KiB value into 1 KiB parts costs a combine per part: 65 x 4 KiB 9.4
    // -> 15.8 us, profiles/r04/fused/.)
    auto keep_whole = [&](uint64_t total, uint32_t maxl) {
        return maxl <= (1ull << (sh > kSegMinShift ? sh : kSegMinShift)) ||
               (uint64_t)maxl * ((n + W - 1) / W) * 2 <= 3 * ((total + W - 1) / W);
    };
    if (wplan) {
        // The wave plan, before any table is requested (no LDS): the real
        // cut and its first chunk loads, then the tables, then the wait for
        // both.
        // lengths < 2^32 on 64 lanes: low 20 bits and the rest, two 32-bit sums
        const uint64_t total = ((uint64_t)wave_sum32(wlen >> 20) << 20) + wave_sum32(wlen & 0xFFFFFu);
        sh = seg_shift(total);
        if (!keep_whole(total, wave_max32(wlen))) {
            const uint32_t m = (uint64_t)lane < n ? segs(wlen) : 0u;
            const uint32_t x = wave_scan32(m, lane);
            wexcl = x - m;
            NTs = (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
        }
        spec = NTs == n;
        split(NTs);
        if (e0 < e1) {
            begin();
            prologue();
        }
        tables();
        __builtin_amdgcn_s_waitcnt(0x0F70); // the tables (and the first chunks)
    } else {
        if (e0 < e1) // speculative start
            begin();
        __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt 0: the tables (and lengths) are in
        if (e0 < e1)
            prologue();
    }

    const LaneConst L = lane_const(lane);
    init_progress<PRIO_MODE, NW>();
    if (lane < 8)
        s_fslot[wave][lane >> 2][lane & 3] = (lane & 3) ? 0u : kFusedNone;
    if (threadIdx.x < kFusedWavePlan) {
        s_dacc[threadIdx.x] = 0u;
        s_dcnt[threadIdx.x] = 0u;
    }

    if (wplan) {
        lds_barrier(); // every wave's tables and LDS slots
    } else {
        uint64_t bytes = 0; // < 2^36
        uint32_t lmax = 0;
#pragma unroll
        for (int j = 0; j < PER; j++) {
            bytes += len[j];
            lmax = max(lmax, len[j]);
        }
        const uint64_t wb = ((uint64_t)wave_sum32((uint32_t)(bytes >> 20)) << 20) +
                            wave_sum32((uint32_t)bytes & 0xFFFFFu); // < 2^42
        const uint32_t wm = wave_max32(lmax);
        if (lane == 0) {
            s_fsum[wave] = wb;
            s_fmax[wave] = wm;
        }
        lds_barrier(); // also the tables
        const uint64_t fs = lane < NW ? s_fsum[lane] : 0u;
        const uint64_t total = ((uint64_t)wave_sum32((uint32_t)(fs >> 21)) << 21) + wave_sum32((uint32_t)fs & 0x1FFFFFu);
        sh = seg_shift(total);
        if (!keep_whole(total, wave_max32(lane < NW ? s_fmax[lane] : 0u))) {
            uint32_t m[PER];
            uint32_t msum = 0;
#pragma unroll
            for (int j = 0; j < PER; j++) {
                m[j] = ((uint32_t)j < per && i0 + j < n) ? segs(len[j]) : 0u;
                msum += m[j];
            }
            const uint32_t x = wave_scan32(msum, lane);
            if (lane == 63)
                s_fcnt[wave] = x;
            lds_barrier();
            const uint32_t fc = lane < NW ? s_fcnt[lane] : 0u;
            const uint32_t all = wave_sum32(fc), before = wave_sum32(lane < wave ? fc : 0u);
            uint32_t run = before + x - msum;
#pragma unroll
            for (int j = 0; j < PER; j++)
                if ((uint32_t)j < per && i0 + j < n) {
                    s_segp[i0 + j] = run;
                    run += m[j];
                }
            if (threadIdx.x == 0)
                s_segp[n] = all;
            NTs = all;
            lds_barrier();
        }
        spec = NTs == n;
        if (!spec) { // some extent is split: the real cut, and a new start
            split(NTs);
            if (e0 < e1) {
                begin();
                prologue();
            }
        }
    }
    // (NTs == n: the plan is the speculation's, segp(i) = i, and so is the cursor)

    // ---- walk ----
    uint32_t nslots = 0;
    if (e0 < e1) {
        uint32_t u = 0;
        // hash one chunk; true after the wave's final one
        auto hash = [&](v4u (&X)[CH], const Tag &tg) -> bool {
            if (tg.lo != kFNoMask) {
                const int32_t lo32 = tg.lo - 16 * lane;
#pragma unroll
                for (int k = 0; k < CH; k++)
                    X[k] = mask_window(X[k], lo32 - k * (int32_t)PRV_ROW_BYTES, 16);
            }
            const bool lastc = (tg.fl & kFLastChunk) != 0;
            const int32_t p = (int32_t)(tg.fl & 31u);
            if (lastc && p)
                X[CH - 1] = mask_window(X[CH - 1], 0, lane == 63 ? 16 - p : 16);
#pragma unroll
            for (int k = 0; k < CH - 1; k++)
                u = piece<false>(u, X[k], L);
            if (!lastc) {
                u = piece<false>(u, X[CH - 1], L);
                return false;
            }
            u = piece_pre(u, X[CH - 1], L);
            uint32_t s4[4];
            row_totals(nib_fold<16>(u, 4u * (uint32_t)(lane & 15)), s4);
            const uint32_t sa = lane < 32 ? s4[0] : s4[2];
            const uint32_t sb = lane < 32 ? s4[1] : s4[3];
            const uint32_t jj = (uint32_t)lane & 31;
            const uint32_t *t = s_rowshift + (uint32_t)p * 128 + (lane < 32 ? 0 : 64) + jj;
            const uint32_t va = ((sa >> jj) & 1u) ? t[0] : 0u;
            const uint32_t vb = ((sb >> jj) & 1u) ? t[32] : 0u;
            const uint32_t crc = wave_xor(va ^ vb);
            u = 0;
            if (tg.fl & kFWhole) {
                if (lane == 0)
                    out[tg.xi] = crc;
            } else {
                // a part of the extent: its share is its CRC moved to the
                // extent's end.  Wave plan: into the workgroup's per-extent
                // accumulators; else a slot (only a wave's first and last
                // ranges can be parts)
                const uint32_t v = zshift_lds(crc, tg.td, lane);
                if (wplan) {
                    if (lane == 0) {
                        __hip_atomic_fetch_xor(&s_dacc[tg.xi], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_fetch_add(&s_dcnt[tg.xi], tg.tn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                } else {
                    if (lane == 0) {
                        s_fslot[wave][nslots][0] = tg.xi;
                        s_fslot[wave][nslots][1] = v;
                        s_fslot[wave][nslots][2] = tg.tn;
                    }
                    nslots++;
                }
            }
            return (tg.fl & kFFinal) != 0;
        };
        // the exit test sits after each full group of NBUF chunks (as in
        // crc_ranges_kernel)
        bool fin = false;
        while (!fin) {
            const uint32_t qp = nck;
            const uint32_t peer = post_progress<PRIO_MODE, NW>(qp, wave, lane);
#pragma unroll
            for (int j = 0; j < NBUF; j++) {
                const int nj = (j + NBUF - 1) % NBUF;
                load(buf[nj], tag[nj]);
                advance();
                __builtin_amdgcn_sched_barrier(0);
                if (!fin)
                    fin = hash(buf[j], tag[j]);
            }
            set_priority<PRIO_MODE, NW>(peer, qp, lane);
        }
    }
    __syncthreads();
    if (wave != 0)
        return;
    // ---- workgroup merge, then the cross-workgroup finish ----
    // An extent shared with other workgroups: this workgroup's share g of c
    // segments goes into acc[x] (finish_shared); the add that completes m
    // takes the CRC.
    auto finish = [&](uint32_t x, uint32_t g, uint32_t c, uint32_t m) { finish_shared(acc, out, x, g, c, m); };
    if (wplan) { // lane x: extent x's accumulators
        const uint32_t c = (uint64_t)lane < n ? s_dcnt[lane] : 0u;
        if (c)
            finish((uint32_t)lane, s_dacc[lane], c, segs(wlen));
        return;
    }
    const uint32_t sx = lane < 2 * NW ? s_fslot[lane >> 1][lane & 1][0] : kFusedNone;
    const uint32_t sv = lane < 2 * NW ? s_fslot[lane >> 1][lane & 1][1] : 0u;
    const uint32_t sn = lane < 2 * NW ? s_fslot[lane >> 1][lane & 1][2] : 0u;
    uint64_t pend = __ballot(sx != kFusedNone);
    while (pend) {
        const uint32_t gx = (uint32_t)__builtin_amdgcn_readlane((int)sx, (int)__builtin_ctzll(pend));
        const bool mine = sx == gx;
        pend &= ~__ballot(mine);
        const uint32_t gv = wave_xor(mine ? sv : 0u), gn = wave_sum32(mine ? sn : 0u);
        if (lane == 0)
            finish(gx, gv, gn, segp(gx + 1) - segp(gx));
    }
}

// ---------------------------------------------------------------------------
// generic path: any size / alignment.  One thread per item, byte-serial
// Sarwate steps (server/crc.c:70-73) against a single LDS table.  Used for
// odd block sizes and for per-value (offset, length) extents.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void crc_generic_kernel(
    const uint8_t *__restrict__ base, uint64_t n, uint64_t stride, uint32_t len_const,
    const uint64_t *__restrict__ offsets, const uint32_t *__restrict__ lengths,
    const uint32_t *__restrict__ sarwate, uint32_t *__restrict__ out)
{
    __shared__ uint32_t t[256];
    t[threadIdx.x] = sarwate[threadIdx.x];
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t *p = base + (offsets ? offsets[i] : i * stride);
        uint32_t len = lengths ? lengths[i] : len_const;
        uint32_t crc = 0;
        // align to 4 bytes, then consume words (still one table step per byte)
        while (len && ((uintptr_t)p & 3)) {
            crc = t[(crc ^ *p++) & 0xff] ^ (crc >> 8);
            len--;
        }
        while (len >= 4) {
            uint32_t w = *reinterpret_cast<const uint32_t *>(p);
            crc ^= w;
            crc = t[crc & 0xff] ^ (crc >> 8);
            crc = t[crc & 0xff] ^ (crc >> 8);
            crc = t[crc & 0xff] ^ (crc >> 8);
            crc = t[crc & 0xff] ^ (crc >> 8);
            p += 4;
            len -= 4;
        }
        while (len--)
            crc = t[(crc ^ *p++) & 0xff] ^ (crc >> 8);
        out[i] = crc;
    }
}

// ---------------------------------------------------------------------------
// head-split blocks: a block of B = h + body bytes whose body (a multiple of
// 1 KiB) the rows kernel hashed at base + h + i*B into out[i].  By linearity
// with no affine term, crc(head | body) = Z_body(crc(head)) ^ crc(body), so
// this kernel adds each block's head term: one thread per block, Sarwate
// steps over the h (<= kHeadMax, a multiple of 4) head bytes from an LDS
// table, then the 32 columns of Z_body (kernel arguments, the same for
// every block).  h and B are multiples of 4 and the base is 4-byte aligned
// (host-checked), so the head loads are aligned dwords.
// ---------------------------------------------------------------------------
constexpr uint32_t kHeadMax = 64;
struct HeadCols {
    uint32_t c[32];
};

__global__ __launch_bounds__(256) void crc_head_kernel(const uint8_t *__restrict__ base, uint64_t n, uint32_t B,
                                                       uint32_t h, const uint32_t *__restrict__ sarwate, HeadCols z,
                                                       uint32_t *__restrict__ out)
{
    __shared__ uint32_t t[256];
    t[threadIdx.x] = sarwate[threadIdx.x];
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t *p = reinterpret_cast<const uint32_t *>(base + i * B);
        uint32_t crc = 0;
        for (uint32_t k = 0; k < h / 4; k++) {
            crc ^= p[k];
            crc = t[crc & 0xff] ^ (crc >> 8);
            crc = t[crc & 0xff] ^ (crc >> 8);
            crc = t[crc & 0xff] ^ (crc >> 8);
            crc = t[crc & 0xff] ^ (crc >> 8);
        }
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 32; b++)
            v ^= ((crc >> b) & 1u) ? z.c[b] : 0u;
        out[i] ^= v;
    }
}

// ---------------------------------------------------------------------------
// segment combine: block i was hashed as S equal segments sub[i*S + k] of
// `seg` bytes each; linearity with no affine term gives
//     crc(block) = XOR_k Z_((S-1-k) seg)(sub_k)
// (crc(A|B) = Z_|B|(crc A) ^ crc B, the identity server/crc.c's table step
// preserves).  One wave per block: with r = max(1, S/64), lane j Horner-
// combines segments [S - (64-j) r, S - (63-j) r) with Z_seg, then shifts its
// partial over the (63-j) r segments after them in at most 6 binary steps
// (Z_(seg r 2^b)), and a wave XOR ends the block -- r + 6 matrix steps per
// lane instead of S sequential ones in one thread (S reaches 2048 for a
// single 32 MiB+ block).  z.c[0] = columns of Z_seg, z.c[1 + b] = Z_(seg r 2^b).
// ---------------------------------------------------------------------------
struct SegCols {
    uint32_t c[7][32];
};

__global__ __launch_bounds__(256) void crc_combine_segments_kernel(const uint32_t *__restrict__ sub, uint64_t n,
                                                                   uint32_t S, uint32_t r, SegCols z,
                                                                   uint32_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const uint64_t W = (uint64_t)gridDim.x * (blockDim.x / 64);
    const int64_t hi = (int64_t)S - (int64_t)(63 - lane) * r;
    const int64_t lo0 = (int64_t)S - (int64_t)(64 - lane) * r;
    const int64_t lo = lo0 < 0 ? 0 : lo0;
    for (uint64_t i = (uint64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); i < n; i += W) {
        uint32_t acc = 0;
        for (int64_t t = lo; t < hi; t++)
            acc = bitmat(acc, z.c[0]) ^ sub[i * S + t];
        const uint32_t d = 63u - (uint32_t)lane;
#pragma unroll
        for (int b = 0; b < 6; b++) {
            const uint32_t sh = bitmat(acc, z.c[1 + b]);
            acc = ((d >> b) & 1u) ? sh : acc;
        }
        const uint32_t crc = wave_xor(acc);
        if (lane == 0)
            out[i] = crc;
    }
}

// ---------------------------------------------------------------------------
// verify: status[0] += #(got != expected), status[1] = min mismatching index
// (status pre-set to {0, UINT64_MAX} on the stream).  One atomic pair per
// wave with a mismatch (ballot + lowest lane), none otherwise.
// ---------------------------------------------------------------------------
// {0, UINT64_MAX} into the verify status, which crc_verify_kernel updates
// only by (memory-side) atomics: written through, as crc_zero_kernel's zeros
__global__ __launch_bounds__(64) void crc_status_init_kernel(unsigned long long *__restrict__ status)
{
    if (threadIdx.x < 2)
        __hip_atomic_store(&status[threadIdx.x], threadIdx.x ? ~0ull : 0ull, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void crc_verify_kernel(const uint32_t *__restrict__ got,
                                                         const uint32_t *__restrict__ expected, uint64_t n,
                                                         unsigned long long *__restrict__ status)
{
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        const bool bad = i < n && got[i] != expected[i];
        const uint64_t m = __ballot(bad);
        if (m && (threadIdx.x & 63) == 0) {
            atomicAdd(&status[0], (unsigned long long)__popcll(m));
            atomicMin(&status[1], (unsigned long long)(base + (threadIdx.x & ~63u) + __ffsll((long long)m) - 1));
        }
    }
}

// ---------------------------------------------------------------------------
// Gathered values (priskv_crc32_combine_dev / _sgl_dev): out[v] = XOR over the
// value's parts j of Z_(s_j)(crc_j), s_j = the bytes after part j in the value
// (the identity above; crc(empty) = 0, so empty values and zero-length parts
// need no case of their own).  The shift amounts differ per part and are
// known only here, so unlike zshift_lds (a wave-uniform amount, the wave's
// lanes holding one matrix's columns) every LANE shifts its own part: one
// apply of Z_(2^b) per set bit b of s, each as 8 nibble lookups in LDS
// (znib[b][k][v] = Z_(2^b) of nibble k holding v: 48 x 8 x 16 words, 24 KiB,
// built by the host from the columns d_zpow holds) XORed together.  A lane whose
// part CRC is 0 or whose s is 0 looks nothing up; a wave takes as many
// applies as the largest popcount(s) among its lanes.  (A 32-step GF(2)[x]
// multiply by x^(8 2^b) per set bit needs 192 B of tables instead and ~160
// VALU instructions per apply against ~25 here: measured 18 against 9 us
// for 512 Ki parts, DESIGN section 11.)
//
// G lanes per value (G = 1 .. 64, chosen by the host from nparts / n): 64 / G
// values per wave.  A group walks its value's parts from the last to the
// first, G at a time, lane g on part hi - 1 - g, so that an inclusive 64-bit
// scan over the group's lanes is the suffix sum of the lengths; the group's
// total carries into the next G parts.  Values of more than kCombLong * G
// parts are left to the whole wave, one after the other with all 64 lanes
// (one value of many parts among values of few).
//
// value_first is a device table the host cannot check: every index derived
// from it is clamped to [0, nparts], and a range that runs backwards is
// empty, so a bad table gives wrong CRCs and never a read outside the part
// arrays.  Shift amounts are taken mod 2^48 (the rows of znib).
// expected != nullptr: compare instead of (or besides) storing, with the
// status protocol of crc_verify_kernel.
// ---------------------------------------------------------------------------
constexpr int kCombThreads = 256;
constexpr int kCombRows = 48;    // = crc_gpu.hip kZpowRows: Z_(2^b), b < 48
constexpr int kCombRowWords = 8 * 16; // one row: 8 nibbles x 16 values
constexpr uint32_t kCombLong = 8; // a group takes values of up to kCombLong * G parts itself

// Z_s(c) for this lane's own c and s (znib in LDS)
__device__ __forceinline__ uint32_t nib_shift(uint32_t c, uint64_t s, const uint32_t *znib)
{
    s = c ? (s & ((1ull << kCombRows) - 1)) : 0;
#pragma unroll 1
    while (s) {
        const uint32_t *t = znib + __builtin_ctzll(s) * kCombRowWords;
        uint32_t r[8];
#pragma unroll
        for (int k = 0; k < 8; k++)
            r[k] = t[k * 16 + ((c >> (4 * k)) & 15u)];
        const uint32_t p = __builtin_amdgcn_bitop3_b32(r[0], r[1], r[2], 0x96);
        const uint32_t q = __builtin_amdgcn_bitop3_b32(r[3], r[4], r[5], 0x96);
        c = __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_bitop3_b32(p, q, r[6], 0x96), r[7], 0u, 0x96);
        s &= s - 1;
    }
    return c;
}

// the parts [a, b) of one value by the W lanes of a group (w = lane in group):
// every lane of the group returns the value's CRC
template <int W>
__device__ __forceinline__ uint32_t comb_span(const uint32_t *__restrict__ crcs, const uint32_t *__restrict__ lens,
                                              uint64_t a, uint64_t b, int w, const uint32_t *znib)
{
    uint32_t acc = 0;
    uint64_t tail = 0; // bytes after the parts still to come
    for (uint64_t hi = b; hi > a; hi = hi - a > W ? hi - W : a) {
        const bool mine = hi - a > (uint64_t)w;
        const uint64_t j = hi - 1 - (uint64_t)w;
        const uint32_t len = mine ? lens[j] : 0u;
        const uint32_t c = mine ? crcs[j] : 0u;
        uint64_t incl = len;
#pragma unroll
        for (int d = 1; d < W; d <<= 1) {
            const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)incl, d, W);
            const uint32_t up = (uint32_t)__shfl_up((int)(uint32_t)(incl >> 32), d, W);
            if (w >= d)
                incl += ((uint64_t)up << 32) | lo;
        }
        acc ^= nib_shift(c, tail + incl - len, znib);
        if (W > 1) {
            const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)incl, W - 1, W);
            const uint32_t up = (uint32_t)__shfl((int)(uint32_t)(incl >> 32), W - 1, W);
            tail += ((uint64_t)up << 32) | lo;
        } else {
            tail += incl;
        }
    }
    return group_xor<W>(acc);
}

template <int G>
__global__ __launch_bounds__(kCombThreads) void crc_combine_parts_kernel(
    const uint32_t *__restrict__ crcs, const uint32_t *__restrict__ lens, uint64_t nparts,
    const uint64_t *__restrict__ first, uint64_t n, const uint32_t *__restrict__ znib_g, uint32_t *__restrict__ out,
    const uint32_t *__restrict__ expected, unsigned long long *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint32_t znib[kCombRows * kCombRowWords];
    copy_to_lds(znib_g, znib, kCombRows * kCombRowWords / 4);
    lds_dma_landed();
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int w = lane & (G - 1);
    constexpr uint64_t kPerWg = kCombThreads / G; // values per workgroup and pass
    // every lane of a wave runs the same number of passes (base is uniform)
    for (uint64_t base = (uint64_t)blockIdx.x * kPerWg; base < n; base += (uint64_t)gridDim.x * kPerWg) {
        const uint64_t v = base + threadIdx.x / G;
        uint64_t a = 0, b = 0;
        if (v < n) {
            a = first[v];
            b = first[v + 1];
            a = a < nparts ? a : nparts;
            b = b < nparts ? b : nparts;
            b = b < a ? a : b;
        }
        const bool far = G < 64 && b - a > (uint64_t)kCombLong * G;
        uint32_t crc = comb_span<G>(crcs, lens, a, far ? a : b, w, znib);
        if (G < 64) {
            uint64_t m = __ballot(far && w == 0);
            while (m) { // wave-uniform
                const int l = __builtin_ctzll(m);
                m &= m - 1;
                const uint32_t c = comb_span<64>(crcs, lens, readlane64(a, l), readlane64(b, l), lane, znib);
                if ((lane & ~(G - 1)) == l)
                    crc = c;
            }
        }
        const bool lead = v < n && w == 0;
        if (lead && out)
            out[v] = crc;
        if (expected) {
            const uint64_t bad = __ballot(lead && crc != expected[v]);
            if (bad && lane == 0) {
                atomicAdd(&status[0], (unsigned long long)__popcll(bad));
                atomicMin(&status[1],
                          (unsigned long long)(base + (uint64_t)((threadIdx.x & ~63u) + __ffsll((long long)bad) - 1) / G));
            }
        }
    }
}

// ---------------------------------------------------------------------------
// XCD dispatch probe (once per context): workgroup b records the XCD (XCC)
// it runs on.  The rows kernel's XCD weights assume round-robin dispatch,
// workgroup b on XCD (b + k) % 8 with k the queue's first XCD (read per launch
// by wave_range); the host falls back to equal shares when this probe
// disagrees (another partition mode, a different XCD count).  Hardware-register read,
// one vector store per workgroup.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void crc_xcd_probe_kernel(uint32_t *__restrict__ out)
{
    if (threadIdx.x == 0) {
        uint32_t x;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(x));
        out[blockIdx.x] = x;
    }
}

// ---------------------------------------------------------------------------
// test-pattern fill: 64-bit word i = splitmix64(seed + (off + i + 1) * phi)
// ---------------------------------------------------------------------------
// zero fill for scratch that must start zeroed (a kernel node: hipMemsetAsync
// on memory allocated inside a stream capture did not replay as a zero fill)
// Zeroes the counters the split / fused kernels combine through.  Those
// kernels touch them only with agent-scope atomics, which execute at the
// memory side; plain zero stores would stay dirty in this kernel's XCD L2s
// until the next release writes them back, and a writeback that lands after
// the next kernel's first atomics erases them (seen inside HIP graphs on
// some boxes: 4 of 1900 split 1 MiB blocks wrong, DESIGN §3).  Agent-scope
// stores (sc1) write through and drop the line, so the zeros are in memory
// when this kernel ends, whatever fence the launch carries.
__global__ __launch_bounds__(256) void crc_zero_kernel(uint32_t *__restrict__ p, uint64_t nwords)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nwords; i += (uint64_t)gridDim.x * 256)
        __hip_atomic_store(&p[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void fill_splitmix_kernel(uint8_t *__restrict__ dst, uint64_t nbytes,
                                                            uint64_t seed, uint64_t word_offset)
{
    const uint64_t nw2 = nbytes / 16; // pairs of words
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw2;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t w = word_offset + 2 * i;
        const uint64_t a = mix64(seed + (w + 1) * 0x9E3779B97F4A7C15ull);
        const uint64_t b = mix64(seed + (w + 2) * 0x9E3779B97F4A7C15ull);
        v4u v = {(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)};
        __builtin_nontemporal_store(v, reinterpret_cast<v4u *>(dst + 16 * i));
    }
    if (blockIdx.x == 0 && threadIdx.x < (nbytes & 15)) {
        const uint64_t pos = (nbytes & ~(uint64_t)15) + threadIdx.x;
        const uint64_t w = word_offset + pos / 8;
        const uint64_t v = mix64(seed + (w + 1) * 0x9E3779B97F4A7C15ull);
        dst[pos] = (uint8_t)(v >> (8 * (pos & 7)));
    }
}

