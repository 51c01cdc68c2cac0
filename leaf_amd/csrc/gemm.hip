// NT GEMM on MFMA for the text tower:  C[M,N] (+)= A[M,K] * B[N,K]^T, 16-bit operands, fp32 accumulate.
// This file: the register-staged kernel and the DISPATCH over the three GEMM kernels (leaf_gemm_family / leaf_launch_gemm at the
// end): the half-stage ring of gemm256h.hip for launches of >= 128 tiles of 256^2, the 64 x 128 ring of gemm64.hip for smaller
// ones, and the kernel below for what neither ring takes: K < 192 (the tiny test config) and operands of 4 GiB or more, which
// the rings' 32-bit byte offsets cannot span.
//
// Both operands are K-contiguous (nn.Linear weight layout [N,K]; activations [rows,K]), which is the
// natural fragment shape of v_mfma_f32_16x16x32_{f16,bf16}: lane l holds 8 consecutive k of row l&15.
// Tile 128x128x64, 256 threads = 4 waves (2x2, 64x64 each), LDS double buffer (2 x 32 KiB), register-
// staged prefetch of tile t+1 issued before the MFMAs of tile t and written to LDS after them
// (one barrier per K-tile).  LDS rows are 128 B with a 16-B-chunk XOR swizzle (chunk ^ (row&7)) so both
// the ds_write_b128 staging stores and the ds_read_b128 fragment loads are bank-conflict free.
// The MFMA is issued as D = Wfrag * Xfrag^T so the accumulator holds 4 CONSECUTIVE n of one row m:
// epilogues then move 8 B (16-bit) or 16 B (fp32) per lane.  Grid is 1-D with an XCD-aware remap so
// the tiles that share an A panel run on one XCD's L2.
//
// Requirements checked on the host: N % 128 == 0, K % 64 == 0, row strides % 8 == 0; M is arbitrary
// (load rows are clamped, stores masked).
#include "gemm_epilogue.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = BM * BK * 2;  // 16 KiB per operand tile

__device__ __forceinline__ int lds_off(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }

// MI = 16-row MFMA tiles per wave in M: MI = 4 is the 128 x 128 tile described above (waves 2 x 2 of 64 x 64); MI = 2 is a
// 64 x 128 tile (waves 2 x 2 of 32 x 64, 48 KiB of LDS, up to 3 workgroups per CU) for launches whose 128-row tiling
// would leave CUs idle (the B-caption passes: 3,200 rows x 768 columns = 150 tiles of 128^2 on 256 CUs).
template <class TT, int EPI, int MI>
__global__ __launch_bounds__(256, 2) void gemm_nt_kernel(GemmArgs p) {
    leaf_fp16_sat_mode();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int BMt = 32 * MI;                 // tile rows
    constexpr int ATILE = BMt * BK * 2;          // A tile bytes; the B tile stays TILE_BYTES
    constexpr int BUF = ATILE + TILE_BYTES;      // one stage
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int tiles_n = p.N / BN;
    const int logical = xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = (logical / tiles_n) * BMt, n0 = (logical % tiles_n) * BN;

    // ---- staging assignment: thread -> (row r0 + 32 i, 16-B chunk c)
    const int c = tid & 7, r0 = tid >> 3;
    const u16* __restrict__ A = (const u16*)p.A;
    const u16* __restrict__ B = (const u16*)p.B;
    // rows r0 + 32 i share (row & 7) -> one swizzled LDS offset + i * 4096
    const int soff = lds_off(r0, c);
    auto arow = [&](int i) { int r = m0 + r0 + 32 * i; return r < p.M ? r : p.M - 1; };
    const u16* a_ptr0 = A + (size_t)arow(0) * p.lda + 8 * c;
    const u16* a_ptr1 = A + (size_t)arow(1) * p.lda + 8 * c;
    const u16* a_ptr2 = A + (size_t)arow(MI > 2 ? 2 : 0) * p.lda + 8 * c;
    const u16* a_ptr3 = A + (size_t)arow(MI > 2 ? 3 : 0) * p.lda + 8 * c;
    const u16* b_ptr0 = B + (size_t)(n0 + r0) * p.ldb + 8 * c;
    const u16* b_ptr1 = b_ptr0 + (size_t)32 * p.ldb;
    const u16* b_ptr2 = b_ptr0 + (size_t)64 * p.ldb;
    const u16* b_ptr3 = b_ptr0 + (size_t)96 * p.ldb;
    // staging registers as first-class vector values (arrays of HIP's uint4 struct end up in scratch)
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    u32x4 sa0, sa1, sa2, sa3, sb0, sb1, sb2, sb3;
#define G_LOAD(k0)                                                                                         \
    sa0 = *(const u32x4*)(a_ptr0 + (k0)); sb0 = *(const u32x4*)(b_ptr0 + (k0));                            \
    sa1 = *(const u32x4*)(a_ptr1 + (k0)); sb1 = *(const u32x4*)(b_ptr1 + (k0));                            \
    if constexpr (MI > 2) { sa2 = *(const u32x4*)(a_ptr2 + (k0)); }                                        \
    sb2 = *(const u32x4*)(b_ptr2 + (k0));                                                                  \
    if constexpr (MI > 2) { sa3 = *(const u32x4*)(a_ptr3 + (k0)); }                                        \
    sb3 = *(const u32x4*)(b_ptr3 + (k0));
#define S_STORE(buf)                                                                                       \
    {                                                                                                      \
        char* base_ = smem + (buf) * BUF + soff;                                                           \
        *(u32x4*)(base_) = sa0;          *(u32x4*)(base_ + ATILE) = sb0;                                   \
        *(u32x4*)(base_ + 4096) = sa1;   *(u32x4*)(base_ + ATILE + 4096) = sb1;                            \
        if constexpr (MI > 2) { *(u32x4*)(base_ + 8192) = sa2; }                                           \
        *(u32x4*)(base_ + ATILE + 8192) = sb2;                                                             \
        if constexpr (MI > 2) { *(u32x4*)(base_ + 12288) = sa3; }                                          \
        *(u32x4*)(base_ + ATILE + 12288) = sb3;                                                            \
    }

    f32x4 acc[MI][4];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fkc = lane >> 4;
    // fragment byte offsets inside a tile (constant over the K loop)
    int xo[2][MI], wo[2][4];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int i = 0; i < MI; ++i) xo[ks][i] = lds_off(wm * (16 * MI) + i * 16 + frow, ks * 4 + fkc);
#pragma unroll
        for (int i = 0; i < 4; ++i) wo[ks][i] = lds_off(wn * 64 + i * 16 + frow, ks * 4 + fkc);
    }
#define COMPUTE(buf)                                                                              \
    {                                                                                             \
        const char* sA_ = smem + (buf) * BUF;                                                     \
        const char* sB_ = sA_ + ATILE;                                                            \
        _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                                        \
            typename TT::vec8 xa[MI], wb[4];                                                      \
            _Pragma("unroll") for (int i = 0; i < MI; ++i)                                        \
                xa[i] = *(const typename TT::vec8*)(sA_ + xo[ks][i]);                             \
            _Pragma("unroll") for (int i = 0; i < 4; ++i)                                         \
                wb[i] = *(const typename TT::vec8*)(sB_ + wo[ks][i]);                             \
            _Pragma("unroll") for (int i = 0; i < MI; ++i)                                        \
                _Pragma("unroll") for (int j = 0; j < 4; ++j)                                     \
                    acc[i][j] = TT::mfma(wb[j], xa[i], acc[i][j]);                                \
        }                                                                                         \
    }

    const int nt = p.K / BK;
    G_LOAD(0)
    S_STORE(0)
    __syncthreads();
    // steady state: prefetch tile t+1 into registers, MFMA on tile t, then park the prefetch in the other buffer
    for (int t = 0; t < nt - 1; ++t) {
        const int cur = t & 1;
        G_LOAD((t + 1) * BK)
        __builtin_amdgcn_sched_barrier(0);   // keep the prefetch issue ABOVE the MFMAs (hipcc sinks it to its use)
        COMPUTE(cur)
        __builtin_amdgcn_sched_barrier(0);
        S_STORE(cur ^ 1)
        __syncthreads();
    }
    COMPUTE((nt - 1) & 1)
#undef G_LOAD
#undef S_STORE
#undef COMPUTE

    // ---- epilogue: lane holds C[m][n..n+3], m = .. + (lane&15), n = .. + 4*(lane>>4)
    {
        const int nbase = n0 + wn * 64 + 4 * (lane >> 4);
        float4 bias4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bias4[j] = p.bias ? *(const float4*)(p.bias + nbase + 16 * j) : float4{0.f, 0.f, 0.f, 0.f};
        int mrow[MI];
#pragma unroll
        for (int i = 0; i < MI; ++i) mrow[i] = m0 + wm * (16 * MI) + i * 16 + frow;
        epilogue_block<TT, EPI, MI, 4>(p, mrow, nbase, bias4, acc);
    }
}

// 128-row tiles unless they would leave CUs idle (fewer tiles than the chip has CUs): then 64-row tiles
template <class TT>
hipError_t launch_t(const GemmArgs& p, int epi, hipStream_t s) {
    const long t128 = (long)((p.M + BM - 1) / BM) * (p.N / BN);
    const bool half_m = t128 < 256 && p.M > 64;
    const int grid = half_m ? ((p.M + 63) / 64) * (p.N / BN) : (int)t128;
    const size_t lds = half_m ? 2 * (64 * BK * 2 + TILE_BYTES) : 4 * TILE_BYTES;
#define LEAF_GEMM_CASE(E)                                                                    \
    case E: {                                                                                \
        static bool attr_done = false;                                                       \
        if (!attr_done) {                                                                    \
            (void)hipFuncSetAttribute((const void*)gemm_nt_kernel<TT, E, 4>,                 \
                                hipFuncAttributeMaxDynamicSharedMemorySize, 4 * TILE_BYTES); \
            (void)hipFuncSetAttribute((const void*)gemm_nt_kernel<TT, E, 2>,                 \
                                hipFuncAttributeMaxDynamicSharedMemorySize, 4 * TILE_BYTES); \
            attr_done = true;                                                                \
        }                                                                                    \
        if (half_m) hipLaunchKernelGGL((gemm_nt_kernel<TT, E, 2>), dim3(grid), dim3(256), lds, s, p); \
        else hipLaunchKernelGGL((gemm_nt_kernel<TT, E, 4>), dim3(grid), dim3(256), lds, s, p); \
        break;                                                                               \
    }
    switch (epi) {
        LEAF_GEMM_CASE(EPI_STORE_T)
        LEAF_GEMM_CASE(EPI_ACT_T)
        LEAF_GEMM_CASE(EPI_RESID_F32)
        LEAF_GEMM_CASE(EPI_STORE_F32)
        LEAF_GEMM_CASE(EPI_ACTGRAD_T)
        LEAF_GEMM_CASE(EPI_LNFOLD_T)
        LEAF_GEMM_CASE(EPI_LNFOLD_ACT_T)
        LEAF_GEMM_CASE(EPI_RESID_LN)
        LEAF_GEMM_CASE(EPI_RESID_LN8)
        default: return hipErrorInvalidValue;
    }
#undef LEAF_GEMM_CASE
    return hipGetLastError();
}

}  // namespace

// THE dispatch rule (kernels.h): 4 = half-stage ring where it is eligible (>= 128 tiles of 256^2), else 6 = 64 x 128 ring, else
// 0 = gemm_nt_kernel above (K < 192, and operands the rings' 32-bit offsets cannot span)
int leaf_gemm_family(const GemmArgs& p, int epi) {
    if (leaf_gemm256h_eligible(p, epi)) return 4;
    if (leaf_gemm64_eligible(p)) return 6;
    return 0;
}

static void* g_stamps = nullptr;
void leaf_gemm_set_stamps(void* p) { g_stamps = p; }
void* leaf_gemm_get_stamps() { return g_stamps; }

hipError_t leaf_launch_gemm(const GemmArgs& p_in, int dtype, int epi, hipStream_t s) {
    GemmArgs p = p_in;
    p.stamps = g_stamps;
    if (p.M <= 0 || p.N <= 0 || p.K <= 0 || p.N % BN || p.K % BK || p.lda % 8 || p.ldb % 8 || p.ldc % 4)
        return hipErrorInvalidValue;
    const int fam = leaf_gemm_family(p, epi);
    if (p.a_wrap && fam != 4) return hipErrorInvalidValue;      // only the half-stage ring kernel re-reads A (the caller duplicates it otherwise)
    switch (fam) {
        case 4: return leaf_launch_gemm256h(p, dtype, epi, s);
        case 6: return leaf_launch_gemm64(p, dtype, epi, s);
        default: return dtype == LEAF_F16 ? launch_t<F16>(p, epi, s) : launch_t<BF16>(p, epi, s);
    }
}
