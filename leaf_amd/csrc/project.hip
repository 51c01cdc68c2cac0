// Final LayerNorm + text projection of the POOLED rows (one row per sequence), exact fp32 on the matrix cores.
//
// Reference: x = ln_final(x); x = text_global_pool(x, text); x = x @ text_projection  (src/open_clip/model.py:276-282,
// transformer.py:653-665,727).  Only the pooled (EOT) row of each sequence reaches the output, so LayerNorm runs on
// those rows alone and the projection is an [M, d] x [d, D] fp32 GEMM with M = sequences (6400 per search stage).
// It runs on v_mfma_f32_16x16x4_f32 (fp32 operands, fp32 accumulate: no operand rounding, so the feature error budget
// of the 16-bit layer GEMMs is not touched) instead of the VALU dot products of pool_project_kernel, which re-read the
// whole projection matrix from L2 once per 8 sequences.
//
//   ln_rows_f32_kernel    one wave per row: two-pass mean / variance in registers, y = (x - mu) * rstd * g + b
//   hidden_rows_kernel    the same rows for the caller: every (sequence, position) of a chunk's residual stream, optionally through
//                         that LayerNorm (leaf_text_forward_hidden)
//   proj_f32_kernel       tile 64 (rows) x 128 (cols), 4 waves of 32 x 64, k-step 16, register-staged double buffer
//   l2norm_rows_kernel    F.normalize(dim=-1) for the 'sim' / 'dissim' objectives
#include "common.h"
#include "kernels.h"

namespace {

constexpr int MAXCH = 8;   // float4 chunks per lane -> d <= 2048

// LayerNorm of ONE row by a wave, the lane holding float4 chunks lane + 64 i (< nq = d / 4) in registers: `get(chunk)` delivers the
// row, two-pass mean and variance of the centred values, `put(chunk, y)` receives y = (x - mu) * rstd * g + b.  The one statement of
// this arithmetic for ln_rows_f32_kernel (the pooled rows in front of the projection) and hidden_rows_kernel (every row, for the
// caller): a row's bits do not depend on which of the two normalised it.
template <class Get, class Put>
__device__ __forceinline__ void ln_row_f32(int lane, int nq, int d, const float* __restrict__ g, const float* __restrict__ b, float eps,
                                           Get get, Put put) {
    float4 v[MAXCH];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int c = lane + 64 * i;
        if (c < nq) { v[i] = get(c); s += (v[i].x + v[i].y) + (v[i].z + v[i].w); }
    }
    const float mu = wave_sum(s) / (float)d;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int c = lane + 64 * i;
        if (c < nq) {
            const float a0 = v[i].x - mu, a1 = v[i].y - mu, a2 = v[i].z - mu, a3 = v[i].w - mu;
            q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + eps);
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int c = lane + 64 * i;
        if (c < nq) {
            const float4 gg = *(const float4*)(g + 4 * c), bb = *(const float4*)(b + 4 * c);
            put(c, float4{(v[i].x - mu) * rstd * gg.x + bb.x, (v[i].y - mu) * rstd * gg.y + bb.y,
                          (v[i].z - mu) * rstd * gg.z + bb.z, (v[i].w - mu) * rstd * gg.w + bb.w});
        }
    }
}

__global__ __launch_bounds__(256) void ln_rows_f32_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                          const float* __restrict__ b, float eps, float* __restrict__ y,
                                                          int M, int d) {
    leaf_fp16_sat_mode();
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int nq = d >> 2;
    const float* xi = x + (size_t)row * d;
    float* yr = y + (size_t)row * d;
    ln_row_f32(lane, nq, d, g, b, eps, [&](int c) { return *(const float4*)(xi + 4 * c); }, [&](int c, float4 o) { *(float4*)(yr + 4 * c) = o; });
}

// Per-token hidden states for the caller (leaf_text_forward_hidden): out[n_seq, ctx, d], one wave per OUTPUT row (sequence,
// position), four rows per workgroup.  position < len(sequence): residual row seq_row + position of the chunk in the stream's
// format -- an fp32 row of x, or (LO8) the pair (x16, remainder bytes x) through the resid_decode4 of the pooled-row gathers --
// optionally through ln_row_f32 with the final LayerNorm's g, b; fp32 or (OUT16) the round-to-nearest 16-bit value of it.
// position >= len (rows a packed pass does not compute): zeros.  No LDS, no scratch, no atomics.
template <class TT, bool LO8, bool OUT16>
__global__ __launch_bounds__(256) void hidden_rows_kernel(const void* __restrict__ x, const u16* __restrict__ x16,
                                                          const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                          int final_ln, void* __restrict__ out, int n_seq, RowMap map, int d) {
    leaf_fp16_sat_mode();
    const int lane = threadIdx.x & 63, orow = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (orow >= n_seq * map.ctx) return;
    const int sg = map.s0 + orow / map.ctx, pos = orow % map.ctx;
    const int nq = d >> 2;
    auto put = [&](int c, float4 o) {
        const size_t at = (size_t)orow * d + 4 * c;
        if (OUT16) *(uint2*)((u16*)out + at) = pack4<TT>(o.x, o.y, o.z, o.w);
        else *(float4*)((float*)out + at) = o;
    };
    if (pos >= seq_len(map, sg)) {
        for (int c = lane; c < nq; c += 64) put(c, float4{0.f, 0.f, 0.f, 0.f});
        return;
    }
    const size_t at = (size_t)(seq_row(map, sg) + pos) * d;
    auto get = [&](int c) {
        if (LO8) return resid_decode4<TT>(*(const uint2*)(x16 + at + 4 * c), *(const unsigned*)((const unsigned char*)x + at + 4 * c));
        return *(const float4*)((const float*)x + at + 4 * c);
    };
    if (final_ln) ln_row_f32(lane, nq, d, g, b, eps, get, put);
    else for (int c = lane; c < nq; c += 64) put(c, get(c));
}

constexpr int BM = 64, BN = 128, BK = 16;
constexpr int A_LD = BK + 1;      // floats; +1: the 16 rows a fragment read touches land on 16 different banks
constexpr int B_LD = BN + 16;     // floats; 144 % 32 = 16: the two k rows a 32-lane half reads use disjoint banks
constexpr int A_TILE = BM * A_LD, B_TILE = BK * B_LD;
typedef float f32x4v __attribute__((ext_vector_type(4)));

// C[M,N] = A[M,K] B[K,N], all fp32 row-major; N % 128 == 0, K % 16 == 0, rows >= M masked
__global__ __launch_bounds__(256) void proj_f32_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                       float* __restrict__ C, int M, int N, int K) {
    leaf_fp16_sat_mode();
    __shared__ float As[2][A_TILE];
    __shared__ float Bs[2][B_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int tiles_n = N / BN;
    const int m0 = (blockIdx.x / tiles_n) * BM, n0 = (blockIdx.x % tiles_n) * BN;
    // staging: A tile 64 x 16 floats = 256 float4 (one per thread); B tile 16 x 128 floats = 512 float4 (two per thread)
    const int ar = tid >> 2, ac = (tid & 3) * 4;
    const int br = tid >> 5, bc = (tid & 31) * 4;
    const bool arow_ok = m0 + ar < M;
    const float* ap = A + (size_t)(arow_ok ? m0 + ar : 0) * K + ac;
    const float* bp = B + (size_t)br * N + n0 + bc;
    f32x4v a4, b4a, b4b;
    const f32x4v z4 = f32x4v{0.f, 0.f, 0.f, 0.f};
#define LOAD_T(k0)                                                                       \
    a4 = arow_ok ? *(const f32x4v*)(ap + (k0)) : z4;                                     \
    b4a = *(const f32x4v*)(bp + (size_t)(k0) * N);                                       \
    b4b = *(const f32x4v*)(bp + (size_t)((k0) + 8) * N);
#define STORE_T(buf)                                                                     \
    As[buf][ar * A_LD + ac] = a4[0]; As[buf][ar * A_LD + ac + 1] = a4[1];                \
    As[buf][ar * A_LD + ac + 2] = a4[2]; As[buf][ar * A_LD + ac + 3] = a4[3];            \
    *(f32x4v*)(&Bs[buf][br * B_LD + bc]) = b4a;                                          \
    *(f32x4v*)(&Bs[buf][(br + 8) * B_LD + bc]) = b4b;
    const int wm = wid >> 1, wn = wid & 1;           // wave tile 32 x 64
    const int r16 = lane & 15, g = lane >> 4;
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nk = K / BK;
    LOAD_T(0)
    STORE_T(0)
    __syncthreads();
    for (int ks = 0; ks < nk; ++ks) {
        const int buf = ks & 1;
        if (ks + 1 < nk) { LOAD_T((ks + 1) * BK) }
#pragma unroll
        for (int kk = 0; kk < BK; kk += 4) {
            // A fragment: lane holds A[m = r16][k = kk + g]; B fragment: B[k = kk + g][n = r16]
            float af[2], bf[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = As[buf][(wm * 32 + 16 * i + r16) * A_LD + kk + g];
#pragma unroll
            for (int j = 0; j < 4; ++j) bf[j] = Bs[buf][(kk + g) * B_LD + wn * 64 + 16 * j + r16];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        if (ks + 1 < nk) { STORE_T(buf ^ 1) }
        __syncthreads();
    }
#undef LOAD_T
#undef STORE_T
    // C layout: lane holds rows 4 g + e, column r16 of each 16 x 16 tile
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int m = m0 + wm * 32 + 16 * i + 4 * g + e;
            if (m < M) {
                float* cp = C + (size_t)m * N + n0 + wn * 64 + r16;
#pragma unroll
                for (int j = 0; j < 4; ++j) cp[16 * j] = acc[i][j][e];
            }
        }
}

__global__ __launch_bounds__(256) void l2norm_rows_kernel(float* __restrict__ x, int M, int D) {
    leaf_fp16_sat_mode();
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float* xr = x + (size_t)row * D;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) s += xr[c] * xr[c];
    const float inv = 1.0f / fmaxf(sqrtf(wave_sum(s)), 1e-12f);   // F.normalize eps
    for (int c = lane; c < D; c += 64) xr[c] *= inv;
}

}  // namespace

bool leaf_project_rows_ok(int d, int D) { return D % BN == 0 && d % BK == 0 && d % 4 == 0 && d <= 4 * 64 * MAXCH; }

// out[M, D] = [normalize](LN(xg[M, d]; g, b) @ proj[d, D]); xn = [M, d] fp32 scratch
hipError_t leaf_launch_project_rows(const float* xg, const float* g, const float* b, float eps, const float* proj,
                                    float* xn, float* out, int M, int d, int D, int normalize, hipStream_t s) {
    if (!leaf_project_rows_ok(d, D) || M < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ln_rows_f32_kernel, dim3((M + 3) / 4), dim3(256), 0, s, xg, g, b, eps, xn, M, d);
    hipLaunchKernelGGL(proj_f32_kernel, dim3(((M + BM - 1) / BM) * (D / BN)), dim3(256), 0, s, xn, proj, out, M, D, d);
    if (normalize) hipLaunchKernelGGL(l2norm_rows_kernel, dim3((M + 3) / 4), dim3(256), 0, s, out, M, D);
    return hipGetLastError();
}

bool leaf_hidden_rows_ok(int d) { return d >= 4 && d % 4 == 0 && d <= 4 * 64 * MAXCH; }

// out[n_seq, ctx, d] (fp32, or 16-bit of `dtype` with out16) = the chunk's residual rows by (sequence, position), zeros behind a
// sequence's kept rows; x16 == null: x = fp32 rows, else x = the remainder bytes beside the 16-bit copy x16 (`dtype`)
hipError_t leaf_launch_hidden_rows(const void* x, const void* x16, const float* g, const float* b, float eps, int final_ln, void* out,
                                   int out16, int n_seq, RowMap map, int d, int dtype, hipStream_t s) {
    if (!leaf_hidden_rows_ok(d) || n_seq < 1 || !x || !out || (final_ln && (!g || !b))) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(((size_t)n_seq * map.ctx + 3) / 4));
#define HIDDEN_ROWS(TT, LO8, OUT16)                                                                                           \
    hipLaunchKernelGGL((hidden_rows_kernel<TT, LO8, OUT16>), grid, dim3(256), 0, s, x, (const u16*)x16, g, b, eps, final_ln, out, n_seq, \
                       map, d)
#define HIDDEN_ROWS_T(TT)                                                 \
    do {                                                                  \
        if (x16) { if (out16) HIDDEN_ROWS(TT, true, true); else HIDDEN_ROWS(TT, true, false); }    \
        else { if (out16) HIDDEN_ROWS(TT, false, true); else HIDDEN_ROWS(TT, false, false); }      \
    } while (0)
    if (dtype == LEAF_F16) HIDDEN_ROWS_T(F16); else HIDDEN_ROWS_T(BF16);
#undef HIDDEN_ROWS_T
#undef HIDDEN_ROWS
    return hipGetLastError();
}
