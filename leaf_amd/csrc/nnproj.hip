// Vocabulary projection of text embedding inversion (PEZ: nn_project, src/pez/optim_utils.py:26-55): every query row is replaced
// by its cosine-nearest row of the token-embedding table,
//   ids[m] = first arg-max over v of (q[m] . table[v]) * inv_norm[v],      cos[m] = that value / ||q[m]||
// an [M, d] x [V, d]^T product fused with a row arg-max, exact fp32 on the matrix cores (v_mfma_f32_16x16x4_f32: fp32 operands,
// fp32 accumulate, as project.hip).  The weights are frozen during an inversion, so the table norms are computed once
// (vocab_inv_norms_kernel) instead of on every call.
//
//   nn_slab_kernel    the VOCABULARY is stationary: a workgroup owns a slab of 16 NJ table rows, loads it into LDS once and sweeps
//                     all M query rows against it (the queries are a few MB and stay in L2), so the table is read once per call
//                     and not once per M tile.  A wave takes 32 query rows at a time: 2 x NJ accumulator tiles.  Per row it writes
//                     the slab's best (value, id) to the workspace.
//   nn_merge_kernel   reduces the slabs of a row in the total order of every selection here (common.h ranks_before: NaN first,
//                     larger value, lower id), so two identical table rows resolve to the lower id and a NaN query returns id 0.
//
// ONE summation order per (query row, vocabulary id): 16 columns per step, k0 ascending; inside a step lane group g multiplies
// columns k0 + 4 g + e in the MFMA of e = 0..3, every product into the same accumulator.  M, the row's slot in its tile, the slab
// height and the launch never enter, so a row gets the same bits alone and inside any batch.  No float atomics, no scratch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int NN_MAX_D = 2048;
constexpr int NN_PAD = 4;                        // floats between LDS slab rows
constexpr size_t NN_LDS_BUDGET = 144 * 1024;     // of the 160 KB of a CU

// inv_norm[v] = 1 / max(||table[v]||, 1e-12) (F.normalize's eps); one wave per row, lane l adds columns 4 l + 256 i in order
__global__ __launch_bounds__(256) void vocab_inv_norms_kernel(const float* __restrict__ table, int V, int d, float* __restrict__ inv_norm) {
    leaf_fp16_sat_mode();
    const int lane = threadIdx.x & 63, v = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= V) return;
    const float* t = table + (size_t)v * d;
    float s = 0.f;
    for (int j = 4 * lane; j < d; j += 256) {
        const float4 x = *(const float4*)(t + j);
        s = fmaf(x.x, x.x, s); s = fmaf(x.y, x.y, s); s = fmaf(x.z, x.z, s); s = fmaf(x.w, x.w, s);
    }
    s = wave_sum(s);
    if (lane == 0) inv_norm[v] = 1.0f / fmaxf(sqrtf(s), 1e-12f);
}

template <int NJ>
__global__ __launch_bounds__(256) void nn_slab_kernel(const float* __restrict__ q, int M, const float* __restrict__ table,
                                                      const float* __restrict__ inv_norm, int V, int d, float* __restrict__ ws_val,
                                                      int32_t* __restrict__ ws_id) {
    leaf_fp16_sat_mode();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* slab = (float*)smem;                  // [16 NJ][d + NN_PAD]
    constexpr int SV = 16 * NJ;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, r16 = lane & 15, g = lane >> 4;
    const int ld = d + NN_PAD, nq = d >> 2;
    const int v0 = blockIdx.x * SV;
    // a row behind the end of the vocabulary repeats the last one; its id is -1 below and never selected
    for (int i = tid; i < SV * nq; i += 256) {
        const int r = i / nq, c = i - r * nq;
        const int v = v0 + r < V ? v0 + r : V - 1;
        *(f32x4*)(slab + (size_t)r * ld + 4 * c) = *(const f32x4*)(table + (size_t)v * d + 4 * c);
    }
    __syncthreads();
    float inv[NJ];
    int vid[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int v = v0 + 16 * j + r16;
        vid[j] = v < V ? v : -1;
        inv[j] = v < V ? inv_norm[v] : 0.f;
    }
    const f32x4 z4 = f32x4{0.f, 0.f, 0.f, 0.f};
    const int mtiles = (M + 31) / 32;
    for (int t = wid; t < mtiles; t += 4) {
        const int m0 = t * 32;
        // a row behind M repeats the last query and is not written
        const float* a0 = q + (size_t)(m0 + r16 < M ? m0 + r16 : M - 1) * d;
        const float* a1 = q + (size_t)(m0 + 16 + r16 < M ? m0 + 16 + r16 : M - 1) * d;
        const float* bs = slab + (size_t)r16 * ld;
        f32x4 acc[2][NJ];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = z4;
        for (int k0 = 0; k0 < d; k0 += 16) {
            // lane (r16, g) holds columns k0 + 4 g .. + 3 of query row r16 and of table row r16 of each tile; MFMA e multiplies
            // column k0 + 4 g + e of both (the MFMA's k index is g).  A step behind d (d % 16 != 0) multiplies zeros.
            const int k = k0 + 4 * g;
            const bool ok = k < d;
            const f32x4 av0 = ok ? *(const f32x4*)(a0 + k) : z4;
            const f32x4 av1 = ok ? *(const f32x4*)(a1 + k) : z4;
            f32x4 bv[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) bv[j] = ok ? *(const f32x4*)(bs + (size_t)16 * j * ld + k) : z4;
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av0[e], bv[j][e], acc[0][j], 0, 0, 0);
                    acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av1[e], bv[j][e], acc[1][j], 0, 0, 0);
                }
        }
        // C layout: lane holds query rows 4 g + e, vocabulary column r16 of each 16 x 16 tile
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float bval = 0.f;
                int bid = -1;
#pragma unroll
                for (int j = 0; j < NJ; ++j) keep_better(bval, bid, acc[i][j][e] * inv[j], vid[j]);
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    const float ov = __shfl_xor(bval, o, 64);
                    const int oi = __shfl_xor(bid, o, 64);
                    keep_better(bval, bid, ov, oi);
                }
                const int m = m0 + 16 * i + 4 * g + e;
                if (r16 == 0 && m < M) {
                    ws_val[(size_t)blockIdx.x * M + m] = bval;
                    ws_id[(size_t)blockIdx.x * M + m] = bid;
                }
            }
    }
}

// 64 query rows per workgroup: lane = row, the four waves share the slabs, then one wave per 16 rows for ||q||
__global__ __launch_bounds__(256) void nn_merge_kernel(const float* __restrict__ ws_val, const int32_t* __restrict__ ws_id, int nslab,
                                                       const float* __restrict__ q, int M, int d, int32_t* __restrict__ ids,
                                                       float* __restrict__ cosv) {
    leaf_fp16_sat_mode();
    __shared__ float s_v[4][64];
    __shared__ int s_j[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int m = blockIdx.x * 64 + lane;
    float bval = 0.f;
    int bid = -1;
    if (m < M)
        for (int s = wid; s < nslab; s += 4) keep_better(bval, bid, ws_val[(size_t)s * M + m], ws_id[(size_t)s * M + m]);
    s_v[wid][lane] = bval;
    s_j[wid][lane] = bid;
    __syncthreads();
    if (wid == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) keep_better(bval, bid, s_v[w][lane], s_j[w][lane]);
        if (m < M) ids[m] = bid;
        s_v[0][lane] = bval;
    }
    if (!cosv) return;
    __syncthreads();
    for (int r = 16 * wid; r < 16 * wid + 16; ++r) {
        const int mr = blockIdx.x * 64 + r;
        if (mr >= M) break;
        const float* x = q + (size_t)mr * d;
        float s = 0.f;
        for (int j = 4 * lane; j < d; j += 256) {
            const float4 v = *(const float4*)(x + j);
            s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
        }
        s = wave_sum(s);
        if (lane == 0) cosv[mr] = s_v[0][r] * (1.0f / fmaxf(sqrtf(s), 1e-12f));
    }
}

// table rows per slab: as many of 64 / 32 / 16 as fit the LDS budget
int slab_tiles(int d) {
    const size_t row = (size_t)(d + NN_PAD) * 4;
    return 64 * row <= NN_LDS_BUDGET ? 4 : 32 * row <= NN_LDS_BUDGET ? 2 : 1;
}

}  // namespace

bool leaf_nn_project_ok(int d) { return d >= 4 && d % 4 == 0 && d <= NN_MAX_D; }

int leaf_nn_project_slabs(int V, int d) {
    const int sv = 16 * slab_tiles(d);
    return (V + sv - 1) / sv;
}

hipError_t leaf_launch_vocab_inv_norms(const float* table, int V, int d, float* inv_norm, hipStream_t s) {
    if (!leaf_nn_project_ok(d) || V < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vocab_inv_norms_kernel, dim3((V + 3) / 4), dim3(256), 0, s, table, V, d, inv_norm);
    return hipGetLastError();
}

hipError_t leaf_launch_nn_project(const float* q, int M, const float* table, const float* inv_norm, int V, int d, int32_t* ids,
                                  float* cosv, void* ws, hipStream_t s) {
    if (!leaf_nn_project_ok(d) || M < 1 || V < 1) return hipErrorInvalidValue;
    const int nj = slab_tiles(d), nslab = leaf_nn_project_slabs(V, d);
    const size_t lds = (size_t)16 * nj * (d + NN_PAD) * 4;
    float* ws_val = (float*)ws;
    int32_t* ws_id = (int32_t*)(ws_val + (size_t)nslab * M);
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute((const void*)nn_slab_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)NN_LDS_BUDGET);
        (void)hipFuncSetAttribute((const void*)nn_slab_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)NN_LDS_BUDGET);
        (void)hipFuncSetAttribute((const void*)nn_slab_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)NN_LDS_BUDGET);
        attr = true;
    }
    if (nj == 4) hipLaunchKernelGGL(nn_slab_kernel<4>, dim3(nslab), dim3(256), lds, s, q, M, table, inv_norm, V, d, ws_val, ws_id);
    else if (nj == 2) hipLaunchKernelGGL(nn_slab_kernel<2>, dim3(nslab), dim3(256), lds, s, q, M, table, inv_norm, V, d, ws_val, ws_id);
    else hipLaunchKernelGGL(nn_slab_kernel<1>, dim3(nslab), dim3(256), lds, s, q, M, table, inv_norm, V, d, ws_val, ws_id);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(nn_merge_kernel, dim3((M + 63) / 64), dim3(256), 0, s, ws_val, ws_id, nslab, q, M, d, ids, cosv);
    return hipGetLastError();
}
