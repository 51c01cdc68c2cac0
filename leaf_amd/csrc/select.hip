// Segmented top-n selection over ragged loss rows (leaf_select_topk, include/leaf_hip.h): the position pick of Charmer's
// stage 1 (torch.topk, utils_attacks.py:506) and the arg-max of its stage 2 and of the brute-force search (:574, :438), for
// many captions per launch.  Rows are padded to a common width; count[b] says how many leading columns of row b are real.
//
// One workgroup (4 waves) per row, n rounds of a block arg-max.  Round r looks only at the elements that rank AFTER round
// r-1's pick in the total order "NaN first, then larger value, then lower column", so no exclusion set is kept and the picks
// come out in descending order with ties broken by column: exactly a stable descending sort.  No arithmetic touches a value.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "engine.h"

namespace {

__global__ __launch_bounds__(256) void select_topk_kernel(const float* __restrict__ loss, int ld, const int32_t* __restrict__ count,
                                                          int n, int col_offset, int accumulate, int32_t* __restrict__ idx,
                                                          float* __restrict__ val) {
    leaf_fp16_sat_mode();            // the convention of every kernel here (tests/test_host_cpu.py), though no 16-bit value is made
    __shared__ float s_v[4];
    __shared__ int s_j[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int cnt = count[b];
    cnt = cnt < 0 ? 0 : (cnt > ld ? ld : cnt);
    const float* row = loss + (size_t)b * ld;
    const int m = n < cnt ? n : cnt;
    float pv = 0.f;
    int pj = -1;                                     // previous pick; -1: round 0 (every element is eligible)
    for (int r = 0; r < m; ++r) {
        float bv = 0.f;
        int bj = -1;
        for (int j = tid; j < cnt; j += 256) {
            const float v = row[j];
            if (pj < 0 || ranks_before(pv, pj, v, j)) keep_better(bv, bj, v, j);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oj = __shfl_xor(bj, o, 64);
            keep_better(bv, bj, ov, oj);
        }
        if (lane == 0) { s_v[wid] = bv; s_j[wid] = bj; }
        __syncthreads();
        bv = s_v[0];
        bj = s_j[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) keep_better(bv, bj, s_v[w], s_j[w]);
        __syncthreads();                             // every thread has read s_v / s_j before the next round writes them
        pv = bv;
        pj = bj;
        if (tid == 0) {
            if (!accumulate) {
                idx[(size_t)b * n + r] = bj;
                val[(size_t)b * n + r] = bv;
            } else {
                // merge into the running (value, index) of the earlier chunks: replaced only by a STRICTLY greater value, so the
                // first maximum of the whole candidate list wins (NaN counts as greater than every number, a later NaN loses)
                const float cv = val[b];
                const int ci = idx[b];
                const bool nb = __builtin_isnan(bv), nc = __builtin_isnan(cv);
                if (ci < 0 || (nb && !nc) || (!nb && !nc && bv > cv)) {
                    idx[b] = col_offset + bj;
                    val[b] = bv;
                }
            }
        }
    }
    if (!accumulate) {
        for (int r = m + tid; r < n; r += 256) {
            idx[(size_t)b * n + r] = -1;
            val[(size_t)b * n + r] = -INFINITY;
        }
    }
}

}  // namespace

extern "C" int leaf_select_topk(const float* loss, int ld, const int32_t* count, int B, int n, int col_offset, int accumulate,
                                int32_t* idx, float* val, leaf_stream_t s) {
    if (B < 0 || ld < 1 || n < 1 || col_offset < 0 || (B > 0 && (!loss || !count || !idx || !val))) {
        leaf_set_error("leaf_select_topk: null/invalid argument");
        return 1;
    }
    if (accumulate && n != 1) { leaf_set_error("leaf_select_topk: accumulate needs n == 1 (got %d)", n); return 1; }
    if (B == 0) return 0;
    hipLaunchKernelGGL(select_topk_kernel, dim3(B), dim3(256), 0, (hipStream_t)s, loss, ld, count, n, col_offset, accumulate ? 1 : 0,
                       idx, val);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { leaf_set_error("leaf_select_topk: %s", hipGetErrorString(e)); return 1; }
    return 0;
}
