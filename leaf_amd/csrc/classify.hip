// Classification margin loss of Charmer's zero-shot attack (attack_text_charmer_classification, utils_attacks.py:582-643;
// margin_loss_lm :145-151) over a class matrix shared by all captions, for many captions per launch:
//   logit[c]  = <feat[b,r], class_feat[c]>                       (both unit rows: the cosine similarity)
//   loss[b,r] = max_{c != label[b]} logit[c] - logit[label[b]]   (NaN when any logit is NaN)
//   pred[b,r] = first arg-max of logit over c                    (:630-631; softmax does not move it)
// and per caption best_idx[b] = first arg-max of loss[b,:] in the order of leaf_select_topk (common.h ranks_before), best_feat.
//
// Two launches.  cls_margin_kernel: one wave per 4 candidates, classes in groups of 4, so a pass over D reads 4 + 4 rows for 16
// inner products.  Every (candidate, class) product is summed the same way whatever the launch looks like: lane l adds columns
// 4 l + 256 i (+0, +1, +2, +3 in that order) with fmaf, i ascending, then the xor butterfly of wave_sum -- B, rho, the candidate's
// place in its tile and the class's place in its group never enter, which is what "batched equals one at a time, bit for bit"
//  needs.  cls_best_kernel: one workgroup per caption, one round of the selection order over its loss row.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int TR = 4;   // candidates per wave
constexpr int TC = 4;   // classes per pass over D

template <bool VEC4>
__global__ __launch_bounds__(256) void cls_margin_kernel(const float* __restrict__ feat, const float* __restrict__ cls,
                                                         const int32_t* __restrict__ label, int n_cand, int rho, int C, int D,
                                                         float* __restrict__ loss, int32_t* __restrict__ pred,
                                                         float* __restrict__ logits) {
    leaf_fp16_sat_mode();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int r0 = (blockIdx.x * 4 + wid) * TR;
    if (r0 >= n_cand) return;
    const float* f[TR];
    int lab[TR];
    float lt[TR], mo[TR], pv[TR];      // logit of the label, maximum of the others, running arg-max of all (value, class)
    int pi[TR];
    bool bad[TR];                      // a NaN logit seen
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        const int i = r0 + r < n_cand ? r0 + r : n_cand - 1;      // a tail slot recomputes the last candidate and writes nothing
        f[r] = feat + (size_t)i * D;
        lab[r] = label[i / rho];
        lt[r] = 0.f; mo[r] = -INFINITY; pv[r] = 0.f; pi[r] = -1; bad[r] = false;
    }
    for (int c0 = 0; c0 < C; c0 += TC) {
        const float* g[TC];
#pragma unroll
        for (int q = 0; q < TC; ++q) g[q] = cls + (size_t)(c0 + q < C ? c0 + q : C - 1) * D;
        float acc[TR][TC];
#pragma unroll
        for (int r = 0; r < TR; ++r)
#pragma unroll
            for (int q = 0; q < TC; ++q) acc[r][q] = 0.f;
        if (VEC4) {
            for (int j = 4 * lane; j < D; j += 256) {
                float4 fv[TR], gv[TC];
#pragma unroll
                for (int r = 0; r < TR; ++r) fv[r] = *(const float4*)(f[r] + j);
#pragma unroll
                for (int q = 0; q < TC; ++q) gv[q] = *(const float4*)(g[q] + j);
#pragma unroll
                for (int r = 0; r < TR; ++r)
#pragma unroll
                    for (int q = 0; q < TC; ++q) {
                        float s = acc[r][q];
                        s = fmaf(fv[r].x, gv[q].x, s); s = fmaf(fv[r].y, gv[q].y, s);
                        s = fmaf(fv[r].z, gv[q].z, s); s = fmaf(fv[r].w, gv[q].w, s);
                        acc[r][q] = s;
                    }
            }
        } else {
            // D % 4 != 0: the same columns per lane, one at a time (rows are not 16-byte aligned)
            for (int j0 = 4 * lane; j0 < D; j0 += 256)
                for (int j = j0; j < j0 + 4 && j < D; ++j) {
                    float fv[TR], gv[TC];
#pragma unroll
                    for (int r = 0; r < TR; ++r) fv[r] = f[r][j];
#pragma unroll
                    for (int q = 0; q < TC; ++q) gv[q] = g[q][j];
#pragma unroll
                    for (int r = 0; r < TR; ++r)
#pragma unroll
                        for (int q = 0; q < TC; ++q) acc[r][q] = fmaf(fv[r], gv[q], acc[r][q]);
                }
        }
        // the bookkeeping is written as selects, not as keep_better's branch: c ascends, so an equal logit never replaces the
        // running arg-max and "NaN first, larger value, lower class" needs only the three cases below
#pragma unroll
        for (int q = 0; q < TC; ++q) {
            const int c = c0 + q;
            const bool real = c < C;                              // wave-uniform; a tail class is summed and dropped
#pragma unroll
            for (int r = 0; r < TR; ++r) {
                const float v = wave_sum(acc[r][q]);              // every lane holds the sum
                if (logits && real && lane == 0 && r0 + r < n_cand) logits[(size_t)(r0 + r) * C + c] = v;
                const bool vn = __builtin_isnan(v), pn = __builtin_isnan(pv[r]);
                const bool is_label = c == lab[r];
                bad[r] = bad[r] | (real & vn);
                lt[r] = (real & is_label) ? v : lt[r];
                mo[r] = (real & !is_label & (v > mo[r])) ? v : mo[r];
                const bool take = real & ((pi[r] < 0) | (vn & !pn) | (!vn & !pn & (v > pv[r])));
                pv[r] = take ? v : pv[r];
                pi[r] = take ? c : pi[r];
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < TR; ++r)
            if (r0 + r < n_cand) {
                if (loss) loss[r0 + r] = bad[r] ? __builtin_nanf("") : mo[r] - lt[r];
                if (pred) pred[r0 + r] = pi[r];
            }
    }
}

// best_idx[b] = first of loss[b, 0..rho) in the order "NaN first, larger value, lower column" (one round of select_topk_kernel),
// best_feat[b,:] = that candidate's feature row
__global__ __launch_bounds__(256) void cls_best_kernel(const float* __restrict__ loss, const float* __restrict__ feat, int rho, int D,
                                                       int32_t* __restrict__ best_idx, float* __restrict__ best_feat) {
    leaf_fp16_sat_mode();
    __shared__ float s_v[4];
    __shared__ int s_j[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float* row = loss + (size_t)b * rho;
    float bv = 0.f;
    int bj = -1;
    for (int j = tid; j < rho; j += 256) keep_better(bv, bj, row[j], j);
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
    if (tid == 0) best_idx[b] = bj;
    if (best_feat) {
        const float* f = feat + ((size_t)b * rho + bj) * D;
        for (int j = tid; j < D; j += 256) best_feat[(size_t)b * D + j] = f[j];
    }
}

}  // namespace

hipError_t leaf_launch_classify(const float* feat, const float* class_feat, const int32_t* label, int B, int rho, int D, int C,
                                float* loss, int32_t* pred, float* logits, int32_t* best_idx, float* best_feat, hipStream_t s) {
    if (B < 1 || D < 1 || rho < 1 || rho > LEAF_SCORE_MAX_RHO || C < LEAF_CLS_MIN_CLASSES || C > LEAF_CLS_MAX_CLASSES || !loss)
        return hipErrorInvalidValue;
    const int n_cand = B * rho;
    const dim3 grid((n_cand + 4 * TR - 1) / (4 * TR));
    if ((D & 3) == 0)
        hipLaunchKernelGGL(cls_margin_kernel<true>, grid, dim3(256), 0, s, feat, class_feat, label, n_cand, rho, C, D, loss, pred, logits);
    else
        hipLaunchKernelGGL(cls_margin_kernel<false>, grid, dim3(256), 0, s, feat, class_feat, label, n_cand, rho, C, D, loss, pred, logits);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cls_best_kernel, dim3(B), dim3(256), 0, s, loss, feat, rho, D, best_idx, best_feat);
    return hipGetLastError();
}
