// The eval-mode forward of NAFAgent.act() for ONE state by one workgroup of PA_THREADS threads, up to the heads' pre-activations in
// LDS: ONE body for policy_act_kernel (csrc/policy_act.hip) and for the vector step's fused launch (csrc/vector_step.hip), which
// goes on to step the state's environment. Every multiply-add is spelled out (act_body.h), so both launches produce the same bits.
//
// One state is a chain of three matrix-VECTOR products (330 KB of weights, L2-resident): they are streamed with
// coalesced 16-byte loads, a wave per group of output rows, every lane holding four consecutive inputs; the per-row
// partial sums of the 64 lanes are folded by a recursive-halving exchange (a lane keeps half of its values and sends
// the other half at each xor level), 32 values in 32 cross-lane moves instead of 192.
#pragma once
#include "act_body.h"
#include "head_body.h"

#define PA_H 256
#define PA_H2 512
#define PA_THREADS 512
#define PA_WAVES (PA_THREADS / 64)
#define PA_ROWS_PER_WAVE (PA_H / PA_WAVES)   // 32 output rows of layer 2 per wave
#define PA_MAX_S ACT_MAX_S
// G: lanes of the state's group in the noise body — 8, or 16 for 9 .. 11 joints (round 6: NH up to 78 rows of Wh; the heads loop walks
// NH as it finds it, so the wider kernel differs in its LDS arrays and in the noise body's lane map only)
#define PA_MAX_NH_WIDE 80
#define PA_MAX_A_WIDE 11

typedef float pa_f4 __attribute__((ext_vector_type(4)));

// v[0..31]: this lane's partial sums of 32 rows. Returns the sum over the 64 lanes of row `*row_out` (every lane ends
// with one finished row; lanes l and l ^ 32 hold the same one).
__device__ static inline float pa_fold32(float (&v)[32], int lane, int* row_out) {
    float a[16], b[8], c[4], d[2];
    const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4, b3 = lane & 8, b4 = lane & 16;
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = (b0 ? v[16 + i] : v[i]) + __shfl_xor(b0 ? v[i] : v[16 + i], 1);
#pragma unroll
    for (int i = 0; i < 8; ++i) b[i] = (b1 ? a[8 + i] : a[i]) + __shfl_xor(b1 ? a[i] : a[8 + i], 2);
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = (b2 ? b[4 + i] : b[i]) + __shfl_xor(b2 ? b[i] : b[4 + i], 4);
#pragma unroll
    for (int i = 0; i < 2; ++i) d[i] = (b3 ? c[2 + i] : c[i]) + __shfl_xor(b3 ? c[i] : c[2 + i], 8);
    float e = (b4 ? d[1] : d[0]) + __shfl_xor(b4 ? d[0] : d[1], 16);
    e += __shfl_xor(e, 32);
    *row_out = (b0 ? 16 : 0) + (b1 ? 8 : 0) + (b2 ? 4 : 0) + (b3 ? 2 : 0) + (b4 ? 1 : 0);
    return e;
}

// Layer size 256. sObs[PA_MAX_S] (zeros beyond S), sA1 / sA2[PA_H] (16-byte aligned), sHeads[NH]: LDS of the calling kernel. On
// return sHeads holds the NH pre-activations of state s and every thread has passed a workgroup barrier behind the last write.
__device__ __forceinline__ static void policy_act_256_body(
    const float* __restrict__ obs, int ldobs, int S, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ g1, const float* __restrict__ be1, const float* __restrict__ W2,
    const float* __restrict__ b2, const float* __restrict__ g2, const float* __restrict__ be2,
    const float* __restrict__ Wh, int ldw, int NH, const float* __restrict__ rm1, const float* __restrict__ rv1,
    const float* __restrict__ rm2, const float* __restrict__ rv2, float eps, float* __restrict__ heads_out, int ldh,
    float* sObs, float* sA1, float* sA2, float* sHeads, const int64_t s) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- layer 1: thread j owns output j (K = S <= 32: a row of W1 is 84 B at S = 21) --------------------------------
    if (tid < PA_MAX_S) sObs[tid] = tid < S ? obs[s * ldobs + tid] : 0.f;
    float w1[PA_MAX_S];
    float p1 = 0.f, q1 = 0.f, r1 = 0.f, t1 = 0.f, u1 = 0.f;
    if (tid < PA_H) {
#pragma unroll
        for (int k = 0; k < PA_MAX_S; ++k) w1[k] = k < S ? W1[(int64_t)tid * S + k] : 0.f;
        p1 = b1[tid]; q1 = g1[tid]; r1 = be1[tid]; t1 = rm1[tid]; u1 = rv1[tid];
    }
    // layer-2 rows of this wave and the BatchNorm parameters of the row this lane will finish: requested now, they do
    // not depend on layer 1
    const int rloc = ((lane & 1) ? 16 : 0) + ((lane & 2) ? 8 : 0) + ((lane & 4) ? 4 : 0) + ((lane & 8) ? 2 : 0) +
                     ((lane & 16) ? 1 : 0);
    const int row2 = wave * PA_ROWS_PER_WAVE + rloc;
    const float p2 = b2[row2], q2 = g2[row2], r2 = be2[row2], t2 = rm2[row2], u2 = rv2[row2];
    pa_f4 w2[PA_ROWS_PER_WAVE];
#pragma unroll
    for (int r = 0; r < PA_ROWS_PER_WAVE; ++r)
        w2[r] = *(const pa_f4*)(W2 + (int64_t)(wave * PA_ROWS_PER_WAVE + r) * PA_H + 4 * lane);
    __syncthreads();
    if (tid < PA_H) sA1[tid] = act_layer1_row(w1, sObs, p1, q1, r1, t1, u1, eps);
    __syncthreads();

    // ---- layer 2: wave w owns rows 32 w .. 32 w + 31, lane l the inputs 4 l .. 4 l + 3 --------------------------------
    {
        const pa_f4 x = *(const pa_f4*)(sA1 + 4 * lane);
        float part[PA_ROWS_PER_WAVE];
#pragma unroll
        for (int r = 0; r < PA_ROWS_PER_WAVE; ++r) part[r] = act_dot4(w2[r], x);
        int rfold;
        const float z = pa_fold32(part, lane, &rfold);      // rfold == rloc
        if (lane < 32) sA2[row2] = act_bn_relu(z + p2, t2, u2, q2, r2, eps);
    }
    __syncthreads();

    // ---- heads: NH <= 45 (G = 16: 78) rows of Wh[NHP][ldw]; column PA_H of Wh is the bias (the activations' constant-1 column) ------
    {
        const pa_f4 x = *(const pa_f4*)(sA2 + 4 * lane);
        for (int h = wave; h < NH; h += PA_WAVES) {
            const pa_f4 w = *(const pa_f4*)(Wh + (int64_t)h * ldw + 4 * lane);
            float p = act_sum64(act_dot4(w, x));
            if (lane == 0) {
                p += Wh[(int64_t)h * ldw + PA_H];
                sHeads[h] = p;
                if (heads_out) heads_out[s * ldh + h] = p;
            }
        }
    }
    __syncthreads();
}

// ---- layer size 512 (round 6: widths in (256, 512] are stored as 512, learner.NetLayout) --------------------------------------------
// The same on 512 hidden units: thread j owns output j of layer 1 (512 threads), a wave owns 64 rows of layer 2 — two rounds
// of the 32-row fold, each row's 512 inputs as two float4 per lane (inputs 4 l .. 4 l + 3 and 256 + 4 l .. 256 + 4 l + 3, one fmaf
// chain through both: act_dot4 -> act_dot4_acc) — and the heads rows likewise. adam_act_kernel<.., 512> (csrc/step_path.hip) runs the
// same arithmetic in the same order. sA1 / sA2[PA_H2].
__device__ __forceinline__ static void policy_act_512_body(
    const float* __restrict__ obs, int ldobs, int S, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ g1, const float* __restrict__ be1, const float* __restrict__ W2,
    const float* __restrict__ b2, const float* __restrict__ g2, const float* __restrict__ be2,
    const float* __restrict__ Wh, int ldw, int NH, const float* __restrict__ rm1, const float* __restrict__ rv1,
    const float* __restrict__ rm2, const float* __restrict__ rv2, float eps, float* __restrict__ heads_out, int ldh,
    float* sObs, float* sA1, float* sA2, float* sHeads, const int64_t s) {
    constexpr int H = PA_H2, RPW = H / PA_WAVES;             // 64 rows of layer 2 per wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < PA_MAX_S) sObs[tid] = tid < S ? obs[s * ldobs + tid] : 0.f;
    float w1[PA_MAX_S];
#pragma unroll
    for (int k = 0; k < PA_MAX_S; ++k) w1[k] = k < S ? W1[(int64_t)tid * S + k] : 0.f;
    const float p1 = b1[tid], q1 = g1[tid], r1 = be1[tid], t1 = rm1[tid], u1 = rv1[tid];
    __syncthreads();
    sA1[tid] = act_layer1_row(w1, sObs, p1, q1, r1, t1, u1, eps);
    __syncthreads();
    // ---- layer 2 ---------------------------------------------------------------------------------------------------------------
    {
        const int rloc = ((lane & 1) ? 16 : 0) + ((lane & 2) ? 8 : 0) + ((lane & 4) ? 4 : 0) + ((lane & 8) ? 2 : 0) + ((lane & 16) ? 1 : 0);
        const pa_f4 x0 = *(const pa_f4*)(sA1 + 4 * lane), x1 = *(const pa_f4*)(sA1 + 256 + 4 * lane);
        for (int rnd = 0; rnd < RPW / 32; ++rnd) {
            const int row0 = wave * RPW + 32 * rnd, row2 = row0 + rloc;
            const float p2 = b2[row2], q2 = g2[row2], r2 = be2[row2], t2 = rm2[row2], u2 = rv2[row2];
            float part[32];
            pa_f4 w[32];
#pragma unroll
            for (int r = 0; r < 32; ++r) w[r] = *(const pa_f4*)(W2 + (int64_t)(row0 + r) * H + 4 * lane);
#pragma unroll
            for (int r = 0; r < 32; ++r) part[r] = act_dot4(w[r], x0);
#pragma unroll
            for (int r = 0; r < 32; ++r) w[r] = *(const pa_f4*)(W2 + (int64_t)(row0 + r) * H + 256 + 4 * lane);
#pragma unroll
            for (int r = 0; r < 32; ++r) part[r] = act_dot4_acc(w[r], x1, part[r]);
            int rfold;
            const float z = pa_fold32(part, lane, &rfold);  // rfold == rloc
            if (lane < 32) sA2[row2] = act_bn_relu(z + p2, t2, u2, q2, r2, eps);
        }
    }
    __syncthreads();
    // ---- heads ------------------------------------------------------------------------------------------------------------------
    {
        const pa_f4 x0 = *(const pa_f4*)(sA2 + 4 * lane), x1 = *(const pa_f4*)(sA2 + 256 + 4 * lane);
        for (int h = wave; h < NH; h += PA_WAVES) {
            const pa_f4 w0 = *(const pa_f4*)(Wh + (int64_t)h * ldw + 4 * lane), w1h = *(const pa_f4*)(Wh + (int64_t)h * ldw + 256 + 4 * lane);
            float p = act_sum64(act_dot4_acc(w1h, x1, act_dot4(w0, x0)));
            if (lane == 0) {
                p += Wh[(int64_t)h * ldw + H];
                sHeads[h] = p;
                if (heads_out) heads_out[s * ldh + h] = p;
            }
        }
    }
    __syncthreads();
}
