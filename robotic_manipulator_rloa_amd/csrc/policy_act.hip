// NAFAgent.act() for E states in ONE launch (gfx950): the eval-mode forward of the main network — Linear, BatchNorm
// with running statistics, ReLU, twice; the three head Linears — and the exploration noise, one workgroup per state.
// Replaces naf_algorithm.py:158-178 / naf_neural_network.py:76-87,119-121 for a batch of states: seven launches before
// (3 GEMMs, 2 BN kernels, noise, counter), and at one state per call (the reference's own loop) nearly all of act()'s
// device time was their launch boundaries.
//
// One state is a chain of three matrix-VECTOR products (330 KB of weights, L2-resident): they are streamed with
// coalesced 16-byte loads, a wave per group of output rows, every lane holding four consecutive inputs; the per-row
// partial sums of the 64 lanes are folded by a recursive-halving exchange (a lane keeps half of its values and sends
// the other half at each xor level), 32 values in 32 cross-lane moves instead of 192.
// The hidden width is the framework's fixed 256 (rl_framework.py:452): H is a compile-time constant here.
#include "policy_act_body.h"

template <int PMODE, int G>
__global__ __launch_bounds__(PA_THREADS) void policy_act_kernel(
    const float* __restrict__ obs, int ldobs, int S, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ g1, const float* __restrict__ be1, const float* __restrict__ W2,
    const float* __restrict__ b2, const float* __restrict__ g2, const float* __restrict__ be2,
    const float* __restrict__ Wh, int ldw, int NH, const float* __restrict__ rm1, const float* __restrict__ rv1,
    const float* __restrict__ rm2, const float* __restrict__ rv2, float eps, float* __restrict__ heads_out, int ldh,
    float* __restrict__ action_out, uint64_t seed, uint64_t* __restrict__ counter_dev, uint32_t* __restrict__ ticket,
    float noise_scale, int E, int A) {
    __shared__ float sObs[PA_MAX_S];
    __shared__ __attribute__((aligned(16))) float sA1[PA_H];
    __shared__ __attribute__((aligned(16))) float sA2[PA_H];
    __shared__ float sHeads[G == 8 ? HEAD_MAX_LDH : PA_MAX_NH_WIDE];
    __shared__ float sL[PMODE == NAF_P_MATMUL ? G * (G + 1) : 1];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.x;
    const uint64_t ctr = *counter_dev;                      // advanced by the LAST workgroup to finish, below

    // ---- the forward up to the heads' pre-activations (csrc/policy_act_body.h) ---------------------------------------------
    policy_act_256_body(obs, ldobs, S, W1, b1, g1, be1, W2, b2, g2, be2, Wh, ldw, NH, rm1, rv1, rm2, rv2, eps, heads_out, ldh,
                        sObs, sA1, sA2, sHeads, s);

    // ---- mu, exploration noise, clamp: the first G lanes are this state's group ------------------------------------------
    naf_act_noise_body<PMODE, G>(sHeads, sL, action_out, seed, ctr, noise_scale, s, tid < G && s < E, A, tid);

    // the noise stream moves on once every workgroup has read the counter: the last one to get here advances it
    if (tid == 0) {
        if (atomicAdd(ticket, 1u) == gridDim.x - 1) {
            *ticket = 0;
            *counter_dev = ctr + 1;
        }
    }
}

// ---- layer size 512: policy_act_512_body --------------------------------------------------------------------------------------------
template <int PMODE, int G>
__global__ __launch_bounds__(PA_THREADS) void policy_act_512_kernel(
    const float* __restrict__ obs, int ldobs, int S, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ g1, const float* __restrict__ be1, const float* __restrict__ W2,
    const float* __restrict__ b2, const float* __restrict__ g2, const float* __restrict__ be2,
    const float* __restrict__ Wh, int ldw, int NH, const float* __restrict__ rm1, const float* __restrict__ rv1,
    const float* __restrict__ rm2, const float* __restrict__ rv2, float eps, float* __restrict__ heads_out, int ldh,
    float* __restrict__ action_out, uint64_t seed, uint64_t* __restrict__ counter_dev, uint32_t* __restrict__ ticket,
    float noise_scale, int E, int A) {
    constexpr int H = PA_H2;
    __shared__ float sObs[PA_MAX_S];
    __shared__ __attribute__((aligned(16))) float sA1[H];
    __shared__ __attribute__((aligned(16))) float sA2[H];
    __shared__ float sHeads[G == 8 ? HEAD_MAX_LDH : PA_MAX_NH_WIDE];
    __shared__ float sL[PMODE == NAF_P_MATMUL ? G * (G + 1) : 1];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.x;
    const uint64_t ctr = *counter_dev;
    policy_act_512_body(obs, ldobs, S, W1, b1, g1, be1, W2, b2, g2, be2, Wh, ldw, NH, rm1, rv1, rm2, rv2, eps, heads_out, ldh,
                        sObs, sA1, sA2, sHeads, s);
    naf_act_noise_body<PMODE, G>(sHeads, sL, action_out, seed, ctr, noise_scale, s, tid < G && s < E, A, tid);
    if (tid == 0) {
        if (atomicAdd(ticket, 1u) == gridDim.x - 1) {
            *ticket = 0;
            *counter_dev = ctr + 1;
        }
    }
}

extern "C" int naf_policy_act(const float* obs, int ldobs, int S, const float* W1, const float* b1, const float* g1,
                              const float* be1, const float* W2, const float* b2, const float* g2, const float* be2,
                              const float* Wh, int ldw, int NH, const float* running_mean1, const float* running_var1,
                              const float* running_mean2, const float* running_var2, float eps, int H, float* heads_out,
                              int ldh, float* action_out, uint64_t seed, uint64_t* counter_dev, uint32_t* ticket,
                              float noise_scale, int E, int A, int p_mode, void* stream) {
    if (!obs || !W1 || !b1 || !g1 || !be1 || !W2 || !b2 || !g2 || !be2 || !Wh || !running_mean1 || !running_var1 ||
        !running_mean2 || !running_var2 || !action_out || !counter_dev || !ticket)
        return NAF_ERR_ARG;
    if ((H != PA_H && H != PA_H2) || S <= 0 || S > PA_MAX_S || ldobs < S || E <= 0 || A <= 0 || A > PA_MAX_A_WIDE) return NAF_ERR_ARG;
    if (NH != A + A * (A + 1) / 2 + 1 || NH > (A > NAF_MAX_A ? PA_MAX_NH_WIDE : HEAD_MAX_LDH) || ldw <= H || (ldw & 3) != 0) return NAF_ERR_ARG;
    if ((((uintptr_t)W2 | (uintptr_t)Wh) & 15) != 0 || (heads_out && ldh < NH)) return NAF_ERR_ARG;
    if (p_mode != NAF_P_HADAMARD && p_mode != NAF_P_MATMUL) return NAF_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
#define PA_GO(PM, GV)                                                                                                         \
    policy_act_kernel<PM, GV><<<E, PA_THREADS, 0, st>>>(obs, ldobs, S, W1, b1, g1, be1, W2, b2, g2, be2, Wh, ldw, NH, running_mean1, \
                                                       running_var1, running_mean2, running_var2, eps, heads_out, ldh, action_out,  \
                                                       seed, counter_dev, ticket, noise_scale, E, A)
#define PA_GO2(PM, GV)                                                                                                        \
    policy_act_512_kernel<PM, GV><<<E, PA_THREADS, 0, st>>>(obs, ldobs, S, W1, b1, g1, be1, W2, b2, g2, be2, Wh, ldw, NH, running_mean1, \
                                                           running_var1, running_mean2, running_var2, eps, heads_out, ldh, action_out,  \
                                                           seed, counter_dev, ticket, noise_scale, E, A)
    if (H == PA_H2) {
        if (p_mode == NAF_P_HADAMARD) {
            if (A > NAF_MAX_A) PA_GO2(NAF_P_HADAMARD, 16);
            else PA_GO2(NAF_P_HADAMARD, 8);
        } else {
            if (A > NAF_MAX_A) PA_GO2(NAF_P_MATMUL, 16);
            else PA_GO2(NAF_P_MATMUL, 8);
        }
    } else if (p_mode == NAF_P_HADAMARD) {
        if (A > NAF_MAX_A) PA_GO(NAF_P_HADAMARD, 16);
        else PA_GO(NAF_P_HADAMARD, 8);
    } else {
        if (A > NAF_MAX_A) PA_GO(NAF_P_MATMUL, 16);
        else PA_GO(NAF_P_MATMUL, 8);
    }
#undef PA_GO2
#undef PA_GO
    NAF_CHECK_LAUNCH();
    return NAF_OK;
}
