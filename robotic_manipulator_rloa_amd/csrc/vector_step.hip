// The launches AROUND the updates of a many-env vector step (engine.DeviceEnvLoop + engine.UpdateChunk), fused (gfx950):
//
//   naf_vec_act_env_append      act() for E states, the E stand-in envs' step, the append of the E rows to the replay ring and the
//                               step counter: ONE launch of E workgroups where there were four (policy_act_kernel,
//                               synth_env_step_kernel, counter_add_kernel, replay_add_small_kernel).
//   naf_vec_draw_gather_moments the draw of U minibatches, their gather and the moments of layer 1's inputs: ONE launch of U
//                               workgroups where there were four (replay_sample_kernel, counter_add_kernel,
//                               replay_gather_rows_kernel, bb_moments_kernel); a minibatch stays in LDS between its gather and its
//                               moments instead of going to memory and back.
//
// Both compile the bodies the separate launches compile (policy_act_body.h, synth_env_body.h, sample_body.h, moments_body.h), so
// every word they leave is the same bits. No workgroup waits for another: what must happen once per launch (the ring's counters, the
// step counter, the stream positions) is done by the LAST workgroup to arrive at a ticket — one returning atomic add, the idiom of
// policy_act_kernel — from the values every workgroup read at its start, which nobody rewrites before the last ticket is taken.
#include "policy_act_body.h"
#include "synth_env_body.h"
#include "sample_body.h"
#include "moments_body.h"
#include "replay_dev.h"

// =====================================================================================================================
// naf_vec_act_env_append
// =====================================================================================================================
#define VS_MAX_ROW_FLOATS 128

struct VecEnvArgs {
    float* env_state;          // [E][ENV_STATE_FLOATS]
    float* rows;               // [E][row_floats]
    uint64_t env_seed;
    uint64_t* step_ctr;
    int max_frames, record_slots;
    naf_episode_record_t* records;
    float4* ring;              // nullable: no replay, nothing appended
    uint64_t* meta;
    uint64_t cap;
    int rf4_shift, row_floats;
};

// Workgroup e: the act body for state e (all eight waves); then wave 0 alone goes on — lane 0 steps env e on LDS copies of the
// env's words, the action, the observation and the row (the body's accesses are LDS round trips, not dependent trips to memory),
// and the wave stores what the separate launches store: the action, the env's words, the next observation, rows[e] and ring slot
// (head + e) % capacity. The observation and the env's words are read into LDS before the first of the act body's barriers.
template <int PMODE, int H>
__global__ __launch_bounds__(PA_THREADS) void naf_vec_act_env_append_kernel(
    float* obs, int S, const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ g1,
    const float* __restrict__ be1, const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ g2,
    const float* __restrict__ be2, const float* __restrict__ Wh, int ldw, int NH, const float* __restrict__ rm1,
    const float* __restrict__ rv1, const float* __restrict__ rm2, const float* __restrict__ rv2, float eps, float* heads_out, int ldh,
    float* action_out, uint64_t seed, uint64_t* counter_dev, uint32_t* ticket, float noise_scale, int A, const VecEnvArgs V) {
    constexpr int G = 8;
    __shared__ float sObs[PA_MAX_S];
    __shared__ __attribute__((aligned(16))) float sA1[H];
    __shared__ __attribute__((aligned(16))) float sA2[H];
    __shared__ float sHeads[HEAD_MAX_LDH];
    __shared__ float sL[PMODE == NAF_P_MATMUL ? G * (G + 1) : 1];
    __shared__ float sAct[G];
    __shared__ __attribute__((aligned(16))) float sSt[ENV_STATE_FLOATS];
    __shared__ __attribute__((aligned(16))) float sRow[VS_MAX_ROW_FLOATS];
    const int tid = threadIdx.x;
    const int e = blockIdx.x, E = gridDim.x;
    // what the launch's last workgroup advances, as every workgroup finds it
    const uint64_t ctr = *counter_dev;
    const uint64_t step = *V.step_ctr;
    uint64_t head = 0, size = 0, total = 0;
    if (V.ring) {
        head = V.meta[META_HEAD];
        size = V.meta[META_SIZE];
        total = V.meta[META_TOTAL];
    }
    if (tid < ENV_STATE_FLOATS) sSt[tid] = V.env_state[(int64_t)e * ENV_STATE_FLOATS + tid];

    if (H == PA_H)
        policy_act_256_body(obs, S, S, W1, b1, g1, be1, W2, b2, g2, be2, Wh, ldw, NH, rm1, rv1, rm2, rv2, eps, heads_out, ldh, sObs,
                            sA1, sA2, sHeads, (int64_t)e);
    else
        policy_act_512_body(obs, S, S, W1, b1, g1, be1, W2, b2, g2, be2, Wh, ldw, NH, rm1, rv1, rm2, rv2, eps, heads_out, ldh, sObs,
                            sA1, sA2, sHeads, (int64_t)e);
    // mu, exploration noise, clamp: the draw of (seed, stream position, state e, lane), the action left in LDS
    const float z = naf_act_noise_z(seed, ctr, (int64_t)e, tid & (G - 1), tid < G && (tid & (G - 1)) < A);
    naf_act_noise_body_z<PMODE, G>(sHeads, sL, sAct, z, noise_scale, 0, tid < G, A, tid);
    if (tid >= 64) return;

    // ---- environment.step of env e: lane 0, on LDS --------------------------------------------------------------------
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");      // (the wave's own LDS stores above: in place before lane 0 reads them)
    __builtin_amdgcn_wave_barrier();
    if (tid == 0)
        synth_env_step_body(sSt, sAct, sRow, sObs, e, E, A, V.row_floats, V.env_seed, step, V.max_frames, V.records, V.record_slots);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    if (tid < A) action_out[(int64_t)e * A + tid] = sAct[tid];
    if (tid < ENV_STATE_FLOATS) V.env_state[(int64_t)e * ENV_STATE_FLOATS + tid] = sSt[tid];
    if (tid < S) obs[(int64_t)e * S + tid] = sObs[tid];
    if (tid < (1 << V.rf4_shift)) {
        const float4 v = ((const float4*)sRow)[tid];
        ((float4*)V.rows)[((int64_t)e << V.rf4_shift) + tid] = v;
        if (V.ring) {
            const uint64_t phys = (head + (uint64_t)e) % V.cap;
            V.ring[(phys << V.rf4_shift) + tid] = v;
        }
    }
    // the ticket, behind the workgroup's stores: the last workgroup to get here does the launch's bookkeeping
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0) {
        if (atomicAdd(ticket, 1u) == (unsigned)E - 1u) {
            *ticket = 0;
            *counter_dev = ctr + 1;                             // the noise stream
            *V.step_ctr = step + 1;
            if (V.ring) {                                       // ReplayBuffer.add of E rows (replay_add_small_kernel)
                V.meta[META_HEAD] = (head + (uint64_t)E) % V.cap;
                const uint64_t s2 = size + (uint64_t)E;
                V.meta[META_SIZE] = s2 > V.cap ? V.cap : s2;
                V.meta[META_TOTAL] = total + (uint64_t)E;
            }
        }
    }
}

extern "C" int naf_vec_act_env_append(float* obs, int S, const float* W1, const float* b1, const float* g1, const float* be1,
                                      const float* W2, const float* b2, const float* g2, const float* be2, const float* Wh, int ldw,
                                      int NH, const float* running_mean1, const float* running_var1, const float* running_mean2,
                                      const float* running_var2, float eps, int H, float* heads_out, int ldh, float* action_out,
                                      uint64_t seed, uint64_t* counter_dev, uint32_t* ticket, float noise_scale, int E, int A,
                                      int p_mode, const naf_vec_env_t* env, void* stream) {
    if (!obs || !W1 || !b1 || !g1 || !be1 || !W2 || !b2 || !g2 || !be2 || !Wh || !running_mean1 || !running_var1 ||
        !running_mean2 || !running_var2 || !action_out || !counter_dev || !ticket || !env)
        return NAF_ERR_ARG;
    if ((H != PA_H && H != PA_H2) || E <= 0 || A <= 0 || A > NAF_MAX_A || S != 2 * A + 9 || S > PA_MAX_S) return NAF_ERR_ARG;
    if (NH != A + A * (A + 1) / 2 + 1 || NH > HEAD_MAX_LDH || ldw <= H || (ldw & 3) != 0) return NAF_ERR_ARG;
    if ((((uintptr_t)W2 | (uintptr_t)Wh) & 15) != 0 || (heads_out && ldh < NH)) return NAF_ERR_ARG;
    if (p_mode != NAF_P_HADAMARD && p_mode != NAF_P_MATMUL) return NAF_ERR_ARG;
    if (!env->env_state || !env->rows || !env->step_ctr || ((uintptr_t)env->rows & 15) != 0) return NAF_ERR_ARG;
    if (env->records && env->record_slots <= 0) return NAF_ERR_ARG;
    VecEnvArgs V;
    V.env_state = env->env_state;
    V.rows = env->rows;
    V.env_seed = env->env_seed;
    V.step_ctr = env->step_ctr;
    V.max_frames = env->max_frames;
    V.record_slots = env->record_slots;
    V.records = env->records;
    V.row_floats = naf_replay_row_floats(S, A);
    if (V.row_floats > VS_MAX_ROW_FLOATS) return NAF_ERR_ARG;
    V.rf4_shift = 0;
    while ((1 << V.rf4_shift) < V.row_floats / 4) ++V.rf4_shift;
    V.ring = nullptr;
    V.meta = nullptr;
    V.cap = 1;
    if (env->replay) {
        const naf_replay_t* h = env->replay;
        if (h->magic != NAF_REPLAY_MAGIC) return NAF_ERR_STATE;
        // the regime of the one-workgroup append: E rows of row_floats / 4 float4 are at most 1024 float4
        if (h->S != S || h->A != A || h->row_floats != V.row_floats || (uint64_t)E > h->capacity ||
            (int64_t)E * (V.row_floats / 4) > 1024)
            return NAF_ERR_ARG;
        V.ring = (float4*)h->rows;
        V.meta = h->meta;
        V.cap = h->capacity;
    }
    hipStream_t st = (hipStream_t)stream;
#define VS_GO(PM, HV)                                                                                                              \
    naf_vec_act_env_append_kernel<PM, HV><<<E, PA_THREADS, 0, st>>>(obs, S, W1, b1, g1, be1, W2, b2, g2, be2, Wh, ldw, NH,           \
                                                                    running_mean1, running_var1, running_mean2, running_var2, eps,  \
                                                                    heads_out, ldh, action_out, seed, counter_dev, ticket,          \
                                                                    noise_scale, A, V)
    if (H == PA_H2) {
        if (p_mode == NAF_P_HADAMARD) VS_GO(NAF_P_HADAMARD, PA_H2);
        else VS_GO(NAF_P_MATMUL, PA_H2);
    } else {
        if (p_mode == NAF_P_HADAMARD) VS_GO(NAF_P_HADAMARD, PA_H);
        else VS_GO(NAF_P_MATMUL, PA_H);
    }
#undef VS_GO
    NAF_CHECK_LAUNCH();
    return NAF_OK;
}

// =====================================================================================================================
// naf_vec_draw_gather_moments
// =====================================================================================================================
#define VD_THREADS 1024
#define VD_RPT 4
#define VD_MAX_B 256
#define VD_MAX_ROWS_BYTES 65536                          // the minibatch in LDS: B rows of out_ld floats
#define VD_MAX_DYN_LDS (146 * 1024)                      // 2 x BmShared (82,176) + the positions (1,024) + the minibatch (65,536)

struct VecDrawArgs {
    const float4* ring;
    uint64_t* meta;
    uint64_t cap;
    int rf4_shift;
    uint64_t seed;
    uint64_t* counter;         // the sampler's stream position: minibatch u draws at *counter + u; advanced by U
    uint32_t* ticket;
    int32_t* idx_out;          // [U][B]
    float4* out_rows;          // [U][B][w4]
    int w4, trunc_lo, trunc_hi, off_s2_4;
    float* mom;                // [U][2][KP + KP * KP]
    int B, without_replacement, hash_bits;
};

// Workgroup u: the draw of minibatch u (sample_body.h), its B rows from the ring into LDS, the moments of both nets' layer-1 inputs
// from there (moments_body.h: threads 0 .. 511 the states, 512 .. 1023 the next states), then everything it leaves in memory in
// one go — batch[u] (the update chain reads it from memory), idx[u], moments[u].
template <int K4>
__global__ __launch_bounds__(VD_THREADS) void naf_vec_draw_gather_moments_kernel(const VecDrawArgs P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vd_smem[];
    constexpr int KP = 4 * K4, REC = KP + KP * KP;
    BmShared* S = (BmShared*)vd_smem;                                  // [2]: one per net; the draw's table lives here first
    int* sPos = (int*)(vd_smem + 2 * sizeof(BmShared));                // [B]: physical ring rows of the minibatch
    float4* sRows = (float4*)(vd_smem + 2 * sizeof(BmShared) + (size_t)naf_round_up(P.B, 4) * sizeof(int));
    int* vals = (int*)vd_smem;
    const int tid = threadIdx.x, B = P.B;
    const int64_t u = blockIdx.x;
    const uint64_t head = P.meta[META_HEAD], size = P.meta[META_SIZE];
    const uint64_t ctr0 = *P.counter;

    // ---- random.sample --------------------------------------------------------------------------------------------------
    replay_sample_body(vals, tid, VD_THREADS, size, ctr0 + (uint64_t)u, P.seed, B, P.without_replacement, P.hash_bits);
    const uint64_t base = head + P.cap - size;          // physical position of deque element 0 (oldest)
    int myidx = 0;                                      // (B <= VD_MAX_B: thread t owns element t)
    if (tid < B) {
        int64_t i = (int64_t)vals[tid];
        myidx = (int)i;
        if (i < 0 || (uint64_t)i >= size) {
            atomicAdd((unsigned long long*)&P.meta[META_BAD_IDX], 1ull);
            i = 0;
        }
        uint64_t pos = base + (uint64_t)i;
        pos = pos >= P.cap ? pos - P.cap : pos;
        pos = pos >= P.cap ? pos - P.cap : pos;
        sPos[tid] = (int)pos;
    }
    __syncthreads();                                    // (the draw's table is dead: it becomes the moments' staging area)

    // ---- the minibatch rows: one lane per output float4, VD_RPT in flight -----------------------------------------------------
    const unsigned w4 = (unsigned)P.w4;
    const int total4 = B * P.w4;
    for (int j0 = tid; j0 < total4; j0 += VD_THREADS * VD_RPT) {
        float4 v[VD_RPT];
        int col[VD_RPT];
#pragma unroll
        for (int k = 0; k < VD_RPT; ++k) {
            const int j = j0 + VD_THREADS * k;
            const unsigned jj = j < total4 ? (unsigned)j : 0u;
            const unsigned r = jj / w4;
            col[k] = (int)(jj - r * w4);
            v[k] = P.ring[((int64_t)sPos[r] << P.rf4_shift) + col[k]];
        }
#pragma unroll
        for (int k = 0; k < VD_RPT; ++k) {
            const int j = j0 + VD_THREADS * k;
            if (j < total4) sRows[j] = naf_row_trunc4(v[k], 4 * col[k], P.trunc_lo, P.trunc_hi);
        }
    }

    // ---- the moments of layer 1's inputs (the body's first barrier orders the rows above before its reads) -----------------------
    const int net = tid >> 9;
    const int c0 = net ? P.off_s2_4 : 0;                // (c0 + K4 <= w4, checked on the host: a record never runs past its row)
    bb_moments_body<K4>([&](int row, int q) { return sRows[row * P.w4 + c0 + q]; }, S[net], tid & (BM_THREADS - 1),
                        P.mom + (u * 2 + net) * REC, B);

    float4* out = P.out_rows + u * (int64_t)total4;
    for (int j = tid; j < total4; j += VD_THREADS) out[j] = sRows[j];
    if (tid < B) P.idx_out[u * B + tid] = myidx;
    // the ticket: the last workgroup to get here moves the sampler's stream on by the launch's U draws
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0) {
        if (atomicAdd(P.ticket, 1u) == gridDim.x - 1) {
            *P.ticket = 0;
            *P.counter = ctr0 + (uint64_t)gridDim.x;
        }
    }
}

extern "C" int naf_vec_draw_gather_moments(naf_replay_t* h, uint64_t seed, uint64_t* counter_dev, uint32_t* ticket, int32_t* idx_out,
                                           float* out_rows, int out_ld, int action_mode, float* mom, int B, int n_batches,
                                           int without_replacement, void* stream) {
    if (!h || h->magic != NAF_REPLAY_MAGIC) return NAF_ERR_STATE;
    if (!counter_dev || !ticket || !idx_out || !out_rows || !mom || B <= 0 || B > VD_MAX_B || n_batches <= 0) return NAF_ERR_ARG;
    if ((((uintptr_t)out_rows | (uintptr_t)mom) & 15) != 0 || ((uintptr_t)counter_dev & 7) != 0) return NAF_ERR_ARG;
    if (action_mode != NAF_ACTION_TRUNC_INT && action_mode != NAF_ACTION_FLOAT) return NAF_ERR_ARG;
    // the row the learner's kernels and the moments expect, all of a net's K4 float4 inside it, and B of them within the LDS
    const int k4 = (h->S + 3) / 4, k4d = k4 <= 6 ? 6 : 8;
    if (k4 > 8 || out_ld != naf_replay_batch_row_floats(h->S, h->A) || naf_row_off_s2(h->S, h->A) + 4 * k4d > out_ld) return NAF_ERR_ARG;
    if ((size_t)B * out_ld * sizeof(float) > VD_MAX_ROWS_BYTES) return NAF_ERR_ARG;
    VecDrawArgs P;
    P.ring = (const float4*)h->rows;
    P.meta = h->meta;
    P.cap = h->capacity;
    P.rf4_shift = 0;
    while ((1 << P.rf4_shift) < h->row_floats / 4) ++P.rf4_shift;
    P.seed = seed;
    P.counter = counter_dev;
    P.ticket = ticket;
    P.idx_out = idx_out;
    P.out_rows = (float4*)out_rows;
    P.w4 = out_ld / 4;
    P.trunc_lo = h->S;
    P.trunc_hi = h->S + h->A;
    if (action_mode == NAF_ACTION_FLOAT) P.trunc_lo = P.trunc_hi = 0x7fffffff;
    P.off_s2_4 = naf_row_off_s2(h->S, h->A) / 4;
    P.mom = mom;
    P.B = B;
    P.without_replacement = without_replacement;
    P.hash_bits = sample_hash_bits(B);
    const size_t lds = 2 * sizeof(BmShared) + (size_t)naf_round_up(B, 4) * sizeof(int) + (size_t)B * out_ld * sizeof(float);
    if (sample_lds_ints(B, P.hash_bits) * sizeof(int) > 2 * sizeof(BmShared) || lds > VD_MAX_DYN_LDS) return NAF_ERR_ARG;
    static int raised_dev[64];                           // per device: the kernels' dynamic-LDS limit raised once
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!raised_dev[dev]) {
        const void* ks[2] = {(const void*)naf_vec_draw_gather_moments_kernel<6>, (const void*)naf_vec_draw_gather_moments_kernel<8>};
        for (const void* k : ks) {
            hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, VD_MAX_DYN_LDS);
            if (e != hipSuccess) return (int)e;
        }
        raised_dev[dev] = 1;
    }
    if (k4d == 6) naf_vec_draw_gather_moments_kernel<6><<<n_batches, VD_THREADS, lds, (hipStream_t)stream>>>(P);
    else naf_vec_draw_gather_moments_kernel<8><<<n_batches, VD_THREADS, lds, (hipStream_t)stream>>>(P);
    NAF_CHECK_LAUNCH();
    return NAF_OK;
}
