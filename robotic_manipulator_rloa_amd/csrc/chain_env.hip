// Kinematic environment of a user's manipulator, E independent copies stepped on the device: the serial chain that
// environment/urdf_chain.py compiles from a URDF (driven joints with folded pre-transforms, capsule segments, observation
// slots), under the reference's environment rule — the contract csrc/synth_env.hip keeps for its one hard-wired chain:
//   state  = [pos(A), vel(A), end-effector xyz, target xyz, obstacle xyz]   (environment.py:431-451, S = 9+2A; slot k of
//            pos / vel reports joint INDEX k, environment.py:442-444)
//   reward = +250 on reaching the target (dist < 0.05), -1000 on obstacle contact, else -(dist - 0.05)
//            (environment.py:345-371, :419-429);  done = 1 on either (environment.py:311-333)
//   step   = velocity control for one 1/240 s tick, applied exactly, then the position limits (environment.py:453-485)
// NOT a port of Bullet: no dynamics, no mesh collision, no self-collision. environment/kinematic.py is its float64 twin.
//
// One lane per env, 64-lane workgroups. The model is the same for every lane and is read through a uniform pointer with
// uniform indices (scalar loads / one broadcast line); nothing of it is copied into per-lane arrays. The walk keeps only the
// current frame (R, p) in registers; joint values and actions are read from and written to env_state / the row as the walk
// reaches them, so there is no runtime-indexed per-lane array and nothing goes to scratch, at any A <= 64.
#include "common.h"
#include "../../include/naf_hip.h"

#include <cmath>
#include <new>

#define CH_DT (1.0f / 240.0f)
#define CH_MAX_A NAF_MAX_A_WIDE
// blob offsets (include/naf_hip.h, "chain model blob")
#define CH_HDR NAF_CHAIN_HEADER_FLOATS
#define CH_JNT NAF_CHAIN_JOINT_FLOATS
#define CH_SEG NAF_CHAIN_SEGMENT_FLOATS

struct naf_chain_env {
    float* model_dev;
    int n_floats, A, n_seg;
};

struct ChainScene {
    float v[NAF_CHAIN_SCENE_FLOATS];    // target | obstacle | jitter | obstacle radius
};

__host__ __device__ static inline int ch_off_begin(int A) { return CH_HDR + CH_JNT * A; }
__host__ __device__ static inline int ch_off_seg(int A) { return ch_off_begin(A) + A + 2; }
__host__ __device__ static inline int ch_off_slot(int A, int n_seg) { return ch_off_seg(A) + CH_SEG * n_seg; }
// env_state record of one env (include/naf_hip.h): q[A] | target[3] | obstacle[3] | obstacle radius | frame | episode | score (double)
__host__ __device__ static inline int ch_off_score(int A) { return naf_round_up(A + 9, 2); }
__host__ __device__ static inline int ch_state_floats(int A) { return naf_round_up(ch_off_score(A) + 2, 4); }

// squared distance from c to the segment a-b, projection clamped to [0, 1]
__device__ static inline float seg_point_dist2(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy,
                                               float cz) {
    const float ux = bx - ax, uy = by - ay, uz = bz - az;
    const float wx = cx - ax, wy = cy - ay, wz = cz - az;
    const float den = ux * ux + uy * uy + uz * uz;
    float t = den > 0.f ? (wx * ux + wy * uy + wz * uz) / den : 0.f;
    t = fminf(1.f, fmaxf(0.f, t));
    const float dx = wx - t * ux, dy = wy - t * uy, dz = wz - t * uz;
    return dx * dx + dy * dy + dz * dz;
}

struct Frame {
    float r00, r01, r02, r10, r11, r12, r20, r21, r22, px, py, pz;
};

// contact of the capsules of frame f with the obstacle sphere, and the end-effector point when it lives in f
__device__ static inline bool frame_geometry(const float* __restrict__ model, int A, int f, const Frame& F, float ox, float oy,
                                             float oz, float orad, int ee_frame, float* ee) {
    const float* begin = model + ch_off_begin(A);
    const float* segs = model + ch_off_seg(A);
    const int s0 = (int)begin[f], s1 = (int)begin[f + 1];
    bool hit = false;
    for (int s = s0; s < s1; ++s) {
        const float* g = segs + s * CH_SEG;
        const float ax = F.px + F.r00 * g[1] + F.r01 * g[2] + F.r02 * g[3];
        const float ay = F.py + F.r10 * g[1] + F.r11 * g[2] + F.r12 * g[3];
        const float az = F.pz + F.r20 * g[1] + F.r21 * g[2] + F.r22 * g[3];
        const float bx = F.px + F.r00 * g[4] + F.r01 * g[5] + F.r02 * g[6];
        const float by = F.py + F.r10 * g[4] + F.r11 * g[5] + F.r12 * g[6];
        const float bz = F.pz + F.r20 * g[4] + F.r21 * g[5] + F.r22 * g[6];
        const float rr = g[7] + orad;
        hit |= seg_point_dist2(ax, ay, az, bx, by, bz, ox, oy, oz) < rr * rr;
    }
    if (f == ee_frame) {
        ee[0] = F.px + F.r00 * model[5] + F.r01 * model[6] + F.r02 * model[7];
        ee[1] = F.py + F.r10 * model[5] + F.r11 * model[6] + F.r12 * model[7];
        ee[2] = F.pz + F.r20 * model[5] + F.r21 * model[6] + F.r22 * model[7];
    }
    return hit;
}

// Walks the chain at the joint values in st[0 .. A): writes the position slots, the constants' slots (velocity 0), the end
// effector, target and obstacle into the observation `o`; the DRIVEN joints' velocity slots are the caller's. Returns contact.
__device__ static inline bool chain_walk(const float* __restrict__ model, int A, int n_seg, const float* st, float* o, float* ee) {
    const int ee_frame = (int)model[4];
    const float ox = st[A + 3], oy = st[A + 4], oz = st[A + 5], orad = st[A + 6];
    Frame F = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    ee[0] = ee[1] = ee[2] = 0.f;
    bool hit = frame_geometry(model, A, 0, F, ox, oy, oz, orad, ee_frame, ee);
    for (int m = 0; m < A; ++m) {
        const float* j = model + CH_HDR + m * CH_JNT;
        const float q = st[m];
        const int slot = (int)j[21];
        if (slot >= 0) o[slot] = q;
        // p += R . t_pre ;  R = R . R_pre
        F.px += F.r00 * j[9] + F.r01 * j[10] + F.r02 * j[11];
        F.py += F.r10 * j[9] + F.r11 * j[10] + F.r12 * j[11];
        F.pz += F.r20 * j[9] + F.r21 * j[10] + F.r22 * j[11];
        Frame G;
        G.r00 = F.r00 * j[0] + F.r01 * j[3] + F.r02 * j[6];
        G.r01 = F.r00 * j[1] + F.r01 * j[4] + F.r02 * j[7];
        G.r02 = F.r00 * j[2] + F.r01 * j[5] + F.r02 * j[8];
        G.r10 = F.r10 * j[0] + F.r11 * j[3] + F.r12 * j[6];
        G.r11 = F.r10 * j[1] + F.r11 * j[4] + F.r12 * j[7];
        G.r12 = F.r10 * j[2] + F.r11 * j[5] + F.r12 * j[8];
        G.r20 = F.r20 * j[0] + F.r21 * j[3] + F.r22 * j[6];
        G.r21 = F.r20 * j[1] + F.r21 * j[4] + F.r22 * j[7];
        G.r22 = F.r20 * j[2] + F.r21 * j[5] + F.r22 * j[8];
        const float x = j[12], y = j[13], z = j[14];
        if (j[15] != 0.f) {      // prismatic: translate along the axis
            F.r00 = G.r00; F.r01 = G.r01; F.r02 = G.r02;
            F.r10 = G.r10; F.r11 = G.r11; F.r12 = G.r12;
            F.r20 = G.r20; F.r21 = G.r21; F.r22 = G.r22;
            F.px += (G.r00 * x + G.r01 * y + G.r02 * z) * q;
            F.py += (G.r10 * x + G.r11 * y + G.r12 * z) * q;
            F.pz += (G.r20 * x + G.r21 * y + G.r22 * z) * q;
        } else {                 // revolute: Rodrigues, Rot = I + s K + (1 - c) K^2 for the unit axis (x, y, z)
            float s, c;
            sincosf(q, &s, &c);
            const float v = 1.f - c;
            const float m00 = 1.f - v * (y * y + z * z), m01 = v * x * y - s * z, m02 = v * x * z + s * y;
            const float m10 = v * x * y + s * z, m11 = 1.f - v * (x * x + z * z), m12 = v * y * z - s * x;
            const float m20 = v * x * z - s * y, m21 = v * y * z + s * x, m22 = 1.f - v * (x * x + y * y);
            F.r00 = G.r00 * m00 + G.r01 * m10 + G.r02 * m20;
            F.r01 = G.r00 * m01 + G.r01 * m11 + G.r02 * m21;
            F.r02 = G.r00 * m02 + G.r01 * m12 + G.r02 * m22;
            F.r10 = G.r10 * m00 + G.r11 * m10 + G.r12 * m20;
            F.r11 = G.r10 * m01 + G.r11 * m11 + G.r12 * m21;
            F.r12 = G.r10 * m02 + G.r11 * m12 + G.r12 * m22;
            F.r20 = G.r20 * m00 + G.r21 * m10 + G.r22 * m20;
            F.r21 = G.r20 * m01 + G.r21 * m11 + G.r22 * m21;
            F.r22 = G.r20 * m02 + G.r21 * m12 + G.r22 * m22;
        }
        hit |= frame_geometry(model, A, m + 1, F, ox, oy, oz, orad, ee_frame, ee);
    }
    const float* slots = model + ch_off_slot(A, n_seg);
    for (int k = 0; k < A; ++k)
        if (slots[2 * k] < 0.f) { o[k] = slots[2 * k + 1]; o[A + k] = 0.f; }
    for (int k = 0; k < 3; ++k) { o[2 * A + k] = ee[k]; o[2 * A + 3 + k] = st[A + k]; o[2 * A + 6 + k] = st[A + 3 + k]; }
    return hit;
}

// initial joint positions + uniform(-variation, +variation): env_reset_one's draw (csrc/synth_env.hip), keyed the same way,
// with init / variation taken from the model; the driven joints' velocity slots of `o` are zeroed
__device__ static inline void chain_reset_one(const float* __restrict__ model, float* st, float* o, int e, int A, uint64_t seed,
                                              uint64_t ctr) {
    for (int k = 0; k < A; k += 4) {
        Philox4 p = philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)e, 0x52455345u + k, (uint32_t)seed,
                                  (uint32_t)(seed >> 32));
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (k + j < A) {
                const float* jr = model + CH_HDR + (k + j) * CH_JNT;
                st[k + j] = fmaf(naf_u01(p.v[j]) * 2.f - 1.f, jr[20], jr[19]);      // 2u - 1 is exact: ONE rounding
                const int slot = (int)jr[21];
                if (slot >= 0) o[A + slot] = 0.f;
            }
    }
    st[A + 7] = 0.f;
    *(double*)(st + ch_off_score(A)) = 0.0;
}

__global__ void chain_env_reset_kernel(const float* __restrict__ model, float* env_state, float* obs, int E, int A, int n_seg,
                                       uint64_t seed, uint64_t ctr, const ChainScene scene) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int nst = ch_state_floats(A);
    float* st = env_state + (int64_t)e * nst;
    float* o = obs + (int64_t)e * (2 * A + 9);
    for (int k = A; k < nst; ++k) st[k] = 0.f;
    for (int k = 0; k < 3; ++k) { st[A + k] = scene.v[k]; st[A + 3 + k] = scene.v[3 + k]; }
    if (scene.v[6] > 0.f) {      // per-env obstacle jitter, drawn once: the stand-in's key
        Philox4 p = philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)e, 0x4f425354u, 0x9E3779B9u, 0x243F6A88u);
        for (int k = 0; k < 3; ++k) st[A + 3 + k] += (naf_u01(p.v[k]) * 2.f - 1.f) * scene.v[6];
    }
    st[A + 6] = scene.v[7];
    chain_reset_one(model, st, o, e, A, seed, ctr);
    float ee[3];
    chain_walk(model, A, n_seg, st, o, ee);
}

__global__ void chain_env_step_kernel(const float* __restrict__ model, float* env_state, const float* __restrict__ actions,
                                      float* __restrict__ out_rows, float* __restrict__ obs_next, int E, int A, int n_seg,
                                      int row_floats, uint64_t seed, const uint64_t* counter_dev, int max_frames,
                                      naf_episode_record_t* __restrict__ records, int record_slots) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int S = 2 * A + 9;
    float* st = env_state + (int64_t)e * ch_state_floats(A);
    float* row = out_rows + (int64_t)e * row_floats;
    float* ob = obs_next + (int64_t)e * S;
    const uint64_t ctr = counter_dev ? *counter_dev : 0ull;
    const int off_s2 = naf_row_off_s2(S, A), off_d = naf_row_off_done(S, A);
    float* o2 = row + off_s2;

    // the observation the action was chosen from is the row's `state`
    for (int k = 0; k < S; ++k) row[k] = ob[k];
    for (int m = 0; m < A; ++m) {
        const float* j = model + CH_HDR + m * CH_JNT;
        const float a = actions[(int64_t)e * A + m];
        row[S + m] = a;
        float q = st[m] + CH_DT * a;      // velocity control: the commanded velocity is reached within the tick
        float vel = a;
        if (j[16] != 0.f) {               // position limits: a joint its limit stopped reports velocity 0
            if (q > j[18]) { q = j[18]; vel = 0.f; }
            if (q < j[17]) { q = j[17]; vel = 0.f; }
        }
        st[m] = q;
        const int slot = (int)j[21];
        if (slot >= 0) o2[A + slot] = vel;
    }
    float ee[3];
    const bool hit = chain_walk(model, A, n_seg, st, o2, ee);
    float dx = ee[0] - st[A], dy = ee[1] - st[A + 1], dz = ee[2] - st[A + 2];
    float dist = sqrtf(dx * dx + dy * dy + dz * dz);
    const bool reached = dist < 0.05f;
    float reward = reached ? 250.f : (hit ? -1000.f : -(dist - 0.05f));
    float done = (reached || hit) ? 1.f : 0.f;
    row[S + A] = reward;
    for (int k = S + A + 1; k < off_s2; ++k) row[k] = 0.f;
    row[off_d] = done;
    for (int k = off_d + 1; k < row_floats; ++k) row[k] = 0.f;

    st[A + 7] += 1.f;
    double* score_p = (double*)(st + ch_off_score(A));
    const double score = *score_p + (double)reward;      // score += reward (naf_algorithm.py:264)
    *score_p = score;
    const bool over = done != 0.f || (max_frames > 0 && st[A + 7] >= (float)max_frames);
    if (records) {
        // one record slot per (vector step mod record_slots, env), written EVERY step: naf_synth_env_step's contract
        naf_episode_record_t rec;
        rec.score = over ? score : 0.0;
        rec.frames = over ? (int32_t)st[A + 7] : 0;
        rec.done = (int32_t)done;
        rec.last_reward = reward;
        rec.episode = (int32_t)st[A + 8] + 1;
        rec.step_lo = (uint32_t)ctr;
        rec.env = (uint32_t)e;
        records[(int64_t)(ctr % (uint64_t)record_slots) * E + e] = rec;
    }
    if (over) {
        // episode over (terminal state, or the frame budget of NAFAgent.run, naf_algorithm.py:249): auto-reset
        st[A + 8] += 1.f;
        chain_reset_one(model, st, ob, e, A, seed, ctr * 0x9E3779B97F4A7C15ull + (uint64_t)st[A + 8]);
        chain_walk(model, A, n_seg, st, ob, ee);
    } else {
        for (int k = 0; k < S; ++k) ob[k] = o2[k];
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static inline bool ch_int(float v, int lo, int hi, int* out) {
    if (!std::isfinite(v) || v != std::floor(v) || v < (float)lo || v > (float)hi) return false;
    *out = (int)v;
    return true;
}

extern "C" int naf_chain_env_model_check(const float* m, int n_floats) {
    if (!m || n_floats < CH_HDR) return NAF_ERR_ARG;
    if (m[0] != (float)NAF_CHAIN_BLOB_VERSION) return NAF_CHAIN_ERR_VERSION;
    int A, n_seg, n_slot, ee_frame, total;
    if (!ch_int(m[1], 1, CH_MAX_A, &A) || !ch_int(m[2], 0, 1 << 20, &n_seg) || !ch_int(m[3], A, A, &n_slot))
        return NAF_CHAIN_ERR_COUNTS;
    if (!ch_int(m[8], CH_HDR, 1 << 24, &total) || total != n_floats || total != ch_off_slot(A, n_seg) + 2 * A)
        return NAF_CHAIN_ERR_SIZE;
    for (int k = 0; k < n_floats; ++k)
        if (!std::isfinite(m[k])) return NAF_CHAIN_ERR_VALUE;
    if (!ch_int(m[4], 0, A, &ee_frame)) return NAF_CHAIN_ERR_EE;
    for (int k = 0; k < A; ++k) {
        const float* j = m + CH_HDR + k * CH_JNT;
        int type, lim, slot;
        const float n2 = j[12] * j[12] + j[13] * j[13] + j[14] * j[14];
        if (!ch_int(j[15], 0, 1, &type) || !ch_int(j[16], 0, 1, &lim) || !ch_int(j[21], -1, A - 1, &slot) ||
            std::fabs(n2 - 1.f) > 1e-4f || (lim && !(j[17] < j[18])) || j[20] < 0.f)
            return NAF_CHAIN_ERR_JOINT;
    }
    const float* begin = m + ch_off_begin(A);
    if (begin[0] != 0.f || begin[A + 1] != (float)n_seg) return NAF_CHAIN_ERR_SEGMENTS;
    for (int f = 0; f <= A; ++f) {
        int b0, b1;
        if (!ch_int(begin[f], 0, n_seg, &b0) || !ch_int(begin[f + 1], b0, n_seg, &b1)) return NAF_CHAIN_ERR_SEGMENTS;
        for (int s = b0; s < b1; ++s) {      // sorted by frame: every segment of [begin[f], begin[f+1]) names frame f
            const float* g = m + ch_off_seg(A) + s * CH_SEG;
            if (g[0] != (float)f || g[7] < 0.f) return NAF_CHAIN_ERR_SEGMENTS;
        }
    }
    const float* slots = m + ch_off_slot(A, n_seg);
    for (int k = 0; k < A; ++k) {
        int src;
        if (!ch_int(slots[2 * k], -1, A - 1, &src)) return NAF_CHAIN_ERR_SLOTS;
        // a driven joint's record and the slot table must name each other
        if (src >= 0 && (int)m[CH_HDR + src * CH_JNT + 21] != k) return NAF_CHAIN_ERR_SLOTS;
    }
    for (int k = 0; k < A; ++k) {
        const int slot = (int)m[CH_HDR + k * CH_JNT + 21];
        if (slot >= 0 && (int)slots[2 * slot] != k) return NAF_CHAIN_ERR_SLOTS;
    }
    return NAF_OK;
}

extern "C" int naf_chain_env_create(const float* model_host, int n_floats, naf_chain_env_t** out) {
    if (!out) return NAF_ERR_ARG;
    *out = nullptr;
    int rc = naf_chain_env_model_check(model_host, n_floats);
    if (rc != NAF_OK) return rc;
    naf_chain_env* h = new (std::nothrow) naf_chain_env();
    if (!h) return NAF_ERR_STATE;
    h->n_floats = n_floats;
    h->A = (int)model_host[1];
    h->n_seg = (int)model_host[2];
    hipError_t e = hipMalloc((void**)&h->model_dev, (size_t)n_floats * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->model_dev, model_host, (size_t)n_floats * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (h->model_dev) (void)hipFree(h->model_dev);
        delete h;
        return (int)e;
    }
    *out = h;
    return NAF_OK;
}

extern "C" int naf_chain_env_destroy(naf_chain_env_t* h) {
    if (!h) return NAF_ERR_ARG;
    hipError_t e = hipFree(h->model_dev);
    delete h;
    return e == hipSuccess ? NAF_OK : (int)e;
}

extern "C" int naf_chain_env_state_floats(const naf_chain_env_t* h) { return h ? ch_state_floats(h->A) : NAF_ERR_ARG; }

extern "C" int naf_chain_env_reset(naf_chain_env_t* h, float* env_state, float* obs, int E, const float* scene_host, uint64_t seed,
                                   uint64_t counter, void* stream) {
    if (!h || !env_state || !obs || !scene_host || E <= 0) return NAF_ERR_ARG;
    ChainScene sc;
    for (int k = 0; k < NAF_CHAIN_SCENE_FLOATS; ++k) sc.v[k] = scene_host[k];
    if (!(sc.v[7] >= 0.f) || !(sc.v[6] >= 0.f)) return NAF_ERR_ARG;
    chain_env_reset_kernel<<<(E + 63) / 64, 64, 0, (hipStream_t)stream>>>(h->model_dev, env_state, obs, E, h->A, h->n_seg, seed,
                                                                          counter, sc);
    NAF_CHECK_LAUNCH();
    return NAF_OK;
}

extern "C" int naf_chain_env_step(naf_chain_env_t* h, float* env_state, const float* actions, float* out_rows, float* obs_next,
                                  int E, uint64_t seed, const uint64_t* counter_dev, int max_frames, naf_episode_record_t* records,
                                  int record_slots, void* stream) {
    if (!h || !env_state || !actions || !out_rows || !obs_next || E <= 0) return NAF_ERR_ARG;
    if (records && (record_slots <= 0 || !counter_dev)) return NAF_ERR_ARG;
    const int A = h->A;
    const int rf = naf_replay_row_floats(2 * A + 9, A);
    if (rf <= 0) return NAF_ERR_ARG;
    chain_env_step_kernel<<<(E + 63) / 64, 64, 0, (hipStream_t)stream>>>(h->model_dev, env_state, actions, out_rows, obs_next, E,
                                                                         A, h->n_seg, rf, seed, counter_dev, max_frames, records,
                                                                         record_slots);
    NAF_CHECK_LAUNCH();
    return NAF_OK;
}
