// Synthetic stand-in for the reference's PyBullet Environment, E independent arms stepped on the device.
// NOT a port of Bullet: a kinematic serial chain (alternating z / y revolute axes, velocity control applied
// exactly) that keeps the reference's observable contract so the hot path sees data of the right shape:
//   state  = [q(A), qdot(A), end-effector xyz, target xyz, obstacle xyz]   (environment.py:431-451, S = 9+2A)
//   reward = +250 on reaching the target (dist < 0.05), -1000 on obstacle contact, else -(dist - 0.05)
//            (environment.py:345-371, :419-429)
//   done   = 1 on either terminal event (environment.py:311-333)
//   step   = velocity control for one 1/240 s simulation tick (environment.py:453-485)
// PyBullet is not installed in the image and has no pinned version upstream: env parity is "unpinned";
// this file exists so env-steps/s can be measured without leaving the GPU.
#include "synth_env_body.h"

// preset: [init_q(8) | target(3) | obstacle(3) | obstacle_jitter | variation(8)] — the demo presets of the reference
// (rl_framework.py:547-555 KUKA, :571-580 xArm6) or the caller's own; obstacle_jitter > 0 gives every env its own
// obstacle position, uniform in a cube of that half-width around the preset (BASELINE configs[3]); variation[k] = half-width
// of the uniform range joint k's initial position is drawn from at every reset (initial_positions_variation_range,
// environment.py:284-293)
struct EnvPreset {
    float v[NAF_SYNTH_PRESET_FLOATS];
};

__global__ void synth_env_reset_kernel(float* env_state, float* obs, int E, int A, uint64_t seed, uint64_t ctr,
                                       const EnvPreset preset) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    float* st = env_state + (int64_t)e * ENV_STATE_FLOATS;
    for (int k = 0; k < 8; ++k) { st[14 + k] = preset.v[k]; st[ENV_OFF_VAR + k] = preset.v[15 + k]; }
    st[34] = st[35] = 0.f;
    for (int k = 0; k < 3; ++k) { st[8 + k] = preset.v[8 + k]; st[11 + k] = preset.v[11 + k]; }
    if (preset.v[14] > 0.f) {
        Philox4 p = philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)e, 0x4f425354u, 0x9E3779B9u, 0x243F6A88u);
        for (int k = 0; k < 3; ++k) st[11 + k] += (naf_u01(p.v[k]) * 2.f - 1.f) * preset.v[14];
    }
    st[23] = 0.f;
    env_reset_one(st, e, A, seed, ctr);
    float qd[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ee[3];
    bool hit;
    fk_chain(st, A, ee, st + 11, 0.06f, &hit);
    write_obs(obs + (int64_t)e * (2 * A + 9), st, qd, ee, st + 8, st + 11, A);
}

__global__ void synth_env_step_kernel(float* env_state, const float* __restrict__ actions, float* __restrict__ out_rows,
                                      float* __restrict__ obs_next, int E, int A, int row_floats, uint64_t seed,
                                      const uint64_t* counter_dev, int max_frames, naf_episode_record_t* __restrict__ records,
                                      int record_slots) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const uint64_t ctr = counter_dev ? *counter_dev : 0ull;
    synth_env_step_body(env_state + (int64_t)e * ENV_STATE_FLOATS, actions + (int64_t)e * A, out_rows + (int64_t)e * row_floats,
                        obs_next + (int64_t)e * (2 * A + 9), e, E, A, row_floats, seed, ctr, max_frames, records, record_slots);
}

extern "C" int naf_synth_env_state_floats(int A) { return (A > 0 && A <= NAF_MAX_A) ? ENV_STATE_FLOATS : NAF_ERR_ARG; }

extern "C" int naf_synth_env_reset(float* env_state, float* obs, int E, int A, uint64_t seed, uint64_t counter,
                                   const float* preset_host, int preset_floats, void* stream) {
    if (!env_state || !obs || E <= 0 || A <= 0 || A > NAF_MAX_A) return NAF_ERR_ARG;
    if (preset_host && preset_floats != 15 && preset_floats != NAF_SYNTH_PRESET_FLOATS) return NAF_ERR_ARG;
    // default: the reference's KUKA demo preset (rl_framework.py:551-553), no obstacle jitter, +-0.1 on every joint
    EnvPreset p = {{0.9f, 0.45f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.4f, 0.85f, 0.71f, 0.45f, 0.55f, 0.55f, 0.f,
                    0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f}};
    if (preset_host)
        for (int k = 0; k < preset_floats; ++k) p.v[k] = preset_host[k];
    synth_env_reset_kernel<<<(E + 63) / 64, 64, 0, (hipStream_t)stream>>>(env_state, obs, E, A, seed, counter, p);
    NAF_CHECK_LAUNCH();
    return NAF_OK;
}

extern "C" int naf_synth_env_step(float* env_state, const float* actions, float* out_rows, float* obs_next, int E, int A,
                                  uint64_t seed, const uint64_t* counter_dev, int max_frames, naf_episode_record_t* records,
                                  int record_slots, void* stream) {
    if (!env_state || !actions || !out_rows || !obs_next || E <= 0 || A <= 0 || A > NAF_MAX_A) return NAF_ERR_ARG;
    if (records && (record_slots <= 0 || !counter_dev)) return NAF_ERR_ARG;
    int rf = naf_replay_row_floats(2 * A + 9, A);
    synth_env_step_kernel<<<(E + 63) / 64, 64, 0, (hipStream_t)stream>>>(env_state, actions, out_rows, obs_next, E, A, rf,
                                                                         seed, counter_dev, max_frames, records, record_slots);
    NAF_CHECK_LAUNCH();
    return NAF_OK;
}
